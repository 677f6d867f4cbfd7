"""-m gpu: the int4 weight-only OPT linears (include/eilev_w4.h, libeilev_hip_w4.so; HipEngine(lm_weights="int4"), hip_lm_weights="int4").

1. eilev_w4_expand bit for bit against the torch twin of eilev_amd/quant.py;
2. the kernel alone through eilev_w4_linear, on the case list of tests/w4_ref.py: exact where every sum is exact in fp32, else against the float64
   reference over (A, W') and the bound of the bf16 decode kernels (tests/test_w4_ref.py holds that reference to its planted mistakes on the CPU);
3. a whole step against the existing bf16 step on an engine loaded with the twin weights;
4. generate() on the model class: the routes, the ids against the CPU oracle on the twin weights, the gross size of the quantisation's effect."""
import ctypes as C

import numpy as np
import pytest
import torch

import w4_ref as ref
from eilev_amd import quant
from hip_utils import host, rel_rms

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0  # bf16 NaN bits: traps around the operands, sentinels around the outputs
GUARD = 64      # elements of guard in front of and behind every buffer


def _w4():
    from eilev_amd import abi

    return abi.load_w4()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(t, fill_bits=NAN16, ld=None):
    """`t` (2-D, or 1-D) on the device inside a buffer of NaN bits: GUARD elements in front and behind, and, with ld > columns, NaN in the padding
    columns of every row.  Returns (whole buffer, the view that holds t)."""
    t2 = t if t.dim() == 2 else t.view(1, -1)
    rows, cols = t2.shape
    ld = ld or cols
    if t2.dtype in (torch.bfloat16,):
        buf = torch.full((GUARD + rows * ld + GUARD,), fill_bits, dtype=torch.int16).view(torch.bfloat16)
    elif t2.dtype == torch.float32:
        buf = torch.full((GUARD + rows * ld + GUARD,), float("nan"), dtype=torch.float32)
    else:
        buf = torch.full((GUARD + rows * ld + GUARD,), 0xFF, dtype=torch.uint8)
    buf = buf.cuda()
    view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t2.cuda())
    return buf, view


def _guard_intact(buf, view, rows, cols, ld):
    """Everything of `buf` outside the rows x cols window is still NaN."""
    b = buf.float().cpu().numpy() if buf.dtype != torch.uint8 else buf.cpu().numpy().astype(np.float32)
    inner = b[GUARD:GUARD + rows * ld].reshape(rows, ld)
    return bool(np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + rows * ld:]).all() and np.isnan(inner[:, cols:]).all())


# ---- 1. the expansion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", ref.EXPAND_CASES)
def test_expand_bit_for_bit(n, k):
    """Codes over all 16 values (-8 included), scales 2^-20 .. 2^6 with non-power-of-two mantissas: the bits of quant.twin_int4; NaN sentinels around
    the output stay."""
    q, s = ref.all_codes(n, k, seed=n), ref.wide_scales(n, k // 128, seed=k)
    assert sorted(set(q.flatten().tolist())) == list(range(-8, 8))
    want = quant.twin_int4(q, s)
    _, pk = _guarded(quant.pack_int4(q))
    sbuf, sv = _guarded(s)
    obuf, ov = _guarded(torch.zeros(n, k, dtype=torch.bfloat16))
    ov.view(torch.int16).fill_(NAN16)
    pk, sv = pk.contiguous(), sv.contiguous()
    assert pk.data_ptr() % 16 == 0 and sv.data_ptr() % 16 == 0 and ov.data_ptr() % 16 == 0
    assert _w4().eilev_w4_expand(pk.data_ptr(), sv.data_ptr(), n, k, ov.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ov.cpu().view(torch.int16), want.view(torch.int16))
    assert _guard_intact(obuf, ov, n, k, k)


# ---- 2. the kernel alone ----------------------------------------------------------------------------------------------------------------------------
class _Linear:
    """One eilev_w4_linear launch with every buffer inside NaN guards; out / ln / scratch are re-poisoned per launch."""

    def __init__(self, A, q, s, bias=None, resid=None, out_f32=False, scale=1.0, scale_cols=0, relu=False, ln=None):
        from eilev_amd import abi

        self.abi, self.lib = abi, _w4()
        self.m, self.k = A.shape
        self.n = q.shape[0]
        self.lda, self.ldc = self.k + 8, self.n + 8
        self.A = _guarded(A, ld=self.lda)
        pk = quant.pack_int4(q)
        self.W = _guarded(pk)
        self.S = _guarded(s)
        self.Wv, self.Sv = self.W[1].contiguous(), self.S[1].contiguous()  # (ld == columns: already dense; the guards sit around them)
        assert self.Wv.data_ptr() == self.W[1].data_ptr() and self.Sv.data_ptr() == self.S[1].data_ptr()
        self.bias = None if bias is None else _guarded(bias)
        self.out_f32, self.scale, self.scale_cols, self.relu = out_f32, scale, scale_cols, relu
        self.resid0 = resid  # in place: the output buffer is loaded with it before every launch
        self.C = _guarded(torch.zeros(self.m, self.n, dtype=torch.float32 if out_f32 else torch.bfloat16), ld=self.ldc)
        self.ln = ln
        if ln is not None:
            self.gamma, self.beta = _guarded(ln[0]), _guarded(ln[1])
            self.ln_out = _guarded(torch.zeros(self.m, self.n, dtype=torch.bfloat16))
        self.form = (C.c_int32 * 5)()
        assert self.lib.eilev_w4_plan(self.m, self.n, self.k, self.form) == 0
        assert tuple(self.form) == abi.w4_plan(self.m, self.n, self.k)
        self.ks = self.form[1]
        self.need = int(self.lib.eilev_w4_linear_scratch_bytes(self.m, self.n, self.k))
        assert self.need == (self.ks * 16 * self.form[0] * self.n * 4 if self.ks > 1 else 0)
        self.scratch = torch.full((GUARD + self.need // 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")

    def launch(self):
        abi = self.abi
        poison = float("nan")
        self.C[1].fill_(poison)
        if self.resid0 is not None:
            self.C[1].copy_(self.resid0.cuda())
        if self.ln is not None:
            self.ln_out[1].fill_(poison)
        self.scratch.fill_(poison)
        l = abi.W4Linear(a=self.A[1].data_ptr(), lda=self.lda, w=abi.W4Matrix(self.Wv.data_ptr(), self.Sv.data_ptr()),
                         bias=None if self.bias is None else self.bias[1].data_ptr(), resid=self.C[1].data_ptr() if self.resid0 is not None else None,
                         ldr=self.ldc, c=self.C[1].data_ptr(), ldc=self.ldc, m=self.m, n=self.n, k=self.k, relu=int(self.relu), out_f32=int(self.out_f32),
                         scale=self.scale, scale_cols=self.scale_cols, scratch=self.scratch[GUARD:].data_ptr() if self.need else None,
                         scratch_bytes=self.need)
        if self.ln is not None:
            l.ln_gamma, l.ln_beta, l.ln_out, l.ln_eps = self.gamma[1].data_ptr(), self.beta[1].data_ptr(), self.ln_out[1].data_ptr(), 1e-5
        rc = self.lib.eilev_w4_linear(C.byref(l), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        out = self.C[1].clone()
        ln = self.ln_out[1].clone() if self.ln is not None else None
        return out, ln

    def check_guards(self):
        assert _guard_intact(self.C[0], self.C[1], self.m, self.n, self.ldc), "a store outside the output"
        if self.ln is not None:
            assert _guard_intact(self.ln_out[0], self.ln_out[1], self.m, self.n, self.n), "a store outside ln_out"
        sc = self.scratch.cpu().numpy()
        assert np.isnan(sc[:GUARD]).all() and np.isnan(sc[GUARD + self.need // 4:]).all(), "a store outside the scratch"
        used = sc[GUARD:GUARD + self.need // 4]
        if self.ks > 1:  # the split form really ran: every partial of the M rows was written (rows M .. 16 MB - 1 of a plane never are)
            planes = used.reshape(self.ks, 16 * self.form[0], self.n)
            assert np.isfinite(planes[:, :self.m]).all() and np.isnan(planes[:, self.m:]).all()


@pytest.mark.parametrize("m,n,k", ref.LINEAR_CASES, ids=lambda v: str(v))
def test_linear_against_float64(m, n, k):
    """Exact operands: the fp32 output equals float64 bit for bit, the bf16 output after one rounding.  Dense operands: the per-element bound of
    the bf16 decode kernels on (A, W'), with every epilogue: bias, the scaled q columns, ReLU, fp32 output, the in-place residual, the LayerNorm
    rows.  NaN traps around A and the scales, sentinels around every output and the scratch; the plan's form is the mirror's; a second launch
    returns the same bits."""
    from eilev_amd import abi

    mb, ks = abi.w4_plan(m, n, k)[:2]
    assert mb == (1 if m <= 16 else 2)
    seed = 1000 * m + n + k
    g = torch.Generator().manual_seed(seed)
    # ---- exact ----
    A, q, s = ref.exact_operands(m, n, k, seed)
    assert int((q == -8).sum()) > 0
    W = ref.twin64(q, s)
    bias_i = torch.randint(-8, 9, (n,), generator=g).to(torch.bfloat16)
    y, _ = ref.linear_ref(A.float().numpy(), W, bias=bias_i.float().numpy())
    assert np.abs(y).max() < 2.0 ** 24
    run = _Linear(A, q, s, bias=bias_i, out_f32=True)
    out, _ = run.launch()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), y), "exact operands, fp32 output"
    run.check_guards()
    run = _Linear(A, q, s, bias=bias_i, out_f32=False)
    out, _ = run.launch()
    assert torch.equal(out.cpu(), torch.from_numpy(y).float().to(torch.bfloat16)), "exact operands, bf16 output: one rounding"
    run.check_guards()
    # ---- dense ----
    A, q, s = ref.dense_operands(m, n, k, seed + 1)
    W = ref.twin64(q, s)
    A64 = A.float().numpy()
    bias = (0.5 * torch.randn(n, generator=g)).to(torch.bfloat16)
    resid = torch.randn(m, n, generator=g).to(torch.bfloat16)
    gamma, beta = (1.0 + 0.1 * torch.randn(n, generator=g)).to(torch.bfloat16), (0.1 * torch.randn(n, generator=g)).to(torch.bfloat16)
    sc_cols = (n // 3) & ~0  # the q third of a q | k | v matrix
    variants = [("fp32 plain", dict(out_f32=True), dict()),
                ("bias, scaled columns, relu", dict(bias=bias, scale=0.125, scale_cols=sc_cols, relu=True), dict(bias=bias.float().numpy(), scale=0.125, scale_cols=sc_cols, relu=True)),
                ("fp32 bias + scaled columns", dict(bias=bias, scale=0.125, scale_cols=sc_cols, out_f32=True), dict(bias=bias.float().numpy(), scale=0.125, scale_cols=sc_cols))]
    if n % 8 == 0 and n <= 4096:  # (what ln_out takes: the header)
        variants.append(("bias + in-place residual + LayerNorm rows", dict(bias=bias, resid=resid, ln=(gamma, beta)), dict(bias=bias.float().numpy(), resid=resid.float().numpy())))
    else:
        variants.append(("bias + in-place residual", dict(bias=bias, resid=resid), dict(bias=bias.float().numpy(), resid=resid.float().numpy())))
    if n % 8 == 0 and n <= 4096:  # LayerNorm rows behind an epilogue the fused reduce does not take: w4_reduce_kernel + a LayerNorm launch when split
        variants.append(("bias, scaled columns, relu + LayerNorm rows", dict(bias=bias, scale=0.125, scale_cols=sc_cols, relu=True, ln=(gamma, beta)),
                         dict(bias=bias.float().numpy(), scale=0.125, scale_cols=sc_cols, relu=True)))
    for name, kw, rkw in variants:
        run = _Linear(A, q, s, **kw)
        out, ln = run.launch()
        y, S = ref.linear_ref(A64, W, **rkw)
        t = ref.tol(y, S, k, ks, kw.get("out_f32", False))
        got = out.float().cpu().numpy().astype(np.float64)
        worst = float(ref.R.ratio(np.abs(got - y), t).max())
        print(f"[w4 linear] M={m} N={n} K={k} MB={mb} ks={ks} {name}: worst err / tol {worst:.3f}")
        assert worst <= 1.0, (name, worst)
        if ln is not None:
            want, lt = ref.ln_ref(got, gamma.float().numpy(), beta.float().numpy(), 1e-5)
            lw = float(ref.R.ratio(np.abs(ln.float().cpu().numpy().astype(np.float64) - want), lt).max())
            print(f"[w4 linear] M={m} N={n} K={k} LayerNorm rows: worst err / tol {lw:.3f}")
            assert lw <= 1.0, lw
        run.check_guards()
        again, ln2 = run.launch()
        assert torch.equal(again.view(torch.int32 if again.dtype == torch.float32 else torch.int16), out.view(torch.int32 if out.dtype == torch.float32 else torch.int16))
        assert ln is None or torch.equal(ln2.view(torch.int16), ln.view(torch.int16))


def test_linear_refusals_launch_nothing():
    A, q, s = ref.dense_operands(3, 40, 512, 5)
    run = _Linear(A, q, s)
    abi = run.abi
    run.C[1].fill_(float("nan"))
    base = dict(a=run.A[1].data_ptr(), lda=run.lda, w=abi.W4Matrix(run.Wv.data_ptr(), run.Sv.data_ptr()), c=run.C[1].data_ptr(), ldc=run.ldc, m=3, n=40, k=512,
                scale=1.0)
    for kw, rc in ((dict(m=33), -1), (dict(k=384), -2), (dict(a=None), -1), (dict(lda=504), -1), (dict(ldc=32), -1),
                   (dict(ln_out=run.C[1].data_ptr()), -1)):
        l = abi.W4Linear(**dict(base, **kw))
        assert run.lib.eilev_w4_linear(C.byref(l), _stream()) == rc, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(run.C[0].float()).all())


# ---- 3. a step is wired right ----------------------------------------------------------------------------------------------------------------------
STEP_BOUND = 1e-2  # the project's decode-step bound (test_hip_prefix.py, test_hip_kv8.py: rel-RMS of a step's logits between two kernel routes)
_LINEARS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight", "fc1.weight", "fc2.weight")


def twin_state_dict(sd, hidden):
    """The state dict with every OPT block linear replaced by its int4 twin (q | k | v quantised as one [3 D, D] matrix, like the engine), on the CPU."""
    out = dict(sd)
    tt = lambda v: v if isinstance(v, torch.Tensor) else torch.from_numpy(v)
    back = (lambda t, v: t) if isinstance(next(iter(sd.values())), torch.Tensor) else (lambda t, v: t.float().numpy().astype(v.dtype))
    layers = sorted({k.split(".layers.")[1].split(".")[0] for k in sd if k.startswith("language_model.model.decoder.layers.")}, key=int)
    for i in layers:
        p = f"language_model.model.decoder.layers.{i}."
        names = [p + f"self_attn.{n}_proj.weight" for n in "qkv"]
        qkv = torch.cat([tt(sd[n]).float() for n in names], 0)
        tw = quant.twin_int4(*quant.quantize_int4(qkv))
        for j, n in enumerate(names):
            out[n] = back(tw[j * hidden:(j + 1) * hidden], sd[n])
        for n in (p + "self_attn.out_proj.weight", p + "fc1.weight", p + "fc2.weight"):
            out[n] = back(quant.twin_int4(*quant.quantize_int4(tt(sd[n]).float())), sd[n])
    return out


_ENGINES = {}


def _engines(cfg_name):
    """(int4 engine, bf16 engine on the twin weights) from the same synthetic weights; language model only."""
    if cfg_name not in _ENGINES:
        from eilev_amd.configs import blip2_config
        from eilev_amd.engine import HipEngine
        from eilev_amd.statedict import state_dict_shapes
        from eilev_amd.synth import synth_param

        cfg = blip2_config("mid_k128" if cfg_name == "mid_k128" else cfg_name[:5])
        if cfg_name != "mid_k128":
            cfg.text_config.num_hidden_layers = 2
        named = {k: torch.from_numpy(synth_param(k, shp, "fanin")).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()
                 if k.startswith("language_model")}
        twin = twin_state_dict(named, cfg.text_config.hidden_size)
        e4 = HipEngine(cfg, {k: v.cuda() for k, v in named.items()}, device="cuda", parts=("opt",), lm_weights="int4")
        e16 = HipEngine(cfg, {k: v.cuda() for k, v in twin.items()}, device="cuda", parts=("opt",))
        # the engine's expand-in-place: its bf16 weights ARE the twin computed on the CPU
        for k in twin:
            if k.endswith(_LINEARS) and ".layers." in k:
                assert torch.equal(e4._keep[k].cpu().view(torch.int16), twin[k].to(torch.bfloat16).view(torch.int16)), k
        _ENGINES.clear()  # (one pair at a time on the device)
        _ENGINES[cfg_name] = (e4, e16)
    return _ENGINES[cfg_name]


@pytest.mark.parametrize("R", [1, 3, 17, 32])
@pytest.mark.parametrize("cfg_name,L", [("mid_k128", 40), ("opt27_2l", 300)])
def test_step_equals_the_bf16_step_on_the_twin(cfg_name, L, R):
    """Prefill on both engines: the same kernels on the same operands, bit-equal logits.  Then 4 eager steps of eilev_w4_decode_step and of
    eilev_opt_decode_step on the twin engine, fed the same tokens: logits within the project's decode-step bound, every emitted id the arg-max of
    its own logits, KV slots behind the newest still NaN.  The captured run (twice: the second from the cached graph) returns the eager ids; an
    EOS id ends a row and pads the rest."""
    from eilev_amd.engine import _ptr

    e4, e16 = _engines(cfg_name)
    w4, table = e4._w4[0], e4._w4[1]
    d = e4.dims
    D, T = d.t_hidden, 4
    cap = L + T + 1
    g = torch.Generator().manual_seed(13 + R)
    emb = (0.5 * torch.randn(R, L, D, generator=g)).to(torch.bfloat16).cuda()
    am = torch.ones(R, L, dtype=torch.int32)
    for r in range(R):
        am[r, :(r * 7) % 13] = 0  # left padding of different amounts
    am = am.cuda()
    caches = []
    for e in (e4, e16):
        kv = e.new_kv_cache(R, cap)
        kv.view(torch.int16).fill_(NAN16)
        caches.append(kv)
    last4, _, _ = e4.prefill(emb, am, kv_cache=caches[0], kv_capacity=cap)
    last16, _, _ = e16.prefill(emb, am, kv_cache=caches[1], kv_capacity=cap)
    assert torch.equal(last4.view(torch.int32), last16.view(torch.int32)), "prefill: same kernels, same operands"
    n_valid = am.sum(dim=1).to(torch.int32).contiguous()
    mk = lambda: dict(state=torch.zeros(2, dtype=torch.int32, device="cuda"), fin=torch.zeros(R, dtype=torch.uint8, device="cuda"),
                      tok=torch.zeros(R, dtype=torch.int64, device="cuda"), out=torch.full((R, T + 1), 1, dtype=torch.int64, device="cuda"),
                      logits=torch.empty((R, d.vocab), dtype=torch.float32, device="cuda"))
    s4, s16 = mk(), mk()
    for s in (s4, s16):
        e4._greedy_select(last4, R, d.vocab, s["state"], s["fin"], -1, 1, s["tok"], s["out"])
    ws4 = torch.empty(int(w4.eilev_w4_workspace_bytes(C.byref(d), R)), dtype=torch.uint8, device="cuda")
    ws16 = torch.empty(int(e16.lib.eilev_opt_workspace_bytes(C.byref(d), R, 1)), dtype=torch.uint8, device="cuda")
    H, hd = d.t_heads, D // d.t_heads
    worst = 0.0
    for k in range(T):
        s16["tok"].copy_(s4["tok"])  # the same tokens are fed
        rc = w4.eilev_w4_decode_step(C.byref(d), C.byref(e4.pack.opt), table, _ptr(s4["tok"]), _ptr(s4["state"]), _ptr(am), _ptr(n_valid), R, L,
                                     _ptr(caches[0]), cap, _ptr(s4["logits"]), _ptr(s4["fin"]), -1, 1, _ptr(s4["out"]), T + 1, _ptr(ws4), ws4.numel(), _stream())
        assert rc == 0, rc
        rc = e16.lib.eilev_opt_decode_step(C.byref(d), C.byref(e16.pack.opt), _ptr(s16["tok"]), _ptr(s16["state"]), _ptr(am), _ptr(n_valid), R, L,
                                           _ptr(caches[1]), cap, _ptr(s16["logits"]), _ptr(s16["fin"]), -1, 1, _ptr(s16["out"]), T + 1, _ptr(ws16), ws16.numel(),
                                           _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        lg4, lg16 = host(s4["logits"]), host(s16["logits"])
        assert np.isfinite(lg4).all()
        dist = rel_rms(lg4, lg16)
        worst = max(worst, dist)
        assert np.array_equal(lg4[:, :d.vocab].argmax(-1), s4["out"][:, k + 1].cpu().numpy()), k
        planes = caches[0].view(torch.bfloat16).view(d.t_layers, 2, R, H, cap, hd)
        assert bool(torch.isfinite(planes[..., L + k, :].float()).all()), "the step's slot"
        assert bool(torch.isnan(planes[..., L + k + 1:, :].float()).all()), "a slot behind the newest was written"
    print(f"[w4 step] {cfg_name} R={R}: worst step rel-rms against the bf16 step on the twin {worst:.2e}")
    assert worst <= STEP_BOUND
    assert int(s4["state"][0]) == T + 1
    ids = s4["out"].clone()
    e4.w4_stats = None
    eager = e4.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=False)
    assert torch.equal(eager, ids) and e4.w4_stats == dict(step="eilev_w4_decode_step", rows=R, route="greedy", steps=T)
    one = e4.greedy_decode(emb, am, 1, eos_id=-1)  # one new token: the prefill alone, no step ran
    assert torch.equal(one, ids[:, :1]) and e4.w4_stats == dict(step=None, rows=R, route="greedy", steps=0)
    captured = e4.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=True)
    assert torch.equal(captured, ids) and e4._dec_cache["key"][1] == "int4" and e4._dec_cache["graph"] is not None
    assert e4.w4_stats == dict(step="eilev_w4_decode_step", rows=R, route="greedy", steps=T)
    graph = e4._dec_cache["graph"]
    again = e4.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=True)  # the cached graph, replayed
    assert torch.equal(again, ids) and e4._dec_cache["graph"] is graph
    # EOS: the id row 0 emits at step 2 ends every row at its first occurrence; what follows is the pad id
    free = ids.cpu().numpy()
    eos, pad = int(free[0, 2]), 1
    want = free.copy()
    for r in range(R):
        hit = np.flatnonzero(free[r] == eos)
        if len(hit):
            want[r, hit[0] + 1:] = pad
    stop = max((np.flatnonzero(free[r] == eos)[0] + 1) if (free[r] == eos).any() else T + 1 for r in range(R))
    for use_graph in (False, True):
        got = e4.greedy_decode(emb, am, T + 1, eos_id=eos, pad_id=pad, use_graph=use_graph, poll_every=1).cpu().numpy()
        assert np.array_equal(got, want[:, :stop]), (use_graph, got, want)
    # (no `as exc` here: the exception's traceback holds this frame, and the cycle would keep the graphs above alive until a later collection)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='fp8' together with lm_weights='int4'"):
        e4.greedy_decode(emb, am, T + 1, kv_dtype="fp8")
    del graph


# ---- 4. the model class ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [2, 4, 5])
def test_generate_on_the_model_class(seed):
    """hip_lm_weights="int4" on mid_k128: greedy, sampling and the logits rules run the int4 step (engine.w4_stats), beams run on the twin and say
    so.  The greedy ids equal the CPU oracle's on the twin weights on every row — after the oracle's own top-2 margin over the rms of its logits
    has been recomputed and found above 0.1 at every step (1.25 .. 1.55 with this quantiser on these seeds), so no near tie decides."""
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration
    from eilev_amd.synth import synth_interleaved_ids, synth_pixels
    from oracle.runner import OracleModel, synth_state_dict

    cfg = blip2_config("mid_k128")
    sd = synth_state_dict(cfg, "fanin")
    sdq = twin_state_dict(sd, cfg.text_config.hidden_size)
    oracle = OracleModel(cfg, sdq, emulate_bf16=True)
    px = synth_pixels(4, 2, cfg.vision_config.image_size)
    rows = [synth_interleaved_ids([1, 1], [6, 7], cfg.num_query_tokens, cfg.text_config.vocab_size, seed=seed),
            synth_interleaved_ids([1, 1], [6, 7], cfg.num_query_tokens, cfg.text_config.vocab_size, seed=seed + 100)]
    ids, vm = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    am = np.ones_like(ids)
    n_new = 6
    want, step_logits = oracle.generate(px, ids, am, vm, n_new, eos_id=-1, return_logits=True)
    margins = []
    for lg in step_logits[:n_new]:
        top2 = np.sort(lg[:, :cfg.text_config.vocab_size].astype(np.float64), axis=1)[:, -2:]
        margins.append((top2[:, 1] - top2[:, 0]) / np.sqrt((lg.astype(np.float64) ** 2).mean(axis=1)))
    margin = float(np.min(margins))
    print(f"[w4 generate] seed {seed}: the oracle's smallest top-2 margin / rms of its logits {margin:.3f}")
    assert margin > 0.1, margin

    m = VideoBlipForConditionalGeneration(cfg).eval()
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    tsd["language_model.lm_head.weight"] = tsd["language_model.model.decoder.embed_tokens.weight"]
    m.load_state_dict(tsd)
    m = m.to("cuda")
    t = lambda a: torch.from_numpy(a).cuda()
    kw = dict(pixel_values=t(px), video_input_mask=t(vm), attention_mask=t(am), max_new_tokens=n_new, min_new_tokens=None, eos_token_id=511)
    fw = dict(input_ids=t(ids), attention_mask=t(am), pixel_values=t(px), video_input_mask=t(vm))
    logits16 = m(**fw).logits.float()
    m.hip_lm_weights = "int4"
    eng = m.engine()
    assert eng.lm_weights == "int4" and eng.w4_stats is None
    got = m.generate(t(ids), **kw)
    assert eng.w4_stats == dict(step="eilev_w4_decode_step", rows=2, route="greedy", steps=n_new - 1)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    eng.w4_stats = None
    sg = m.generate(t(ids), do_sample=True, generator=torch.Generator(device="cuda").manual_seed(3), **kw)
    assert eng.w4_stats == dict(step="eilev_w4_decode_step", rows=2, route="sample", steps=n_new - 1) and eng.sample_stats["path"] == "device" and sg.shape == got.shape
    eng.w4_stats = None
    rg = m.generate(t(ids), repetition_penalty=1.5, no_repeat_ngram_size=3, **kw)
    assert eng.w4_stats == dict(step="eilev_w4_decode_step", rows=2, route="rules", steps=n_new - 1) and eng.rules_stats["path"] == "device" and rg.shape == got.shape
    eng.w4_stats = None
    bg = m.generate(t(ids), num_beams=3, **kw)
    assert eng.w4_stats["step"] == "twin" and bg.shape[0] == 2
    # the gross size of the quantisation: the int4 model's logits are the bf16 model's, perturbed (test_fp8_weights.py makes this check for e4m3)
    logits4 = m(**fw).logits.float()
    assert bool(torch.isfinite(logits4).all())
    rel = ((logits4 - logits16).pow(2).mean().sqrt() / logits16.pow(2).mean().sqrt()).item()
    print(f"[w4 generate] seed {seed}: int4 logits against bf16 logits rel-rms {rel:.3f}")
    assert 0 < rel < 0.5, rel
    with pytest.raises(NotImplementedError, match="int4"):
        m.generate(t(ids), kv_cache_dtype="fp8", **kw)
