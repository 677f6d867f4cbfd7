"""-m gpu: the fp8 KV cache (include/eilev_kv8.h, libeilev_hip_kv8.so; HipEngine._select_decode_device(kv_dtype="fp8"),
generate(kv_cache_dtype="fp8")).

1. eilev_kv8_quantize bit for bit against tests/kv8_ref.py;
2. the attention kernel alone, on the case list of tests/kv8_ref.py, against the float64 reference over the dequantised planes and the derived
   tolerance (tests/test_kv8_ref.py holds the same list to its preconditions and planted mistakes on the CPU);
3. a whole step against the existing bf16 step on the cache's exact bf16 twin;
4. generate(kv_cache_dtype="fp8") on the goldens: the routes, the graph key, and the quantisation loss as a recorded number."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kv8_ref as ref
from hip_utils import host, load_case, models, rel_rms

pytestmark = pytest.mark.gpu

SENT16 = 0x7FA5  # poison around the output (a NaN as bf16)
_WORST: dict = {}


def _kv():
    from eilev_amd import abi

    return abi.load_kv8()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dims(layers, heads, hd):
    from eilev_amd import abi

    return abi.Dims(t_hidden=heads * hd, t_heads=heads, t_ffn=2 * heads * hd, t_layers=layers, vocab=128, max_pos=64, t_eps=1e-5)


# ---- 1. the quantiser -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [80, 128])
def test_quantize_bit_for_bit(hd):
    """Planes (layers 2, k | v, batch 3, heads 2, cap 37, hd), slots [0, 29) into a cache of capacity 41 that sits inside a poisoned buffer:
    bytes and exponents equal kv8_ref.quantize; slots at or beyond 29 and everything outside the cache are unchanged."""
    layers, B, H, src_cap, slots, dst_cap, guard = 2, 3, 2, 37, 29, 41, 256
    d = _dims(layers, H, hd)
    g = torch.Generator().manual_seed(hd)
    src = torch.randn((layers, 2, B, H, src_cap, hd), generator=g)
    src = src * torch.pow(2.0, torch.randint(-140, 118, (layers, 2, B, H, src_cap, 1), generator=g).float())  # every scale, the clamp included
    src = src * torch.pow(2.0, -torch.randint(0, 12, src.shape, generator=g).float())                          # ... and subnormal bytes
    src[0, 0, 0, 0, 3] = 0.0
    src[1, 1, 2, 1, 7, 5:] = 0.0
    src = src.to(torch.bfloat16)
    kv = _kv()
    nb = int(kv.eilev_kv8_cache_bytes(C.byref(d), B, dst_cap))
    n8 = layers * 2 * B * H * dst_cap * hd
    exp_off = -(-n8 // 256) * 256
    assert nb == -(-(exp_off + n8 // hd) // 256) * 256
    buf = torch.full((guard + nb + guard,), ref.NAN_BYTE, dtype=torch.uint8)
    buf[guard + exp_off:guard + nb] = ref.NAN_EXP
    before = buf.clone()
    dev, src_dev = buf.cuda(), src.cuda()
    rc = kv.eilev_kv8_quantize(C.byref(d), src_dev.data_ptr(), B, src_cap, slots, dev.data_ptr() + guard, dst_cap, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = dev.cpu()
    got8 = got[guard:guard + n8].view(layers, 2, B, H, dst_cap, hd)
    gote = got[guard + exp_off:guard + exp_off + n8 // hd].view(layers, 2, B, H, dst_cap)
    want8, wante = ref.quantize(src[..., :slots, :])
    assert torch.equal(gote[..., :slots], wante), "exponents"
    assert torch.equal(got8[..., :slots, :], want8), "bytes"
    assert int((wante == 1).sum()) > 0 and int((wante > 200).sum()) > 0 and int(((want8 & 0x78) == 0).sum()) > 0  # (the input reaches the clamp, large scales, subnormals)
    # everything else: as it was
    got8[..., :slots, :] = ref.NAN_BYTE
    gote[..., :slots] = ref.NAN_EXP
    assert torch.equal(got, before), "a byte outside slots [0, 29) changed"
    assert torch.equal(src_dev.cpu().view(torch.int16), src.view(torch.int16))


# ---- 2. the attention kernel alone ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(name):
    c = ref.build_case(ref.by_name(name))
    return (c, *ref.reference(c))


def _launch(c, pk, out, part, part_bytes=None, **over):
    """One eilev_kv8_attention call on the case's buffers; `out` and `part` are the poisoned tensors of _device_case (64 sentinels on each side)."""
    sp = c.spec
    a = dict(qkv=pk["qkv"].data_ptr(), ldq=c.ldq, k8=pk["k8"].data_ptr(), v8=pk["v8"].data_ptr(), ek=pk["ek"].data_ptr(), ev=pk["ev"].data_ptr(),
             mask=None if pk["mask"] is None else pk["mask"].data_ptr(), state=None if pk["state"] is None else pk["state"].data_ptr(), batch=sp.batch,
             seq=sp.seq_len, cap=sp.cap, heads=sp.heads, hd=sp.hd, fuse=sp.fuse_new)
    a.update(over)
    return _kv().eilev_kv8_attention(a["qkv"], a["ldq"], a["k8"], a["v8"], a["ek"], a["ev"], a["mask"], a["state"], a["batch"], a["seq"], a["cap"], a["heads"],
                                     a["hd"], a["fuse"], part.data_ptr() + 256, 4 * (part.numel() - 128) if part_bytes is None else part_bytes,
                                     out.data_ptr() + 128, _stream())


def _device_case(c):
    p = ref.pack(c)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    pk = {k: dev(getattr(p, k)) for k in ("qkv", "k8", "v8", "ek", "ev", "mask", "state")}
    sp = c.spec
    n_part = sp.batch * sp.heads * (-(-sp.cap // ref.RANGE)) * (sp.hd + 2)
    out = torch.full((64 + sp.batch * c.d + 64,), SENT16, dtype=torch.int16, device="cuda")
    part = torch.full((64 + n_part + 64,), float("nan"), dtype=torch.float32, device="cuda")
    return p, pk, out, part, n_part


@pytest.mark.parametrize("sp", ref.CASES, ids=lambda sp: sp.name)
def test_attention_against_float64(sp):
    """Acceptance: err <= 1.0 tol on every element (the derived bound of kv8_ref.py), a finite output (any read of an unwritten slot is
    NaN or inf); the sentinels around `out` and the partials, the q|k|v rows, the mask and every slot but the newest are bit-unchanged; after a
    fuse_new launch the newest slot holds kv8_ref.quantize of the step's rows."""
    from hip_utils import record_parity

    c, want, A = _built(sp.name)
    p, pk, out, part, n_part = _device_case(c)
    rc = _launch(c, pk, out, part)
    torch.cuda.synchronize()
    assert rc == 0, (sp.name, rc)
    raw = out.cpu().numpy()
    assert (raw[:64] == np.int16(SENT16)).all() and (raw[-64:] == np.int16(SENT16)).all(), "the sentinels around out"
    pr = part.cpu().numpy()
    assert np.isnan(pr[:64]).all() and np.isnan(pr[-64:]).all(), "the sentinels around the partials"
    got = ref.bits_to_f32(raw[64:-64]).reshape(sp.batch, c.d)
    ratio = ref.worst_ratio(got, want, A)
    print(f"[kv8 attention] {sp.name}: {ratio:.3f} tol")
    group = f"hd{sp.hd}"
    _WORST[group] = max(_WORST.get(group, 0.0), ratio)
    record_parity("kv8_attention", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element over the dequantised planes, no floor",
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()})
    if not ratio <= 1.0:
        err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - want) / ref.tolerance(A)
        b, e = np.unravel_index(np.argmax(err), err.shape)
        pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at row {b} head {e // sp.hd} dim {e % sp.hd} (got {got[b, e]}, ref {want[b, e]}); its spike at key "
                    f"{c.spike_pos[b, e // sp.hd]} of {sp.n}")
    assert np.array_equal(pk["qkv"].cpu().numpy(), p.qkv), "the q|k|v rows changed"
    if p.mask is not None:
        assert np.array_equal(pk["mask"].cpu().numpy(), p.mask)
    after = {k: pk[k].cpu().numpy() for k in ("k8", "ek", "v8", "ev")}
    if sp.fuse_new:
        new = sp.n - 1
        for k, exp in zip(("k8", "ek", "v8", "ev"), ref.new_slot_expected(c)):
            assert np.array_equal(after[k][:, :, new], exp), f"{sp.name}: {k} of the newest slot"
            after[k][:, :, new] = getattr(p, k)[:, :, new]
    for k in after:
        assert np.array_equal(after[k], getattr(p, k)), f"{sp.name}: {k} changed outside the newest slot"


def test_attention_refusals_launch_nothing():
    c, _, _ = _built("sweep-hd80-n257-state")
    sp = c.spec
    p, pk, out, part, n_part = _device_case(c)
    o, q = out, part
    assert _launch(c, pk, o, q, hd=64, ldq=3 * sp.heads * 64) == -2
    assert _launch(c, pk, o, q, cap=sp.seq_len - 1) == -1
    assert _launch(c, pk, o, q, k8=pk["k8"].data_ptr() + 8) == -1 and _launch(c, pk, o, q, v8=pk["v8"].data_ptr() + 4) == -1
    assert _launch(c, pk, o, q, part_bytes=4 * n_part - 1) == -3
    assert _launch(c, pk, o, q, batch=0) == -1 and _launch(c, pk, o, q, ldq=3 * c.d - 8) == -1
    torch.cuda.synchronize()
    assert bool((out == SENT16).all()) and bool(torch.isnan(part).all())
    for k in ("k8", "ek", "v8", "ev"):
        assert np.array_equal(pk[k].cpu().numpy(), getattr(p, k))
    assert _launch(c, pk, o, q, part_bytes=4 * n_part) == 0  # (exactly enough)
    torch.cuda.synchronize()


# ---- 3. a step is wired right ----------------------------------------------------------------------------------------------------------------------
STEP_BOUND = 1e-2  # the project's decode-step bound (test_hip_prefix.py, test_hip_varied.py: rel-RMS of a step's logits between two kernel routes)


def _engine(cfg_name):
    if cfg_name in ("mid", "mid_k128"):
        return models(cfg_name)[2]
    from test_hip_prefix import _lm_engine

    return _lm_engine(cfg_name)


def _planes(eng, kv8, B, cap):
    """The fp8 cache's byte planes [layers][k | v][B][H][cap][hd] and exponent planes [...][cap] as views."""
    d = eng.dims
    H, hd = d.t_heads, d.t_hidden // d.t_heads
    n8 = d.t_layers * 2 * B * H * cap * hd
    off = -(-n8 // 256) * 256
    return kv8[:n8].view(d.t_layers, 2, B, H, cap, hd), kv8[off:off + n8 // hd].view(d.t_layers, 2, B, H, cap)


@pytest.mark.parametrize("R", [3, 32])
@pytest.mark.parametrize("cfg_name,L", [("mid", 40), ("mid_k128", 40), ("opt27_2l", 300)])
def test_step_equals_the_bf16_step_on_the_twin(cfg_name, L, R):
    """Prefill, eilev_kv8_quantize, the exact bf16 twin of the fp8 cache (kv8_ref.dequantize); then 4 eager steps of eilev_kv8_decode_step
    and of eilev_opt_decode_step on the twin, fed the same tokens, the twin's new slot overwritten after each step with the dequantised
    form of the fp8 cache's.  Both steps see the same operands — in the step that writes a slot both score it from the bf16 row — so their
    logits differ by kernel arithmetic alone: within the project's decode-step bound.  Every emitted id is the arg-max of its own logits; the
    captured run (twice: the second from the cached graph) returns the eager ids; an EOS id ends a row and pads the rest."""
    from eilev_amd.engine import _ptr

    eng, kv = _engine(cfg_name), _kv()
    d = eng.dims
    D, T = d.t_hidden, 4
    cap = L + T + 1
    g = torch.Generator().manual_seed(13 + R)
    emb = (0.5 * torch.randn(R, L, D, generator=g)).to(torch.bfloat16).cuda()
    am = torch.ones(R, L, dtype=torch.int32)
    for r in range(R):
        am[r, :(r * 7) % 13] = 0  # left padding of different amounts
    am = am.cuda()
    last, _, kv16 = eng.prefill(emb, am, kv_capacity=L)
    kv8 = eng.new_kv8_cache(R, cap)
    kv8.fill_(ref.NAN_BYTE)
    b8, e8 = _planes(eng, kv8, R, cap)
    e8.fill_(ref.NAN_EXP)
    assert kv.eilev_kv8_quantize(C.byref(d), _ptr(kv16), R, L, L, _ptr(kv8), cap, _stream()) == 0
    H, hd = d.t_heads, D // d.t_heads
    twin = torch.full((d.t_layers, 2, R, H, cap, hd), float("nan"), dtype=torch.bfloat16, device="cuda")
    dq = ref.dequantize(b8[..., :L, :], e8[..., :L])
    assert torch.equal(dq.to(torch.bfloat16).float(), dq)
    twin[..., :L, :] = dq.to(torch.bfloat16)
    src = kv16.view(torch.bfloat16).view(d.t_layers, 2, R, H, L, hd).float()
    loss = rel_rms(host(dq), host(src))
    print(f"[kv8 step] {cfg_name} R={R}: the quantised prompt cache against the bf16 one: rel-rms {loss:.2e}")
    assert loss < 2.0 ** -4  # (e4m3: 3 mantissa bits; a gross check that the twin is the prompt's cache)
    n_valid = am.sum(dim=1).to(torch.int32).contiguous()
    mk = lambda: dict(state=torch.zeros(2, dtype=torch.int32, device="cuda"), fin=torch.zeros(R, dtype=torch.uint8, device="cuda"),
                      tok=torch.zeros(R, dtype=torch.int64, device="cuda"), out=torch.full((R, T + 1), 1, dtype=torch.int64, device="cuda"),
                      logits=torch.empty((R, d.vocab), dtype=torch.float32, device="cuda"))
    s8, s16 = mk(), mk()
    for s in (s8, s16):
        eng._greedy_select(last, R, d.vocab, s["state"], s["fin"], -1, 1, s["tok"], s["out"])
    ws8 = torch.empty(int(kv.eilev_kv8_workspace_bytes(C.byref(d), R)), dtype=torch.uint8, device="cuda")
    ws16 = torch.empty(int(eng.lib.eilev_opt_workspace_bytes(C.byref(d), R, 1)), dtype=torch.uint8, device="cuda")
    eng.ensure_stream_layout(R)
    worst = 0.0
    for k in range(T):
        s16["tok"].copy_(s8["tok"])  # the same tokens are fed
        for fn, s, cache, ws in ((kv.eilev_kv8_decode_step, s8, kv8, ws8), (eng.lib.eilev_opt_decode_step, s16, twin, ws16)):
            rc = fn(C.byref(d), C.byref(eng.pack.opt), _ptr(s["tok"]), _ptr(s["state"]), _ptr(am), _ptr(n_valid), R, L, _ptr(cache), cap, _ptr(s["logits"]),
                    _ptr(s["fin"]), -1, 1, _ptr(s["out"]), T + 1, _ptr(ws), ws.numel(), _stream())
            assert rc == 0, (fn, rc)
        torch.cuda.synchronize()
        lg8, lg16 = host(s8["logits"]), host(s16["logits"])
        assert np.isfinite(lg8).all()
        dist = rel_rms(lg8, lg16)
        worst = max(worst, dist)
        assert np.array_equal(lg8[:, :d.vocab].argmax(-1), s8["out"][:, k + 1].cpu().numpy()), k
        # the slot this step wrote: quantised from the step's rows; the twin gets its dequantised form
        dq = ref.dequantize(b8[..., L + k, :], e8[..., L + k])
        assert bool(torch.isfinite(dq).all()) and rel_rms(host(dq), host(twin[..., L + k, :].float())) < 2.0 ** -4
        twin[..., L + k, :] = dq.to(torch.bfloat16)
        assert bool((b8[..., L + k + 1:, :] == ref.NAN_BYTE).all()) and bool((e8[..., L + k + 1:] == ref.NAN_EXP).all()), "a slot behind the newest was written"
    print(f"[kv8 step] {cfg_name} R={R}: worst step rel-rms against the bf16 step on the twin {worst:.2e}")
    assert worst <= STEP_BOUND
    assert int(s8["state"][0]) == T + 1
    ids = s8["out"].clone()
    eager = eng.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=False, kv_dtype="fp8")
    assert torch.equal(eager, ids)
    captured = eng.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=True, kv_dtype="fp8")
    assert torch.equal(captured, ids) and eng._dec_cache["key"][-1] == "fp8" and eng._dec_cache["graph"] is not None
    graph = eng._dec_cache["graph"]
    again = eng.greedy_decode(emb, am, T + 1, eos_id=-1, use_graph=True, kv_dtype="fp8")  # the cached graph, replayed
    assert torch.equal(again, ids) and eng._dec_cache["graph"] is graph
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
        got = eng.greedy_decode(emb, am, T + 1, eos_id=eos, pad_id=pad, use_graph=use_graph, poll_every=1, kv_dtype="fp8").cpu().numpy()
        assert np.array_equal(got, want[:, :stop]), (use_graph, got, want)


# ---- 4. generate(kv_cache_dtype="fp8") ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid_b1", "mid_v1"])
def test_generate_with_an_fp8_cache(golden_dir, name):
    """The three device routes run with the fp8 cache; the cached graph's key carries the dtype, so a following bf16 call of the same shape
    does not reuse the fp8 graph and returns exactly what it returned before.  The quantisation loss is RECORDED, not asserted: no honest
    bound for it can be derived here (synthetic weights have near-tied logits) — test_step_equals_the_bf16_step_on_the_twin guards the wiring."""
    from hip_utils import record_parity
    from test_hip_prefix import _build_model

    g, meta, px = load_case(golden_dir, name)
    m = _build_model(meta)
    t = lambda a: torch.from_numpy(a).cuda()
    ids, vm = t(g["input_ids"]), t(g["video_input_mask"])
    n_new = meta["new_tokens"]
    kw = dict(pixel_values=t(px), video_input_mask=vm, max_new_tokens=n_new, min_new_tokens=None, eos_token_id=meta.get("never_id", 511))
    before = m.generate(ids, **kw)
    eng = m.engine()
    assert eng._dec_cache["key"][-1] == "bf16"
    out8 = m.generate(ids, kv_cache_dtype="fp8", **kw)
    assert out8.shape == before.shape and eng._dec_cache["key"][-1] == "fp8"
    graph8 = eng._dec_cache["graph"]
    assert torch.equal(m.generate(ids, kv_cache_dtype="fp8", **kw), out8) and eng._dec_cache["graph"] is graph8
    after = m.generate(ids, kv_cache_dtype="bf16", **kw)
    assert torch.equal(after, before) and eng._dec_cache["key"][-1] == "bf16" and eng._dec_cache["graph"] is not graph8
    assert torch.equal(m.generate(ids, **kw), before)
    # sampling with fixed uniforms, and the logits rules: both on their device routes
    emb = m._encode(kw["pixel_values"], ids, vm)[0]
    am = torch.ones_like(ids)
    uni = torch.rand((n_new, ids.shape[0]), generator=torch.Generator().manual_seed(5)).cuda()
    eng.sample_stats = None
    s8 = eng.sample_decode_device(emb, am, n_new, eos_id=-1, top_k=0, uniforms=uni, kv_dtype="fp8")
    assert eng.sample_stats["path"] == "device" and eng._dec_cache["key"][-1] == "fp8" and s8.shape == before.shape
    assert torch.equal(eng.sample_decode_device(emb, am, n_new, eos_id=-1, top_k=0, uniforms=uni, kv_dtype="fp8"), s8)
    eng.sample_stats = None
    sg = m.generate(ids, do_sample=True, generator=torch.Generator(device="cuda").manual_seed(3), kv_cache_dtype="fp8", **kw)
    assert eng.sample_stats["path"] == "device" and sg.shape == before.shape
    eng.rules_stats = None
    r8 = m.generate(ids, repetition_penalty=1.5, no_repeat_ngram_size=3, kv_cache_dtype="fp8", **kw)
    assert eng.rules_stats["path"] == "device" and eng._dec_cache["key"][-1] == "fp8" and r8.shape == before.shape
    r16 = m.generate(ids, repetition_penalty=1.5, no_repeat_ngram_size=3, **kw)
    assert eng._dec_cache["key"][-1] == "bf16"
    # the quality report
    want = g["fp32_greedy_free"]
    _, tr16 = eng.greedy_decode(emb, am, 2, eos_id=-1, use_graph=False, return_step_logits=True)
    _, tr8 = eng.greedy_decode(emb, am, 2, eos_id=-1, use_graph=False, return_step_logits=True, kv_dtype="fp8")
    assert torch.equal(tr8[0], tr16[0])  # (the prefill is the same call)
    step_rms = rel_rms(host(tr8[1]), host(tr16[1]))
    total = int(np.prod(want.shape))
    print(f"[kv8 generate] {name}: ids equal to the reference {int((out8.cpu().numpy() == want).sum())} / {total} (bf16 cache: "
          f"{int((before.cpu().numpy() == want).sum())}), first decode step's logits against the bf16 route rel-rms {step_rms:.2e}")
    record_parity(f"generate_kv8[{name}]", ids_equal_reference=int((out8.cpu().numpy() == want).sum()), ids_total=total,
                  ids_equal_reference_bf16_cache=int((before.cpu().numpy() == want).sum()), ids_equal_bf16_route=int((out8 == before).sum()),
                  rules_ids_equal_bf16_route=int((r8 == r16).sum()) if r8.shape == r16.shape else -1, first_step_logits_rel_rms_vs_bf16=step_rms)
