"""-m gpu: the shared-prompt decode step (include/eilev_prefix.h eilev_prefix_decode_*; HipEngine.shared_prompt_reads,
generate(shared_prompt_reads=True)): OPT beam search and the rows after a context read a sample's prompt keys once for all its rows.

a. the attention alone through eilev_prefix_decode_attention, on the case list of tests/shared_prompt_cases.py, against attn_decode_ref's
   float64 reference and derived tolerance (tests/test_shared_prompt_ref.py holds the same list to the fp32 restatement on the CPU);
b. one captured launch replayed at three successive state[0];
c. the step on the context route = teacher forcing;  d. the step under beam search = teacher forcing of the hypothesis in each row;
e. generate(context=, shared_prompt_reads=True) on the goldens."""
import ctypes as C
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import attn_decode_ref as R
import shared_prompt_cases as cases
from hip_utils import host, load_case, models, record_parity, rel_rms

pytestmark = pytest.mark.gpu

SENT32 = 0x7FA5A5A5  # poison of `part` (a NaN as float)
SENT16 = 0x7FA5      # poison of `out` (a NaN as bf16)
GUARD = 64           # sentinel elements in front of and behind `out` and `part`
STEP_BOUND = 1e-2    # the project's decode-step bound (test_hip_varied.py, test_hip_prefix.py: rel-RMS of a step's logits)
_WORST: dict = {}


def _px():
    from eilev_amd import abi

    return abi.load_prefix()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_bits(a):
    return torch.from_numpy(R.bf16_bits(a)).cuda().view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _built(sp):
    c = cases.build(sp)
    return (c, *R.reference(c))


class Launch:
    """The device buffers of one case, `out` and `part` poisoned and guarded; launch() = one eilev_prefix_decode_attention call."""

    def __init__(self, c):
        sp = self.sp = c.spec
        self.c = c
        self.qkv, self.kc, self.vc, self.kg, self.vg = (_dev_bits(getattr(c, n)) for n in ("qkv", "kc", "vc", "kg", "vg"))
        self.anc = torch.from_numpy(c.anc_raw).cuda().contiguous()
        self.mask = torch.from_numpy(c.mask).cuda().contiguous() if c.mask is not None else None
        self.state = torch.tensor([sp.n_gen, 0], dtype=torch.int32, device="cuda")
        self.nrec = sp.batch * sp.heads * cases.nsplit_of(sp) * (sp.hd + 2)
        assert 4 * self.nrec == cases.part_bytes_of(sp)
        self.part = torch.full((GUARD + self.nrec + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.out = torch.full((GUARD + sp.batch * c.d + GUARD,), SENT16, dtype=torch.int16, device="cuda")

    def load(self, c):
        """Another case of the same shape into the same device buffers (the captured launch keeps their addresses)."""
        self.c = c
        for n in ("qkv", "kc", "vc", "kg", "vg"):
            getattr(self, n).copy_(_dev_bits(getattr(c, n)))
        self.anc.copy_(torch.from_numpy(c.anc_raw))
        self.state[0] = c.spec.n_gen
        self.part.fill_(SENT32)
        self.out.fill_(SENT16)

    def launch(self, part_bytes=None):
        sp, c = self.sp, self.c
        return _px().eilev_prefix_decode_attention(
            self.qkv.data_ptr(), c.ldq, self.kc.data_ptr(), self.vc.data_ptr(), sp.seq_len, sp.cap, None if self.mask is None else self.mask.data_ptr(),
            self.state.data_ptr(), self.kg.data_ptr(), self.vg.data_ptr(), sp.cap_g, self.anc.data_ptr(), sp.batch, sp.beams, sp.heads, sp.hd,
            self.out.data_ptr() + 2 * GUARD, self.part.data_ptr() + 4 * GUARD, 4 * self.nrec if part_bytes is None else part_bytes, _stream())

    def check(self, ref, A):
        """Every check of one launch; returns the worst err / tol."""
        sp, c = self.sp, self.c
        torch.cuda.synchronize()
        part, out = self.part.cpu().numpy(), self.out.cpu().numpy()
        assert (part[:GUARD] == SENT32).all() and (part[GUARD + self.nrec:] == SENT32).all(), f"{sp.name}: writes around `part`"
        assert (out[:GUARD] == SENT16).all() and (out[GUARD + sp.batch * c.d:] == SENT16).all(), f"{sp.name}: writes around `out`"
        rec = part[GUARD:GUARD + self.nrec].reshape(sp.batch, sp.heads, cases.nsplit_of(sp), sp.hd + 2)
        assert (rec[..., :2] != SENT32).all(), f"{sp.name}: a key range left no (max, sum)"
        f = rec.view(np.float32)
        empty = f[..., 1] == 0
        assert (f[..., 0][empty] == np.float32(-1e30)).all(), f"{sp.name}: an empty range's maximum"
        assert (rec[..., 2:][~empty] != SENT32).all() and np.isfinite(f[..., 2:][~empty]).all(), f"{sp.name}: a live range's o"
        got = R.bits_to_f32(out[GUARD:GUARD + sp.batch * c.d]).reshape(sp.batch, c.d)
        ratio = R.worst_ratio(got, ref, A)
        if not ratio <= 1.0:
            err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - ref) / R.tolerance(A)
            b, col = np.unravel_index(np.argmax(err), err.shape)
            pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at row {b} head {col // sp.hd} dim {col % sp.hd} (got {got[b, col]}, ref {ref[b, col]}); "
                        f"kv_total {c.n}, that head's spike at key {c.spike_pos[b, col // sp.hd]}; heads beyond tol: "
                        f"{int((err.reshape(sp.batch, sp.heads, -1).max(-1) > 1).sum())}")
        # the caches: bit-identical, but for the new generation slot of each (row, head), which holds the step's k / v bit for bit
        d = c.d
        for name in ("kc", "vc", "kg", "vg"):
            want = R.bf16_bits(getattr(c, name)).copy()
            if c.writes and name in ("kg", "vg"):
                cols = slice(d, 2 * d) if name == "kg" else slice(2 * d, 3 * d)
                want[:, :, c.n - 1 - sp.seq_len] = R.bf16_bits(c.qkv[:, cols]).reshape(sp.batch, sp.heads, sp.hd)
            assert np.array_equal(_bits(getattr(self, name)), want), f"{sp.name}: {name} changed outside the new slot (or the new slot is wrong)"
        return ratio


def _record(group, ratio):
    _WORST[group] = max(_WORST.get(group, 0.0), ratio)
    record_parity("shared_prompt_attention", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element, no floor",
                  prompt_keys=cases.PROMPT_KEYS, gen_keys=cases.GEN_KEYS, **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()})


# ---- a. the kernel alone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", cases.all_specs(), ids=lambda sp: sp.name)
def test_shared_prompt_attention_against_float64(sp):
    """err <= 1.0 tol on every element; NaN sentinels around `out` and `part` untouched; every range leaves its (max, sum), an empty one
    (-1e30, 0); the new generation slot equals the q|k|v row bit for bit and every other byte of both caches is unchanged — with
    n_gen = cap_g + 3 nothing is written at all.  Stale prompt slots, masked keys and generation slots beyond the count hold traps or NaN."""
    c, ref, A = _built(sp)
    L = Launch(c)
    assert L.launch() == 0, sp.name
    ratio = L.check(ref, A)
    print(f"[shared prompt attention] {sp.name}: {ratio:.3f} tol")
    _record(f"hd{sp.hd}", ratio)


def test_workspace_one_byte_short_launches_nothing():
    sp = next(s for s in cases.all_specs() if s.name == "gen-full-80")
    L = Launch(_built(sp)[0])
    assert L.launch(part_bytes=4 * L.nrec - 1) == -3
    torch.cuda.synchronize()
    assert (L.part.cpu().numpy() == SENT32).all() and (L.out.cpu().numpy() == SENT16).all()
    assert np.array_equal(_bits(L.kg), R.bf16_bits(L.c.kg))


# ---- b. capture ----------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_state_on_the_device():
    """One launch captured once; replayed at state[0] = 127, 128, 129 (the newest key crosses from the first generated range into the
    second) with that count's caches, ancestor table and q|k|v row in the same buffers, each against the float64 reference."""
    base = next(s for s in cases.all_specs() if s.name == "gen-full-80")
    steps = [replace(base, name=f"graph-{t}", n_gen=t) for t in (127, 128, 129)]
    built = [_built(sp) for sp in steps]
    L = Launch(built[0][0])
    assert L.launch() == 0  # (outside capture first: the library loads its kernels lazily)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert L.launch() == 0
    torch.cuda.current_stream().wait_stream(side)
    outs = []
    for c, ref, A in built:
        L.load(c)
        g.replay()
        ratio = L.check(ref, A)
        print(f"[shared prompt attention] {c.spec.name} (replayed): {ratio:.3f} tol")
        _record("replayed", ratio)
        outs.append(L.out.cpu().numpy().copy())
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


# ---- c. the step, context route ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lm_engine(cfg_name):
    """mid (weights that make the ids change from step to step), or the real OPT-2.7B / OPT-6.7B widths (hd 80 / 128, 32 heads) with two layers."""
    if cfg_name == "mid":
        return models("mid", "varied", seed=176)[2]
    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.statedict import state_dict_shapes
    from eilev_amd.synth import synth_param

    cfg = blip2_config(cfg_name[:5])
    cfg.text_config.num_hidden_layers = 2
    named = {k: torch.from_numpy(synth_param(k, shp, "fanin")).to(torch.bfloat16).cuda()
             for k, shp in state_dict_shapes(cfg).items() if k.startswith("language_model")}
    return HipEngine(cfg, named, device="cuda", parts=("opt",))


class _shared:
    """engine.shared_prompt_reads on for a block (the engines are shared with other tests)."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.was = self.eng.shared_prompt_reads
        self.eng.shared_prompt_reads = True

    def __exit__(self, *exc):
        self.eng.shared_prompt_reads = self.was


@pytest.mark.parametrize("cfg_name,P,n,R", [("mid", 70, 12, 3), ("mid", 70, 12, 32), ("opt27_2l", 300, 12, 3), ("opt27_2l", 300, 12, 32),
                                            ("opt67_2l", 300, 12, 3), ("opt67_2l", 300, 12, 32)])
def test_decode_after_context_equals_teacher_forcing(cfg_name, P, n, R):
    """test_hip_prefix.py's method with the switch on: 8 greedy tokens after extend_shared, eager with a trace; one existing-route prefill
    with all logits over [prefix | new | the generated ids] of every row: every step's logits within the decode-step bound of it, the
    emitted id the arg-max of the step's own logits, the captured run the same ids.  (The ids need not equal the switch-off route's: the
    two attentions round differently.)"""
    eng = _lm_engine(cfg_name)
    d = eng.dims
    D, T = d.t_hidden, 8
    g = torch.Generator().manual_seed(7 + R)
    prefix = (0.5 * torch.randn(1, P, D, generator=g)).to(torch.bfloat16).cuda()
    new = (0.5 * torch.randn(R, n, D, generator=g)).to(torch.bfloat16).cuda()
    ctx = eng.prefill_context(prefix)
    trace = []
    with _shared(eng):
        ids = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=False, trace=trace)
        assert eng.context_stats == dict(path="shared", rows=R, prefix=P, new=n, steps=T, reads="shared")
        captured = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=True)
        again = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=True)  # the cached graph, replayed
        assert eng.context_stats["reads"] == "shared"
    assert ids.shape == (R, T) and len(trace) == T
    gen = eng.embed_scatter(ids[:, :T - 1], None, None)
    full_emb = torch.cat((prefix.expand(R, -1, -1), new, gen), dim=1).contiguous()
    _, full, _ = eng.prefill(full_emb, torch.ones(R, P + n + T - 1, dtype=torch.int32, device="cuda"), all_logits=True, last_logits=False)
    torch.cuda.synchronize()
    worst = 0.0
    for k in range(T):
        step, ref = host(trace[k]), host(full[:, P + n - 1 + k])
        worst = max(worst, rel_rms(step, ref))
        assert np.array_equal(step[:, :d.vocab].argmax(-1), ids[:, k].cpu().numpy()), k
    print(f"[shared decode after context] {cfg_name} R={R}: worst step rel-rms {worst:.2e}")
    record_parity("shared_prompt_step", **{f"context_{cfg_name}_R{R}_worst_step_rel_rms": worst})
    assert worst <= STEP_BOUND
    assert torch.equal(captured, ids) and torch.equal(again, ids)
    # the switch is per call: off again, the record says nothing of reads and the cached shared graph is not reused
    plain = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=True)
    assert eng.context_stats == dict(path="shared", rows=R, prefix=P, new=n, steps=T) and plain.shape == ids.shape


def test_decode_after_context_in_two_parts():
    """33 rows on mid: 32 + 1, each part through the shared step; the ids are those of the parts run alone."""
    eng = _lm_engine("mid")
    P, n, R, T = 70, 12, 33, 8
    g = torch.Generator().manual_seed(40)
    prefix = (0.5 * torch.randn(1, P, eng.dims.t_hidden, generator=g)).to(torch.bfloat16).cuda()
    new = (0.5 * torch.randn(R, n, eng.dims.t_hidden, generator=g)).to(torch.bfloat16).cuda()
    ctx = eng.prefill_context(prefix)
    with _shared(eng):
        ids = eng.greedy_decode_context(ctx, new, T, eos_id=-1)
        assert eng.context_stats == dict(path="shared", rows=R, prefix=P, new=n, steps=T, reads="shared")
        head = eng.greedy_decode_context(ctx, new[:32].contiguous(), T, eos_id=-1)
        tail = eng.greedy_decode_context(ctx, new[32:].contiguous(), T, eos_id=-1)
    assert torch.equal(ids, torch.cat((head, tail)))


# ---- d. the step, beams --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb,use_graph", [("mid_v2", 3, True), ("mid_v1", 5, False)])
def test_beam_steps_teacher_forced(golden_dir, name, nb, use_graph):
    """test_hip_varied.py's tie-proof method with the switch on (2 samples x 3 beams with left-padded prompts of different lengths; 1 x 5):
    whatever the search decides, row r's logits are within the decode-step bound of the teacher-forced logits of the hypothesis in row r."""
    from test_hip_varied import load, prompt

    g, meta, px = load(golden_dir, name)
    cfg, oracle, eng = models(meta["config"], meta["weight_mode"], seed=meta["weight_seed"])
    emb, am = prompt(eng, g, px)
    B = emb.shape[0]
    if nb == 3:
        lens = g["attention_mask"].sum(1)
        assert B == 2 and lens[0] != lens[1] and (g["attention_mask"][:, 0] == 0).any()  # left padding, different lengths
    else:
        assert B == 1
    n = meta.get("beam_new_tokens", meta["new_tokens"])
    trace = []
    eng.beam_stats = None
    with _shared(eng):
        ids = eng.beam_decode(emb, am, n, nb, 1.0, eos_id=-1, use_graph=use_graph, trace=trace)
    assert eng.beam_stats == dict(rows=B * nb, beams=nb, prompt=emb.shape[1], reads="shared")
    R_ = B * nb
    assert ids.shape == (B, n) and len(trace) == n - 1
    emb_o = oracle.encode(px, g["input_ids"], g["video_input_mask"])
    hyp = [[] for _ in range(R_)]
    parents_used = set()
    worst = 0.0
    for t, (tok, src, lg) in enumerate(trace):
        tok, src = tok.cpu().numpy(), src.cpu().numpy()
        parents_used.update(int(src[r]) - (r // nb) * nb for r in range(R_))
        hyp = [hyp[int(src[r])] + [int(tok[r])] for r in range(R_)]
        cont = oracle.embed_scatter(np.asarray(hyp, np.int64), None, None)
        full = np.concatenate([np.repeat(emb_o, nb, axis=0), cont], axis=1)
        am_full = np.concatenate([np.repeat(g["attention_mask"], nb, axis=0), np.ones((R_, t + 1), np.int64)], axis=1)
        ref, _, _ = oracle.prefill(np.ascontiguousarray(full), am_full, all_logits=False)
        got = host(lg)
        for r in range(R_):
            e = rel_rms(got[r], ref[r])
            worst = max(worst, e)
            assert e <= STEP_BOUND, (t, r, e)
    assert len(parents_used) >= 2  # the search really re-parented rows
    record_parity("shared_prompt_step", **{f"beam_{name}_x{nb}_teacher_forced_rel_rms_max": worst})
    eng.beam_decode(emb, am, 3, nb, 1.0, eos_id=-1, use_graph=False, trace=[])
    assert eng.beam_stats["reads"] == "per_row"


# ---- e. generate ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid_v1", "mid_b1"])
def test_generate_after_context_with_shared_reads(golden_dir, name):
    """generate(context=ctx, shared_prompt_reads=True) on the golden prompt split at a clip boundary.  mid_v1: oracle.parity's
    greedy_ids_vs_reference with its defaults says ok.  mid_b1 has no per-step logits to judge a flip by: ids_equal_reference is recorded."""
    from oracle.parity import greedy_ids_vs_reference
    from test_hip_prefix import SPLIT, _build_model

    g, meta, px = load_case(golden_dir, name)
    m = _build_model(meta)
    t = lambda a: torch.from_numpy(a).cuda()
    ids, vm = t(g["input_ids"]), t(g["video_input_mask"])
    n_new = meta["new_tokens"]
    ctx = m.encode_context(ids[:, :SPLIT], pixel_values=t(px[:2]), video_input_mask=vm[:, :SPLIT])
    kw = dict(max_new_tokens=n_new, min_new_tokens=None, eos_token_id=meta.get("never_id", 511))
    out = m.generate(ids[:, SPLIT:], pixel_values=t(px[2:]), video_input_mask=vm[:, SPLIT:], context=ctx, shared_prompt_reads=True, **kw)
    eng = m.engine()
    assert eng.context_stats == dict(path="shared", rows=1, prefix=SPLIT, new=ids.shape[1] - SPLIT, steps=n_new, reads="shared")
    assert eng.shared_prompt_reads is False  # restored after the call
    got = out.cpu().numpy()
    record_parity(f"generate_context_shared_reads[{name}]", ids_equal_reference=float(np.array_equal(got, g["fp32_greedy_free"])))
    if name == "mid_v1":
        verdict = greedy_ids_vs_reference(got, g)
        assert verdict["ok"], verdict
    # beams through the model class: served, and the record says which reads ran
    eng.beam_stats = None
    beams = m.generate(ids, pixel_values=t(px), video_input_mask=vm, num_beams=3, max_new_tokens=4, eos_token_id=meta.get("never_id", 511),
                       shared_prompt_reads=True)
    assert beams.shape[0] == 1 and eng.beam_stats["reads"] == "shared" and eng.shared_prompt_reads is False
