"""-m gpu: sampling on the device (libeilev_hip_sample.so, include/eilev_sample.h; HipEngine.sample_decode_device / t5_sample_device;
generate(do_sample=True)).

The kernel is pinned to its float64 restatement (eilev_amd/sampling.py: keep_bounds, draw_ok, sample_select_reference); the engine paths
to greedy search (top_k = 1), to themselves (seed, graph vs eager) and to a replay of their own step logits through the restatement.

The tolerance.  The rule is tol = 2 x (longest sequential chain + tree depth of the kernel's sums) x 2^-24, at most 1e-5.  The
kernel's sums have no rounding at all: every probability is floor(expf(x - max) * 2^40) and the sums are 64-bit integers, so the
"chain" is the roundings that ONE weight carries, as a multiple of the half-ulp 2^-24 relative to the row's total mass:
  - x - max is rounded to fp32: a relative error of d * 2^-24 on exp(-d), d = max - x; summed over the row with the probabilities as
    weights this is E_p[d] * 2^-24, and E_p[d] = H(p) - log(sum exp(-d)) <= H(p) <= ln(65536) = 11.1;
  - expf is good to 1 ulp = 2 half-ulps;
  - the 2^-40 quantisation of <= 65536 weights, against a total >= 2^40 (the maximum's weight): <= 2^-24, 1 half-ulp.
11.1 + 2 + 1 < 16 roundings, so tol = 2 x 16 x 2^-24 = 1.9e-6 (the factor 2: a mass is a quotient of two such sums)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from eilev_amd import abi
from eilev_amd.sampling import SampleSpec, draw_ok, keep_bounds, processed_scores, row_history, sample_select_reference
from hip_utils import P, load_case, models, stream_ptr

pytestmark = pytest.mark.gpu

TOL = 2 * 16 * 2.0 ** -24
assert TOL <= 1e-5
SETTINGS = [(1.0, 50, 1.0), (0.7, 0, 0.9), (1.5, 3, 1.0), (1.0, 0, 1.0), (0.7, 50, 0.9)]  # (temperature, top_k, top_p)


@functools.lru_cache(maxsize=None)
def _logits(rows, vocab):
    g = torch.Generator().manual_seed(1000 * rows + vocab)
    return torch.randn((rows, vocab), generator=g) * 3


def _select(logits, uniforms, state, finished, tokens, out, spec: SampleSpec, step_offset=0, finalize=1, want_warped=True):
    """One eilev_sample_select call on device copies of the host buffers -> (rc, dict of host results)."""
    smp = abi.load_sample()
    R, V = logits.shape
    max_new = out.shape[1]
    dv = lambda a, dt: torch.as_tensor(a).to(dt).cuda().contiguous()
    lg, un = dv(logits, torch.float32), dv(uniforms, torch.float32)
    st, fin, tok, o = dv(state, torch.int32), dv(finished, torch.uint8), dv(tokens, torch.int64), dv(out, torch.int64)
    warped = torch.full((R, V), float("nan"), dtype=torch.float32, device="cuda") if want_warped else None
    scratch = torch.empty(max(16, int(smp.eilev_sample_scratch_bytes(R, V))), dtype=torch.uint8, device="cuda")
    prm = abi.sample_params(spec.temperature, spec.top_k, spec.top_p, spec.repetition_penalty, spec.min_new, max_new, spec.eos, spec.pad_id,
                            spec.prefix_id, step_offset, finalize)
    rc = smp.eilev_sample_select(C.byref(prm), P(lg), R, V, P(un), P(st), P(fin), P(tok), P(o), P(warped), P(scratch), scratch.numel(), stream_ptr())
    torch.cuda.synchronize()
    return rc, dict(warped=None if warped is None else warped.cpu(), state=st.cpu().tolist(), finished=fin.cpu(), tokens=tok.cpu(), out=o.cpu())


def _check_call(logits, uniforms, state, finished, tokens, out, spec, step_offset=0, finalize=1):
    """Every check of one call against the restatement; returns the kernel's results."""
    rc, got = _select(logits, uniforms, state, finished, tokens, out, spec, step_offset, finalize)
    assert rc == 0, rc
    R, V = logits.shape
    max_new = out.shape[1]
    step = int(state[0]) + step_offset
    fin0 = torch.as_tensor(finished).bool()
    hist = row_history(torch.as_tensor(out), step, spec.prefix_id)
    scores = processed_scores(logits, hist, spec, step)
    must, may = keep_bounds(logits, hist, spec, TOL, step)
    kept = torch.isfinite(got["warped"])
    # the kept set: everything that must stay is finite, everything that may not stay is -inf; what stays keeps its processed value
    assert not bool((must & ~kept).any()), int((must & ~kept).sum())
    assert not bool((kept & ~may).any()), int((kept & ~may).sum())
    assert bool((got["warped"][~kept] == float("-inf")).all())
    assert torch.equal(got["warped"][kept], scores[kept])
    band = (may & ~must).sum(dim=1)
    assert int(band.max()) <= 2, band.tolist()  # the band cannot hide a wrong threshold
    if spec.top_p >= 1.0:
        assert torch.equal(must, may)  # the top-k tie rule is exact
    # the draw, over the set the kernel kept
    u = torch.as_tensor(uniforms)[step]
    ok = draw_ok(kept, scores, u, got["tokens"], TOL)
    assert bool(ok[~fin0].all()), (ok.tolist(), got["tokens"].tolist())
    # bookkeeping, exact
    pad = torch.full((R,), int(spec.pad_id), dtype=torch.int64)
    assert torch.equal(got["tokens"][fin0], pad[fin0])
    want_out = torch.as_tensor(out).long().clone()
    want_out[:, step] = got["tokens"]
    assert torch.equal(got["out"], want_out)
    eos = torch.zeros(R, dtype=torch.bool)
    for e in spec.eos:
        eos |= got["tokens"] == int(e)
    fin1 = fin0 | eos
    assert torch.equal(got["finished"].bool(), fin1)
    assert got["state"] == [step + 1 if finalize else int(state[0]), int(bool((~fin1).any()))]
    # and the float64 restatement agrees wherever its own draw is not within tol of an edge of the kernel's interval
    ref = sample_select_reference(logits, uniforms, state, finished, tokens, out, spec, step_offset, finalize)
    same_set = (torch.isfinite(ref["scores"]) == kept).all(dim=1)
    diff = (ref["tokens"] != got["tokens"]) & same_set
    assert int(diff.sum()) <= 1, (ref["tokens"].tolist(), got["tokens"].tolist())
    return got


def _fresh(rows, max_new, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((max_new, rows), generator=g), [0, 1], torch.zeros(rows, dtype=torch.uint8), torch.zeros(rows, dtype=torch.int64),
            torch.full((rows, max_new), -7, dtype=torch.int64))


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
@pytest.mark.parametrize("vocab", [1000, 32128, 50272])
@pytest.mark.parametrize("rows", [1, 7, 32])
def test_kernel_equals_the_restatement(rows, vocab, setting):
    T, k, p = setting
    uni, state, fin, tok, out = _fresh(rows, 4, seed=rows + vocab)
    _check_call(_logits(rows, vocab), uni, state, fin, tok, out, SampleSpec(T, k, p))


def test_repetition_penalty_history_with_duplicates_and_the_prefix():
    rows, vocab, max_new = 7, 32128, 6
    logits = _logits(rows, vocab)
    uni, _, fin, tok, out = _fresh(rows, max_new, seed=5)
    top = logits.topk(3, dim=1).indices  # penalise what would otherwise be drawn: ids of both signs, one of them twice
    low = logits.argmin(dim=1)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = top[:, 0], low, top[:, 0], top[:, 2]
    _check_call(logits, uni, [4, 1], fin, tok, out, SampleSpec(0.7, 50, 0.9, repetition_penalty=1.5, prefix_id=int(top[0, 1])))
    spec = SampleSpec(0.7, 0, 1.0, repetition_penalty=1.5, prefix_id=int(top[0, 1]))  # nothing removed: every penalised score is visible
    w = _check_call(logits, uni, [4, 1], fin, tok, out, spec)["warped"]
    hist = row_history(out, 4, spec.prefix_id)
    assert all(len(h) == 5 and len(set(h)) < 5 for h in hist)
    for b in range(rows):  # once per distinct id, from the unpenalised value
        for i in set(hist[b]):
            x = logits[b, i]
            assert w[b, i] == (x * torch.tensor(1.5) if x < 0 else x / torch.tensor(1.5)) / torch.tensor(0.7), (b, i)
    assert bool((w[:, low[0]] < 0).any()) and bool((w[torch.arange(rows), top[:, 0]] > 0).all())  # both signs


@pytest.mark.parametrize("step,banned", [(1, True), (2, False)])
def test_min_new_bans_the_eos_ids_below_it(step, banned):
    rows, vocab, max_new = 7, 1000, 4
    logits = _logits(rows, vocab).clone()
    eos = (17, 500)
    logits[:, 17] = 40.0  # would be drawn with certainty
    uni, _, fin, tok, out = _fresh(rows, max_new, seed=9)
    out[:, :step] = 3
    got = _check_call(logits, uni, [step, 1], fin, tok, out, SampleSpec(1.0, 0, 1.0, min_new=2, eos=eos, pad_id=1))
    assert bool((got["tokens"] == 17).all()) != banned
    assert bool(torch.isfinite(got["warped"][:, [17, 500]]).any()) != banned
    assert got["state"][1] == (1 if banned else 0)


def test_finished_rows_pad_and_a_drawn_eos_finishes_its_row():
    rows, vocab, max_new = 7, 1000, 4
    logits = _logits(rows, vocab).clone()
    logits[1, 11] = 40.0  # row 1 draws the first EOS id, row 4 the second
    logits[4, 900] = 40.0
    uni, _, _, tok, out = _fresh(rows, max_new, seed=11)
    fin = torch.tensor([0, 0, 1, 0, 0, 1, 0], dtype=torch.uint8)
    got = _check_call(logits, uni, [1, 1], fin, tok, out, SampleSpec(1.0, 50, 1.0, eos=(11, 900), pad_id=1))
    assert got["tokens"][[2, 5]].tolist() == [1, 1] and got["tokens"][[1, 4]].tolist() == [11, 900]
    assert got["finished"].tolist() == [0, 1, 1, 0, 1, 1, 0] and got["state"] == [2, 1]
    # every row finished: state[1] = 0 (one row and several rows take different code paths)
    for r in (1, 7):
        lg = _logits(r, vocab).clone()
        lg[:, 11] = 40.0
        uni, _, fin, tok, out = _fresh(r, max_new, seed=12)
        assert _check_call(lg, uni, [0, 1], fin, tok, out, SampleSpec(1.0, 50, 1.0, eos=(11, 900), pad_id=1))["state"] == [1, 0]


@pytest.mark.parametrize("rows", [1, 7])
def test_step_offset_and_finalize(rows):
    vocab, max_new = 1000, 4
    logits = _logits(rows, vocab)
    uni, _, fin, tok, out = _fresh(rows, max_new, seed=13)
    spec = SampleSpec(0.7, 50, 0.9)
    a = _check_call(logits, uni, [2, 1], fin, tok, out, spec, step_offset=0, finalize=1)
    b = _check_call(logits, uni, [3, 1], fin, tok, out, spec, step_offset=-1, finalize=0)  # after a decode step that advanced state[0]
    assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["out"], b["out"])
    assert a["state"] == [3, 1] and b["state"] == [3, 1]


@pytest.mark.parametrize("vocab", [1000, 50272])
@pytest.mark.parametrize("rows", [1, 7])
def test_sample_select_and_rules_select_share_their_steps(rows, vocab):
    """The steps the two kernels share (csrc/row_select.h: tables, rules on the row, commit of the token, finalize), pinned to each other:
    sampling with top_k = 1, top_p = 1, temperature = 1 and u = 0 draws the arg-max after the rules, which is what eilev_rules_select
    with no n-gram ban takes.  tokens, out_tokens, finished and state must be equal."""
    rl = abi.load_rules()
    max_new, min_new, pen, pad = 12, 7, 1.5, 1
    logits = _logits(rows, vocab)
    top = logits.topk(3, dim=1).indices
    best, second = top[:, 0], top[:, 1]
    low = logits.argmin(dim=1)
    out = torch.full((rows, max_new), -7, dtype=torch.int64)  # duplicates, ids of both signs, one id outside the vocabulary
    hist = (best, torch.full_like(best, 3), second, best, torch.full_like(best, vocab + 5), torch.full_like(best, 3), low, second)
    out[:, :len(hist)] = torch.stack(hist, dim=1)
    prefix = int(top[0, 2])
    free = SampleSpec(1.0, 1, 1.0, repetition_penalty=pen, pad_id=pad, prefix_id=prefix)
    # the first EOS id is row 0's arg-max after the penalty: banned below min_new (another id wins), taken above it (the row finishes)
    eos = (int(processed_scores(logits, row_history(out, min_new, prefix), free, min_new)[0].argmax()), 5)
    spec = SampleSpec(1.0, 1, 1.0, repetition_penalty=pen, min_new=min_new, eos=eos, pad_id=pad, prefix_id=prefix)
    uni = torch.zeros((max_new, rows))
    fins = [torch.zeros(rows, dtype=torch.uint8)]
    fins[0][rows // 2] = 1  # one row has finished (rows = 1: that row, and the call with it unfinished as well)
    if rows == 1:
        fins.append(torch.zeros(rows, dtype=torch.uint8))
    # (state[0], step_offset, finalize): step 5 is below min_new, step 7 is not
    for state0, step_offset, finalize in ((5, 0, 1), (8, -1, 0)):
        step = state0 + step_offset
        scores = processed_scores(logits, row_history(out, step, prefix), spec, step)
        top2 = scores.topk(2, dim=1).values
        assert bool((top2[:, 0] > top2[:, 1]).all())  # the arg-max after the rules is unique: both kernels must find it
        for fin in fins:
            tok = torch.zeros(rows, dtype=torch.int64)
            rc, got = _select(logits, uni, [state0, 1], fin, tok, out, spec, step_offset, finalize, want_warped=False)
            assert rc == 0, rc
            dv = lambda a, dt: torch.as_tensor(a).to(dt).cuda().contiguous()
            lg, st, f, t, o = dv(logits, torch.float32), dv([state0, 1], torch.int32), dv(fin, torch.uint8), dv(tok, torch.int64), dv(out, torch.int64)
            prm = abi.rules_params(pen, 0, min_new, max_new, eos, pad, prefix, step_offset, finalize)
            rc = rl.eilev_rules_select(C.byref(prm), P(lg), rows, vocab, P(st), P(f), P(t), P(o), None, None, 0, stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, rc
            assert torch.equal(got["tokens"], t.cpu()) and torch.equal(got["out"], o.cpu())
            assert torch.equal(got["finished"], f.cpu()) and got["state"] == st.cpu().tolist()
            live = ~fin.bool()
            assert torch.equal(got["tokens"][live], scores.argmax(dim=1)[live]) and bool((got["tokens"][~live] == pad).all())
            if live[0]:
                assert (int(got["tokens"][0]) == eos[0]) == (step >= min_new) and int(got["finished"][0]) == int(step >= min_new)


def test_grid_uniforms_give_the_distribution():
    """4096 draws of ONE row as 128 calls of 32 rows with u_j = (j + 0.5) / 4096: every id is drawn 4096 p_i times, +-1."""
    vocab, calls, R = 1000, 128, 32
    smp = abi.load_sample()
    row = _logits(1, vocab)
    spec = SampleSpec(0.7, 50, 0.9)
    lg = row.expand(R, vocab).contiguous().cuda()
    uni = ((torch.arange(calls * R, dtype=torch.float64) + 0.5) / (calls * R)).float().view(calls, R).cuda()
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    fin = torch.zeros(R, dtype=torch.uint8, device="cuda")
    tok = torch.zeros(R, dtype=torch.int64, device="cuda")
    out = torch.full((R, calls), -1, dtype=torch.int64, device="cuda")
    warped = torch.empty((R, vocab), dtype=torch.float32, device="cuda")
    prm = abi.sample_params(spec.temperature, spec.top_k, spec.top_p, max_new=calls)
    for _ in range(calls):  # finalize = 1: the kernel advances the step itself
        abi.check(smp.eilev_sample_select(C.byref(prm), P(lg), R, vocab, P(uni), P(state), P(fin), P(tok), P(out), P(warped), None, 0, stream_ptr()),
                  "eilev_sample_select")
    torch.cuda.synchronize()
    assert state.tolist() == [calls, 1]
    w = warped[0].double().cpu()
    must, may = keep_bounds(row, None, spec, TOL)
    kept = torch.isfinite(w)
    assert not bool((must[0] & ~kept).any()) and not bool((kept & ~may[0]).any())
    prob = torch.where(kept, torch.exp(w - w.max()), torch.zeros_like(w))
    prob = prob / prob.sum()
    counts = torch.bincount(out.cpu().flatten(), minlength=vocab).double()
    assert int(counts.sum()) == calls * R
    assert float((counts - calls * R * prob).abs().max()) <= 1.0


def test_unsupported_vocabulary_goes_to_the_host_loop():
    uni, state, fin, tok, out = _fresh(2, 4)
    rc, _ = _select(torch.randn(2, 1002), uni, state, fin, tok, out, SampleSpec(), want_warped=False)
    assert rc == -2  # EILEV_E_UNSUPPORTED
    _, _, eng = models("mid")
    sampler = dict(temperature=1.0, top_k=50, top_p=1.0, generator=None)
    from eilev_amd.route import Caps, plan_decode

    dev_kw = lambda vocab, eos_id: plan_decode(Caps.of(eng)._replace(vocab=vocab), 1, sampler, None, eos_id, 0, 8, False).dev_kw
    assert dev_kw(1002, -1) is None
    assert dev_kw(1000, -1) is not None
    assert dev_kw(1000, list(range(9))) is None  # more than 8 EOS ids


def test_engine_reports_the_host_path_for_an_unsupported_vocabulary(monkeypatch):
    """End to end: the engine asks abi.sample_supported(vocab); with the answer that vocab = 1002 gets, a sampling call runs the host loop
    (with the penalty as transformers' processor) and says so."""
    eng, emb, am = _opt_prompt()
    real = abi.sample_supported
    assert not real(1002)
    monkeypatch.setattr(abi, "sample_supported", lambda vocab: real(1002))
    ids = eng.sample_decode(emb, am, 4, eos_id=-1, top_k=1, repetition_penalty=1.5)
    assert eng.sample_stats == dict(path="host", steps=4) and ids.shape == (3, 4)
    with pytest.raises(NotImplementedError):
        eng.sample_decode_device(emb, am, 4, eos_id=-1)
    monkeypatch.undo()
    dev = eng.sample_decode(emb, am, 4, eos_id=-1, top_k=1, repetition_penalty=1.5)
    assert eng.sample_stats == dict(path="device", steps=4) and torch.equal(dev, ids)  # top_k = 1: both paths take the penalised arg-max


# ---- the OPT engine ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _opt_prompt():
    from eilev_amd.synth import synth_interleaved_ids, synth_pixels

    cfg, _, eng = models("mid")
    nq, vocab = cfg.num_query_tokens, cfg.text_config.vocab_size
    ids, vm = zip(*[synth_interleaved_ids([1, 1], [5, 4], nq, vocab, seed=11 + s) for s in range(3)])
    px = torch.from_numpy(synth_pixels(6, 2, cfg.vision_config.image_size)).cuda()
    ids, vm = torch.from_numpy(np.stack(ids)).cuda(), torch.from_numpy(np.stack(vm)).cuda()
    return eng, eng.embed_scatter(ids, vm, eng.encode_clips(px)), torch.ones_like(ids, dtype=torch.int32)


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _replay(trace, uniforms, spec: SampleSpec, ids, max_new):
    """The engine's step logits through the restatement, teacher-forced with the engine's ids: every id is a valid draw."""
    R = trace[0].shape[0]
    fin = torch.zeros(R, dtype=torch.uint8)
    out = torch.full((R, max_new), int(spec.pad_id), dtype=torch.int64)
    for t, lg in enumerate(trace[:ids.shape[1]]):
        hist = row_history(out, t, spec.prefix_id)
        scores = processed_scores(lg.cpu(), hist, spec, t)
        must, may = keep_bounds(lg.cpu(), hist, spec, TOL, t)
        live = ~fin.bool()
        # any kept set between must and may is the kernel's right: the draw must be valid for one of the two extremes' neighbours; the
        # band holds at most 2 tokens, so check against `may` and `must` and accept either
        ok = draw_ok(may, scores, uniforms[t].cpu(), ids[:, t].cpu(), TOL) | draw_ok(must, scores, uniforms[t].cpu(), ids[:, t].cpu(), TOL)
        assert bool(ok[live].all()), (t, ids[:, t].tolist())
        out[:, t] = torch.where(live, ids[:, t].cpu(), out[:, t])  # teacher forcing; finished rows keep the pad id
        assert torch.equal(out[:, t], ids[:, t].cpu())
        for e in spec.eos:
            fin = fin | ((ids[:, t].cpu() == int(e)) & live).to(torch.uint8)


def test_opt_top1_is_greedy_seed_reproduces_graph_equals_eager():
    eng, emb, am = _opt_prompt()
    greedy = eng.greedy_decode(emb, am, 8, eos_id=-1, use_graph=True)
    assert torch.equal(eng.sample_decode(emb, am, 8, eos_id=-1, top_k=1), greedy)
    assert eng.sample_stats == dict(path="device", steps=8)
    a = eng.sample_decode(emb, am, 8, eos_id=-1, temperature=1.5, top_k=3, generator=_gen(123))
    b = eng.sample_decode(emb, am, 8, eos_id=-1, temperature=1.5, top_k=3, generator=_gen(123))
    c = eng.sample_decode_device(emb, am, 8, eos_id=-1, temperature=1.5, top_k=3, generator=_gen(123), use_graph=False)
    assert torch.equal(a, b) and torch.equal(a, c) and a.shape == (3, 8) and not torch.equal(a, greedy)
    assert eng.sample_stats["path"] == "device"
    eng.device_sampling = False
    try:
        h = eng.sample_decode(emb, am, 8, eos_id=-1, top_k=1)
        assert eng.sample_stats == dict(path="host", steps=8) and h.shape == (3, 8)
    finally:
        eng.device_sampling = True


def test_opt_trace_replays_through_the_restatement():
    eng, emb, am = _opt_prompt()
    spec = SampleSpec(0.7, 0, 0.9, repetition_penalty=1.5, min_new=2, eos=(5, 9), pad_id=1)
    uni = torch.rand((8, 3), generator=torch.Generator().manual_seed(7))
    trace = []
    ids = eng.sample_decode_device(emb, am, 8, eos_id=list(spec.eos), pad_id=1, temperature=0.7, top_k=0, top_p=0.9, repetition_penalty=1.5,
                                   min_new_tokens=2, use_graph=False, trace=trace, uniforms=uni)
    assert len(trace) >= ids.shape[1] and trace[0].shape == (3, eng.dims.vocab)
    _replay(trace, uni, spec, ids, 8)
    graph = eng.sample_decode_device(emb, am, 8, eos_id=list(spec.eos), pad_id=1, temperature=0.7, top_k=0, top_p=0.9, repetition_penalty=1.5,
                                     min_new_tokens=2, uniforms=uni)
    assert torch.equal(graph, ids)


def test_opt_eos_ends_early_and_finished_rows_pad():
    eng, emb, am = _opt_prompt()
    free = eng.sample_decode(emb, am, 12, eos_id=-1, temperature=1.5, top_k=3, generator=_gen(5))
    eos = int(free[0, 2])  # row 0 reaches it at its third token at the latest
    ids = eng.sample_decode(emb, am, 12, eos_id=eos, pad_id=1, temperature=1.5, top_k=3, generator=_gen(5))
    hit = (ids == eos)
    assert bool(hit[0].any()) and int(hit[0].float().argmax()) <= 2
    for b in range(3):
        n = int(hit[b].float().argmax()) + 1 if bool(hit[b].any()) else ids.shape[1]
        assert torch.equal(ids[b, :n], free[b, :n]) and bool((ids[b, n:] == 1).all())
    every = eng.sample_decode(emb, am, 12, eos_id=[int(t) for t in free[:, 1].tolist()] + [int(free[0, 0])], pad_id=1, temperature=1.5, top_k=3,
                              generator=_gen(5))
    assert every.shape[1] <= 2 and eng.sample_stats["steps"] == every.shape[1]  # every row has stopped by its second token: the call ends there


def test_opt_more_than_32_rows_run_in_chunks_of_32():
    eng, emb, am = _opt_prompt()
    big, big_am = emb.repeat(11, 1, 1), am.repeat(11, 1)  # 33 rows
    uni = torch.rand((4, 33), generator=torch.Generator().manual_seed(21))
    kw = dict(eos_id=-1, temperature=1.5, top_k=3)
    ids = eng.sample_decode_device(big, big_am, 4, uniforms=uni, **kw)
    assert ids.shape == (33, 4) and eng.sample_stats == dict(path="device", steps=4)
    assert torch.equal(ids[:32], eng.sample_decode_device(big[:32], big_am[:32], 4, uniforms=uni[:, :32], **kw))
    assert torch.equal(ids[32:], eng.sample_decode_device(big[32:], big_am[32:], 4, uniforms=uni[:, 32:], **kw))


# ---- flan-t5 -----------------------------------------------------------------------------------------------------------------------
def _t5_case(golden_dir, name):
    g, meta, px = load_case(golden_dir, name)
    _, _, eng = models(meta["config"])
    t = lambda a: torch.from_numpy(a).cuda()
    return eng, eng.embed_scatter(t(g["input_ids"]), t(g["video_input_mask"]), eng.encode_clips(t(px))), t(g["attention_mask"])


@pytest.mark.parametrize("name", ["mid_t5_b1", "tiny_t5_b2"])
def test_t5_top1_is_t5_greedy_and_the_penalty_sees_the_start_token(golden_dir, name):
    eng, emb, am = _t5_case(golden_dir, name)
    R = emb.shape[0]
    greedy = eng.t5_greedy(emb, am, 6, eos_id=-1)
    a = eng.t5_sample(emb, am, 6, eos_id=-1, top_k=1)
    assert torch.equal(a, greedy) and int(a[0, 0]) == 0 and a.shape == (R, 7)
    assert eng.sample_stats == dict(path="device", steps=6)
    spec = SampleSpec(1.0, 0, 1.0, repetition_penalty=1.5, prefix_id=0, pad_id=0)
    uni = torch.rand((6, R), generator=torch.Generator().manual_seed(3))
    trace = []
    ids = eng.t5_sample_device(emb, am, 6, eos_id=-1, start_id=0, top_k=0, repetition_penalty=1.5, use_graph=False, trace=trace, uniforms=uni)
    assert bool((ids[:, 0] == 0).all()) and len(trace) == 6
    _replay(trace, uni, spec, ids[:, 1:], 6)
    assert torch.equal(eng.t5_sample_device(emb, am, 6, eos_id=-1, start_id=0, top_k=0, repetition_penalty=1.5, uniforms=uni), ids)


@pytest.mark.parametrize("name", ["mid_t5_b1", "tiny_t5_b2"])
def test_t5_engine_penalises_the_start_token(golden_dir, name):
    """The first draw of t5_sample_device with a uniform chosen where the start token's penalty decides the id: from the engine's own first
    logits, the restatement draws with and without the start id in the history over a grid of uniforms; the engine is then run on a
    uniform at which the two differ (and whose grid neighbours agree with it: far from every CDF edge)."""
    eng, emb, am = _t5_case(golden_dir, name)
    R, G, pen = emb.shape[0], 16384, 8.0
    trace = []
    eng.t5_sample_device(emb, am, 1, eos_id=-1, start_id=0, top_k=0, uniforms=torch.zeros((1, R)), trace=trace)
    lg = trace[0].cpu()
    grid = ((torch.arange(G, dtype=torch.float64) + 0.5) / G).float()
    u, want, other = torch.zeros((1, R)), torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.int64)
    for b in range(R):
        draws = []
        for prefix in (0, -1):
            ref = sample_select_reference(lg[b:b + 1].expand(G, -1), grid.view(1, G), [0, 1], torch.zeros(G), torch.zeros(G), torch.zeros((G, 1)),
                                          SampleSpec(1.0, 0, 1.0, repetition_penalty=pen, prefix_id=prefix))
            draws.append(ref["drawn"])
        w, wo = draws
        calm = lambda d: (d[1:-1] == d[:-2]) & (d[1:-1] == d[2:])
        pick = torch.nonzero((w[1:-1] != wo[1:-1]) & calm(w) & calm(wo)).flatten()
        assert pick.numel() > 0, f"row {b}: the start token's penalty never decides a draw on this grid"
        j = int(pick[pick.numel() // 2]) + 1
        u[0, b], want[b], other[b] = grid[j], w[j], wo[j]
    ids = eng.t5_sample_device(emb, am, 1, eos_id=-1, start_id=0, top_k=0, repetition_penalty=pen, uniforms=u)
    assert torch.equal(ids[:, 1].cpu(), want) and not bool((ids[:, 1].cpu() == other).any())


def test_t5_more_than_32_rows_keep_the_penalty_on_both_paths(golden_dir):
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor

    eng, emb, am = _t5_case(golden_dir, "tiny_t5_b2")
    big, big_am = emb.repeat(17, 1, 1)[:33], am.repeat(17, 1)[:33]
    kw = dict(eos_id=-1, top_k=0, repetition_penalty=4.0)
    # the device path: chunks of 32 on slices of the same uniforms; a 32-row call is what the replay test above pins to the restatement
    uni = torch.rand((5, 33), generator=torch.Generator().manual_seed(31))
    ids = eng.t5_sample_device(big, big_am, 5, uniforms=uni, **kw)
    assert ids.shape == (33, 6) and eng.sample_stats == dict(path="device", steps=5)
    assert torch.equal(ids[:32], eng.t5_sample_device(big[:32], big_am[:32], 5, uniforms=uni[:, :32], **kw))
    assert torch.equal(ids[32:], eng.t5_sample_device(big[32:], big_am[32:], 5, uniforms=uni[:, 32:], **kw))
    assert not torch.equal(ids, eng.t5_sample_device(big, big_am, 5, uniforms=uni, eos_id=-1, top_k=0))  # the penalty moves draws
    pub = eng.t5_sample(big, big_am, 5, generator=_gen(9), **kw)
    assert eng.sample_stats["path"] == "device"
    assert torch.equal(pub, eng.t5_sample_device(big, big_am, 5, uniforms=torch.rand((5, 33), generator=_gen(9), device="cuda"), **kw))
    # the host loop: the numeric penalty becomes transformers' processor again, with the start token in front
    eng.device_sampling = False
    try:
        host = eng.t5_sample(big, big_am, 5, generator=_gen(9), **kw)
        assert eng.sample_stats == dict(path="host", steps=5)
    finally:
        eng.device_sampling = True
    rules = dict(processors=LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=4.0)]), stopping=None,
                 prefix=torch.zeros((33, 1), dtype=torch.int64, device="cuda"))
    explicit = eng.t5_beam(big, big_am, 5, 1, eos_id=-1, sampler=dict(temperature=1.0, top_k=0, top_p=1.0, generator=_gen(9)), rules=rules)
    plain = eng.t5_beam(big, big_am, 5, 1, eos_id=-1, sampler=dict(temperature=1.0, top_k=0, top_p=1.0, generator=_gen(9)), rules=None)
    assert torch.equal(host, explicit) and not torch.equal(host, plain)


# ---- the model API --------------------------------------------------------------------------------------------------------------------
def _model(config_name):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration
    from eilev_amd.synth import synth_interleaved_ids, synth_pixels

    torch.manual_seed(0)
    cfg = blip2_config(config_name)
    model = VideoBlipForConditionalGeneration(cfg).to(torch.bfloat16).cuda().eval()
    nq, vocab = cfg.num_query_tokens, cfg.text_config.vocab_size
    ids, vm = zip(*[synth_interleaved_ids([1, 1], [5, 4], nq, vocab, seed=3 + s) for s in range(2)])
    px = torch.from_numpy(synth_pixels(4, 2, cfg.vision_config.image_size)).cuda()
    return model, dict(input_ids=torch.from_numpy(np.stack(ids)).cuda(), pixel_values=px, video_input_mask=torch.from_numpy(np.stack(vm)).cuda())


@pytest.mark.parametrize("config_name", ["tiny", "tiny_t5"])
def test_generate_routes_sampling_to_the_device(config_name):
    from transformers import LogitsProcessorList, TemperatureLogitsWarper

    model, kw = _model(config_name)
    is_t5 = config_name.endswith("t5")
    demo = dict(do_sample=True, temperature=0.7, top_p=0.9, repetition_penalty=1.5, min_new_tokens=2, max_new_tokens=5, eos_token_id=None)
    out = model.generate(**kw, **demo)
    eng = model.engine()
    assert eng.sample_stats["path"] == "device"
    assert out.shape == (2, 5 + is_t5) and int(out.min()) >= 0 and int(out.max()) < model.config.text_config.vocab_size
    rep = model.generate(**kw, **demo, num_return_sequences=2, top_k=1)  # rows of one prompt adjacent (top_k = 1: equal rows)
    assert rep.shape == (4, 5 + is_t5) and torch.equal(rep[0], rep[1]) and torch.equal(rep[2], rep[3])
    assert eng.sample_stats["path"] == "device"
    eng.sample_stats = None
    model.generate(**kw, **demo, logits_processor=LogitsProcessorList([TemperatureLogitsWarper(0.9)]))
    assert eng.sample_stats["path"] == "host"
    eng.sample_stats = None
    model.generate(**kw, **demo, num_beams=2)
    assert eng.sample_stats["path"] == "host"  # beam-search sampling stays in the host beam loop
    eng.device_sampling = False
    try:
        host = model.generate(**kw, **demo)
        assert eng.sample_stats["path"] == "host" and host.shape == out.shape
    finally:
        eng.device_sampling = True
