"""-m gpu: the logits rules of greedy and beam search on the device (libeilev_hip_rules.so, include/eilev_rules.h;
HipEngine.rules_decode_device / t5_rules_device / the rules' top-k inside beam_decode / eilev_rules_ban in front of the draw;
generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, eos_token_id=[..])).

The kernels are pinned to their CPU restatement (eilev_amd/rules.py, itself pinned to transformers in tests/test_rules_ref.py):
eilev_rules_select and eilev_rules_ban bit for bit (the same fp32 operations), eilev_rules_topk_logprob to the rounding of its log-sum-exp.
The engine paths are pinned to a replay of their own step logits through the restatement, to themselves (graph vs eager) and to the host
loops with transformers' processors.

The tolerance of the top-k values: the kernel sums exp(x - max) in another order than torch; tests/test_hip_topk_logprob.py bounds that
at 4e-6 on the log-probability.  The repetition penalty multiplies a log-probability by p, so tol = p * 4e-6 + one fp32 ulp of the
reference value (the penalty's and the row score's own rounding)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from eilev_amd import abi
from eilev_amd.rules import RulesSpec, banned_ngram_ids, row_histories, rules_scores, rules_select_reference, rules_topk_reference
from eilev_amd.sampling import SampleSpec, draw_ok, keep_bounds, processed_scores
from hip_utils import P, load_case, models, stream_ptr

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


@functools.lru_cache(maxsize=None)
def _logits(rows, vocab):
    g = torch.Generator().manual_seed(1000 * rows + vocab)
    return torch.randn((rows, vocab), generator=g) * 3


def _params(spec: RulesSpec, max_new, step_offset=0, finalize=1):
    return abi.rules_params(spec.repetition_penalty, spec.no_repeat_ngram, spec.min_new, max_new, spec.eos, spec.pad_id, spec.prefix_id, step_offset,
                            finalize)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. eilev_rules_select --------------------------------------------------------------------------------------------------------------
def _select(logits, state, finished, tokens, out, spec: RulesSpec, step_offset=0, finalize=1):
    """One eilev_rules_select call on device copies of the host buffers, checked against the restatement: `processed` bit for bit, tokens,
    out_tokens, finished and state equal.  Returns the restatement's results."""
    rl = abi.load_rules()
    R, V = logits.shape
    dv = lambda a, dt: torch.as_tensor(a).to(dt).cuda().contiguous()
    lg, st, fin, tok, o = dv(logits, torch.float32), dv(state, torch.int32), dv(finished, torch.uint8), dv(tokens, torch.int64), dv(out, torch.int64)
    proc = torch.full((R, V), float("nan"), dtype=torch.float32, device="cuda")
    prm = _params(spec, out.shape[1], step_offset, finalize)
    rc = rl.eilev_rules_select(C.byref(prm), P(lg), R, V, P(st), P(fin), P(tok), P(o), P(proc), None, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ref = rules_select_reference(logits, state, finished, tokens, out, spec, step_offset, finalize)
    assert torch.equal(_bits(proc.cpu()), _bits(ref["processed"]))
    assert torch.equal(tok.cpu(), ref["tokens"]), (tok.cpu().tolist(), ref["tokens"].tolist())
    assert torch.equal(o.cpu(), ref["out_tokens"]) and torch.equal(fin.cpu(), ref["finished"]) and st.cpu().tolist() == ref["state"]
    return ref


def _history5(lg):
    """(rows, 5): [best, 3, second, best, 3] — duplicates, the row's current best id, a low id; the 2-gram [3, second] and the 3-gram
    [best, 3, second] are what a size-2 / size-3 ban finds."""
    top = torch.topk(lg, 2, dim=1).indices
    best, second = top[:, 0], top[:, 1]
    three = torch.full_like(best, 3)
    return torch.stack((best, three, second, best, three), dim=1)


@pytest.mark.parametrize("vocab", [1000, 32128, 50272])
@pytest.mark.parametrize("rows", [1, 7, 32])
def test_rules_select_equals_the_restatement(rows, vocab):
    T = 12
    lg = _logits(rows, vocab)
    zeros = lambda dt: torch.zeros(rows, dtype=dt)
    out5 = torch.full((rows, T), 1, dtype=torch.int64)
    out5[:, :5] = _history5(lg)
    best, second = out5[:, 0], out5[:, 2]
    # step 5: the penalty and every ban size; the ban must change the choice where it hits the (penalised) best id
    for n in (0, 1, 2, 3):
        ref = _select(lg, [5, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(repetition_penalty=1.5, no_repeat_ngram=n, pad_id=1))
        banned = torch.isinf(ref["processed"]).sum(dim=1)
        assert banned.tolist() == [{0: 0, 1: len(set(h)), 2: 1, 3: 1}[n] for h in out5[:, :5].tolist()]
        if n in (2, 3):
            assert bool(torch.isinf(ref["processed"][torch.arange(rows), second]).all())
    # a history shorter than n - 1: nothing is banned
    ref = _select(lg, [1, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(no_repeat_ngram=3, pad_id=1))
    assert not bool(torch.isinf(ref["processed"]).any()) and torch.equal(ref["tokens"], best)
    # the prefix id inside an n-gram: h = [7, 9, 4, 7] bans 9 at size 2; without the prefix nothing repeats
    outp = torch.full((rows, T), 1, dtype=torch.int64)
    outp[:, :3] = torch.tensor([9, 4, 7])
    lgp = lg.clone()
    lgp[:, 9] = 50.0  # (9 would win)
    ref = _select(lgp, [3, 1], zeros(torch.uint8), zeros(torch.int64), outp, RulesSpec(no_repeat_ngram=2, prefix_id=7, pad_id=1))
    assert bool(torch.isinf(ref["processed"][:, 9]).all()) and not bool((ref["tokens"] == 9).any())
    ref = _select(lgp, [3, 1], zeros(torch.uint8), zeros(torch.int64), outp, RulesSpec(no_repeat_ngram=2, prefix_id=-1, pad_id=1))
    assert bool((ref["tokens"] == 9).all())
    # min_new above and below the step: the EOS ids (row 0's best among them) are banned while step < min_new
    eos = (int(best[0]), 5)
    ref = _select(lg, [2, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(min_new=3, eos=eos, pad_id=1))
    assert int(ref["tokens"][0]) == int(second[0]) and int(ref["finished"][0]) == 0
    ref = _select(lg, [3, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(min_new=3, eos=eos, pad_id=1))
    assert int(ref["tokens"][0]) == int(best[0]) and int(ref["finished"][0]) == 1
    # two EOS ids, one of them row 0's arg-max AFTER the rules (the penalised best loses to it or keeps the lead: taken from the restatement)
    spec = RulesSpec(repetition_penalty=1.5, no_repeat_ngram=2, pad_id=1)
    after = int(rules_select_reference(lg, [5, 1], zeros(torch.uint8), zeros(torch.int64), out5, spec)["tokens"][0])
    ref = _select(lg, [5, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(1.5, 2, eos=(vocab - 1, after), pad_id=1))
    assert int(ref["finished"][0]) == 1 and ref["state"] == [6, int(rows > 1 and bool((ref["finished"] == 0).any()))]
    # finished rows emit the pad id and stay finished
    fin = (torch.arange(rows) % 2 == 0).to(torch.uint8)
    ref = _select(lg, [5, 1], fin, zeros(torch.int64), out5, RulesSpec(1.5, 2, eos=(after,), pad_id=1))
    assert bool((ref["tokens"][fin.bool()] == 1).all())
    # an all-banned row: only the ids of its history are finite, and size 1 bans them: id 0
    lga = lg.clone()
    lga[0] = NEG_INF
    lga[0, out5[0, :5]] = 1.0
    ref = _select(lga, [5, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(no_repeat_ngram=1, pad_id=1))
    assert int(ref["tokens"][0]) == 0 and not bool(torch.isfinite(ref["processed"][0]).any())
    # step_offset / finalize in both forms
    a = _select(lg, [6, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(1.5, 3, pad_id=1), step_offset=-1, finalize=0)
    b = _select(lg, [5, 1], zeros(torch.uint8), zeros(torch.int64), out5, RulesSpec(1.5, 3, pad_id=1), step_offset=0, finalize=1)
    assert a["state"][0] == 6 and b["state"][0] == 6 and torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["out_tokens"], b["out_tokens"])


def test_rules_select_with_a_512_id_history():
    """max_new = 512, step 511, size 3, one row: every start position of the scan is in use; ids over a small alphabet so that 2-grams repeat."""
    V, T = 32128, 512
    lg = _logits(1, V)
    g = torch.Generator().manual_seed(512)
    out = torch.randint(0, 12, (1, T), generator=g)
    ref = _select(lg, [511, 1], torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), out, RulesSpec(1.5, 3, pad_id=1))
    want = banned_ngram_ids(out[0, :511].tolist(), 3)
    assert len(want) >= 2 and torch.nonzero(torch.isinf(ref["processed"][0])).flatten().tolist() == want


def test_rules_calls_refuse_what_the_header_excludes():
    rl = abi.load_rules()
    lg = torch.zeros((2, 1002), device="cuda")
    st, fin, tok, out = (torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda"),
                         torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((2, 4), dtype=torch.int64, device="cuda"))
    prm = _params(RulesSpec(), 4)
    assert rl.eilev_rules_select(C.byref(prm), P(lg), 2, 1002, P(st), P(fin), P(tok), P(out), None, None, 0, stream_ptr()) == -2
    assert rl.eilev_rules_ban(C.byref(prm), P(lg), 2, 1002, P(st), P(out), stream_ptr()) == -2
    bad = _params(RulesSpec(repetition_penalty=0.0), 4)
    assert rl.eilev_rules_select(C.byref(bad), P(lg), 2, 1000, P(st), P(fin), P(tok), P(out), None, None, 0, stream_ptr()) == -1
    torch.cuda.synchronize()


# ---- 2. eilev_rules_topk_logprob -------------------------------------------------------------------------------------------------------
TOPK_T = 8
TOPK_PEN = 1.5


def _topk_case(B, nb, n_eos, vocab, cur):
    """Logits, row scores, run_seq and the spec of one case.  run_seq[r] = [best, second, third, 3, best, ..]: at cur = 5 the 2-gram
    [best, second] bans the second-best id, the best and the third-best carry the penalty."""
    R = B * nb
    lg = _logits(R, vocab)
    g = torch.Generator().manual_seed(77 * R + vocab + cur)
    score = torch.randn(R, generator=g) * 2 - 3
    top = torch.topk(lg, 3, dim=1).indices
    seq = torch.full((R, TOPK_T), 1, dtype=torch.int64)
    seq[:, 0], seq[:, 1], seq[:, 2], seq[:, 3], seq[:, 4] = top[:, 0], top[:, 1], top[:, 2], 3, top[:, 0]
    spec = RulesSpec(repetition_penalty=TOPK_PEN, no_repeat_ngram=2, min_new=2, eos=(3, 11, 17)[:n_eos], pad_id=1)
    return lg, score, seq, spec, max(2, 1 + n_eos) * nb


def _tol(v):
    """p * 4e-6 + one fp32 ulp of |v| (0 where v is not finite)"""
    mag = v.abs().clamp(min=2.0 ** -126)
    tol = TOPK_PEN * 4e-6 + (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag)
    return torch.where(torch.isfinite(v), tol, torch.zeros_like(tol))


def _topk_reference(B, nb, n_eos, vocab, cur):
    """The reference alone: (values + row score (R, V), tol (R, V), banned (R, V), ids_decided) — ids_decided: the smallest gap among the
    reference's top keep + 1 values of every row exceeds 2 tol, so the kernel's ids must be the reference's, in order."""
    lg, score, seq, spec, keep = _topk_case(B, nb, n_eos, vocab, cur)
    ref = rules_topk_reference(lg, score, seq, cur, spec, keep + 1)
    tot = ref["processed"] + score.view(-1, 1)
    tol = _tol(tot)
    v = ref["values"]
    gap = (v[:, :-1] - v[:, 1:])
    tol_top = torch.gather(tol, 1, ref["ids"].long())
    decided = bool((gap > 2 * torch.maximum(tol_top[:, :-1], tol_top[:, 1:])).all())
    return tot, tol, torch.isinf(ref["processed"]), decided, ref


# where the reference decides the ids at cur = 5 (derived from the reference alone, on the CPU; the test re-derives it and compares).
# Smallest gaps there: (2, 3) 1.9e-3 .. 7.0e-3, (1, 5) 1.6e-3, 2.4e-3 and 5.7e-6 (vocab 50272: below 2 tol = 1.4e-5), (6, 5) 4.0e-5, 1.7e-5, 6.0e-5.
TOPK_DECIDED_AT_5 = {(2, 3, 1000): True, (2, 3, 32128): True, (2, 3, 50272): True, (1, 5, 1000): True, (1, 5, 32128): True, (1, 5, 50272): False,
                     (6, 5, 1000): True, (6, 5, 32128): True, (6, 5, 50272): True}


@pytest.mark.parametrize("cur", [0, 1, 5])
@pytest.mark.parametrize("vocab", [1000, 32128, 50272])
@pytest.mark.parametrize("B,nb,n_eos", [(2, 3, 1), (1, 5, 1), (6, 5, 3)])
def test_rules_topk_logprob_against_the_restatement(B, nb, n_eos, vocab, cur):
    rl = abi.load_rules()
    lg, score, seq, spec, keep = _topk_case(B, nb, n_eos, vocab, cur)
    R = B * nb
    tot, tol, banned, decided, ref = _topk_reference(B, nb, n_eos, vocab, cur)
    dlg, dsc, dseq = lg.cuda().contiguous(), score.cuda().contiguous(), seq.cuda().contiguous()
    state = torch.tensor([cur + 1, 1], dtype=torch.int32, device="cuda")
    val = torch.empty((R, keep), dtype=torch.float32, device="cuda")
    idx = torch.empty((R, keep), dtype=torch.int32, device="cuda")
    proc = torch.full((R, vocab), float("nan"), dtype=torch.float32, device="cuda")
    prm = _params(spec, TOPK_T, 0, 0)
    rc = rl.eilev_rules_topk_logprob(C.byref(prm), P(dlg), P(dsc), R, vocab, keep, P(state), P(dseq), P(val), P(idx), P(proc), None, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    val, idx, proc = val.cpu(), idx.cpu().long(), proc.cpu()
    assert state.cpu().tolist() == [cur + 1, 1] and torch.equal(dseq.cpu(), seq)  # nothing but the outputs is written
    # the processed log-probabilities: -inf exactly where the reference bans, else within tol (without the row score: tol is an upper bound there too)
    assert torch.equal(torch.isinf(proc), banned)
    fin = ~banned
    assert bool(((proc - ref["processed"]).abs()[fin] <= _tol(ref["processed"])[fin]).all())
    # (a) every value within tol of the reference's value at the returned id
    ref_at = torch.gather(tot, 1, idx)
    tol_at = torch.gather(tol, 1, idx)
    both_inf = torch.isinf(val) & torch.isinf(ref_at) & (val < 0) & (ref_at < 0)
    assert bool((((val - ref_at).abs() <= tol_at) | both_inf).all()), float((val - ref_at).abs().max())
    # (b) descending, equal values by ascending id; no id twice
    assert bool(((val[:, :-1] > val[:, 1:]) | ((val[:, :-1] == val[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all())
    assert all(len(set(r)) == keep for r in idx.tolist())
    # (c) every id whose reference value exceeds the last kept value by more than 2 tol is present
    present = torch.zeros_like(banned).scatter_(1, idx, True)
    must = tot > (val[:, -1:] + 2 * tol)
    assert not bool((must & ~present).any())
    # (d) no banned id with a finite value
    assert not bool((torch.gather(banned, 1, idx) & torch.isfinite(val)).any())
    # the rules bite: at cur = 5 the second-best id of every row is banned, at cur < min_new the EOS ids are
    if cur == 5:
        assert bool(banned[torch.arange(R), seq[:, 1]].all())
        assert decided == TOPK_DECIDED_AT_5[(B, nb, vocab)]
    if cur < 2:
        assert bool(banned[:, list(spec.eos)].all())
    if decided:
        assert torch.equal(idx, ref["ids"][:, :keep].long())


# ---- 3. eilev_rules_ban -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1000, 50272])
def test_rules_ban_writes_minus_infinity_at_the_banned_ids_only(vocab):
    rl = abi.load_rules()
    R, T = 7, 12
    lg = _logits(R, vocab)
    g = torch.Generator().manual_seed(vocab)
    out = torch.randint(0, 5, (R, T), generator=g)
    out[3, 2] = vocab + 5  # an id outside the vocabulary: no write, still part of its n-grams
    for n, prefix, step, off in ((1, -1, 9, 0), (2, -1, 9, 0), (3, 2, 10, -1), (2, 4, 1, 0), (4, -1, 2, 0)):
        d = lg.cuda().contiguous()
        state = torch.tensor([step - off, 1], dtype=torch.int32, device="cuda")
        prm = _params(RulesSpec(no_repeat_ngram=n, prefix_id=prefix), T, off, 0)
        assert rl.eilev_rules_ban(C.byref(prm), P(d), R, vocab, P(state), P(out.cuda()), stream_ptr()) == 0
        torch.cuda.synchronize()
        hist = row_histories(out, step, prefix)
        want = lg.clone()
        n_banned = 0
        for b in range(R):
            ids = [i for i in banned_ngram_ids(hist[b], n) if 0 <= i < vocab]
            want[b, ids] = NEG_INF
            n_banned += len(ids)
        assert torch.equal(_bits(d.cpu()), _bits(want)), (n, prefix, step)
        assert (n_banned > 0) == (n < 4)
        assert torch.equal(_bits(d.cpu()), _bits(rules_scores(lg, hist, RulesSpec(no_repeat_ngram=n), step)))  # (randn holds no -0)


# ---- 4. the OPT engine: greedy search ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _opt_prompt():
    from eilev_amd.synth import synth_interleaved_ids, synth_pixels

    cfg, _, eng = models("mid")
    nq, vocab = cfg.num_query_tokens, cfg.text_config.vocab_size
    ids, vm = zip(*[synth_interleaved_ids([1, 1], [5, 4], nq, vocab, seed=11 + s) for s in range(3)])
    px = torch.from_numpy(synth_pixels(6, 2, cfg.vision_config.image_size)).cuda()
    ids, vm = torch.from_numpy(np.stack(ids)).cuda(), torch.from_numpy(np.stack(vm)).cuda()
    return eng, eng.embed_scatter(ids, vm, eng.encode_clips(px)), torch.ones_like(ids, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _plain_greedy(T):
    eng, emb, am = _opt_prompt()
    return eng.greedy_decode(emb, am, T, eos_id=-1).cpu()


def _replay_select(trace, ids, spec: RulesSpec, max_new):
    """The engine's step logits through the restatement: every id is the restatement's choice (exact: the arithmetic is)."""
    R = trace[0].shape[0]
    st = dict(state=[0, 1], finished=torch.zeros(R, dtype=torch.uint8), tokens=torch.zeros(R, dtype=torch.int64),
              out_tokens=torch.full((R, max_new), int(spec.pad_id), dtype=torch.int64))
    for t in range(ids.shape[1]):
        r = rules_select_reference(trace[t].cpu(), st["state"], st["finished"], st["tokens"], st["out_tokens"], spec)
        assert torch.equal(r["tokens"], ids[:, t].cpu()), (t, r["tokens"].tolist(), ids[:, t].tolist())
        st = dict(state=r["state"], finished=r["finished"], tokens=r["tokens"], out_tokens=r["out_tokens"])


def _no_repeated_ngram(row, n):
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) == len(set(grams))


def _opt_rule_sets():
    plain = _plain_greedy(10)
    return [dict(repetition_penalty=1.5), dict(no_repeat_ngram_size=1),
            dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_new_tokens=3, eos_id=[int(plain[0, 4]), int(plain[1, 5])])]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_opt_greedy_with_rules_replays_equals_graph_and_host_loop(which):
    eng, emb, am = _opt_prompt()
    T = 10
    kw = dict(_opt_rule_sets()[which])
    eos = kw.pop("eos_id", -1)
    spec = RulesSpec(kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), kw.get("min_new_tokens", 0),
                     tuple(eos) if isinstance(eos, list) else (), pad_id=1)
    trace = []
    eager = eng.rules_decode_device(emb, am, T, eos_id=eos, pad_id=1, use_graph=False, trace=trace, **kw)
    assert eng.rules_stats == dict(path="device", steps=eager.shape[1]) and len(trace) >= eager.shape[1] and trace[0].shape == (3, eng.dims.vocab)
    _replay_select(trace, eager, spec, T)
    graph = eng.rules_decode_device(emb, am, T, eos_id=eos, pad_id=1, **kw)
    assert torch.equal(graph, eager)
    again = eng.rules_decode_device(emb, am, T, eos_id=eos, pad_id=1, **kw)  # (the cached graph entry)
    assert torch.equal(again, eager)
    # the public route: the same call through beam_decode, on the device and — switched off — in the host loop with transformers' processors
    rules = {k: v for k, v in kw.items() if k != "min_new_tokens"}
    call = lambda: eng.beam_decode(emb, am, T, 1, eos_id=eos, pad_id=1, sampler=dict(greedy=True, min_new_tokens=kw.get("min_new_tokens", 0)),
                                   rules=dict(rules) if rules else None)
    eng.rules_stats = None
    dev = call()
    assert eng.rules_stats == dict(path="device", steps=eager.shape[1]) and torch.equal(dev, eager)
    eng.device_rules = False
    try:
        host = call()
        assert eng.rules_stats == dict(path="host", steps=host.shape[1])
    finally:
        eng.device_rules = True
    assert torch.equal(host, eager), (host.tolist(), eager.tolist())
    # the rules bite: the synthetic model repeats itself
    plain = _plain_greedy(T)
    assert not torch.equal(eager.cpu(), plain[:, :eager.shape[1]])
    if kw.get("no_repeat_ngram_size"):
        assert all(_no_repeated_ngram(r, kw["no_repeat_ngram_size"]) for r in eager.tolist())
    if kw.get("min_new_tokens"):
        assert not bool(torch.isin(eager[:, :3].cpu(), torch.tensor(eos)).any())


def test_opt_greedy_with_rules_more_than_32_rows_run_in_chunks_of_32():
    eng, emb, am = _opt_prompt()
    big, big_am = emb.repeat(11, 1, 1), am.repeat(11, 1)  # 33 rows
    kw = dict(eos_id=-1, repetition_penalty=1.5, no_repeat_ngram_size=2)
    ids = eng.rules_decode_device(big, big_am, 4, **kw)
    assert ids.shape == (33, 4) and eng.rules_stats == dict(path="device", steps=4)
    assert torch.equal(ids[:32], eng.rules_decode_device(big[:32], big_am[:32], 4, **kw))
    assert torch.equal(ids[32:], eng.rules_decode_device(big[32:], big_am[32:], 4, **kw))


def test_opt_greedy_sampling_and_rules_share_one_cached_decode_entry():
    """greedy_decode, sample_decode_device and rules_decode_device run through one loop and one `_dec_cache` slot: calls of one shape replace
    each other there, and greedy gives the same ids before, between and after them (= its eager ids).  Then the cached greedy entry is
    replayed on OTHER inputs of the same shape (what the benchmark does every step): rows rolled by one, one row left-padded by two."""
    eng, emb, am = _opt_prompt()
    T = 8
    kind = lambda: eng._dec_cache["key"][0]
    eager = eng.greedy_decode(emb, am, T, eos_id=-1, use_graph=False)
    first = eng.greedy_decode(emb, am, T, eos_id=-1, use_graph=True)
    assert kind() == "greedy"
    assert "argmax_out" not in eng._dec_cache  # the decode step's arg-max is the selection: no scratch buffers for it
    eng.sample_decode_device(emb, am, T, eos_id=-1, top_k=1, use_graph=True)
    assert kind() == "sample"
    second = eng.greedy_decode(emb, am, T, eos_id=-1, use_graph=True)
    assert kind() == "greedy"
    eng.rules_decode_device(emb, am, T, eos_id=-1, repetition_penalty=1.5, use_graph=True)
    assert kind() == "rules"
    third = eng.greedy_decode(emb, am, T, eos_id=-1, use_graph=True)
    assert kind() == "greedy"
    assert eager.shape == (3, T)
    for ids in (first, second, third):
        assert torch.equal(ids, eager), (ids.tolist(), eager.tolist())
    ent = eng._dec_cache
    emb2, am2 = torch.roll(emb, 1, dims=0).contiguous(), am.clone()
    am2[1, :2] = 0
    replayed = eng.greedy_decode(emb2, am2, T, eos_id=-1, use_graph=True)
    assert eng._dec_cache is ent and ent["graph"] is not None  # (the entry of `third`, replayed)
    eager2 = eng.greedy_decode(emb2, am2, T, eos_id=-1, use_graph=False)
    assert torch.equal(replayed, eager2), (replayed.tolist(), eager2.tolist())


# ---- 5. the OPT engine: beam search -----------------------------------------------------------------------------------------------------
class _BanEven:
    """a user LogitsProcessor: even token ids above 9 are forbidden"""

    def __call__(self, input_ids, scores):
        scores = scores.clone()
        scores[:, 10::2] = NEG_INF
        return scores


@pytest.mark.parametrize("rules", [dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.3),
                                   dict(repetition_penalty=1.15, no_repeat_ngram_size=3, min_new_tokens=2)])
@pytest.mark.parametrize("B,nb", [(2, 3), (1, 5)])
def test_opt_beam_search_with_rules_equals_the_host_loop(B, nb, rules):
    eng, emb, am = _opt_prompt()
    emb, am, T = emb[:B].contiguous(), am[:B].contiguous(), 8
    plain = eng.beam_decode(emb, am, T, nb, 1.0, eos_id=-1, pad_id=1)
    eos = int(plain[0, 0])  # the plain search's first id: as an EOS id it would end hypotheses at once
    rules = dict(rules)
    min_new = rules.pop("min_new_tokens", 0)
    call = lambda extra=None: eng.beam_decode(emb, am, T, nb, 1.0, eos_id=eos, pad_id=1, min_new_tokens=min_new, rules=dict(rules, **(extra or {})))
    eng.rules_stats = None
    dev = call()
    assert eng.rules_stats == dict(path="device", steps=dev.shape[1])
    eng.device_rules = False
    try:
        host = call()
        assert eng.rules_stats == dict(path="host", steps=host.shape[1])
    finally:
        eng.device_rules = True
    assert torch.equal(dev, host), (dev.tolist(), host.tolist())
    rows = []
    for r in dev.tolist():  # (a hypothesis that ended early is filled up with the pad id 1)
        while r and r[-1] == 1:
            r = r[:-1]
        rows.append(r)
    if rules.get("no_repeat_ngram_size"):
        assert all(_no_repeated_ngram(r, rules["no_repeat_ngram_size"]) for r in rows)
    if min_new:
        assert not bool((dev[:, :min_new] == eos).any())
    from transformers import LogitsProcessorList

    user = call(dict(processors=LogitsProcessorList([_BanEven()]), stopping=None))
    assert eng.rules_stats["path"] == "host"
    assert not bool(((user >= 10) & (user % 2 == 0)).any())


# ---- 6. flan-t5: greedy search ----------------------------------------------------------------------------------------------------------
def _t5_case(golden_dir, name):
    g, meta, px = load_case(golden_dir, name)
    _, _, eng = models(meta["config"])
    t = lambda a: torch.from_numpy(a).cuda()
    return eng, eng.embed_scatter(t(g["input_ids"]), t(g["video_input_mask"]), eng.encode_clips(t(px))), t(g["attention_mask"])


@pytest.mark.parametrize("name", ["mid_t5_b1", "tiny_t5_b2"])
def test_t5_greedy_with_rules_sees_the_start_token(golden_dir, name):
    eng, emb, am = _t5_case(golden_dir, name)
    R, T = emb.shape[0], 6
    for kw in (dict(no_repeat_ngram_size=1), dict(repetition_penalty=1.5, no_repeat_ngram_size=2, min_new_tokens=2)):
        spec = RulesSpec(kw.get("repetition_penalty", 1.0), kw["no_repeat_ngram_size"], kw.get("min_new_tokens", 0), (), pad_id=0, prefix_id=0)
        trace = []
        eager = eng.t5_rules_device(emb, am, T, eos_id=-1, start_id=0, use_graph=False, trace=trace, **kw)
        assert eager.shape == (R, T + 1) and bool((eager[:, 0] == 0).all()) and len(trace) == T
        assert eng.rules_stats == dict(path="device", steps=T)
        _replay_select(trace, eager[:, 1:], spec, T)
        if kw["no_repeat_ngram_size"] == 1:  # the start token is in the history: no id equals it, none repeats
            assert not bool((eager[:, 1:] == 0).any()) and all(len(set(r)) == len(r) for r in eager.tolist())
        assert torch.equal(eng.t5_rules_device(emb, am, T, eos_id=-1, start_id=0, **kw), eager)
        rules = {k: v for k, v in kw.items() if k != "min_new_tokens"}
        call = lambda: eng.t5_beam(emb, am, T, 1, eos_id=-1, pad_id=0, start_id=0, sampler=dict(greedy=True, min_new_tokens=kw.get("min_new_tokens", 0)),
                                   rules=dict(rules))
        eng.rules_stats = None
        assert torch.equal(call(), eager) and eng.rules_stats == dict(path="device", steps=T)
        eng.device_rules = False
        try:
            host = call()
            assert eng.rules_stats == dict(path="host", steps=T)
        finally:
            eng.device_rules = True
        assert torch.equal(host, eager), (host.tolist(), eager.tolist())


# ---- 7. sampling with no_repeat_ngram_size ----------------------------------------------------------------------------------------------
SAMPLE_TOL = 2 * 16 * 2.0 ** -24  # (tests/test_hip_device_sampling.py derives it)


def _replay_draws(trace, uniforms, spec: SampleSpec, ngram, ids, max_new):
    """The engine's step logits through the restatements, teacher-forced with the engine's ids: the n-gram ban first (hf's order), then the
    sampler's own rules; every id is a valid draw and lies outside the banned set of its step."""
    from eilev_amd.sampling import row_history

    R = trace[0].shape[0]
    out = torch.full((R, max_new), int(spec.pad_id), dtype=torch.int64)
    hits = 0
    for t, lg in enumerate(trace[:ids.shape[1]]):
        hist = row_history(out, t, spec.prefix_id)
        lg = rules_scores(lg.cpu(), hist, RulesSpec(no_repeat_ngram=ngram), t)
        for b in range(R):
            ban = banned_ngram_ids(hist[b], ngram)
            hits += len(ban)
            assert int(ids[b, t]) not in ban, (t, b)
        scores = processed_scores(lg, hist, spec, t)
        must, may = keep_bounds(lg, hist, spec, SAMPLE_TOL, t)
        ok = draw_ok(may, scores, uniforms[t].cpu(), ids[:, t].cpu(), SAMPLE_TOL) | draw_ok(must, scores, uniforms[t].cpu(), ids[:, t].cpu(), SAMPLE_TOL)
        assert bool(ok.all()), (t, ids[:, t].tolist())
        out[:, t] = ids[:, t].cpu()
    return hits


def test_opt_sampling_with_the_ngram_ban_stays_on_the_device():
    eng, emb, am = _opt_prompt()
    T = 8
    uni = torch.rand((T, 3), generator=torch.Generator().manual_seed(17))
    for n in (1, 2):
        spec = SampleSpec(1.5, 3, 1.0, repetition_penalty=1.2, pad_id=1)
        kw = dict(eos_id=-1, pad_id=1, temperature=1.5, top_k=3, repetition_penalty=1.2, no_repeat_ngram_size=n, uniforms=uni)
        trace = []
        ids = eng.sample_decode_device(emb, am, T, use_graph=False, trace=trace, **kw)
        assert eng.sample_stats == dict(path="device", steps=T)
        hits = _replay_draws(trace, uni, spec, n, ids, T)
        assert hits > 0 or n > 1  # (size 1 bans from the second step on; whether a 2-gram's first id comes back depends on the draws)
        assert all(_no_repeated_ngram(r, n) for r in ids.tolist())
        assert torch.equal(eng.sample_decode_device(emb, am, T, **kw), ids)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    eng.sample_stats = None
    out = eng.beam_decode(emb, am, T, 1, eos_id=-1, pad_id=1, sampler=dict(temperature=1.5, top_k=3, top_p=1.0, generator=g, no_repeat_ngram_size=1))
    assert eng.sample_stats == dict(path="device", steps=T) and all(len(set(r)) == T for r in out.tolist())


@pytest.mark.parametrize("name", ["mid_t5_b1", "tiny_t5_b2"])
def test_t5_sampling_with_the_ngram_ban_stays_on_the_device(golden_dir, name):
    eng, emb, am = _t5_case(golden_dir, name)
    R, T = emb.shape[0], 6
    uni = torch.rand((T, R), generator=torch.Generator().manual_seed(19))
    spec = SampleSpec(1.5, 3, 1.0, pad_id=0, prefix_id=0)
    kw = dict(eos_id=-1, start_id=0, temperature=1.5, top_k=3, no_repeat_ngram_size=1, uniforms=uni)
    trace = []
    ids = eng.t5_sample_device(emb, am, T, use_graph=False, trace=trace, **kw)
    assert eng.sample_stats == dict(path="device", steps=T)
    assert _replay_draws(trace, uni, spec, 1, ids[:, 1:], T) > 0
    assert all(len(set(r)) == T + 1 for r in ids.tolist())  # the start token included
    assert torch.equal(eng.t5_sample_device(emb, am, T, **kw), ids)


# ---- 8. the model API -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
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


class _Never:
    """a user StoppingCriteria that never fires"""

    def __call__(self, input_ids, scores, **kw):
        return torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)


@pytest.mark.parametrize("config_name", ["tiny", "tiny_t5"])
def test_generate_routes_the_rules_to_the_device(config_name):
    from transformers import LogitsProcessorList, StoppingCriteriaList

    model, kw = _model(config_name)
    is_t5 = config_name.endswith("t5")
    eng = model.engine()
    vocab = model.config.text_config.vocab_size
    plain = model.generate(**kw, max_new_tokens=6, eos_token_id=None)
    a, b = int(plain[0, 2 + is_t5]), int(plain[1, 3 + is_t5])
    calls = [dict(repetition_penalty=1.5, no_repeat_ngram_size=2, max_new_tokens=6, eos_token_id=None),
             dict(eos_token_id=[a, b], min_new_tokens=2, max_new_tokens=6)]
    if not is_t5:
        calls.append(dict(num_beams=3, no_repeat_ngram_size=2, max_new_tokens=6, eos_token_id=None))
    for call in calls:
        eng.rules_stats = None
        out = model.generate(**kw, **call)
        assert eng.rules_stats is not None and eng.rules_stats["path"] == "device", call
        assert out.dtype == torch.int64 and out.shape[0] == 2 and out.shape[1] <= 6 + is_t5 and int(out.min()) >= 0 and int(out.max()) < vocab
        if "min_new_tokens" in call:
            assert not bool(torch.isin(out[:, is_t5:is_t5 + 2], torch.tensor([a, b], device=out.device)).any())
        for extra in (dict(logits_processor=LogitsProcessorList([_BanEven()])), dict(stopping_criteria=StoppingCriteriaList([_Never()]))):
            eng.rules_stats = None
            host = model.generate(**kw, **call, **extra)
            assert eng.rules_stats is not None and eng.rules_stats["path"] == "host", (call, extra)
            assert host.dtype == out.dtype and host.shape[0] == 2
            if "stopping_criteria" in extra:  # a criterion that never fires changes nothing: the host loop returns the device path's ids
                assert torch.equal(host, out), (call, host.tolist(), out.tolist())
