"""The CPU restatement of the logits-rules library (eilev_amd/rules.py; include/eilev_rules.h) against transformers' own processors, bit for
bit, and — free running on a tiny random `transformers` OPT — against that model's `generate()` token for token: greedy search through
`rules_select_reference`, beam search through `beam_search_device` with `rules_topk_reference` as its per-row selection.  Plus the
library's export list and the engine's routing rule on a stub."""
import ctypes as C

import pytest
import torch

from eilev_amd import abi
from eilev_amd.beam import beam_search, beam_search_device
from eilev_amd.rules import RulesSpec, banned_ngram_ids, row_histories, rules_scores, rules_select_reference, rules_topk_reference


def _hf_rules(scores, history, rp, n, width):
    """transformers' two processors on one row; the scores are widened to `width` columns so that an id outside the vocabulary is one hf can
    index (the restatement ignores it), then cut back."""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    V = scores.shape[-1]
    x = torch.cat((scores, torch.zeros(scores.shape[0], width - V)), dim=1)
    ids = torch.tensor([history], dtype=torch.int64)
    if rp != 1.0:
        x = RepetitionPenaltyLogitsProcessor(penalty=rp)(ids, x)
    if n:
        x = NoRepeatNGramLogitsProcessor(n)(ids, x)
    return x[:, :V]


def _bits(t):
    return t.contiguous().view(torch.int32)


# (the restatement's one stated deviation from hf is "-0 is +0": hf's results are compared after the same `+ 0.0`)


def _scores(g, V):
    x = torch.randn(1, V, generator=g) * 3
    x[0, 1], x[0, 2], x[0, 3] = 0.0, float("-inf"), 2.5   # +0, -inf and a positive entry at ids the histories below use
    x[0, 5] = -1.25
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_banned_ids_and_scores_equal_transformers(n):
    """Random histories over 4 ids (duplicates, repeated n-grams), every length 0..8, both signs, +0 and -inf entries: fp32 bit-equal."""
    from transformers import NoRepeatNGramLogitsProcessor

    def hf_banned(h):  # the ids hf's class sets to -inf on a row of zeros
        out = NoRepeatNGramLogitsProcessor(n)(torch.tensor([h], dtype=torch.int64), torch.zeros(1, V))
        return torch.nonzero(torch.isinf(out[0])).flatten().tolist()

    g = torch.Generator().manual_seed(100 + n)
    V = 16
    for m in range(0, 9):
        for _ in range(12):
            h = torch.randint(0, 4, (m,), generator=g).tolist()
            want_ban = hf_banned(h)
            assert banned_ngram_ids(h, n) == want_ban, (n, h)
            for rp in (1.0, 1.3):
                x = _scores(g, V)
                spec = RulesSpec(repetition_penalty=rp, no_repeat_ngram=n)
                got = rules_scores(x, [h], spec, 0)
                want = _hf_rules(x, h, rp, n, V)
                assert torch.equal(_bits(got), _bits(want + 0.0)), (n, h, rp)


def test_scores_with_signed_zero_nan_and_an_id_outside_the_vocabulary():
    g = torch.Generator().manual_seed(7)
    V = 16
    x = _scores(g, V)
    x[0, 4] = -0.0
    # ids 20 and 17 are outside the vocabulary: they receive nothing, but still stand inside 2-grams ([20, 5] repeats: 5 is banned after 20)
    h = [3, 20, 5, 1, 1, 4, 17, 2, 20]
    got = rules_scores(x, [h], RulesSpec(repetition_penalty=1.5, no_repeat_ngram=2), 0)
    want = _hf_rules(x, h, 1.5, 2, 24)
    assert torch.equal(_bits(got), _bits(want + 0.0))
    assert got[0, 5] == float("-inf") and got[0, 3] == x[0, 3] / torch.tensor(1.5) and got[0, 2] == float("-inf")
    assert _bits(got)[0, 4] == 0 and _bits(got)[0, 1] == 0  # -0 / 1.5 = -0 -> +0; +0 stays
    assert banned_ngram_ids(h, 2) == [5]
    x[0, 7] = float("nan")
    got = rules_scores(x, [[7]], RulesSpec(repetition_penalty=1.5), 0)
    assert got[0, 7] == float("-inf")
    # min_new: the EOS ids are banned while step < min_new, ids outside the vocabulary are ignored
    spec = RulesSpec(min_new=3, eos=(6, 9, 99))
    assert torch.isinf(rules_scores(x, [[]], spec, 2)[0, [6, 9]]).all() and torch.isfinite(rules_scores(x, [[]], spec, 3)[0, [6, 9]]).all()


def test_scores_with_a_512_id_history():
    g = torch.Generator().manual_seed(9)
    V = 64
    h = torch.randint(0, V, (512,), generator=g).tolist()
    x = torch.randn(1, V, generator=g) * 3
    for n in (1, 2, 3, 4):
        got = rules_scores(x, [h], RulesSpec(repetition_penalty=1.2, no_repeat_ngram=n), 0)
        assert torch.equal(_bits(got), _bits(_hf_rules(x, h, 1.2, n, V) + 0.0)), n
    assert len(banned_ngram_ids(h, 2)) > 0 and len(banned_ngram_ids(h, 1)) == len(set(h))


# ---- free running against transformers' generate() -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_opt():
    from transformers import OPTConfig, OPTForCausalLM

    torch.manual_seed(0)
    cfg = OPTConfig(vocab_size=40, hidden_size=32, num_hidden_layers=2, ffn_dim=64, num_attention_heads=4, max_position_embeddings=64,
                    word_embed_proj_dim=32, pad_token_id=1, bos_token_id=2, eos_token_id=3, do_layer_norm_before=True)
    m = OPTForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(8.0)  # sharper distributions: EOS ids actually win some steps
    return m


def _hf(model, prompt, **kw):
    with torch.no_grad():
        out = model.generate(prompt, attention_mask=torch.ones_like(prompt), pad_token_id=1, **kw)
    return out[:, prompt.shape[1]:]


def _eq(ours, hf, pad=1):
    n = max(ours.shape[1], hf.shape[1])
    f = lambda t: torch.nn.functional.pad(t, (0, n - t.shape[1]), value=pad)
    assert torch.equal(f(ours), f(hf)), (ours.tolist(), hf.tolist())


@pytest.mark.parametrize("rp,ngram,eos,min_new", [(1.3, 0, 3, 0), (1.0, 2, 3, 0), (1.2, 3, [3, 7, 11], 2)])
def test_greedy_loop_over_the_restatement_equals_transformers(tiny_opt, rp, ngram, eos, min_new):
    """hf's processors see the prompt ids in front of the generated ones: the history buffer starts with the prompt and the step counter at
    its length (min_new counts from there)."""
    from eilev_amd.sampling import eos_list

    torch.manual_seed(3)
    prompt = torch.randint(4, 40, (3, 6))
    R, P, T = 3, prompt.shape[1], 12
    spec = RulesSpec(repetition_penalty=rp, no_repeat_ngram=ngram, min_new=P + min_new, eos=tuple(eos_list(eos)), pad_id=1)
    st = dict(state=[P, 1], finished=torch.zeros(R, dtype=torch.uint8), tokens=torch.zeros(R, dtype=torch.int64),
              out_tokens=torch.cat((prompt, torch.ones(R, T, dtype=torch.int64)), dim=1))
    seq = prompt
    for _ in range(T):
        with torch.no_grad():
            logits = tiny_opt(seq).logits[:, -1].float()
        r = rules_select_reference(logits, st["state"], st["finished"], st["tokens"], st["out_tokens"], spec)
        st = dict(state=r["state"], finished=r["finished"], tokens=r["tokens"], out_tokens=r["out_tokens"])
        seq = torch.cat((seq, r["tokens"].view(R, 1)), dim=1)
        if r["state"][1] == 0:
            break
    ours = seq[:, P:]
    hf = _hf(tiny_opt, prompt, max_new_tokens=T, do_sample=False, num_beams=1, eos_token_id=eos, repetition_penalty=rp if rp != 1.0 else None,
             no_repeat_ngram_size=ngram or None, min_new_tokens=min_new or None)
    _eq(ours, hf)


def _oracle_advance(B, nb, T, state, anc):
    """eilev_beam_advance as the CPU oracle restates it (oracle/eilev_ref.c): the fused bookkeeping the engine pairs with the rules' top-k."""
    from oracle import runner

    lib = runner.lib()
    P = lambda t: C.c_void_p(t.data_ptr())

    def fn(row_lp, row_tok, st):
        eos = st["eos"]
        eos_arr = (C.c_int64 * max(1, len(eos)))(*eos)
        tokens = st.setdefault("tokens", torch.zeros(B * nb, dtype=torch.int64))
        rc = lib.eilev_beam_advance(P(row_lp), P(row_tok), B, nb, st["keep"], T, P(state), eos_arr, len(eos), P(st["pow_tab"]), int(st["reciprocal"]),
                                    int(st["early"]), P(st["run_seq"]), P(st["run_score"]), P(st["fin_seq"]), P(st["fin_score"]), P(st["fin_len"]),
                                    P(st["finished"]), P(st["can_improve"]), P(tokens), P(anc), T, None, 0, None)
        assert rc == 0, rc
    return fn


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("rp,ngram,nb,lp", [(1.3, None, 3, 1.0), (None, 2, 4, -1.0), (1.15, 3, 3, 1.0)])
def test_device_beam_loop_with_the_rules_hook_equals_transformers(tiny_opt, rp, ngram, nb, lp, fused):
    """beam_search_device with rules_topk_reference as topk_fn (topk_history=True), with the torch bookkeeping and with the fused
    eilev_beam_advance restatement, = hf generate() = the host loop `beam_search` with transformers' processors.  The model is driven with
    inputs_embeds, as the engine drives it: hf's processors then see the generated ids only."""
    from transformers import LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    torch.manual_seed(4)
    prompt = torch.randint(4, 40, (2, 6))
    B, T, V = 2, 9, 40
    R = B * nb
    emb = tiny_opt.get_input_embeddings()(prompt).detach()
    with torch.no_grad():
        hf = tiny_opt.generate(inputs_embeds=emb, attention_mask=torch.ones_like(prompt), pad_token_id=1, max_new_tokens=T, do_sample=False,
                               num_beams=nb, length_penalty=lp, eos_token_id=3, repetition_penalty=rp, no_repeat_ngram_size=ngram, early_stopping=False)
        first = tiny_opt(prompt).logits[:, -1].float()

    def stepper():
        seqs = {"s": prompt.repeat_interleave(nb, dim=0)}

        @torch.no_grad()
        def step(tokens, src):
            seqs["s"] = torch.cat((seqs["s"].index_select(0, src), tokens.view(-1, 1)), dim=1)
            return tiny_opt(seqs["s"]).logits[:, -1].float()
        return step

    procs = LogitsProcessorList()
    if rp:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=rp))
    if ngram:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    host = beam_search(stepper(), first, B, nb, T, lp, 3, 1, False, 1, processors=procs)
    _eq(host, hf)

    spec = RulesSpec(repetition_penalty=rp or 1.0, no_repeat_ngram=ngram or 0, eos=(3,), pad_id=1)
    keep = 2 * nb
    buf = torch.empty(R, V)
    state = torch.ones(2, dtype=torch.int32)  # the decode step's counter: cur = state[0] - 1
    step = stepper()
    seen = []

    def topk_fn(logits_buf, run_score, run_seq, cur_t):
        cur = int(state[0]) - 1 if fused else int(cur_t)
        seen.append(cur)
        r = rules_topk_reference(logits_buf, run_score, run_seq, cur, spec, keep)
        return r["values"], r["ids"]

    if fused:
        anc = torch.zeros((T, R), dtype=torch.int32)
        adv = _oracle_advance(B, nb, T, state, anc)
        holder = {}

        def advance(row_lp, row_tok, st):
            adv(row_lp, row_tok, st)
            holder["st"] = st

        def step_dev(_t, _s):
            # the hypothesis now in row r is run_seq[r, 0 .. cur + 1): a full forward over it is what the ancestor table gives the engine
            st = holder["st"]
            n = int(state[0])
            seq = torch.cat((prompt.repeat_interleave(nb, dim=0), st["run_seq"].reshape(R, T)[:, :n]), dim=1)
            with torch.no_grad():
                buf.copy_(tiny_opt(seq).logits[:, -1].float())
            state[0] += 1

        got = beam_search_device(step_dev, buf, first, B, nb, T, lp, 3, 1, False, 1, use_graph=False, check_every=1, topk_fn=topk_fn,
                                 advance_fn=advance, topk_history=True)
    else:
        got = beam_search_device(lambda t, s: buf.copy_(step(t.clone(), s.clone())), buf, first, B, nb, T, lp, 3, 1, False, 1, use_graph=False,
                                 check_every=1, topk_fn=topk_fn, topk_history=True)
    assert seen[:3] == [0, 1, 2]
    _eq(got, hf)
    _eq(got, host)


# ---- the library and the routing ------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    """libeilev_hip_rules.so: the entry points of include/eilev_rules.h = abi.RULES_EXPORTS = the library's dynamic symbols; checked in a
    child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    import os
    import re
    import shutil
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "eilev_rules.h")).read()
    assert sorted(set(re.findall(r"\b(eilev_rules_\w+)\s*\(", header))) == sorted(abi.RULES_EXPORTS)
    assert int(re.search(r"#define EILEV_RULES_ABI_VERSION (\d+)", header).group(1)) == abi.RULES_ABI_VERSION
    assert int(re.search(r"#define EILEV_RULES_MAX_EOS (\d+)", header).group(1)) == abi.RULES_MAX_EOS
    assert int(re.search(r"#define EILEV_RULES_MAX_VOCAB (\d+)", header).group(1)) == abi.RULES_MAX_VOCAB
    assert int(re.search(r"#define EILEV_RULES_MAX_KEEP (\d+)", header).group(1)) == abi.RULES_MAX_KEEP
    assert C.sizeof(abi.RulesParams) == 2 * 4 + 3 * 8 + 8 * abi.RULES_MAX_EOS + 2 * 8 + 2 * 4
    assert os.path.exists(abi.RULES_LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    code = ("import ctypes, sys; sys.path.insert(0, %r); from eilev_amd import abi; h = ctypes.CDLL(abi.RULES_LIB_PATH); "
            "assert all(hasattr(h, s) for s in abi.RULES_EXPORTS); assert h.eilev_rules_abi_version() == abi.RULES_ABI_VERSION; "
            "h.eilev_rules_scratch_bytes.restype = ctypes.c_size_t; assert h.eilev_rules_scratch_bytes(ctypes.c_int64(32), ctypes.c_int64(50272)) == 0") % root
    subprocess.check_call([sys.executable, "-c", code])
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.RULES_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.RULES_EXPORTS), syms
    p = abi.rules_params(1.5, 3, 2, 64, [2, 5], 1, 0, -1, 0)
    assert (p.repetition_penalty, p.no_repeat_ngram, p.min_new, p.max_new, p.n_eos, list(p.eos)[:2], p.pad_id, p.prefix_id, p.step_offset,
            p.finalize) == (1.5, 3, 2, 64, 2, [2, 5], 1, 0, -1, 0)
    with pytest.raises(NotImplementedError):
        abi.rules_params(eos_ids=list(range(9)))
    assert abi.rules_supported(50272) and abi.rules_supported(32128) and not abi.rules_supported(1002) and not abi.rules_supported(65540)


def test_routing_on_a_stub():
    """route.plan_decode without an engine: the numeric case goes to the device; more than 8 EOS ids, a vocabulary the library does not
    take, a user processor, a stopping criterion, a trace or the switch send it to the host with transformers' processors rebuilt."""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    from eilev_amd.route import Caps, plan_decode

    eng = dict(device_rules=True)

    def route(rules, vocab, eos_id, min_new_tokens=0, trace=None, allow_device=True):
        """(device keywords, host-form rules, with_rules) of a greedy search call: asked as the greedy sampler of num_beams == 1, which the
        device takes; ``allow_device=False``: asked as a one-beam search, which it does not."""
        sampler = dict(greedy=True, min_new_tokens=min_new_tokens) if allow_device else None
        plan = plan_decode(Caps("opt", vocab, 80, device_rules=eng["device_rules"]), 1, sampler, rules, eos_id, min_new_tokens, 8, trace is not None,
                           in_search_loop=True)
        assert (plan.route == "rules_device") == (plan.dev_kw is not None)
        return plan.dev_kw, plan.rules, plan.with_rules

    nums = dict(repetition_penalty=1.5, no_repeat_ngram_size=3)
    kw, rules, on = route(dict(nums), 50272, [2, 5], 2)
    assert kw == dict(repetition_penalty=1.5, no_repeat_ngram_size=3, min_new_tokens=2) and rules is None and on
    assert route(None, 50272, [2, 5], 0)[0] == dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)  # several EOS ids alone
    assert route(None, 50272, 2, 3)[0] is not None                                                                     # min_new_tokens alone
    assert route(None, 50272, 2, 0) == (None, None, False)                                                             # a plain call is not routed

    def host(*a, **k):
        kw, rules, on = route(*a, **k)
        assert kw is None and on
        return rules

    for rules in (host(dict(nums), 50272, list(range(9))), host(dict(nums), 1002, 2), host(dict(nums), 50272, 2, trace=[]),
                  host(dict(nums), 50272, 2, allow_device=False)):
        assert [type(p) for p in rules["processors"]] == [RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor] and rules["stopping"] is None
        assert rules["processors"][0].penalty == 1.5 and rules["processors"][1].ngram_size == 3
    user = lambda ids, scores: scores
    rules = host(dict(nums, processors=[user], stopping=None), 50272, 2)
    assert len(rules["processors"]) == 3 and rules["processors"][2] is user
    assert host(dict(processors=None, stopping=lambda ids, scores: False), 50272, 2)["stopping"] is not None
    eng["device_rules"] = False
    assert host(dict(nums), 50272, 2)["processors"] is not None
