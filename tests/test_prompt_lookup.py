"""Prompt-lookup decoding on the CPU (eilev_amd/pld.py): the draft rule against transformers' PromptLookupCandidateGenerator, the host
loop (the one the engine runs) against plain greedy decoding on a deterministic toy model for every draft policy, and generate()'s
argument checks, which run before any encode."""
import random

import pytest
import torch

from eilev_amd.pld import PldState, draft_cap, draft_ref, lookup_loop, step_ref


def _corpus(rng, vocab, n):
    ids = [rng.randrange(vocab) for _ in range(n)]
    for _ in range(rng.randrange(1, 4)):  # planted repeats: a segment copied elsewhere, often onto the tail
        ln = rng.randrange(1, 6)
        src = rng.randrange(0, max(1, n - ln))
        dst = n - ln if rng.random() < 0.5 else rng.randrange(0, max(1, n - ln))
        ids[dst:dst + ln] = ids[src:src + ln]
    return ids[:n]


@pytest.mark.parametrize("ngram", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 4, 10])
def test_draft_rule_equals_hf_prompt_lookup(ngram, k):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

    rng = random.Random(1000 * ngram + k)
    found = 0
    for trial in range(300):
        vocab = rng.choice([3, 6, 20])
        n = rng.randrange(1, 40)
        corpus = _corpus(rng, vocab, n)
        eos = [rng.randrange(vocab)] if rng.random() < 0.6 else []
        budget = rng.choice([1, 2, 3, k, k + 1, 50])  # 1: hf's max_length == input_length + 1 edge
        hf = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos) if eos else None, num_output_tokens=k, max_matching_ngram_size=ngram,
                                            max_length=n + budget)
        cand, _ = hf.get_candidates(torch.tensor([corpus], dtype=torch.long))
        want = cand[0, n:].tolist()[:max(budget - 1, 0)]  # the verify commits one id more than the draft: budget - 1 drafts at most
        st = PldState(k=k, ngram=ngram, max_new=budget, slot_base=0, slot_limit=10 ** 6, eos=eos, corpus=list(corpus))
        m = draft_ref(st)
        assert st.draft == want and m == len(want), (trial, corpus, eos, budget, st.draft, want)
        found += m > 0
    assert found > 50


def test_draft_caps():
    st = PldState(k=10, ngram=2, max_new=20, slot_base=5, slot_limit=5 + 6, eos=[], corpus=[1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2])
    st.status[0] = 3
    assert draft_cap(st, 3) == 3 and draft_ref(st) == 3 and st.draft == [3, 4, 5]  # the window must fit below slot_limit
    st.status[0] = 19
    assert draft_ref(st) == 0  # budget 1: the bonus id alone
    st.status[0], st.status[2] = 3, 1
    assert draft_ref(st) == 0  # done


# ---- the host loop on a toy model --------------------------------------------------------------------------------------------------
V = 12


class Toy:
    """Deterministic next-token logits of a sequence: a random table over the last two ids; some rows tie two ids (the lower wins)."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.table = torch.randint(0, V, (V, V), generator=g)
        self.tie = torch.rand((V, V), generator=g) < 0.3
        self.noise = -torch.rand((V, V, V), generator=g)

    def logits(self, seq):
        a, b = seq[-2], seq[-1]
        row = self.noise[a, b].clone()
        t = int(self.table[a, b])
        row[t] = 1.0
        if self.tie[a, b] and t + 1 < V:
            row[t + 1] = 1.0  # a tie: arg max takes t, the lower id
        return row

    def greedy(self, prompt, max_new, eos):
        seq, out = list(prompt), []
        for _ in range(max_new):
            x = int(torch.argmax(self.logits(seq)))
            out.append(x)
            seq.append(x)
            if x in eos:
                break
        return out


def run_lookup(toy, prompt, max_new, eos, k, ngram, policy, rng):
    """The engine's loop with the restated kernels and a toy model; `policy` may replace every draft (adversarial drafts)."""
    st = PldState(k=k, ngram=ngram, max_new=max_new, slot_base=len(prompt), slot_limit=len(prompt) + max_new + k, eos=eos, corpus=list(prompt))
    stats = dict(verify=0, single=0, accepted=0)

    def commit(logits, rows):
        assert logits.shape[0] == rows
        status = step_ref(st, logits)
        if policy is not None and not status[2]:
            d = policy(st, st.status[0])
            assert len(d) <= max(draft_cap(st, st.status[0]), 0)
            st.window[1:1 + len(d)] = d
            st.status[1] = status[1] = len(d)
        return status

    def verify(c, m):  # the window [last, d1 .. dm] after prompt + the committed ids before `last`
        ctx = list(prompt) + st.out[:c - 1]
        return torch.stack([toy.logits(ctx + st.window[:i + 1]) for i in range(m + 1)])

    def single(c):
        return toy.logits(list(prompt) + st.out[:c])[None]

    status = commit(toy.logits(list(prompt))[None], 1)  # the prefill's last logits
    c = lookup_loop(status, verify, single, commit, stats)
    assert c == len(st.out) and st.status[0] == c
    return st.out, stats


def _policies(toy, prompt, eos, rng):
    def truth(st, c):  # the true greedy continuation: every draft accepted
        seq, d = list(prompt) + st.out, []
        for _ in range(draft_cap(st, c)):
            x = int(torch.argmax(toy.logits(seq)))
            d.append(x)
            seq.append(x)
        return d

    def adversarial(st, c):  # random ids, EOS ids among them, or the truth with one id wrong
        cap = max(draft_cap(st, c), 0)
        n = rng.randint(0, cap)
        if rng.random() < 0.5:
            d = truth(st, c)[:n]
            if d and rng.random() < 0.5:
                d[rng.randrange(len(d))] = rng.randrange(V)
            return d
        pool = list(range(V)) + eos * 3
        return [rng.choice(pool) for _ in range(n)]

    return {"lookup": None, "none": lambda st, c: [], "truth": truth, "adversarial": adversarial}


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_new", [1, 2, 3, 7, 24])
def test_loop_returns_plain_greedy_ids_for_every_draft_policy(seed, max_new):
    rng = random.Random(seed * 100 + max_new)
    toy = Toy(seed)
    prompt = _corpus(rng, V, 30)
    for eos in ([], [int(toy.table[prompt[-2], prompt[-1]])], [3, 7]):  # no EOS; EOS as the very first id; several EOS ids
        want = toy.greedy(prompt, max_new, eos)
        for name, policy in _policies(toy, prompt, eos, rng).items():
            for k, ngram in ((1, 1), (4, 2), (10, 3)):
                got, stats = run_lookup(toy, prompt, max_new, eos, k, ngram, policy, rng)
                assert got == want, (name, k, ngram, eos, got, want)
                steps = 1 + stats["verify"] + stats["single"]  # every step commits its accepted drafts + 1 (fewer when an EOS draft ends it)
                assert len(got) == steps + stats["accepted"] if not eos else len(got) <= steps + stats["accepted"]
                if name == "none":
                    assert stats["verify"] == 0
                if name == "truth" and len(want) > 2 and k > 1:
                    assert stats["accepted"] > 0 and stats["verify"] < len(want) - 1


def test_loop_commits_eos_as_draft_and_as_bonus():
    """A draft that contains the EOS id: accepted up to it, the output ends there; EOS as the bonus id after an accepted draft."""
    toy = Toy(3)
    prompt = [1, 2, 3, 4, 5, 6]
    want = toy.greedy(prompt, 12, [])
    for cut in range(1, 6):
        eos = [want[cut]]
        ref = toy.greedy(prompt, 12, eos)

        def policy(st, c, want=want):
            cap = max(draft_cap(st, c), 0)
            return want[c:c + cap]  # the truth, EOS included (the lookup rule itself never drafts an EOS)

        got, _ = run_lookup(toy, prompt, 12, eos, 10, 2, policy, random.Random(0))
        assert got == ref and got[-1] == want[cut]


def test_step_ref_ties_and_nan():
    st = PldState(k=4, ngram=2, max_new=10, slot_base=0, slot_limit=100, eos=[], corpus=[5])
    st.window[1:3] = [2, 3]
    st.status[1] = 2
    lg = torch.full((3, 6), -1.0)
    lg[0, 2] = lg[0, 4] = 7.0  # tie: 2 wins, = d1
    lg[1, 3] = float("nan")
    lg[1, 1] = 0.5  # NaN never wins: 1 != d2 = 3 -> bonus 1
    status = step_ref(st, lg)
    assert st.out == [2, 1] and status[0] == 2 and status[3] == 1
    st2 = PldState(k=4, ngram=2, max_new=10, slot_base=0, slot_limit=100, eos=[], corpus=[5])
    step_ref(st2, torch.full((1, 6), float("nan")))
    assert st2.out == [0]


# ---- generate() argument checks (CPU model: they run before any encode, so no GPU is touched) ---------------------------------------
def _model():
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    return VideoBlipForConditionalGeneration(blip2_config("tiny"))


def test_generate_prompt_lookup_argument_checks():
    from transformers import LogitsProcessorList, MinLengthLogitsProcessor, StoppingCriteriaList, MaxLengthCriteria

    m = _model()
    one, two = torch.ones(1, 4, dtype=torch.long), torch.ones(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        m.generate(two, max_new_tokens=2, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, num_beams=2)
    with pytest.raises(NotImplementedError, match="do_sample"):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(NotImplementedError, match="logits processors"):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, logits_processor=LogitsProcessorList([MinLengthLogitsProcessor(2, 1)]))
    with pytest.raises(NotImplementedError, match="stopping criteria"):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(8)]))
    with pytest.raises(NotImplementedError, match="min_new_tokens"):
        m.generate(one, max_new_tokens=4, prompt_lookup_num_tokens=3, min_new_tokens=2)
    with pytest.raises(NotImplementedError, match="output_scores"):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, return_dict_in_generate=True, output_scores=True)
    with pytest.raises(ValueError):
        m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=0)
    # the route itself: past the checks the call reaches the engine, which needs a GPU (no CPU fallback)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            m.generate(one, max_new_tokens=2, prompt_lookup_num_tokens=3, max_matching_ngram_size=1)
    # unchanged: without prompt_lookup_num_tokens, max_matching_ngram_size is an unsupported argument as before
    with pytest.raises(NotImplementedError, match="unsupported generate"):
        m.generate(one, max_new_tokens=2, max_matching_ngram_size=2)
