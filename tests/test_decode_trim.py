"""The one trim of the decode loops (HipEngine._trim_at_eos: greedy, sampling and rules calls, OPT and flan-t5) against a direct restatement
of its rule, over simulated decodes.  No engine, no GPU.

The rule: with EOS ids, cut after the column where the last row emits its first EOS id, or at the steps done if some row never does;
without EOS ids, cut at the steps done."""
import random

import torch

from eilev_amd.engine import HipEngine


def _rule(rows, n, eos):
    if not eos:
        return [r[:n] for r in rows]
    cut = max(next((t + 1 for t in range(n) if r[t] in eos), n) for r in rows)
    return [r[:cut] for r in rows]


def _simulate(rng, B, T, eos, pad, poll, t5):
    """What the device leaves in `out` (B, T), and the steps done.  A row emits free ids until its first EOS id, then the pad id; columns
    never reached hold the pad id.  OPT: one selection from the prefill, then up to T - 1 steps, `finished` polled every `poll` steps;
    flan-t5: up to T steps, also polled after the last one."""
    out = [[pad] * T for _ in range(B)]
    fin = [False] * B

    def emit(t):
        for b in range(B):
            tok = pad if fin[b] else rng.randint(2, 5)
            out[b][t] = tok
            fin[b] = fin[b] or tok in eos

    n = 0
    if not t5:
        emit(0)
        n = 1
    steps = 0
    while n < T:
        emit(n)
        n += 1
        steps += 1
        if eos and (steps % poll == 0 or (t5 and n == T)) and all(fin):
            break
    return out, n


def test_trim_equals_the_rule_on_simulated_decodes():
    rng = random.Random(0)
    cut_early = with_pad_as_eos = never = 0
    for it in range(6000):
        B, T, poll = rng.randint(1, 4), rng.randint(1, 12), rng.randint(1, 4)
        eos = [[], [2], [3], [2, 4]][rng.randint(0, 3)]
        pad = rng.randint(1, 3)  # the pad id equals an EOS id in some cases
        out, n = _simulate(rng, B, T, eos, pad, poll, t5=bool(it % 2))
        got = HipEngine._trim_at_eos(torch.tensor(out, dtype=torch.int64).view(B, T), n, eos)
        want = _rule(out, n, eos)
        assert got.tolist() == want, (out, n, eos)
        assert got.dtype == torch.int64 and got.shape[0] == B
        cut_early += len(want[0]) < n
        with_pad_as_eos += pad in eos
        never += bool(eos) and any(not any(t in eos for t in r[:n]) for r in out)
    assert cut_early > 100 and with_pad_as_eos > 100 and never > 100  # the cases the rule distinguishes all occur


def test_trim_returns_a_copy():
    out = torch.arange(12, dtype=torch.int64).view(2, 6)
    ids = HipEngine._trim_at_eos(out, 4, [])
    ids[0, 0] = 99
    assert out[0, 0] == 0 and ids.shape == (2, 4)
