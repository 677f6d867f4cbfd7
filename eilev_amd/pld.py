"""Prompt-lookup decoding at batch 1 [hf generation/candidate_generator.py PromptLookupCandidateGenerator, generation/utils.py
`_assisted_decoding` with greedy verification].

Two things live here:
  - the plain-torch restatement of the two kernels of libeilev_hip_pld.so (include/eilev_pld.h): `draft_ref` and `step_ref`, on a
    host-side `PldState` that mirrors the device buffers.  The tests pin the HIP kernels to them bit for bit;
  - `lookup_loop`, the host loop the engine runs (eilev_amd/engine.py greedy_lookup_decode / t5_greedy_lookup): each step either
    verifies the draft window or, with no draft, runs one plain decode step, then commits.  It only sees the status block.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch


@dataclass
class PldState:
    """Host mirror of the device state of one generation (include/eilev_pld.h)."""
    k: int
    ngram: int
    max_new: int
    slot_base: int
    slot_limit: int
    eos: list
    corpus: list = field(default_factory=list)  # text ids, then every committed id
    window: list = None                          # [last committed id, d1 .. dm, stale ...] (k + 1)
    out: list = field(default_factory=list)      # committed ids
    status: list = field(default_factory=lambda: [0, 0, 0, 0])  # committed, draft length, done, accepted by the last step

    def __post_init__(self):
        if self.window is None:
            self.window = [0] * (self.k + 1)

    @property
    def draft(self):
        return self.window[1:1 + self.status[1]]


def draft_cap(st: PldState, c: int) -> int:
    """At most k ids, at most budget - 1 (the verify also commits the bonus id), and the window must fit below slot_limit."""
    return min(st.k, st.max_new - c - 1, st.slot_limit - st.slot_base - c)


def lookup_candidates(corpus, k: int, ngram: int, eos) -> list:
    """PromptLookupCandidateGenerator.get_candidates without processors, on a corpus of ids (before the budget caps)."""
    ids = [int(x) for x in corpus]
    n_len = len(ids)
    for n in range(min(ngram, n_len - 1), 0, -1):
        suffix = ids[n_len - n:]
        for idx in range(0, n_len - n):
            if ids[idx:idx + n] == suffix:  # idx + n < n_len: the continuation is not empty
                cont = ids[idx + n:min(idx + n + k, n_len)]
                for j, x in enumerate(cont):
                    if x in eos:
                        return cont[:j]
                return cont
    return []


def draft_ref(st: PldState) -> int:
    """eilev_pld_draft: window[1 .. m] and status[1] = m from the corpus and status[0] (committed count)."""
    c, done = st.status[0], st.status[2]
    cap = draft_cap(st, c)
    d = [] if done or cap <= 0 else lookup_candidates(st.corpus, st.k, st.ngram, st.eos)[:cap]
    st.window[1:1 + len(d)] = d
    st.status[1] = len(d)
    return len(d)


def argmax_rows(logits: torch.Tensor) -> list:
    """eilev_greedy_select's rule per row: the largest value, ties to the lowest id, NaN never wins, 0 when no row entry is a number."""
    x = logits.float()
    v = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
    best = v.max(dim=-1, keepdim=True).values
    hit = x == best
    first = hit.int().argmax(dim=-1)
    return [int(i) if h else 0 for i, h in zip(first.tolist(), hit.any(dim=-1).tolist())]


def step_ref(st: PldState, logits: torch.Tensor) -> list:
    """eilev_pld_step on the window's logits (rows = m + 1): accept the longest draft prefix the arg-maxima agree with, commit it and
    the bonus id (up to the first EOS, up to max_new ids), then the next draft.  Returns the status block."""
    g = argmax_rows(logits)
    m = len(g) - 1
    d = st.window[1:1 + m]
    a = 0
    while a < m and g[a] == d[a]:
        a += 1
    c = st.status[0]
    done = c >= st.max_new
    for i in range(a + 1):
        if done:
            break
        x = d[i] if i < a else g[a]
        st.out.append(x)
        st.corpus.append(x)
        st.window[0] = x
        c += 1
        done = x in st.eos or c >= st.max_new
    st.status[0], st.status[2], st.status[3] = c, int(done), a
    draft_ref(st)
    return list(st.status)


def lookup_loop(status, verify, single, commit, stats: dict) -> int:
    """The host loop of greedy prompt-lookup decoding, after the start (OPT: the commit of the prefill's last logits; flan-t5: the draft
    of the encoder's text ids).  status = (committed c, draft length m, done, accepted).  verify(c, m) runs the window [last, d1 .. dm]
    and returns its logits; single(c) runs one plain decode step on the last committed id; commit(logits, rows) -> the next status.
    Returns the committed count."""
    c, m, done = int(status[0]), int(status[1]), bool(status[2])
    while not done:
        if m > 0:
            logits, rows = verify(c, m), m + 1
            stats["verify"] += 1
        else:
            logits, rows = single(c), 1
            stats["single"] += 1
        status = commit(logits, rows)
        c, m, done = int(status[0]), int(status[1]), bool(status[2])
        stats["accepted"] += int(status[3])
    return c
