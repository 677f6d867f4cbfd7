"""The logits rules of greedy and beam search — `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens`, several EOS ids — restated
on the CPU: what libeilev_hip_rules.so (include/eilev_rules.h, csrc/rules.hip) computes, in pure torch, fp32.  This is to rules.hip what
the second half of eilev_amd/sampling.py is to sample.hip.  Nothing here imports transformers, so the tests can hold it against
transformers' RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor.

Per row, with the history h = [prefix_id if >= 0] + the row's generated ids so far (m = len(h)):
  - repetition penalty: every distinct id of h, x = x < 0 ? x * p : x / p (fp32 multiply and true division);
  - n-gram ban, size n: nothing if m + 1 < n; else for every i in 0 .. m-n with h[i .. i+n-2] == h[m-n+1 .. m-1], id h[i+n-1] -> -inf;
  - min_new: the EOS ids are -inf while step < min_new.
NaN counts as -inf, -0 is +0, ids outside [0, vocab) receive nothing (they still compare as ids inside an n-gram)."""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class RulesSpec:
    """The fields of EilevRulesParams that describe the rules and the stopping rule of a call."""
    repetition_penalty: float = 1.0
    no_repeat_ngram: int = 0
    min_new: int = 0
    eos: tuple = ()
    pad_id: int = 0
    prefix_id: int = -1


def row_histories(ids: torch.Tensor, step: int, prefix_id: int = -1) -> list:
    """Per row of ``ids`` (rows, max_new): prefix_id if >= 0, then ids[b, 0 .. step)."""
    head = [int(prefix_id)] if int(prefix_id) >= 0 else []
    n = max(0, min(int(step), ids.shape[1]))
    return [head + [int(t) for t in row[:n]] for row in ids.tolist()]


def banned_ngram_ids(history, n: int) -> list:
    """The ids that would complete an n-gram already in ``history`` (sorted, distinct; not filtered by any vocabulary)."""
    h = [int(t) for t in history]
    n, m = int(n), len(h)
    if n <= 0 or m + 1 < n:
        return []
    tail = h[m - n + 1:] if n > 1 else []
    return sorted({h[i + n - 1] for i in range(0, m - n + 1) if h[i:i + n - 1] == tail})


def rules_scores(scores: torch.Tensor, history, spec: RulesSpec, step: int = 0) -> torch.Tensor:
    """The rules on ``scores`` (rows, vocab) — logits (greedy search, sampling) or log-probabilities (beam search) — with ``history`` = one
    list of ids per row: (rows, vocab) fp32 on the CPU."""
    x = scores.detach().float().cpu().clone()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    R, V = x.shape
    pen = torch.tensor(float(spec.repetition_penalty), dtype=torch.float32)
    for b in range(R):
        h = history[b] if history is not None else []
        if float(spec.repetition_penalty) != 1.0:
            ids = sorted({int(i) for i in h if 0 <= int(i) < V})
            if ids:
                idx = torch.tensor(ids, dtype=torch.int64)
                v = x[b, idx]
                x[b, idx] = torch.where(v < 0, v * pen, v / pen)
        ban = [i for i in banned_ngram_ids(h, spec.no_repeat_ngram) if 0 <= i < V]
        if ban:
            x[b, torch.tensor(ban, dtype=torch.int64)] = float("-inf")
    if int(step) < int(spec.min_new):
        for e in spec.eos:
            if 0 <= int(e) < V:
                x[:, int(e)] = float("-inf")
    return x + 0.0


def _first_argmax(x: torch.Tensor) -> torch.Tensor:
    """Per row the lowest id that holds the row's maximum; 0 when the maximum is -inf."""
    mx = x.max(dim=-1, keepdim=True).values
    first = (x == mx).int().argmax(dim=-1)
    return torch.where(mx.squeeze(-1) > float("-inf"), first, torch.zeros_like(first))


def rules_select_reference(logits: torch.Tensor, state, finished, tokens, out_tokens, spec: RulesSpec, step_offset: int = 0,
                           finalize: int = 1) -> dict:
    """One eilev_rules_select call on host copies of its buffers (nothing is modified): logits (rows, vocab), state [2], finished (rows,),
    tokens (rows,), out_tokens (rows, max_new).  Returns dict(processed=(rows, vocab) fp32, tokens, out_tokens, finished, state)."""
    out_tokens = out_tokens.detach().cpu().long().clone()
    finished = finished.detach().cpu().to(torch.bool).clone()
    state = [int(v) for v in (state.tolist() if torch.is_tensor(state) else state)]
    R, max_new = out_tokens.shape
    step = state[0] + int(step_offset)
    x = rules_scores(logits, row_histories(out_tokens, step, spec.prefix_id), spec, step)
    tok = torch.where(finished, torch.full((R,), int(spec.pad_id), dtype=torch.int64), _first_argmax(x))
    eos = torch.zeros(R, dtype=torch.bool)
    for e in spec.eos:
        if int(e) >= 0:
            eos |= tok == int(e)
    if 0 <= step < max_new:
        out_tokens[:, step] = tok
    finished = finished | eos
    if finalize:
        state[0] = step + 1
    state[1] = int(bool((~finished).any()))
    return dict(processed=x, tokens=tok.clone(), out_tokens=out_tokens, finished=finished.to(torch.uint8), state=state)


def rules_topk_reference(logits: torch.Tensor, row_score, run_seq: torch.Tensor, cur: int, spec: RulesSpec, keep: int) -> dict:
    """One eilev_rules_topk_logprob call: torch's fp32 log_softmax of ``logits`` (rows, vocab) on the CPU, the rules with the history
    run_seq[r, 0 .. cur) (run_seq: (rows, max_new) or (B, K, max_new)), + row_score, then per row the best ``keep`` — descending, equal
    values by ascending id.  Returns dict(values=(rows, keep) fp32, ids=(rows, keep) int32, processed=(rows, vocab) fp32 without row_score)."""
    x = logits.detach().float().cpu()
    R, V = x.shape
    seq = run_seq.detach().cpu().long().reshape(R, -1)
    proc = rules_scores(torch.log_softmax(x, dim=-1), row_histories(seq, int(cur), spec.prefix_id), spec, int(cur))
    tot = proc if row_score is None else proc + row_score.detach().float().cpu().reshape(R, 1)
    srt, order = torch.sort(tot, dim=-1, descending=True, stable=True)  # stable: equal values keep ascending ids
    return dict(values=srt[:, :keep].contiguous(), ids=order[:, :keep].to(torch.int32).contiguous(), processed=proc)
