"""Multinomial sampling over the HIP decode step (host-side plumbing; the step itself — one token through the language model on the
KV cache — is the HIP kernel path).

What `transformers` does for `generate(do_sample=True, num_beams=1)` [hf generation/utils.py `_sample`; the reference inherits it:
ref:eilev/model/v2.py:312-322, exercised by ref:tests/model/test_model_v2.py:194]: per step the next-token logits go through the
warpers in this order — temperature (logits / T), top-k (keep the k largest, rest -inf), top-p (smallest set of tokens whose
probability mass reaches top_p, at least one kept) — then softmax and one `torch.multinomial` draw per row; rows that produced EOS
emit the pad id from then on; the loop ends when every row has finished.  HF's defaults when only `do_sample=True` is given:
temperature 1.0, top_k 50, top_p 1.0."""
from __future__ import annotations

import torch


def warp_logits(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """(rows, vocab) fp32 -> warped scores (filtered entries are -inf)."""
    scores = logits.float()
    if temperature is not None and temperature != 1.0:
        if temperature <= 0:
            raise ValueError("temperature must be > 0")
        scores = scores / float(temperature)
    if top_k and top_k > 0:
        k = min(int(top_k), scores.shape[-1])
        kth = torch.topk(scores, k, dim=-1).values[..., -1:]
        scores = scores.masked_fill(scores < kth, float("-inf"))
    if top_p is not None and top_p < 1.0:
        if not 0.0 < top_p:
            raise ValueError("top_p must be in (0, 1]")
        srt, idx = torch.sort(scores, dim=-1, descending=False)
        cum = srt.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1.0 - float(top_p))   # the low-probability tail whose mass stays below 1 - top_p
        remove[..., -1:] = False               # min_tokens_to_keep = 1
        scores = scores.masked_fill(remove.scatter(-1, idx, remove), float("-inf"))
    return scores


def eos_list(eos_id) -> list:
    """`eos_token_id` as HF accepts it (None / negative = disabled, an int, or several ids) -> list of ints."""
    if eos_id is None:
        return []
    if isinstance(eos_id, (list, tuple)):
        return [int(e) for e in eos_id if e is not None and int(e) >= 0]
    return [int(eos_id)] if int(eos_id) >= 0 else []


def sample_loop(step, first_logits: torch.Tensor, max_new_tokens: int, eos_id=-1, pad_id: int = 0, temperature: float = 1.0,
                top_k: int = 50, top_p: float = 1.0, generator: torch.Generator | None = None, min_new_tokens: int = 0,
                greedy: bool = False, processors=None, stopping=None, prefix: torch.Tensor | None = None) -> torch.Tensor:
    """`step(next_tokens (R,), row_src (R,)) -> logits (R, vocab)` is the decode step of engine.beam_decode / t5_beam (row_src is the
    identity here).  Returns (R, n) new tokens, n <= max_new_tokens (the loop stops once every row has produced EOS, as HF does).

    ``eos_id`` may be a list (any of the ids finishes a row); ``min_new_tokens`` is HF's MinNewTokensLengthLogitsProcessor (the EOS
    logits are -inf while fewer tokens than that have been generated; applied before the warpers); ``greedy=True`` takes the argmax
    instead of drawing (the host-side form of greedy search used for the stopping rules the captured device step does not cover).

    ``processors``: a `transformers.LogitsProcessorList` (or any callable ``(input_ids, scores) -> scores``) applied to every step's scores
    before the warpers, as hf `_sample` does — `repetition_penalty`, `no_repeat_ngram_size` and user `logits_processor`s arrive here;
    ``stopping``: a `StoppingCriteriaList` / callable ``(input_ids, scores) -> bool per row`` (`stopping_criteria`, `max_time`), a row it
    flags is finished like one that produced EOS.  ``prefix`` (R, P): the ids the processors see in front of the generated ones — none for
    the OPT path (the reference drives the LM with inputs_embeds: hf then starts from an empty id tensor), the start token for T5."""
    R = first_logits.shape[0]
    dev = first_logits.device
    ident = torch.arange(R, device=dev)
    unfinished = torch.ones(R, dtype=torch.bool, device=dev)
    eos = eos_list(eos_id)
    eos_t = torch.tensor(eos, dtype=torch.int64, device=dev) if eos else None
    out = []
    logits = first_logits
    prev = prefix.to(dev, torch.int64) if prefix is not None else torch.zeros((R, 0), dtype=torch.int64, device=dev)
    for t in range(max_new_tokens):
        if processors is not None:
            logits = processors(prev, logits.float())
        if eos_t is not None and t < int(min_new_tokens):
            logits = logits.float().index_fill(-1, eos_t, float("-inf"))
        if greedy:
            nxt = logits.argmax(dim=-1)
        else:
            probs = warp_logits(logits, temperature, top_k, top_p).softmax(dim=-1)
            nxt = torch.multinomial(probs, 1, generator=generator).squeeze(1)
        if eos_t is not None:  # hf `_sample` pads finished rows only when an EOS criterion exists (`has_eos_stopping_criteria`); rows finished
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, int(pad_id)))  # by a custom criterion alone keep their real tokens
        out.append(nxt)
        prev = torch.cat((prev, nxt.view(R, 1)), dim=1)
        if eos_t is not None:
            unfinished = unfinished & ~torch.isin(nxt, eos_t)
        if stopping is not None:
            done = stopping(prev, logits)
            unfinished = unfinished & ~(done.to(dev) if torch.is_tensor(done) else torch.full((R,), bool(done), device=dev))
        if (eos_t is not None or stopping is not None) and not bool(unfinished.any()):
            break
        if t + 1 < max_new_tokens:
            logits = step(nxt, ident)
    return torch.stack(out, dim=1)


# ---- the CPU restatement of libeilev_hip_sample.so (include/eilev_sample.h) -------------------------------------------------------------------
# `sample_select_reference` is one eilev_sample_select call in float64; `keep_bounds` / `draw_ok` are what a test may demand of an
# implementation whose probabilities carry a relative error of at most `tol` (the kernel's are fp32 exponentials held as 40-bit fixed
# point).  This is to sample.hip what eilev_amd/pld.py is to pld.hip.
from dataclasses import dataclass


@dataclass
class SampleSpec:
    """The fields of EilevSampleParams that describe the distribution and the stopping rule."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    min_new: int = 0
    eos: tuple = ()
    pad_id: int = 0
    prefix_id: int = -1


def _as_f32(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


def row_history(out_tokens: torch.Tensor, step: int, prefix_id: int = -1) -> list:
    """The ids the repetition penalty sees per row: prefix_id if >= 0, then out_tokens[b, 0 .. step)."""
    head = [int(prefix_id)] if int(prefix_id) >= 0 else []
    return [head + [int(t) for t in row[:max(0, int(step))]] for row in out_tokens.tolist()]


def processed_scores(logits: torch.Tensor, history, spec: SampleSpec, step: int = 0) -> torch.Tensor:
    """Steps 1 - 3 in fp32, as hf's processors and the kernel evaluate them: repetition penalty (once per distinct id, from the unpenalised
    value), the EOS ban while step < min_new, the temperature.  NaN counts as -inf; -0 is +0.  (rows, vocab) fp32 on the CPU."""
    x = logits.detach().float().cpu().clone()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    R, V = x.shape
    pen = _as_f32(spec.repetition_penalty)
    if float(spec.repetition_penalty) != 1.0 and history is not None:
        for b in range(R):
            ids = sorted({int(i) for i in history[b] if 0 <= int(i) < V})
            if ids:
                idx = torch.tensor(ids, dtype=torch.int64)
                v = x[b, idx]
                x[b, idx] = torch.where(v < 0, v * pen, v / pen)
    if int(step) < int(spec.min_new):
        for e in spec.eos:
            if 0 <= int(e) < V:
                x[:, int(e)] = float("-inf")
    if float(spec.temperature) != 1.0:
        x = x / _as_f32(spec.temperature)
    return x + 0.0


def _topk_keep(x64: torch.Tensor, top_k: int) -> torch.Tensor:
    """The exact top-k rule: finite and >= the k-th largest (its ties stay)."""
    keep = torch.isfinite(x64)
    k = int(top_k or 0)
    if 0 < k < x64.shape[-1]:
        kth = torch.topk(x64, k, dim=-1).values[..., -1:]
        keep = keep & (x64 >= kth)
    return keep


def _tail_masses(x64: torch.Tensor, keep: torch.Tensor):
    """Per token, with float64 probabilities over `keep`: (mass of the kept tokens strictly smaller, mass of those not larger — its ties and
    itself included, its own probability, the row maximum)."""
    neg = torch.full_like(x64, float("-inf"))
    xk = torch.where(keep, x64, neg)
    mx = xk.max(dim=-1, keepdim=True).values
    w = torch.where(keep, torch.exp(xk - mx), torch.zeros_like(xk))
    w = w / w.sum(dim=-1, keepdim=True)
    srt, order = torch.sort(xk, dim=-1)
    cum = torch.cat((torch.zeros_like(mx), torch.gather(w, -1, order).cumsum(dim=-1)), dim=-1)
    lt = torch.gather(cum, -1, torch.searchsorted(srt, xk.contiguous(), right=False))
    le = torch.gather(cum, -1, torch.searchsorted(srt, xk.contiguous(), right=True))
    return lt, le, w, mx


def keep_bounds(logits: torch.Tensor, history, spec: SampleSpec, tol: float, step: int = 0):
    """(must_keep, may_keep), bool (rows, vocab): every implementation of steps 1 - 5 whose masses are within `tol` of the exact ones keeps
    all of must_keep and nothing outside may_keep.  The top-k rule is exact.  Top-p: a token must stay when the mass of the tokens not
    larger than it, counted with itself first among its ties, exceeds 1 - top_p + tol; it may stay when that mass with all its ties
    counted exceeds 1 - top_p - tol.  The largest value always stays."""
    x = processed_scores(logits, history, spec, step).double()
    keep = _topk_keep(x, spec.top_k)
    if float(spec.top_p) >= 1.0:
        return keep, keep.clone()
    lt, le, w, mx = _tail_masses(x, keep)
    cut = 1.0 - float(_as_f32(spec.top_p))
    top = keep & (x == mx)
    must = keep & (((lt + w) > cut + tol) | top)
    may = keep & ((le > cut - tol) | top)
    return must, may


def draw_ok(kept: torch.Tensor, scores: torch.Tensor, u: torch.Tensor, ids: torch.Tensor, tol: float) -> torch.Tensor:
    """Per row: is `ids[b]` a valid inverse-CDF draw for u[b] over the set `kept` (bool (rows, vocab)) of `scores` (the processed scores)?
    With float64 probabilities over `kept`, in token-id order: the id is kept and CDF(id - 1) - tol <= u <= CDF(id) + tol."""
    x = scores.detach().double().cpu()
    kept = kept.cpu()
    xk = torch.where(kept, x, torch.full_like(x, float("-inf")))
    w = torch.exp(xk - xk.max(dim=-1, keepdim=True).values)
    cdf = (w / w.sum(dim=-1, keepdim=True)).cumsum(dim=-1)
    ids = ids.detach().cpu().long().view(-1, 1)
    hi = torch.gather(cdf, -1, ids).squeeze(1)
    lo = torch.where(ids.squeeze(1) > 0, torch.gather(cdf, -1, (ids - 1).clamp(min=0)).squeeze(1), torch.zeros_like(hi))
    u = u.detach().double().cpu().view(-1)
    return torch.gather(kept, -1, ids).squeeze(1) & (lo - tol <= u) & (u <= hi + tol)


def sample_select_reference(logits: torch.Tensor, uniforms: torch.Tensor, state, finished, tokens, out_tokens, spec: SampleSpec,
                            step_offset: int = 0, finalize: int = 1) -> dict:
    """One eilev_sample_select call in float64 on host copies of its buffers (nothing is modified): logits (rows, vocab), uniforms
    (max_new, rows), state [2], finished (rows,), tokens (rows,), out_tokens (rows, max_new).  Returns dict(scores=(rows, vocab) float64 after
    step 5 with -inf where removed, drawn=(rows,) the ids drawn before padding, tokens, out_tokens, finished, state)."""
    out_tokens = out_tokens.detach().cpu().long().clone()
    finished = finished.detach().cpu().to(torch.bool).clone()
    state = [int(v) for v in (state.tolist() if torch.is_tensor(state) else state)]
    R, max_new = out_tokens.shape
    step = state[0] + int(step_offset)
    x = processed_scores(logits, row_history(out_tokens, min(step, max_new), spec.prefix_id), spec, step).double()
    keep = _topk_keep(x, spec.top_k)
    if float(spec.top_p) < 1.0:
        lt, le, w, mx = _tail_masses(x, keep)
        keep = keep & ((le > 1.0 - float(_as_f32(spec.top_p))) | (x == mx))
    scores = torch.where(keep, x, torch.full_like(x, float("-inf")))
    w = torch.where(keep, torch.exp(scores - scores.max(dim=-1, keepdim=True).values), torch.zeros_like(scores))
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)  # (a row without a finite score)
    cdf = w.cumsum(dim=-1)
    u = uniforms.detach().cpu().double()[step] if 0 <= step < max_new else torch.zeros(R, dtype=torch.float64)
    over = cdf > (u * cdf[:, -1]).view(R, 1)
    V = x.shape[1]
    last_kept = (V - 1) - torch.flip(keep, dims=(-1,)).int().argmax(dim=-1)
    drawn = torch.where(over.any(dim=-1), over.int().argmax(dim=-1), last_kept)
    drawn = torch.where(keep.any(dim=-1), drawn, torch.zeros_like(drawn))
    tok = torch.where(finished, torch.full_like(drawn, int(spec.pad_id)), drawn)
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
    return dict(scores=scores, drawn=drawn, tokens=tok.clone(), out_tokens=out_tokens, finished=finished.to(torch.uint8), state=state)
