"""Which decoding route a call takes: decided here, once, for OPT and flan-t5, without a device and without the library.

``plan_decode`` is the only place that chooses between the captured greedy step, the device draw, the device rules, the fused beam loop
and the host loops (eilev_amd/sampling.py, beam.py).  HipEngine.beam_decode / t5_beam execute the plan they get; generate() asks for
the same plan before any encode and derives its fp8 refusal from it.
"""
from __future__ import annotations

from typing import NamedTuple

from . import abi
from .sampling import eos_list

CAPTURED = ("greedy", "sample_device", "rules_device")  # the routes of num_beams == 1 that end in one captured decode step
SWITCHES = ("device_sampling", "device_rules", "beam_device_loop", "beam_topk_kernel", "beam_advance_kernel")


class Caps(NamedTuple):
    """What the machinery can take: the language model, its vocabulary, OPT's head size, the engine's switches."""
    lm: str  # "opt" | "t5"
    vocab: int
    head_size: int | None = None
    device_sampling: bool = True
    device_rules: bool = True
    beam_device_loop: bool = True
    beam_topk_kernel: bool = True
    beam_advance_kernel: bool = True
    t5beam_supported: bool = False

    @classmethod
    def of(cls, engine):
        return cls.of_config(engine.config, engine)

    @classmethod
    def of_config(cls, config, engine=None):
        """From a configuration alone: every switch at its constructor default, or as ``engine`` (one that exists) has it."""
        t = config.text_config
        switches = {s: bool(getattr(engine, s, True)) for s in SWITCHES}
        if getattr(t, "model_type", "opt") == "t5":
            return cls("t5", int(t.vocab_size), t5beam_supported=int(t.d_kv) == 64, **switches)
        heads = int(getattr(t, "num_attention_heads", 0) or 0)
        return cls("opt", int(t.vocab_size), int(t.hidden_size) // heads if heads else None, **switches)


class Plan(NamedTuple):
    route: str               # greedy | sample_device | rules_device | beam_device | sample_host | search_host
    dev_kw: dict | None      # the device keyword set: of sample_*_device, of rules_*_device, of the rules inside the fused beam loop
    sampler: dict | None     # sampler and rules in the form the host loops take: the numbers as transformers' processors again
    rules: dict | None
    with_rules: bool         # a greedy / beam search call that carries any rule at all (a plain one leaves rules_stats alone)
    topk_ok: bool            # the fused beam loop: eilev_topk_logprob takes the call, and so does eilev_beam_advance
    advance_ok: bool
    loop: str | None         # the host loop of a host route: "sample_loop" | "beam_search"
    chunk: int | None        # samples per call where a call of more decode rows than 32 runs in parts (None: it never does)
    pad_from_eos: bool       # flan-t5 beams: a pad id of 0 is falsy to hf, finished hypotheses are filled with the first EOS id
    start_prefix: bool       # flan-t5 host loop: the processors see the decoder start token in front of the ids
    host_reasons: tuple      # on a host or beam route: every condition that keeps the call off the captured routes
    switches_off: tuple      # ... and the switches behind its "switch off"


def host_processors(pen, ngram, more=None):
    """The numeric rules as transformers' own processors, in hf's order, in front of the caller's."""
    from transformers import LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    lst = LogitsProcessorList()
    if pen != 1.0:
        lst.append(RepetitionPenaltyLogitsProcessor(penalty=pen))
    if ngram:
        lst.append(NoRepeatNGramLogitsProcessor(ngram))
    lst.extend(list(more or []))
    return lst


def _rule_numbers(carrier, rules):
    """Pops the numbers repetition_penalty / no_repeat_ngram_size from ``carrier`` (the plan's own copy of the dict that carries them).
    Returns (pen, ngram, host_only, to_host): host_only — ``rules`` holds a user processor or a stopping criterion; to_host(rules) — the
    rules with the numbers as transformers' processors again."""
    pen = float(carrier.pop("repetition_penalty", None) or 1.0)
    ngram = int(carrier.pop("no_repeat_ngram_size", None) or 0)
    host_only = bool(rules) and (rules.get("processors") is not None or rules.get("stopping") is not None)

    def to_host(rules):
        if pen != 1.0 or ngram:
            rules = dict(rules or {})
            rules["processors"] = host_processors(pen, ngram, rules.get("processors"))
            rules.setdefault("stopping", None)
        return rules

    return pen, ngram, host_only, to_host


def beam_kernels_ok(caps, num_beams, n_eos, gen_cap):
    """(topk_ok, advance_ok) of a beam search call: the per-row top-k kernel takes it (its vocabulary, `keep` candidates per row), and so
    does the kernel that advances the hypotheses."""
    keep = max(2, 1 + n_eos) * num_beams
    topk_ok = caps.beam_topk_kernel and caps.vocab <= 65536 and caps.vocab % 4 == 0 and keep <= 64
    advance_ok = topk_ok and caps.beam_advance_kernel and num_beams * keep <= 2048 and gen_cap * num_beams <= 2048 and n_eos <= 8
    return topk_ok, advance_ok


def plan_decode(caps, num_beams, sampler, rules, eos_ids, min_new_tokens, max_new_tokens, trace: bool, kv_dtype="bf16", in_search_loop=False) -> Plan:
    """The route of one decoding call.  ``sampler``: None (greedy / beam search), dict(greedy=True, ...) (greedy search asked of the
    sampling loop: how a num_beams == 1 call carries rules) or the warpers of a drawing call; ``rules``: dict(processors=, stopping=,
    prefix=, fill_id=) and the numbers repetition_penalty= / no_repeat_ngram_size=, which a drawing num_beams == 1 call carries in its
    sampler.  ``in_search_loop``: the caller is beam_decode / t5_beam itself, so a plain greedy call — which generate() sends to
    greedy_decode / t5_greedy, route "greedy" — stays in the host loop it was asked of.  ``kv_dtype`` does not move a call: the captured
    routes serve "fp8", and the callers refuse it on every other route."""
    t5, vocab = caps.lm == "t5", caps.vocab
    n_eos = len(eos_list(eos_ids))
    drawing = sampler is not None and not sampler.get("greedy")
    topk_ok, advance_ok = beam_kernels_ok(caps, num_beams, n_eos, max(1, max_new_tokens))
    # the fused beam loop: plain beam search and the numeric rules; flan-t5's takes head size 64 and at most 32 beams
    device_loop = (sampler is None and num_beams > 1 and caps.beam_device_loop and
                   (not t5 or (num_beams <= 32 and max_new_tokens > 0 and caps.t5beam_supported)))
    dev_kw, with_rules, host_sampler = None, False, sampler
    if drawing and num_beams == 1:
        host_sampler = dict(sampler)
        pen, ngram, host_only, to_host = _rule_numbers(host_sampler, rules)
        if (caps.device_sampling and not host_only and not trace and n_eos <= abi.SAMPLE_MAX_EOS and abi.sample_supported(vocab) and
                (not ngram or abi.rules_supported(vocab))):
            dev_kw = dict(temperature=host_sampler.get("temperature", 1.0), top_k=host_sampler.get("top_k", 50), top_p=host_sampler.get("top_p", 1.0),
                          repetition_penalty=pen, min_new_tokens=host_sampler.get("min_new_tokens", 0), generator=host_sampler.get("generator"))
            if ngram:
                dev_kw["no_repeat_ngram_size"] = ngram
            route, host_rules = "sample_device", rules
        else:
            route, host_rules = "sample_host", to_host(rules)
    else:
        # greedy search (num_beams == 1, a greedy sampler) and beam search: the rules run on the device when nothing below says no and, for
        # beams, when the search takes the fused form; beam-search sampling keeps the host loop
        min_new = int(min_new_tokens) if sampler is None else int(sampler.get("min_new_tokens", 0) or 0)
        greedy1 = sampler is not None and num_beams == 1
        host_rules = dict(rules or {})
        pen, ngram, host_only, to_host = _rule_numbers(host_rules, host_rules)
        with_rules = pen != 1.0 or ngram > 0 or min_new > 0 or n_eos > 1 or host_only
        if (with_rules and (greedy1 or (device_loop and advance_ok)) and caps.device_rules and not host_only and not trace and
                n_eos <= abi.RULES_MAX_EOS and abi.rules_supported(vocab)):
            dev_kw, host_rules = dict(repetition_penalty=pen, no_repeat_ngram_size=ngram, min_new_tokens=min_new), (host_rules or None)
        else:
            host_rules = to_host(host_rules) or None
        if dev_kw is not None and greedy1:
            route = "rules_device"
        elif device_loop and (dev_kw is not None or (not host_rules and int(min_new_tokens) == 0)) and not trace:
            route = "beam_device"
        elif num_beams == 1 and not with_rules and not trace and not in_search_loop:
            route = "greedy"
        else:
            route = "search_host"
    loop = None if route in CAPTURED + ("beam_device",) else "sample_loop" if sampler is not None and num_beams == 1 else "beam_search"
    # more decode rows than 32: OPT runs every route that does not return above sample group by sample group, flan-t5 its device loop only
    chunk = max(1, 32 // num_beams) if route == "beam_device" or (not t5 and loop is not None) else None
    start_prefix = bool(t5 and loop == "sample_loop" and host_rules and host_rules.get("processors") is not None and host_rules.get("prefix") is None)
    reasons, off = ((), ()) if route in CAPTURED else _host_reasons(caps, num_beams, sampler, rules, drawing, n_eos, min_new_tokens, trace)
    return Plan(route, dev_kw, host_sampler, host_rules, with_rules, topk_ok, advance_ok, loop, chunk, t5 and num_beams > 1, start_prefix, reasons, off)


def _host_reasons(caps, num_beams, sampler, rules, drawing, n_eos, min_new_tokens, trace):
    """Every condition that keeps the call off the captured routes, by name, and the switches that are off for it."""
    carrier = dict(rules or {}, **(sampler or {}))  # (the numbers ride in the sampler of a drawing call, else in the rules)
    min_new = int(min_new_tokens) or int((sampler or {}).get("min_new_tokens", 0) or 0)
    procs, crit = bool(rules) and rules.get("processors") is not None, bool(rules) and rules.get("stopping") is not None
    any_rule = (float(carrier.get("repetition_penalty") or 1.0) != 1.0 or bool(carrier.get("no_repeat_ngram_size")) or min_new > 0 or n_eos > 1 or
                procs or crit)
    off = tuple(s for s, on in (("device_sampling", drawing), ("device_rules", not drawing and any_rule),
                                ("beam_device_loop", num_beams > 1), ("beam_topk_kernel", num_beams > 1), ("beam_advance_kernel", num_beams > 1))
                if on and not getattr(caps, s))
    named = (("user processor", procs), ("stopping criterion", crit), ("trace", bool(trace)),
             ("more than 8 EOS ids", n_eos > min(abi.SAMPLE_MAX_EOS, abi.RULES_MAX_EOS)),
             ("vocabulary not taken", (drawing or any_rule) and not (abi.sample_supported(caps.vocab) and abi.rules_supported(caps.vocab))),
             ("switch off", bool(off)), ("beams", num_beams > 1))
    reasons = tuple(n for n, on in named if on)
    return (reasons or ("plain search",)), off  # (one row, no rule, asked of beam_decode / t5_beam directly: generate() never does)
