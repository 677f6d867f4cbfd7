"""Which decoding route every kind of generate() call takes, recorded on the CPU without the built library.

Drives the real ``VideoBlipForConditionalGeneration.generate`` and the real engine entry points ``beam_decode``, ``t5_beam``,
``sample_decode`` and ``t5_sample`` over a grid of requests.  The engine is a HipEngine subclass made with ``object.__new__``: real
``abi.Dims``, a stand-in ``lib`` whose size queries return a small integer, and prefill / encoder stubs that return zero tensors of the
right shape.  The LEAVES — the functions a route ends in — are replaced by recorders: each notes its name and its arguments reduced to JSON
(tensors to dtype + shape, processor lists to class names, generators to None / "given", functions to "fn"), leaves the stats record the
real function leaves and returns zero ids of the real shape, so a call that runs in parts records every part.  A call that raises records
the exception's type and message.

    python tools/route_table.py --write tests/golden/route_table.json.gz   # record (done once, at the commit before eilev_amd/route.py)
    python tools/route_table.py --check tests/golden/route_table.json.gz   # replay and compare

The record is gzip'd JSON (5.5 MB as text): ``load_table`` reads it.

tests/test_route_table.py replays the same grid.  The tool asserts itself that the table holds every leaf, every route, every refusal
and every condition that keeps a call off the device, for both language models where the model has it: a grid that loses one does not pass.
"""
from __future__ import annotations

import argparse
import gzip
import hashlib
import inspect
import itertools
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eilev_amd import abi, beam, configs, sampling  # noqa: E402
from eilev_amd.engine import HipEngine  # noqa: E402
from eilev_amd.model import v2  # noqa: E402

MAX_NEW = 4
SWITCHES = ("device_sampling", "device_rules", "beam_device_loop", "beam_topk_kernel", "beam_advance_kernel")
# the leaf a call ends in names its route
ROUTE_OF_LEAF = dict(_select_decode_device="greedy", _t5_select_device="greedy", sample_decode_device="sample_device",
                     t5_sample_device="sample_device", rules_decode_device="rules_device", t5_rules_device="rules_device",
                     _beam_device_loop="beam_device", _t5_beam_device="beam_device", sample_loop="sample_host", beam_search="search_host",
                     greedy_lookup_decode="greedy", t5_greedy_lookup="greedy", greedy_decode_context="greedy")
ROUTES = ("greedy", "sample_device", "rules_device", "beam_device", "sample_host", "search_host")
HOST_REASONS = ("user processor", "stopping criterion", "trace", "more than 8 EOS ids", "vocabulary not taken", "switch off", "beams")
FP8_CAUSES = ("the flan-t5 language model", "num_beams > 1", "context=", "prompt_lookup_num_tokens", "a head size other than 80 / 128",
              "logits_processor (a host loop)", "stopping criteria / max_time (a host loop)", "more than 8 EOS ids (a host loop)",
              "a vocabulary the device selection does not take (a host loop)", "device_sampling off (a host loop)",
              "device_rules off (a host loop)")
REFUSALS = ("num_beams > 32", "kv_cache_dtype='fp8' is built for the captured device routes only", "trace: at most 32 decode rows",
            "prefix ids with more than 32 decode rows", "generate(kv_cache_dtype='fp8') with")
EOS_IDS = {0: [], 1: [2], 2: [2, 3], 9: list(range(2, 11))}


# ---- the engine and the model without a GPU ---------------------------------------------------------------
class _SizeLib:
    """Every size query answers a small integer that grows with its integer arguments (a cache of more rows is larger)."""

    def __getattr__(self, name):
        def size(*args):
            n = 64
            for a in args:
                if isinstance(a, int) and a > 0:
                    n *= a
            return n
        return size


def reduce(x):
    """An argument as JSON."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, torch.Tensor):
        return f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}"
    if isinstance(x, torch.Generator):
        return "given"
    if isinstance(x, dict):
        return {str(k): reduce(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        if len(x) and not all(isinstance(e, (int, float, str, torch.Tensor, list, tuple, dict, type(None))) for e in x):
            return [type(e).__name__ for e in x]  # a processor / criteria list: its classes, in order
        return [reduce(e) for e in x]
    if callable(x):
        return "fn"
    return type(x).__name__


class StubEngine(HipEngine):
    """HipEngine with the device taken away: everything up to a leaf runs as written."""

    def prefill(self, inputs_embeds, attention_mask, kv_cache=None, kv_capacity=None, **kw):
        B = inputs_embeds.shape[0]
        return torch.zeros((B, self.dims.vocab)), None, torch.zeros(8, dtype=torch.uint8)

    def t5_encode(self, inputs_embeds, attention_mask):
        return torch.zeros_like(inputs_embeds)

    def t5_cross_kv(self, enc_out):
        return torch.zeros(2 * self.t5dims.dec_layers * enc_out.shape[0] * 8, dtype=torch.uint8)

    def t5_decode(self, dec_ids, enc_mask, past_len, self_kv, cap, cross_kv, enc_len):
        return torch.zeros((dec_ids.shape[0], dec_ids.shape[1], self.t5dims.vocab))

    def _workspace(self, tag, nbytes):
        return torch.zeros(8, dtype=torch.uint8)


def _ids(rows, n, start=False):
    return torch.zeros((int(rows), max(0, int(n)) + (1 if start else 0)), dtype=torch.int64)


def _leaf_result(eng, name, a):
    """What the real leaf leaves behind: its stats record and ids of its shape."""
    n = a.get("max_new_tokens", MAX_NEW)
    dev = dict(path="device", steps=max(0, int(n)))
    if name in ("sample_decode_device", "t5_sample_device"):
        eng.sample_stats = dev
        return _ids(a["inputs_embeds"].shape[0], n, name.startswith("t5"))
    if name in ("rules_decode_device", "t5_rules_device"):
        eng.rules_stats = dev
        return _ids(a["inputs_embeds"].shape[0], n, name.startswith("t5"))
    if name in ("_select_decode_device", "_t5_select_device"):
        return _ids(a["inputs_embeds"].shape[0], n)
    if name == "_beam_device_loop":
        if a["rules_kw"] is not None:
            eng.rules_stats = dev
        return _ids(a["B"] * a["num_return_sequences"], n)
    if name == "_t5_beam_device":
        eng.t5_beam_stats = dev
        return _ids(a["inputs_embeds"].shape[0] * a["num_return_sequences"], n, True)
    if name == "greedy_lookup_decode":
        eng.pld_stats = dict(verify=0, single=0, accepted=0)
        return _ids(1, n)
    if name == "t5_greedy_lookup":
        eng.pld_stats = dict(verify=0, single=0, accepted=0)
        return _ids(1, n, True)
    if name == "greedy_decode_context":
        eng.context_stats = dict(path="shared", rows=a["new_embeds"].shape[0], prefix=a["ctx"].P, new=a["new_embeds"].shape[1], steps=int(n))
        return _ids(a["new_embeds"].shape[0], n)
    if name == "sample_loop":
        return _ids(a["first_logits"].shape[0], n)
    if name == "beam_search":
        return _ids(a["batch"] * a["num_return_sequences"], n)
    raise KeyError(name)


ENGINE_LEAVES = ("sample_decode_device", "rules_decode_device", "t5_sample_device", "t5_rules_device", "_select_decode_device",
                 "_t5_select_device", "_beam_device_loop", "_t5_beam_device", "greedy_lookup_decode", "t5_greedy_lookup",
                 "greedy_decode_context")
MODULE_LEAVES = ((sampling, "sample_loop"), (beam, "beam_search"))
LEAVES = ENGINE_LEAVES + tuple(n for _, n in MODULE_LEAVES)


class Recorder:
    """``with Recorder() as rec``: the leaves are replaced inside the block; ``rec.calls`` receives (leaf, arguments by name)."""

    def __enter__(self):
        self.calls = []
        self.engine = None  # the engine of the call in progress (the module leaves have no self)
        self._saved = [(mod, name, getattr(mod, name)) for mod, name in MODULE_LEAVES + ((abi, "load_kv8"),)]
        for name in ENGINE_LEAVES:
            setattr(StubEngine, name, self._wrap(getattr(HipEngine, name), name, True))
        for mod, name in MODULE_LEAVES:
            setattr(mod, name, self._wrap(getattr(mod, name), name, False))
        abi.load_kv8 = lambda: _SizeLib()  # (the late fp8 refusal of beam_decode asks for the library before it refuses)
        return self

    def __exit__(self, *exc):
        for mod, name, real in self._saved:
            setattr(mod, name, real)
        for name in ENGINE_LEAVES:
            delattr(StubEngine, name)

    def _wrap(self, real, name, method):
        sig = inspect.signature(real)

        def leaf(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            a = dict(bound.arguments)
            if method:
                a.pop("self")
            flat = {k: v for k, v in a.items() if k != "kw"}
            flat.update(a.get("kw", {}))
            self.calls.append([name, reduce(flat)])
            return _leaf_result(self.engine, name, flat)
        return leaf


def make_engine(lm, vocab, head_ok=True):
    """(config, engine): the tiny configurations with the vocabulary of the grid point.  ``head_ok``: OPT head size 80 (the fp8 KV cache
    and the shared prefix take it) instead of tiny's 8; flan-t5 head size 64 (the device beam loop takes it) instead of 8."""
    cfg = configs.blip2_config("tiny_t5" if lm == "t5" else "tiny")
    t = cfg.text_config
    t.vocab_size = vocab
    if head_ok and lm == "opt":
        t.hidden_size = t.word_embed_proj_dim = 160
    if head_ok and lm == "t5":
        t.d_kv = 64
    eng = object.__new__(StubEngine)
    eng.config, eng.lib, eng.device, eng.is_t5 = cfg, _SizeLib(), torch.device("cpu"), lm == "t5"
    eng.dims = abi.dims_from_config(cfg)
    eng.t5dims = abi.t5_dims_from_config(cfg) if lm == "t5" else None
    eng.pack = SimpleNamespace(opt=None, t5=None, embed_tokens=None)
    eng.timing, eng._decode_warm, eng._dec_cache, eng._ctx_cache = None, False, None, None
    eng.beam_capture = False
    for s in SWITCHES:
        setattr(eng, s, True)
    return cfg, eng


_MODELS = {}


def make_model(lm, vocab, head_ok=True):
    """(model, engine): a real VideoBlipForConditionalGeneration on the CPU whose engine() is the stub and whose _encode counts."""
    key = (lm, vocab, head_ok)
    if key not in _MODELS:
        cfg, eng = make_engine(lm, vocab, head_ok)
        with torch.device("meta"):
            model = v2.VideoBlipForConditionalGeneration(cfg)
        hip_key = (v2._params_key(model), "bf16", True)
        model._hip = (hip_key, eng)
        model.engine = lambda: eng
        model.encodes = 0
        width = cfg.text_config.d_model if lm == "t5" else cfg.text_config.hidden_size

        def encode(pixel_values, input_ids, video_input_mask, vision_debug=(False, False)):
            model.encodes += 1
            return torch.zeros(tuple(input_ids.shape) + (width,)), None, None

        model._encode = encode
        _MODELS[key] = (model, eng)
    return _MODELS[key]


# ---- a grid point -----------------------------------------------------------------------------------------
class _Proc:  # a user logits processor
    def __call__(self, input_ids, scores):
        return scores


class _Crit:  # a user stopping criterion
    def __call__(self, input_ids, scores, **kw):
        return False


def point(lm="opt", beams=1, mode="none", numbers="none", host="none", eos=1, min_new=0, vocab=1000, trace=False, kv="bf16", rows=2, off=None,
          entry="generate", extra=None):
    return dict(lm=lm, beams=beams, mode=mode, numbers=numbers, host=host, eos=eos, min_new=min_new, vocab=vocab, trace=trace, kv=kv, rows=rows,
                off=off, entry=entry, extra=extra)


def key_of(p):
    return "|".join(str(p[k]) for k in ("entry", "lm", "beams", "mode", "numbers", "host", "eos", "min_new", "vocab", "trace", "kv", "rows", "off", "extra"))


def _numbers(p):
    return {k: v for k, v, on in (("repetition_penalty", 1.3, p["numbers"] in ("pen", "both")),
                                  ("no_repeat_ngram_size", 2, p["numbers"] in ("ngram", "both"))) if on}


def generate_kwargs(p):
    kw = dict(max_new_tokens=MAX_NEW, num_beams=p["beams"], eos_token_id=list(EOS_IDS[p["eos"]]), **_numbers(p))
    if p["mode"] == "draw":
        kw.update(do_sample=True, temperature=0.7, top_k=5, top_p=0.9)
    if p["min_new"]:
        kw["min_new_tokens"] = p["min_new"]
    if p["host"] == "proc":
        kw["logits_processor"] = [_Proc()]
    if p["host"] == "crit":
        kw["stopping_criteria"] = [_Crit()]
    if p["kv"] == "fp8":
        kw["kv_cache_dtype"] = "fp8"
    if p["extra"] == "lookup":
        kw["prompt_lookup_num_tokens"] = 3
    if p["extra"] == "max_time":
        kw["max_time"] = 5.0
    return kw


def engine_args(p):
    """beam_decode / t5_beam arguments in the form generate() hands them over: the numbers in the sampler of a num_beams == 1 sampling
    call, else in the rules."""
    from transformers import LogitsProcessorList, StoppingCriteriaList

    eos = EOS_IDS[p["eos"]]
    eos_id = eos if len(eos) > 1 else (eos[0] if eos else -1)
    sampler = {"none": None, "greedy": dict(greedy=True), "draw": dict(temperature=0.7, top_k=5, top_p=0.9, generator=None)}[p["mode"]]
    nums = _numbers(p)
    if sampler is not None and p["beams"] == 1:
        sampler["min_new_tokens"] = p["min_new"]
        if p["mode"] == "draw":
            sampler.update(nums)
            nums = {}
    rules = None
    if p["host"] != "none" or nums:
        rules = dict(processors=LogitsProcessorList([_Proc()]) if p["host"] == "proc" else None,
                     stopping=StoppingCriteriaList([_Crit()]) if p["host"] == "crit" else None, **nums)
    return eos_id, sampler, rules


def run_point(p, rec):
    """One grid point -> its table entry."""
    head_ok = p["off"] not in ("head_size", "t5beam_supported")
    model, eng = make_model(p["lm"], p["vocab"], head_ok)
    for s in SWITCHES:
        setattr(eng, s, p["off"] != s)
    eng.sample_stats = eng.rules_stats = eng.t5_beam_stats = eng.pld_stats = eng.context_stats = None
    eng._decode_warm = False
    rec.calls, rec.engine, model.encodes = [], eng, 0
    L = 5
    ids = torch.ones((p["rows"], L), dtype=torch.int64)
    am = torch.ones((p["rows"], L), dtype=torch.int64)
    width = eng.t5dims.d_model if p["lm"] == "t5" else eng.dims.t_hidden
    emb = torch.zeros((p["rows"], L, width))
    entry = {}
    try:
        if p["entry"] == "generate":
            kw = generate_kwargs(p)
            if p["extra"] == "context":
                kw["context"] = v2.VideoContext(SimpleNamespace(P=3), torch.ones((1, 3), dtype=torch.int64), model._hip[0])
            out = model.generate(ids, attention_mask=am, **kw)
        elif p["entry"] == "sample":  # the thin wrappers sample_decode / t5_sample
            eos = EOS_IDS[p["eos"]]
            fn = eng.t5_sample if p["lm"] == "t5" else eng.sample_decode
            out = fn(emb, am, MAX_NEW, eos_id=eos if len(eos) > 1 else (eos[0] if eos else -1), temperature=0.7, top_k=5, top_p=0.9,
                     repetition_penalty=_numbers(p).get("repetition_penalty", 1.0), min_new_tokens=p["min_new"])
        else:
            eos_id, sampler, rules = engine_args(p)
            if p["lm"] == "t5":
                out = eng.t5_beam(emb, am, MAX_NEW, p["beams"], 1.0, eos_id=eos_id, pad_id=0, start_id=0, sampler=sampler,
                                  min_new_tokens=p["min_new"], rules=rules)
            else:
                if p["extra"] == "prefix" and rules is not None:
                    rules["prefix"] = torch.zeros((p["rows"], 1), dtype=torch.int64)
                out = eng.beam_decode(emb, am, MAX_NEW, p["beams"], 1.0, eos_id=eos_id, pad_id=1, sampler=sampler, min_new_tokens=p["min_new"],
                                      trace=[] if p["trace"] else None, rules=rules, kv_dtype=p["kv"])
        entry["returns"] = reduce(out)
    except Exception as e:  # noqa: BLE001 (the table records every refusal)
        entry["raises"] = [type(e).__name__, str(e)]
    entry["calls"] = rec.calls
    if p["entry"] == "generate":
        entry["encodes"] = model.encodes
    stats = {k: getattr(eng, k) for k in ("sample_stats", "rules_stats", "t5_beam_stats") if getattr(eng, k) is not None}
    if stats:
        entry["stats"] = stats
    return entry


def route_of(entry):
    """The route of a table entry: named by the last leaf it reached (None: the call was refused, or returned before any leaf)."""
    if not entry["calls"]:
        return None
    leaf, args = entry["calls"][-1]
    return "search_host" if leaf == "sample_loop" and args.get("greedy") else ROUTE_OF_LEAF[leaf]  # (greedy search with host rules)


def grid():
    """The grid points, in a fixed order.  All switches on: the full product of the request axes, except that of num_beams x rows the
    pair (33, 40) is left out (1320 decode rows of stub logits per point).  A switch off: the product over the axes that switch can
    affect."""
    pts = []
    shape = ((1, 2), (1, 40), (3, 2), (3, 40), (33, 2))
    for lm, (beams, rows), numbers, host, eos, min_new, vocab in itertools.product(
            ("opt", "t5"), shape, ("none", "pen", "ngram", "both"), ("none", "proc", "crit"), (0, 1, 2, 9), (0, 2), (1000, 1002)):
        for kv in (("bf16", "fp8") if lm == "opt" else ("bf16",)):
            for mode in ("none", "draw"):
                pts.append(point(lm, beams, mode, numbers, host, eos, min_new, vocab, False, kv, rows, entry="generate"))
            if lm == "t5" and kv == "bf16" and beams == 1 and rows == 2 and vocab == 1000 and host == "none":
                pts.append(point(lm, beams, "none", numbers, host, eos, min_new, vocab, False, "fp8", rows, entry="generate"))
            for mode in ("none", "greedy", "draw"):
                for trace in ((False, True) if lm == "opt" else (False,)):
                    pts.append(point(lm, beams, mode, numbers, host, eos, min_new, vocab, trace, kv, rows, entry="engine"))
    for lm, numbers, eos, min_new, vocab, rows in itertools.product(("opt", "t5"), ("none", "pen"), (0, 1, 2, 9), (0, 2), (1000, 1002), (2, 40)):
        pts.append(point(lm, 1, "draw", numbers, "none", eos, min_new, vocab, rows=rows, entry="sample"))
    # every switch off singly, over what it can affect
    for off, lm, beams, numbers, eos, kv in itertools.product(SWITCHES + ("head_size", "t5beam_supported"), ("opt", "t5"), (1, 3),
                                                              ("none", "pen", "ngram", "both"), (1, 2, 9), ("bf16", "fp8")):
        if (off == "head_size" and lm == "t5") or (off == "t5beam_supported" and (lm == "opt" or beams == 1)) or (lm == "t5" and kv == "fp8"):
            continue
        if off.startswith("beam_") and (beams == 1 or kv == "fp8"):
            continue
        if off in ("device_sampling", "device_rules") and beams > 1 and (off == "device_sampling" or kv == "fp8"):
            continue
        modes = ("draw",) if off == "device_sampling" else ("none", "greedy") if off == "device_rules" else ("none", "draw")
        for mode in modes:
            if mode != "greedy":
                pts.append(point(lm, beams, mode, numbers, "none", eos, 0, 1000, False, kv, 2, off, "generate"))
            pts.append(point(lm, beams, mode, numbers, "none", eos, 0, 1000, False, kv, 2, off, "engine"))
    # what lies beside the product: prompt lookup, a shared context, max_time, prefix ids with more than 32 rows
    for lm in ("opt", "t5"):
        for kv in ("bf16", "fp8"):
            pts.append(point(lm, kv=kv, rows=1, extra="lookup"))
            pts.append(point(lm, kv=kv, extra="context"))
            pts.append(point(lm, kv=kv, extra="max_time"))
    pts.append(point("opt", 3, numbers="pen", host="proc", rows=40, entry="engine", extra="prefix"))
    return pts


def build_table(points=None, observe=None):
    """The table of ``points``: the distinct outcomes and, point by point, which one it is.  ``observe(point, entry)``: called after each."""
    points = grid() if points is None else points
    outcomes, index, rows = [], {}, []
    with Recorder() as rec:
        for p in points:
            e = run_point(p, rec)
            if observe is not None:
                observe(p, e)
            s = json.dumps(e, sort_keys=True)
            if s not in index:
                index[s] = len(outcomes)
                outcomes.append(e)
            rows.append(index[s])
    keys = [key_of(p) for p in points]
    return dict(keys_sha256=hashlib.sha256("\n".join(keys).encode()).hexdigest(), outcomes=outcomes, points=rows)


def fp8_causes(entry):
    msg = entry.get("raises", ["", ""])[1]
    if not msg.startswith("generate(kv_cache_dtype='fp8') with "):
        return []
    return msg[len("generate(kv_cache_dtype='fp8') with "):].split(" is not built")[0].split(", ")


def assert_covers(points, table):
    """The table holds every leaf, every route, every refusal, every cause of the fp8 refusal and, on a host or beam route, every
    condition that keeps a call off the device — for both language models where the model has it."""
    per_lm = {lm: dict(leaves=set(), routes=set(), refusals=set(), causes=set(), reasons=set()) for lm in ("opt", "t5")}
    for p, i in zip(points, table["points"]):
        e, got = table["outcomes"][i], per_lm[p["lm"]]
        got["leaves"].update(c[0] for c in e["calls"])
        r = route_of(e)
        if r is not None:
            got["routes"].add(r)
        msg = e.get("raises", ["", ""])[1]
        got["refusals"].update(m for m in REFUSALS if msg.startswith(m))
        got["causes"].update(fp8_causes(e))
        if r in ("sample_host", "search_host", "beam_device"):
            axes = (("user processor", p["host"] == "proc"), ("stopping criterion", p["host"] == "crit"), ("trace", p["trace"]),
                    ("more than 8 EOS ids", p["eos"] == 9), ("vocabulary not taken", p["vocab"] == 1002),
                    ("switch off", p["off"] is not None), ("beams", p["beams"] > 1))
            got["reasons"].update(n for n, on in axes if on)
    t5_leaves = {n for n in LEAVES if n.startswith(("t5_", "_t5_"))} | {"sample_loop", "beam_search"}
    opt_leaves = (set(LEAVES) - t5_leaves) | {"sample_loop", "beam_search"}
    assert per_lm["opt"]["leaves"] == opt_leaves, opt_leaves ^ per_lm["opt"]["leaves"]
    assert per_lm["t5"]["leaves"] == t5_leaves, t5_leaves ^ per_lm["t5"]["leaves"]
    for lm in ("opt", "t5"):
        assert per_lm[lm]["routes"] == set(ROUTES), (lm, set(ROUTES) ^ per_lm[lm]["routes"])
        want = set(HOST_REASONS) - ({"trace"} if lm == "t5" else set())
        assert per_lm[lm]["reasons"] == want, (lm, want ^ per_lm[lm]["reasons"])
    assert per_lm["opt"]["refusals"] == set(REFUSALS), set(REFUSALS) ^ per_lm["opt"]["refusals"]
    assert "generate(kv_cache_dtype='fp8') with" in per_lm["t5"]["refusals"]
    causes = per_lm["opt"]["causes"] | per_lm["t5"]["causes"]
    assert causes == set(FP8_CAUSES), set(FP8_CAUSES) ^ causes


def load_table(path):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", help="record the table to this JSON file")
    ap.add_argument("--check", help="replay the grid and compare with this JSON file")
    args = ap.parse_args()
    points = grid()
    table = build_table(points)
    assert_covers(points, table)
    print(f"{len(points)} grid points, {len(table['outcomes'])} distinct outcomes")
    if args.write:  # (mtime 0: the same table gives the same bytes)
        with open(args.write, "wb") as f:
            f.write(gzip.compress(json.dumps(table, sort_keys=True, separators=(",", ":")).encode(), 9, mtime=0))
    if args.check:
        want = load_table(args.check)
        assert want["keys_sha256"] == table["keys_sha256"], "the grid changed"
        bad = [key_of(p) for p, i, j in zip(points, table["points"], want["points"]) if table["outcomes"][i] != want["outcomes"][j]]
        assert not bad, f"{len(bad)} grid points differ, the first: {bad[:5]}"
        print("the table is unchanged")


if __name__ == "__main__":
    main()
