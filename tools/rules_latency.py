"""Per-token latency of greedy and beam search with logits rules: the host loops against the rules in the captured decode step (one GPU).

The configs[1] language model (OPT-2.7B widths, synthetic weights) on the 17-clip prompt of tools/pld_latency.py, L = 819; 64 new
tokens, EOS off.  Greedy search at 1 row and at 32 rows, beam search at 1 sample x 5 beams.  Reports ms per generated token (decode time:
prefill subtracted; `reps` runs: min and spread = max - min) for
  (a) plain greedy search under hipGraph;
  (b) greedy search with repetition_penalty 1.5 and no_repeat_ngram_size 3 in the host loop (eilev_amd/sampling.py sample_loop);
  (c) the same on the device (HipEngine.rules_decode_device);
  (d) plain beam search (eilev_amd/beam.py beam_search_device);
  (e) beam search with the same rules in the host loop (beam.py beam_search);
  (f) the same on the device (eilev_rules_topk_logprob inside beam_search_device).
The host legs go through beam_decode(..., rules=) with transformers' processor objects, a call that an engine without the device path
takes too (--legs host), so the same file measures a checkout from before the device path.

The kernels' own time: rocprofv3 --kernel-trace --stats -- python tools/rules_latency.py --legs device --rows 1 --reps 1

    python tools/rules_latency.py [--new 64] [--reps 3] [--rows 1,32] [--beams 5] [--legs all|host|device] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eilev_amd.configs import blip2_config  # noqa: E402
from eilev_amd.engine import HipEngine  # noqa: E402
from eilev_amd.synth import synth_param_torch  # noqa: E402
from oracle.runner import state_dict_shapes  # noqa: E402
from tools.pld_latency import prompt_ids  # noqa: E402

PENALTY = 1.5
NGRAM = 3


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="1,32")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--legs", default="all", choices=("all", "host", "device"))
    ap.add_argument("--mode", default="varied")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from transformers import LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    cfg = blip2_config("opt27")
    dev = torch.device("cuda", 0)
    ids, vm = prompt_ids(cfg)
    L = ids.shape[1]
    n_vid = int(vm.sum())
    sd = {k: synth_param_torch(k, shp, args.mode, 0, device=dev).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()
          if k.startswith("language_model.")}
    eng = HipEngine(cfg, sd, device=dev, parts=("opt",))
    del sd
    g = torch.Generator(device=dev).manual_seed(1)
    feats = (torch.randn((n_vid, cfg.text_config.hidden_size), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    emb1 = eng.embed_scatter(ids.to(dev), vm.to(dev), feats)
    n, nb = args.new, args.beams
    report = dict(config="opt27 language model (configs[1] widths), synthetic weights", weight_mode=args.mode, prompt_len=L, new_tokens=n,
                  reps=args.reps, legs=args.legs, repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM, greedy={}, beam={})

    def objects():  # transformers' own processors: the form every engine's host loop takes
        return dict(processors=LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=PENALTY), NoRepeatNGramLogitsProcessor(NGRAM)]), stopping=None)

    def measure(legs, emb, am, rows_out):
        eng.prefill(emb, am, kv_capacity=L + n)
        t_pre = min(timed(lambda: eng.prefill(emb, am, kv_capacity=L + n), args.reps))
        row = dict(prefill_ms=round(t_pre * 1e3, 3))
        outs = {}
        for name, fn in legs.items():
            outs[name] = fn()  # warm-up: graph capture, lazy module loading
            assert outs[name].shape == (rows_out, n), (name, outs[name].shape)
            per_tok = [(t - t_pre) * 1e3 / n for t in timed(fn, args.reps)]
            row[name] = dict(ms_per_token=round(min(per_tok), 4), spread_ms=round(max(per_tok) - min(per_tok), 4),
                             distinct_ids_row0=len(set(outs[name][0].tolist())))
            stats = getattr(eng, "rules_stats", None)
            if stats is not None and "rules" in name:
                row[name]["path"] = stats["path"]
        return row, outs

    host_on, dev_on = args.legs in ("all", "host"), args.legs in ("all", "device")
    for R in [int(r) for r in args.rows.split(",")]:
        emb = emb1.expand(R, -1, -1).contiguous()
        am = torch.ones((R, L), dtype=torch.int64, device=dev)
        legs = {"a_greedy_graph": lambda: eng.greedy_decode(emb, am, n, eos_id=-1)}
        if host_on:
            legs["b_greedy_rules_host"] = lambda: eng.beam_decode(emb, am, n, 1, eos_id=-1, sampler=dict(greedy=True), rules=objects())
        if dev_on:
            legs["c_greedy_rules_device"] = lambda: eng.rules_decode_device(emb, am, n, eos_id=-1, repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM)
        row, outs = measure(legs, emb, am, R)
        if host_on and dev_on:
            row["host_equals_device"] = bool(torch.equal(outs["b_greedy_rules_host"], outs["c_greedy_rules_device"]))
        if dev_on:
            row["c_minus_a_ms"] = round(row["c_greedy_rules_device"]["ms_per_token"] - row["a_greedy_graph"]["ms_per_token"], 4)
        report["greedy"][str(R)] = row
        print(json.dumps({f"greedy rows={R}": row}), flush=True)

    am1 = torch.ones((1, L), dtype=torch.int64, device=dev)
    legs = {"d_beam_plain": lambda: eng.beam_decode(emb1, am1, n, nb, eos_id=-1)}
    if host_on:
        legs["e_beam_rules_host"] = lambda: eng.beam_decode(emb1, am1, n, nb, eos_id=-1, rules=objects())
    if dev_on:
        legs["f_beam_rules_device"] = lambda: eng.beam_decode(emb1, am1, n, nb, eos_id=-1, rules=dict(repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM))
    row, outs = measure(legs, emb1, am1, 1)
    if host_on and dev_on:
        row["host_equals_device"] = bool(torch.equal(outs["e_beam_rules_host"], outs["f_beam_rules_device"]))
    if dev_on:
        row["f_minus_d_ms"] = round(row["f_beam_rules_device"]["ms_per_token"] - row["d_beam_plain"]["ms_per_token"], 4)
    report["beam"][f"1x{nb}"] = row
    print(json.dumps({f"beam 1x{nb}": row}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
