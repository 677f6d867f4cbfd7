"""Per-token latency of generate(do_sample=True): the host sampling loop against the draw in the captured decode step (one GPU).

The configs[1] language model (OPT-2.7B widths, synthetic weights) on the 17-clip prompt of tools/pld_latency.py, L = 819; 64 new
tokens, EOS off, at 1 row and at 32 rows.  Reports ms per generated token (decode time: prefill subtracted; `reps` runs: min and
spread = max - min) for
  (a) greedy search under hipGraph;
  (b) the host loop (eilev_amd/sampling.py sample_loop over the beam step) with hf's defaults (temperature 1, top_k 50, top_p 1);
  (c) the host loop with the demo's arguments (temperature 0.7, top_p 0.9, repetition_penalty 1.5, top_k 0);
  (d), (e) the device path (HipEngine.sample_decode_device) with the same two argument sets.
The host legs go through beam_decode(num_beams=1, sampler=, rules=) with transformers' processor object, a call that an engine without
the device path takes too (--legs host), so the same file measures a checkout from before the device path.

The sampling kernel's own time: rocprofv3 --kernel-trace --stats -- python tools/sample_latency.py --legs device --rows 1

    python tools/sample_latency.py [--new 64] [--reps 3] [--rows 1,32] [--legs all|host|device] [--json out.json]
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

DEFAULTS = dict(temperature=1.0, top_k=50, top_p=1.0)
DEMO = dict(temperature=0.7, top_k=0, top_p=0.9)
DEMO_PENALTY = 1.5


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
    ap.add_argument("--legs", default="all", choices=("all", "host", "device"))
    ap.add_argument("--mode", default="varied")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor

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
    report = dict(config="opt27 language model (configs[1] widths), synthetic weights", weight_mode=args.mode, prompt_len=L, new_tokens=args.new,
                  reps=args.reps, legs=args.legs, rows={})
    n = args.new

    def host(emb, am, warp, penalty):
        rules = None if penalty == 1.0 else dict(processors=LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=penalty)]), stopping=None)
        return eng.beam_decode(emb, am, n, 1, eos_id=-1, sampler=dict(warp, generator=g), rules=rules)

    for R in [int(r) for r in args.rows.split(",")]:
        emb = emb1.expand(R, -1, -1).contiguous()
        am = torch.ones((R, L), dtype=torch.int64, device=dev)
        legs = {}
        if args.legs in ("all", "device"):
            legs["a_greedy_graph"] = lambda: eng.greedy_decode(emb, am, n, eos_id=-1)
        if args.legs in ("all", "host"):
            eng.device_sampling = False  # (an engine without the device path ignores the attribute)
            legs["b_host_defaults"] = lambda: host(emb, am, DEFAULTS, 1.0)
            legs["c_host_demo"] = lambda: host(emb, am, DEMO, DEMO_PENALTY)
        if args.legs in ("all", "device"):
            legs["d_device_defaults"] = lambda: eng.sample_decode_device(emb, am, n, eos_id=-1, generator=g, **DEFAULTS)
            legs["e_device_demo"] = lambda: eng.sample_decode_device(emb, am, n, eos_id=-1, generator=g, repetition_penalty=DEMO_PENALTY, **DEMO)
        eng.prefill(emb, am, kv_capacity=L + n)
        t_pre = min(timed(lambda: eng.prefill(emb, am, kv_capacity=L + n), args.reps))
        row = dict(prefill_ms=round(t_pre * 1e3, 3))
        for name, fn in legs.items():
            out = fn()  # warm-up: graph capture, lazy module loading
            assert out.shape == (R, n), out.shape
            per_tok = [(t - t_pre) * 1e3 / n for t in timed(fn, args.reps)]
            row[name] = dict(ms_per_token=round(min(per_tok), 4), spread_ms=round(max(per_tok) - min(per_tok), 4))
            if name.startswith(("b_", "c_", "d_", "e_")):
                row[name]["distinct_ids_row0"] = len(set(out[0].tolist()))
        if "d_device_defaults" in row:
            row["d_minus_a_ms"] = round(row["d_device_defaults"]["ms_per_token"] - row["a_greedy_graph"]["ms_per_token"], 4)
            row["e_minus_a_ms"] = round(row["e_device_demo"]["ms_per_token"] - row["a_greedy_graph"]["ms_per_token"], 4)
        report["rows"][str(R)] = row
        print(json.dumps({f"rows={R}": row}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
