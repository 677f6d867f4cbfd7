"""Per-token latency and peak memory of flan-t5 beam search: the host loop against the device loop (one GPU).

The flan-t5-xl language model (configs[3] widths, full depth, synthetic weights) on the 17-clip prompt of tools/pld_latency.py; 64 new
tokens, EOS off, num_beams = 5, length_penalty = -1 (the sample script's call), at 1 sample and at 6 samples (5 and 30 decode rows).  Reports
per leg ms per generated token (decode time: encoder + cross K/V subtracted; `reps` runs: min and spread = max - min) and the peak device
memory of the call (torch.cuda.max_memory_allocated, weights included) for
  (a) the host loop (HipEngine.t5_beam with beam_device_loop = False: cross K/V replicated to the beams, the self-attention cache
      reordered every step, eilev_t5_decode once per token, the selection as torch ops);
  (b) the device loop (eilev_t5beam_decode_step + eilev_topk_logprob + eilev_beam_advance, nothing copied or replicated).
Leg (a) is a call that an engine without the device loop takes too (--legs host), so the same file measures a checkout from before it.

The kernels' own time: rocprofv3 --kernel-trace --stats -- python tools/t5_beam_latency.py --legs device --samples 1 --reps 1

    python tools/t5_beam_latency.py [--new 64] [--reps 3] [--samples 1,6] [--beams 5] [--legs all|host|device] [--json out.json]
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
    ap.add_argument("--samples", default="1,6")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--legs", default="all", choices=("all", "host", "device"))
    ap.add_argument("--mode", default="varied")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    cfg = blip2_config("t5xl")
    dev = torch.device("cuda", 0)
    ids, vm = prompt_ids(cfg)
    L = ids.shape[1]
    n_vid = int(vm.sum())
    sd = {k: synth_param_torch(k, shp, args.mode, 0, device=dev).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()
          if k.startswith("language_model.")}
    eng = HipEngine(cfg, sd, device=dev, parts=("t5",))
    del sd
    g = torch.Generator(device=dev).manual_seed(1)
    feats = (torch.randn((n_vid, cfg.text_config.d_model), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    emb1 = eng.embed_scatter(ids.to(dev), vm.to(dev), feats)
    n, nb = args.new, args.beams
    has_device = hasattr(eng, "_t5_beam_device")
    host_on, dev_on = args.legs in ("all", "host"), args.legs in ("all", "device") and has_device
    report = dict(config="flan-t5-xl language model (configs[3] widths, full depth), synthetic weights", weight_mode=args.mode, prompt_len=L,
                  new_tokens=n, reps=args.reps, legs=args.legs, num_beams=nb, length_penalty=-1.0, device_loop_available=has_device, shapes={})

    def call(emb, am, device_loop):
        eng.beam_device_loop = device_loop
        try:
            return eng.t5_beam(emb, am, n, nb, -1.0, eos_id=-1)
        finally:
            eng.beam_device_loop = True

    for B in [int(s) for s in args.samples.split(",")]:
        emb = emb1.expand(B, -1, -1).contiguous()
        am = torch.ones((B, L), dtype=torch.int64, device=dev)
        pre = lambda: eng.t5_cross_kv(eng.t5_encode(emb, am))
        pre()
        t_pre = min(timed(pre, args.reps))
        row = dict(rows=B * nb, encoder_and_cross_kv_ms=round(t_pre * 1e3, 3))
        legs = {}
        if host_on:
            legs["a_host_loop"] = lambda: call(emb, am, False)
        if dev_on:
            legs["b_device_loop"] = lambda: call(emb, am, True)
        outs = {}
        for name, fn in legs.items():
            outs[name] = fn()  # warm-up: lazy module loading, workspaces
            assert outs[name].shape == (B, n + 1), (name, outs[name].shape)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            per_tok = [(t - t_pre) * 1e3 / n for t in timed(fn, args.reps)]
            peak = torch.cuda.max_memory_allocated(dev)
            row[name] = dict(ms_per_token=round(min(per_tok), 4), spread_ms=round(max(per_tok) - min(per_tok), 4),
                             peak_memory_mb=round(peak / 2 ** 20, 1), peak_above_resident_mb=round((peak - base) / 2 ** 20, 1),
                             distinct_ids_row0=len(set(outs[name][0].tolist())))
            stats = getattr(eng, "t5_beam_stats", None)
            if stats is not None:
                row[name]["path"] = stats["path"]
        if host_on and dev_on:
            row["host_equals_device"] = bool(torch.equal(outs["a_host_loop"], outs["b_device_loop"]))
            row["b_minus_a_ms"] = round(row["b_device_loop"]["ms_per_token"] - row["a_host_loop"]["ms_per_token"], 4)
        report["shapes"][f"{B}x{nb}"] = row
        print(json.dumps({f"{B} x {nb}": row}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
