"""Per-token latency and memory of greedy decoding with the bf16 KV cache against the fp8 (e4m3) one (one GPU).

The configs[1] language model (OPT-2.7B widths, synthetic weights) on the 17-clip prompt of tools/pld_latency.py, L = 819; 64 new tokens,
EOS off, at 1, 8 and 32 rows.  Per row count and cache dtype (greedy_decode under hipGraph; `reps` timed runs after one warm-up run):
  * ms per generated token: decode time = the call minus the prefill alone (the fp8 call's one-off eilev_kv8_quantize is part of it and is
    also reported on its own), minimum and spread = max - min of the runs;
  * torch.cuda.max_memory_allocated of one call (the engine's weights and workspaces included; the fp8 call still holds one bf16 cache
    of the prompt while it quantises);
  * the cost of eilev_kv8_quantize alone (device events, minimum of `reps`);
  * how many of the generated ids agree with the bf16 route (synthetic weights have near-tied logits: the ids may part early).
--legs bf16 runs the bf16 leg alone through a call that an engine without the fp8 route takes too, so the same file measures a checkout
from before it (the figure in brackets in the README).

The attention kernels' own time: rocprofv3 --kernel-trace --stats -- python tools/kv8_latency.py --rows 32 --legs fp8 (and --legs bf16)

    python tools/kv8_latency.py [--new 64] [--reps 3] [--rows 1,8,32] [--legs all|bf16|fp8] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eilev_amd.configs import blip2_config  # noqa: E402
from eilev_amd.engine import HipEngine, _ptr  # noqa: E402
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


def quantize_ms(eng, emb, am, cap, reps):
    """eilev_kv8_quantize of the prompt's cache alone, ms (device events)."""
    from eilev_amd import abi

    kv = abi.load_kv8()
    R, L, _ = emb.shape
    _, _, kv16 = eng.prefill(emb, am, kv_capacity=L)
    kv8 = eng.new_kv8_cache(R, cap)
    best = float("inf")
    for _ in range(reps + 1):  # (the first one loads the kernel)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        abi.check(kv.eilev_kv8_quantize(C.byref(eng.dims), _ptr(kv16), R, L, L, _ptr(kv8), cap, eng._stream()), "eilev_kv8_quantize")
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best, int(kv8.numel()), int(kv16.numel()) * cap // L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--legs", default="all", choices=("all", "bf16", "fp8"))
    ap.add_argument("--mode", default="varied")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

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
    n = args.new
    report = dict(config="opt27 language model (configs[1] widths), synthetic weights", weight_mode=args.mode, prompt_len=L, new_tokens=n, reps=args.reps,
                  legs=args.legs, rows={})
    for R in [int(r) for r in args.rows.split(",")]:
        emb = emb1.expand(R, -1, -1).contiguous()
        am = torch.ones((R, L), dtype=torch.int64, device=dev)
        legs = {}
        if args.legs in ("all", "bf16"):
            legs["bf16"] = lambda: eng.greedy_decode(emb, am, n, eos_id=-1)
        if args.legs in ("all", "fp8"):
            legs["fp8"] = lambda: eng.greedy_decode(emb, am, n, eos_id=-1, kv_dtype="fp8")
        eng.prefill(emb, am, kv_capacity=L)
        t_pre = min(timed(lambda: eng.prefill(emb, am, kv_capacity=L), args.reps))
        row = dict(prefill_ms=round(t_pre * 1e3, 3))
        outs = {}
        for name, fn in legs.items():
            eng._dec_cache = None  # (the other leg's cache must not count towards this leg's peak)
            outs[name] = fn()  # warm-up: graph capture, lazy module loading
            assert outs[name].shape == (R, n), outs[name].shape
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            per_tok = [(t - t_pre) * 1e3 / n for t in timed(fn, args.reps)]
            row[name] = dict(ms_per_token=round(min(per_tok), 4), spread_ms=round(max(per_tok) - min(per_tok), 4),
                             max_memory_allocated_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
        eng._dec_cache = None
        if "fp8" in legs:
            ms, nb8, nb16 = quantize_ms(eng, emb, am, L + n, args.reps)
            row["fp8"].update(quantize_ms=round(ms, 3), cache_gb=round(nb8 / 2 ** 30, 3), bf16_cache_gb=round(nb16 / 2 ** 30, 3))
        if len(outs) == 2:
            same = (outs["fp8"] == outs["bf16"])
            row["ids_equal_bf16_route"] = int(same.sum())
            row["ids_total"] = int(same.numel())
            row["first_row_agrees_up_to"] = int((~same[0]).float().argmax()) if not bool(same[0].all()) else n
            row["fp8_over_bf16"] = round(row["fp8"]["ms_per_token"] / row["bf16"]["ms_per_token"], 4)
        report["rows"][str(R)] = row
        print(json.dumps({f"rows={R}": row}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
