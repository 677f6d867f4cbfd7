"""Per-token latency of greedy decoding with bf16, fp8 (e4m3, per-channel) and int4 (group scales, include/eilev_w4.h) OPT linears (one GPU).

The configs[1] language model (OPT-2.7B widths, full depth, synthetic weights) on the 17-clip prompt of tools/pld_latency.py, L = 819; 64 new
tokens, EOS off, greedy_decode under hipGraph, at 1, 8 and 32 rows.  One engine per leg (lm_weights = "bf16" | "fp8" | "int4"), built one after
the other.  Per leg and row count (`reps` timed runs after one warm-up run): ms per generated token — decode time = the call minus the prefill
alone — as the minimum with the spread = max - min of the runs.  --legs bf16 runs on a checkout from before the int4 mode too.

--accuracy: on the tests/golden/full_c1.npz fixture (1 clip x 8 frames, L = 48, 32 tokens; every stack at full depth, weights by recipe) the int4
route's greedy ids against the reference's (n / 32) and the rel-RMS of the first step's logits against the bf16 route.  Recorded, not bounded:
Gaussian synthetic weights are not a checkpoint.

The kernels' own time: rocprofv3 --kernel-trace --stats -- python tools/w4_latency.py --rows 1 --legs int4

    python tools/w4_latency.py [--new 64] [--reps 3] [--rows 1,8,32] [--legs bf16,fp8,int4] [--accuracy] [--json out.json]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eilev_amd.configs import blip2_config  # noqa: E402
from eilev_amd.engine import HipEngine  # noqa: E402
from eilev_amd.synth import synth_param_torch, synth_pixels  # noqa: E402
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


def rel_rms(a, ref):
    a, ref = a.double(), ref.double()
    return float(((a - ref) ** 2).mean().sqrt() / ref.pow(2).mean().sqrt())


def accuracy(dev):
    """full_c1: greedy ids of the int4 route against the reference's, first-step logits against the bf16 route."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_c1.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = blip2_config(meta["config"])
    px = torch.from_numpy(synth_pixels(1, meta["frames"], cfg.vision_config.image_size)).to(dev)
    ids, vm, am = (torch.from_numpy(g[k]).to(dev) for k in ("input_ids", "video_input_mask", "attention_mask"))
    n, out = meta["new_tokens"], {}
    for mode in ("bf16", "int4"):
        sd = {k: synth_param_torch(k, shp, meta["weight_mode"], meta["weight_seed"], device=dev).to(torch.bfloat16)
              for k, shp in state_dict_shapes(cfg).items()}
        eng = HipEngine(cfg, sd, device=dev, lm_weights=mode)
        del sd
        emb = eng.embed_scatter(ids, vm, eng.encode_clips(px))
        got, steps = eng.greedy_decode(emb, am, n, eos_id=-1, use_graph=False, return_step_logits=True)
        out[mode] = (got.cpu().numpy(), steps[0].float().cpu(), steps[1].float().cpu())
        del eng, emb
        gc.collect()
        torch.cuda.empty_cache()
    ref_ids = g["fp32_greedy_free"]
    return dict(fixture="full_c1", new_tokens=int(n),
                int4_ids_equal_reference=int((out["int4"][0] == ref_ids).sum()), bf16_ids_equal_reference=int((out["bf16"][0] == ref_ids).sum()),
                prefill_logits_rel_rms_int4_vs_bf16=round(rel_rms(out["int4"][1], out["bf16"][1]), 4),
                first_step_logits_rel_rms_int4_vs_bf16=round(rel_rms(out["int4"][2], out["bf16"][2]), 4),
                note="Gaussian synthetic weights, not a checkpoint; the first decode step is fed each route's own first id")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--legs", default="bf16,fp8,int4")
    ap.add_argument("--mode", default="varied")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    cfg = blip2_config("opt27")
    dev = torch.device("cuda", 0)
    ids, vm = prompt_ids(cfg)
    L = ids.shape[1]
    n_vid = int(vm.sum())
    n = args.new
    rows = [int(r) for r in args.rows.split(",")]
    legs = [s for s in args.legs.split(",") if s]
    report = dict(config="opt27 language model (configs[1] widths, 32 blocks), synthetic weights", weight_mode=args.mode, prompt_len=L, new_tokens=n,
                  reps=args.reps, legs=legs, rows={str(r): {} for r in rows})
    g = torch.Generator(device=dev).manual_seed(1)
    feats = (torch.randn((n_vid, cfg.text_config.hidden_size), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    first_ids = {}
    for leg in legs:
        sd = {k: synth_param_torch(k, shp, args.mode, 0, device=dev).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()
              if k.startswith("language_model.")}
        eng = HipEngine(cfg, sd, device=dev, parts=("opt",), **({} if leg == "bf16" else dict(lm_weights=leg)))
        del sd
        emb1 = eng.embed_scatter(ids.to(dev), vm.to(dev), feats)
        for R in rows:
            emb = emb1.expand(R, -1, -1).contiguous()
            am = torch.ones((R, L), dtype=torch.int64, device=dev)
            fn = lambda: eng.greedy_decode(emb, am, n, eos_id=-1)  # noqa: E731
            eng.prefill(emb, am, kv_capacity=L)
            t_pre = min(timed(lambda: eng.prefill(emb, am, kv_capacity=L), args.reps))
            eng._dec_cache = None
            out = fn()  # warm-up: graph capture, lazy module loading
            assert out.shape == (R, n), out.shape
            per_tok = [(t - t_pre) * 1e3 / n for t in timed(fn, args.reps)]
            row = dict(ms_per_token=round(min(per_tok), 4), spread_ms=round(max(per_tok) - min(per_tok), 4), prefill_ms=round(t_pre * 1e3, 3))
            if leg == "int4":
                row["step"] = (eng.w4_stats or {}).get("step")
            first_ids.setdefault(R, {})[leg] = out[0].cpu()
            report["rows"][str(R)][leg] = row
            print(json.dumps({f"{leg} rows={R}": row}), flush=True)
        del eng, emb1, emb
        gc.collect()
        torch.cuda.empty_cache()
    for R in rows:
        row = report["rows"][str(R)]
        for leg in ("fp8", "int4"):
            if leg in row and "bf16" in row:
                row[f"{leg}_over_bf16"] = round(row[leg]["ms_per_token"] / row["bf16"]["ms_per_token"], 4)
                row[f"{leg}_ids_equal_bf16_route"] = int((first_ids[R][leg] == first_ids[R]["bf16"]).sum())
    if args.accuracy:
        report["accuracy"] = accuracy(dev)
        print(json.dumps(dict(accuracy=report["accuracy"])), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
