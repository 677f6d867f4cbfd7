"""What shared prompt reads buy per generated token (one GPU): the configs[1] language model at full depth (OPT-2.7B widths, 32 layers,
random-init weights, EOS off), the engine's switch `shared_prompt_reads` off (eilev_opt_decode_step_beam: the prompt keys once per row)
and on (eilev_prefix_decode_step: once per sample), in the same process.

  context route: 16 shots = a prefix of 913 positions, 47 new positions per row, at 1, 8 and 32 rows (greedy_decode_context);
  beam search at L = 819: 1 x 5 and 6 x 5 rows (beam_decode, the device loop).

ms per generated token is the MARGINAL cost of a step, (t(32 tokens) - t(8 tokens)) / 24, so that the prefill / extend in front of the
steps, which both legs share, is not in it; each t is the minimum of --reps runs, the spread given is the sum of the two (max - min).
A gain counts where it exceeds that spread.

The driver runs each shape in a child process under its own `timeout` and stops at the first failure.  `--parent DIR`: a built checkout
of the parent commit, whose off leg is reported next to this build's; `--variant NAME=DIR`: a built checkout with another prompt range
size, whose on leg is reported under NAME (the range-size A/B).  `--profile SHAPE:LEG`: a few steps of one leg in this process, for a
`rocprofv3 --kernel-trace --stats -- python tools/shared_reads_latency.py --profile ctx32:on` run.

    python tools/shared_reads_latency.py [--reps 3] [--parent DIR] [--variant keys64=DIR] [--json profiles/shared_reads_latency.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_LIMIT_S = 300
PREFIX, NEW_POS, BEAM_L, LONG, SHORT = 913, 47, 819, 32, 8
SHAPES = {"ctx1": ("context", 1), "ctx8": ("context", 8), "ctx32": ("context", 32), "beam1x5": ("beam", 1), "beam6x5": ("beam", 6)}
BEAMS = 5


def _engine():
    import torch

    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.statedict import state_dict_shapes

    cfg = blip2_config("opt27")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    named = {}
    for k, shp in state_dict_shapes(cfg).items():  # bench.py's random initialisation: N(0, 0.02) matrices, unit LayerNorms, zero biases
        if not k.startswith("language_model"):
            continue
        low = k.lower()
        if "layernorm" in low or "layer_norm" in low:
            t = torch.ones(shp, device=dev) if k.endswith("weight") else torch.zeros(shp, device=dev)
        elif k.endswith(".bias"):
            t = torch.zeros(shp, device=dev)
        else:
            t = torch.randn(shp, device=dev, generator=g) * 0.02
        named[k] = t.to(torch.bfloat16)
    return cfg, dev, HipEngine(cfg, named, device=dev, parts=("opt",))


def _call(shape):
    """fn(new_tokens) -> ids for one shape, and the engine."""
    import torch

    cfg, dev, eng = _engine()
    kind, B = SHAPES[shape]
    D = cfg.text_config.hidden_size
    g = torch.Generator(device=dev).manual_seed(3)
    if kind == "context":
        ctx = eng.prefill_context((0.5 * torch.randn((1, PREFIX, D), device=dev, generator=g)).to(torch.bfloat16))
        new = (0.5 * torch.randn((B, NEW_POS, D), device=dev, generator=g)).to(torch.bfloat16)
        return eng, lambda T: eng.greedy_decode_context(ctx, new, T, eos_id=-1)
    emb = (0.5 * torch.randn((B, BEAM_L, D), device=dev, generator=g)).to(torch.bfloat16)
    am = torch.ones((B, BEAM_L), dtype=torch.int32, device=dev)
    return eng, lambda T: eng.beam_decode(emb, am, T, BEAMS, -1.0, eos_id=-1)


def _min_ms(fn, reps):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), max(ts) - min(ts)


def run_shape(shape, reps, legs):
    eng, fn = _call(shape)
    out = {}
    for leg in legs:
        eng.shared_prompt_reads = leg == "on"
        fn(LONG), fn(SHORT)  # (kernels loaded, graphs captured, workspaces made)
        t_long, s_long = _min_ms(lambda: fn(LONG), reps)
        t_short, s_short = _min_ms(lambda: fn(SHORT), reps)
        stats = eng.context_stats if SHAPES[shape][0] == "context" else getattr(eng, "beam_stats", None)
        out[leg] = dict(ms_per_token=round((t_long - t_short) / (LONG - SHORT), 4), spread_ms_per_token=round((s_long + s_short) / (LONG - SHORT), 4),
                        call_ms_32_tokens=round(t_long, 2), call_ms_8_tokens=round(t_short, 2), reads=(stats or {}).get("reads", "per_row"))
        print(json.dumps({f"{shape} {leg}": out[leg]}), file=sys.stderr, flush=True)
    eng.shared_prompt_reads = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="run ONE shape in this process and print its JSON (what the driver starts)")
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose eilev_amd package is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its off leg is reported as `parent`")
    ap.add_argument("--variant", action="append", default=[], help="NAME=DIR: a built checkout with another prompt range size, its on leg as NAME")
    ap.add_argument("--profile", default=None, help="SHAPE:LEG — 12 tokens of one leg in this process (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(HERE), "profiles", "shared_reads_latency.json"))
    args = ap.parse_args()
    if args.profile:
        sys.path.insert(0, os.path.abspath(args.root))
        shape, leg = args.profile.split(":")
        eng, fn = _call(shape)
        eng.shared_prompt_reads = leg == "on"
        fn(12)
        return 0
    if args.shape:
        sys.path.insert(0, os.path.abspath(args.root))
        print(json.dumps(run_shape(args.shape, args.reps, args.legs.split(","))))
        return 0
    report = dict(config=f"configs[1] language model at full depth (OPT-2.7B widths, random-init), EOS off; context route: prefix {PREFIX} + {NEW_POS} new "
                         f"positions; beam search: L = {BEAM_L}, {BEAMS} beams; ms per token = (t({LONG} tokens) - t({SHORT} tokens)) / {LONG - SHORT}, each t the "
                         f"min of {args.reps} runs, spread = the sum of their (max - min)")
    runs = [("this", os.path.dirname(HERE), "off,on")] + ([("parent", args.parent, "off")] if args.parent else [])
    runs += [(v.split("=", 1)[0], v.split("=", 1)[1], "on") for v in args.variant]
    rc = 0
    for shape in args.shapes.split(","):
        for tag, root, legs in runs:
            cmd = ["timeout", "-k", "10", str(SHAPE_LIMIT_S), sys.executable, os.path.abspath(__file__), "--shape", shape, "--reps", str(args.reps),
                   "--root", root, "--legs", legs]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:  # a failed or hung GPU step: nothing more is started on the device
                print(f"shared_reads_latency: {shape} ({tag}) ended with status {r.returncode}; stopping", file=sys.stderr)
                rc = r.returncode
                break
            report.setdefault(tag, {})[shape] = json.loads(r.stdout.strip().splitlines()[-1])
        if rc:
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    return rc


if __name__ == "__main__":
    sys.exit(main())
