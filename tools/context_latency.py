"""What one prefilled in-context prefix saves (one GPU): configs[1] at full depth (ViT-g, Q-Former, OPT-2.7B; synthetic weights), the
headline prompt shape — 16 example clips x 8 frames with their texts, then one query clip and a question (L = 960).

  generate leg: B = 1, 8, 32 rows that share the 16 examples, 32 new tokens each.  The existing route encodes and prefills every row's
      whole prompt (17 clips, 960 positions: what generate() does); the shared route encodes and prefills the examples ONCE
      (encode_context: its one-off cost is reported on its own) and then, per call, encodes only the query clips and runs
      greedy_decode_context (generate(context=)).  Both routes are driven at the engine level, as generate() drives them.
  classify leg: B = 1, class length 4, 128 and 512 classes; classify_loglik with share_prompt_cache False / True: time and the peak of
      torch.cuda.max_memory_allocated over the call, workspaces included.  (The default route holds one copy of the prompt's cache
      per class, 315 MB each: it runs in class chunks of 64, as its callers run it; the shared route takes all classes at once.)

Every figure is the minimum of --reps runs with the spread (max - min).  The driver runs each leg in a child process under its own
`timeout` and stops at the first failure; `--root DIR --existing-only` runs the existing-route legs on another checkout (the parent
commit), whose figures the report carries as `parent`.

    python tools/context_latency.py [--reps 3] [--parent DIR] [--json profiles/context_latency.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
LEG_LIMIT_S = {"generate": 540, "classify": 420}
SHOTS, FRAMES, NEW_TOKENS, TEXT, QUESTION, CLASS_LEN = 16, 8, 32, 24, 14, 4
DEFAULT_CHUNK = 64  # class_batch_size of the default classify route: a copy of the prompt's cache per class of a chunk (20 GB at 64)


def _random_weights(cfg, dev):
    """bench.py's random initialisation: N(0, 0.02) matrices, unit LayerNorms, zero biases."""
    import torch

    from oracle.runner import state_dict_shapes

    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for k, shp in state_dict_shapes(cfg).items():
        low = k.lower()
        if "layernorm" in low or "layer_norm" in low:
            t = torch.ones(shp, device=dev) if k.endswith("weight") else torch.zeros(shp, device=dev)
        elif k.endswith(".bias"):
            t = torch.zeros(shp, device=dev)
        else:
            t = torch.randn(shp, device=dev, generator=g) * 0.02
        out[k] = t.to(torch.bfloat16)
    return out


def _timed(fn, reps):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(min(ts), 2), spread_ms=round(max(ts) - min(ts), 2)), r


def _setup():
    import numpy as np
    import torch

    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.synth import synth_interleaved_ids

    cfg = blip2_config("opt27")
    dev = torch.device("cuda", 0)
    eng = HipEngine(cfg, _random_weights(cfg, dev), device=dev)
    ids, vm = synth_interleaved_ids([1] * (SHOTS + 1), [TEXT] * SHOTS + [QUESTION], cfg.num_query_tokens, cfg.text_config.vocab_size, seed=1)
    ids, vm = torch.from_numpy(np.asarray(ids))[None].to(dev), torch.from_numpy(np.asarray(vm))[None].to(dev)
    P = ids.shape[1] - cfg.num_query_tokens - 1 - QUESTION  # the split: in front of the query clip's slots (then a separator and the question)
    assert not bool(vm[0, P - 1]) and bool(vm[0, P]) and int(vm[0, :P].sum()) == SHOTS * cfg.num_query_tokens
    img = cfg.vision_config.image_size

    def pixels(clips, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.randn((clips, 3, FRAMES, img, img), device=dev, generator=g).clamp_(-2.5, 2.5).to(torch.bfloat16)

    return cfg, dev, eng, ids, vm, P, pixels


def leg_generate(reps, existing_only):
    import torch

    cfg, dev, eng, ids, vm, P, pixels = _setup()
    L = ids.shape[1]
    px_ctx = pixels(SHOTS, 7)
    rows = {}
    out = dict(prompt_len=L, context_len=P, new_positions=L - P, new_tokens=NEW_TOKENS, rows=rows)
    ctx = None
    if not existing_only:
        def make_context():
            return eng.prefill_context(eng.embed_scatter(ids[:, :P], vm[:, :P], eng.encode_clips(px_ctx)))

        make_context()
        out["context_once"], ctx = _timed(make_context, reps)
    for B in (1, 8, 32):
        px_q = pixels(B, 100 + B)
        # every row: the same 16 examples, its own query clip
        px_all = torch.cat((px_ctx[None].expand(B, -1, -1, -1, -1, -1), px_q[:, None]), dim=1).reshape(B * (SHOTS + 1), *px_q.shape[1:])
        ids_b, vm_b = ids.expand(B, -1).contiguous(), vm.expand(B, -1).contiguous()
        am = torch.ones((B, L), dtype=torch.int32, device=dev)

        def existing():
            emb = eng.embed_scatter(ids_b, vm_b, eng.encode_clips(px_all))
            return eng.greedy_decode(emb, am, NEW_TOKENS, eos_id=-1)

        existing()
        row = dict(existing=_timed(existing, reps)[0])
        want = existing()
        if not existing_only:
            def shared():
                emb = eng.embed_scatter(ids_b[:, P:], vm_b[:, P:], eng.encode_clips(px_q))
                return eng.greedy_decode_context(ctx, emb, NEW_TOKENS, eos_id=-1)

            shared()
            row["shared_per_call"], got = _timed(shared, reps)
            row["rows_with_equal_ids"] = int((got == want).all(dim=1).sum())
            row["speedup_per_call"] = round(row["existing"]["ms"] / row["shared_per_call"]["ms"], 2)
        rows[str(B)] = row
        print(json.dumps({f"generate B={B}": row}), file=sys.stderr, flush=True)
        del px_all
    return out


def leg_classify(reps, existing_only):
    import torch

    cfg, dev, eng, ids, vm, P, pixels = _setup()
    L = ids.shape[1]
    emb = eng.embed_scatter(ids, vm, eng.encode_clips(pixels(SHOTS + 1, 7)))
    am = torch.ones((1, L), dtype=torch.int32, device=dev)
    out = dict(prompt_len=L, class_len=CLASS_LEN, classes={})
    for n_cls in (128, 512):
        g = torch.Generator().manual_seed(n_cls)
        cls = torch.randint(4, cfg.text_config.vocab_size, (n_cls, CLASS_LEN), generator=g).to(dev)

        def measure(fn):
            fn()
            eng._ws.clear()  # the engine keeps its workspaces: dropped, so that the peak below holds what the route needs
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t, ll = _timed(fn, reps)
            t["peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            return t, ll

        row = {}
        if not existing_only:
            row["shared"], ll_s = measure(lambda: eng.classify_loglik(emb, am, cls, share_prompt_cache=True))
        row["default"], ll_d = measure(lambda: eng.classify_loglik(emb, am, cls, class_batch_size=DEFAULT_CHUNK))
        row["default"]["class_batch_size"] = DEFAULT_CHUNK
        if not existing_only:
            row["max_abs_diff"] = round(float((ll_s - ll_d).abs().max()), 4)
            row["speedup"] = round(row["default"]["ms"] / row["shared"]["ms"], 2)
        out["classes"][str(n_cls)] = row
        print(json.dumps({f"classify {n_cls} classes": row}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", choices=sorted(LEG_LIMIT_S), default=None, help="run ONE leg in this process and print its JSON (what the driver starts)")
    ap.add_argument("--existing-only", action="store_true", help="only the routes that exist without the shared-prefix library")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose eilev_amd package is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its existing-route legs are reported as `parent`")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(HERE), "profiles", "context_latency.json"))
    args = ap.parse_args()
    if args.leg:
        sys.path.insert(0, os.path.abspath(args.root))
        res = (leg_generate if args.leg == "generate" else leg_classify)(args.reps, args.existing_only)
        print(json.dumps(res))
        return 0
    report = dict(config="configs[1] at full depth (eilev-blip2-opt-2.7b widths, random-init), 16 shots x 8 frames, L = 960; min of "
                         f"{args.reps} runs, spread = max - min")
    rc = 0
    runs = [("this", os.path.dirname(HERE), False)] + ([("parent", args.parent, True)] if args.parent else [])
    for tag, root, existing_only in runs:
        for leg, limit in LEG_LIMIT_S.items():
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps), "--root", root]
            r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:  # a failed or hung GPU step: nothing more is started on the device
                print(f"context_latency: leg {leg} ({tag}) ended with status {r.returncode}; stopping", file=sys.stderr)
                rc = r.returncode
                break
            report.setdefault(tag, {})[leg] = json.loads(r.stdout.strip().splitlines()[-1])
        if rc:
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    return rc


if __name__ == "__main__":
    sys.exit(main())
