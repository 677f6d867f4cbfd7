"""Batch-1 latency of prompt-lookup decoding against plain greedy decoding (one GPU).

The configs[1] language model (OPT-2.7B widths, synthetic weights) on a 17-clip prompt of the EILeV form: 16 in-context shots of
(32 video rows, a narration of text ids) and the query clip, L = 819; 64 new tokens, EOS off.  The video rows are random feature
rows (the language model only sees inputs_embeds), the narrations are drawn from a small phrase book, as EILeV's are.

Reports, per weight mode ('fanin': a repetitive continuation; 'varied': little to find):
  - ms per generated token of plain greedy (hipGraph) and of prompt lookup with k = 4 and 10 (decode time: prefill subtracted);
  - mean accepted draft ids per verify step;
and eilev_opt_extend's time for new_len 1 .. 11 against one eilev_opt_decode_step.

    python tools/pld_latency.py [--new 64] [--reps 3] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eilev_amd.configs import blip2_config  # noqa: E402
from eilev_amd.engine import HipEngine  # noqa: E402
from eilev_amd.synth import synth_param_torch  # noqa: E402
from oracle.runner import state_dict_shapes  # noqa: E402


def prompt_ids(cfg, clips=17, seed=0):
    """(ids, video mask) of one EILeV-style prompt: per clip 32 video positions, then a narration (not after the query clip)."""
    rng = random.Random(seed)
    V = cfg.text_config.vocab_size
    book = [[rng.randrange(4, V) for _ in range(rng.randrange(2, 5))] for _ in range(24)]  # phrases: "picks up", "the knife", ...
    head = [rng.randrange(4, V) for _ in range(4)]  # "The camera wearer"
    ids, vm = [2], [0]
    for c in range(clips):
        ids += [0] * cfg.num_query_tokens
        vm += [1] * cfg.num_query_tokens
        text = head + [x for _ in range(rng.randrange(3, 6)) for x in rng.choice(book)] if c + 1 < clips else head
        ids += text
        vm += [0] * len(text)
    return torch.tensor([ids]), torch.tensor([vm])


def timed(fn, reps):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="fanin,varied")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cfg = blip2_config("opt27")
    dev = torch.device("cuda", 0)
    ids, vm = prompt_ids(cfg)
    L = ids.shape[1]
    text = ids[0][vm[0] == 0].to(dev)
    am = torch.ones((1, L), dtype=torch.int64, device=dev)
    n_vid = int(vm.sum())
    report = dict(config="opt27 language model (configs[1] widths), synthetic weights", prompt_len=L, new_tokens=args.new, modes={})
    eng = None
    for mode in args.modes.split(","):
        del eng
        torch.cuda.empty_cache()
        sd = {k: synth_param_torch(k, shp, mode, 0, device=dev).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()
              if k.startswith("language_model.")}
        eng = HipEngine(cfg, sd, device=dev, parts=("opt",))
        del sd
        g = torch.Generator(device=dev).manual_seed(1)
        feats = (torch.randn((n_vid, cfg.text_config.hidden_size), generator=g, device=dev) * 0.05).to(torch.bfloat16)
        emb = eng.embed_scatter(ids.to(dev), vm.to(dev), feats)
        eng.greedy_decode(emb, am, args.new, eos_id=-1)  # warm-up: graph capture, lazy module loading
        t_pre, _ = timed(lambda: eng.prefill(emb, am, kv_capacity=L + args.new + 10), args.reps)
        t_plain, plain = timed(lambda: eng.greedy_decode(emb, am, args.new, eos_id=-1), args.reps)
        row = dict(prefill_ms=round(t_pre * 1e3, 3), greedy_graph_ms_per_token=round((t_plain - t_pre) * 1e3 / args.new, 4),
                   greedy_distinct_ids=len(set(plain[0].tolist())))
        for k in (4, 10):
            eng.greedy_lookup_decode(emb, am, text, args.new, k, 2, eos_id=-1)
            t_pld, out = timed(lambda: eng.greedy_lookup_decode(emb, am, text, args.new, k, 2, eos_id=-1), args.reps)
            st = dict(eng.pld_stats)
            row[f"lookup_k{k}"] = dict(ms_per_token=round((t_pld - t_pre) * 1e3 / args.new, 4),
                                       speedup_vs_greedy=round((t_plain - t_pre) / max(t_pld - t_pre, 1e-9), 3),
                                       verify_steps=st["verify"], single_steps=st["single"], accepted=st["accepted"],
                                       mean_accepted_per_verify=round(st["accepted"] / max(st["verify"], 1), 3),
                                       ids_equal_greedy=bool(torch.equal(out, plain)))
        report["modes"][mode] = row
        print(json.dumps({mode: row}), flush=True)
    # eilev_opt_extend at new_len 1 .. 11 against one decode step (the last engine's weights; the time does not depend on them)
    d, lib = eng.dims, eng.lib
    cap = L + args.new + 11
    kv = eng.new_kv_cache(1, cap)
    eng.prefill(emb, am, kv_cache=kv, kv_capacity=cap)
    past = L + 32
    full = torch.ones((1, cap), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.eilev_opt_workspace_bytes(C.byref(d), 1, cap)), dtype=torch.uint8, device=dev)
    logits = torch.empty((11, d.vocab), dtype=torch.float32, device=dev)
    x = eng.embed_scatter(ids[:, :11].to(dev), None, None)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    reps = 20

    def events(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    ext = {}
    for n in range(1, 12):
        ext[n] = round(events(lambda: lib.eilev_opt_extend(C.byref(d), C.byref(eng.pack.opt), P(x), P(full), 1, n, past, P(kv), cap, P(logits), P(ws),
                                                           ws.numel(), stream())), 4)
    state = torch.tensor([33, 1], dtype=torch.int32, device=dev)
    tok = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.zeros(args.new, dtype=torch.int64, device=dev)
    fin = torch.zeros(1, dtype=torch.uint8, device=dev)
    am32 = am.to(torch.int32)
    nv = am32.sum(1, dtype=torch.int32)
    ws1 = torch.empty(int(lib.eilev_opt_workspace_bytes(C.byref(d), 1, 1)), dtype=torch.uint8, device=dev)

    def step():  # each launch advances the counter by one: positions L + 32 .. L + 52, all inside the cache
        lib.eilev_opt_decode_step(C.byref(d), C.byref(eng.pack.opt), P(tok), P(state), P(am32), P(nv), 1, L, P(kv), cap, P(logits), P(fin), -1, 1,
                                  P(out), args.new, P(ws1), ws1.numel(), stream())

    report["extend_ms_by_new_len"] = ext
    report["decode_step_eager_ms"] = round(events(step), 4)
    print(json.dumps({"extend_ms_by_new_len": ext, "decode_step_eager_ms": report["decode_step_eager_ms"]}), flush=True)

    # a generation in which no draft is ever found: the engine's no-draft step (eilev_opt_decode_step, eilev_pld_step on its one row,
    # the status read-back) args.new - 1 times, with a window that has no room in the cache (slot_limit == slot_base: no draft)
    from eilev_amd import abi

    pld = abi.load_pld()
    n_text = int(text.numel())
    params = abi.pld_params(4, 2, args.new, L, L, n_text + args.new, [])
    corpus = torch.zeros(n_text + args.new, dtype=torch.int64, device=dev)
    corpus[:n_text] = text
    clen = torch.tensor([n_text], dtype=torch.int32, device=dev)
    window = torch.zeros(5, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(pld.eilev_pld_scratch_bytes(5, d.vocab)), dtype=torch.uint8, device=dev)

    def no_draft_generation():
        last, _, _ = eng.prefill(emb, am, kv_cache=kv, kv_capacity=cap)
        state.zero_()
        status.zero_()
        clen.fill_(n_text)
        rows, lg = 1, last
        for _ in range(args.new):
            abi.check(pld.eilev_pld_step(C.byref(params), P(lg), rows, d.vocab, P(corpus), P(clen), P(window), P(state), P(out), P(status), P(scratch),
                                         scratch.numel(), stream()), "eilev_pld_step")
            c, m, done, _ = status.tolist()
            assert m == 0
            if done:
                break
            lib.eilev_opt_decode_step(C.byref(d), C.byref(eng.pack.opt), P(window), P(state), P(am32), P(nv), 1, L, P(kv), cap, P(logits), P(fin), -1, 1,
                                      P(out), args.new, P(ws1), ws1.numel(), stream())
            lg = logits

    no_draft_generation()
    t_nd, _ = timed(no_draft_generation, args.reps)
    last_mode = args.modes.split(",")[-1]
    t_pre_ms = report["modes"][last_mode]["prefill_ms"]
    report["no_draft_ms_per_token"] = round((t_nd * 1e3 - t_pre_ms) / args.new, 4)
    report["no_draft_vs_greedy_graph"] = round(report["no_draft_ms_per_token"] / report["modes"][last_mode]["greedy_graph_ms_per_token"], 3)
    print(json.dumps({"no_draft_ms_per_token": report["no_draft_ms_per_token"], "no_draft_vs_greedy_graph": report["no_draft_vs_greedy_graph"]}),
          flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
