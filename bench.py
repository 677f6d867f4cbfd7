#!/usr/bin/env python
"""Benchmark: clips/sec, encode + generate, eilev-blip2-opt-2.7b, 8 frames x 16 in-context (BASELINE.json).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One STEP = one pass of the hot path over one batch of synthetic input per GPU: `--samples` (default 32)
16-shot samples, each 17 clips x 8 frames of 224x224 pixels (bf16, resident in HBM) through ViT-g/14 ->
Q-Former -> projection -> [all-gather of clip tokens when N > 1] -> embed+scatter -> OPT-2.7B prefill
(L = 960) -> 32 greedy tokens (EOS disabled, decode under hipGraph).  Weak scaling: every rank gets its own
`--samples` samples; clips of the global step are dealt round-robin over the ranks (eilev_amd/sharding.py).

Prints ONE JSON line (rank 0) with the contract fields plus `roofline` (dominant kernel = the ViT MLP GEMM,
timed live with hipEvents on the launch stream inside the timed region).  A plain run sets up, warms up, times
the steps, writes its outputs (`--dump-outputs`) and prints that line.  `--full` adds everything that takes work
of its own after the timed steps: the oracle check and the reference-fixture replay (`verified`), `cpu_baseline`
(the CPU oracle and stock transformers timed on a bounded sample of the same workload, rank 0 at N = 1 only),
the strong-scaling phase, the rocprofv3 --pmc re-measurement of `roofline.traffic` and, at N > 1, `sharded_check`.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from eilev_amd import abi  # noqa: E402
from eilev_amd.configs import CONFIGS, blip2_config  # noqa: E402
from eilev_amd.sharding import ExchangePlan  # noqa: E402
from eilev_amd.synth import synth_interleaved_ids  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md: dense bf16 MFMA peak
N_CTX, FRAMES, NEW_TOKENS = 16, 8, 32
# algorithmic work, SURVEY §8(d): ViT 520.72 GF/frame, Q-Former 60.50 GF/clip, projection 0.126 GF/clip,
# prefill 4.98 TF/sample, decode(32) 0.18 TF/sample  ->  77.0 TFLOP per 16-shot sample
TFLOP_PER_SAMPLE = 77.0


def random_weights(cfg, device, seed=0):
    """Random-init bf16 weights of the named architecture, N(0, 0.02) matrices, LN weight 1 / bias 0."""
    from eilev_amd.statedict import state_dict_shapes

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    for k, shp in state_dict_shapes(cfg).items():
        low = k.lower()
        if ("layernorm" in low or "layer_norm" in low):
            t = torch.ones(shp, device=device) if k.endswith("weight") else torch.zeros(shp, device=device)
        elif k.endswith(".bias"):
            t = torch.zeros(shp, device=device)
        else:
            t = torch.randn(shp, device=device, generator=g) * 0.02
        out[k] = t.to(torch.bfloat16)
    return out


def build_inputs(cfg, samples, device, seed=1234):
    nq = cfg.num_query_tokens
    vocab = cfg.text_config.vocab_size
    n_clips = samples * (N_CTX + 1)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    px = torch.randn((n_clips, 3, FRAMES, cfg.vision_config.image_size, cfg.vision_config.image_size), device=device,
                     generator=g).clamp_(-2.5, 2.5).to(torch.bfloat16)
    ids, vm = [], []
    for s in range(samples):
        i, m = synth_interleaved_ids([1] * (N_CTX + 1), [24] * N_CTX + [14], nq, vocab, seed=1 + s)
        ids.append(i)
        vm.append(m)
    ids = torch.from_numpy(np.stack(ids)).to(device)
    vm = torch.from_numpy(np.stack(vm)).to(device)
    am = torch.ones_like(ids, dtype=torch.int32)
    return px, ids, vm, am


def cpu_baseline(cfg, host_weights, full_c2=False):
    """The host-CPU number printed beside the GPU number: stock transformers modules (the classes the
    reference instantiates, ref:eilev/model/v2.py:111-127) composed by oracle/hf_baseline.py and timed on every host core —
    configs[0] (C1: 1 clip, 0-shot, greedy) end to end, and a bounded sample of the headline 16-shot workload (one clip's
    encode + one sample's L = 960 prefill and 32-token decode, scaled by the clip count) — `kind: "hf"`.  The CPU oracle
    (the C restatement the parity tests use) is timed too and reported under `oracle_port`."""
    port = cpu_baseline_port(cfg)
    try:
        from oracle.hf_baseline import time_hf_cpu

        hf = time_hf_cpu(cfg, host_weights, N_CTX, FRAMES, NEW_TOKENS, synth_interleaved_ids, full_c2=full_c2)
    except Exception as e:  # no transformers on the box (or a module API drift): report the port, say why
        port["hf_unavailable"] = f"{type(e).__name__}: {e}"[:200]
        return port
    cpu_model = ""
    try:
        with open("/proc/cpuinfo") as fh:
            cpu_model = next((ln.split(":", 1)[1].strip() for ln in fh if ln.startswith("model name")), "")
    except OSError:
        pass
    # `cores` = the threads the timed run really used (the probe picks them under the container's CPU quota), not the logical CPUs the
    # box reports; `value` is EXTRAPOLATED from a bounded sample (BASELINE.md 3 wanted C2 timed once in full: ~20 min of CPU per sample)
    if "c2_full_clips_per_s" in hf:  # --cpu-full: one whole headline sample was run (profiles/r06_cpu_full.json holds such a line)
        return {"value": hf["c2_full_clips_per_s"], "unit": "clips/s", "cores": hf["threads"], "logical_cpus": hf["cores"],
                "effective_cpus": hf.get("effective_cpus"), "kind": "hf", "extrapolated": False,
                "sample": (f"ONE COMPLETE 16-shot sample, nothing scaled: stock transformers Blip2VisionModel + Blip2QFormerModel + OPTForCausalLM (torch {hf['torch']}, fp32, "
                           f"{hf['threads']} threads, {cpu_model}) on the same random-init weights: 17 different clips x 8 frames encoded one by one "
                           f"({hf['c2_full_encode_seconds']} s), L=960 prefill + 32 greedy tokens: {hf['c2_full_seconds']} s in all"),
                "extrapolation_of_the_default_run": hf["c2_clips_per_s"], "c1_clips_per_s": hf["c1_clips_per_s"], "c1_seconds": hf["c1_seconds"], "oracle_port": port}
    return {"value": hf["c2_clips_per_s"], "unit": "clips/s", "cores": hf["threads"], "logical_cpus": hf["cores"],
            "effective_cpus": hf.get("effective_cpus"), "kind": "hf", "extrapolated": True,
            "sample": (f"EXTRAPOLATED from a bounded sample, not a full C2 run: stock transformers Blip2VisionModel + Blip2QFormerModel + OPTForCausalLM (torch {hf['torch']}, fp32, {hf['threads']} threads, "
                       f"{cpu_model}) on the same random-init weights: C1 = 1 clip x 8 frames, L=48, 32 greedy tokens end to end in {hf['c1_seconds']} s; "
                       f"headline workload sampled as 1 clip encode ({hf['clip_encode_seconds']} s) x 17 + one 16-shot sample's L=960 prefill + 32 "
                       f"decode steps ({hf['lm_16shot_seconds']} s)"),
            "c1_clips_per_s": hf["c1_clips_per_s"], "c1_seconds": hf["c1_seconds"], "oracle_port": port}


def cpu_baseline_port(cfg, seconds_budget=30.0):
    """Oracle (CPU restatement, fp32) timed on a bounded sample of the same workload, scaled by layer counts."""
    from transformers import Blip2Config

    from eilev_amd.statedict import state_dict_shapes
    from oracle.runner import OracleModel

    c = CONFIGS["opt27"]
    small = Blip2Config(vision_config={**c["vision_config"], "num_hidden_layers": 1},
                        qformer_config={**c["qformer_config"], "num_hidden_layers": 2},
                        text_config={**c["text_config"], "num_hidden_layers": 1}, num_query_tokens=c["num_query_tokens"])
    rng = np.random.default_rng(0)
    w = {}
    for k, shp in state_dict_shapes(small).items():
        low = k.lower()
        if "layernorm" in low or "layer_norm" in low:
            w[k] = np.ones(shp, np.float32) if k.endswith("weight") else np.zeros(shp, np.float32)
        else:
            w[k] = (0.02 * rng.standard_normal(shp, dtype=np.float32))
    m = OracleModel(small, w)
    cores = os.cpu_count() or 1
    px = np.clip(rng.standard_normal((1, 3, FRAMES, 224, 224), dtype=np.float32), -2.5, 2.5)
    t0 = time.perf_counter(); img = m.vit(px); t_vit1 = time.perf_counter() - t0            # embed + 1 block + post LN, 8 frames
    t0 = time.perf_counter(); q = m.qformer(img); t_qf2 = time.perf_counter() - t0          # 1 cross + 1 plain block, 1 clip
    L = 1 + 17 * 33 + 16 * 24 + 14
    emb = (0.02 * rng.standard_normal((1, L, 2560), dtype=np.float32))
    am = np.ones((1, L), np.int32)
    t0 = time.perf_counter(); last, _, kv = m.prefill(emb, am, kv_capacity=L + 4, all_logits=False); t_pre1 = time.perf_counter() - t0
    state = np.array([1, 1], np.int32); fin = np.zeros(1, np.uint8); tok = np.array([5], np.int64)
    out = np.zeros((1, 8), np.int64); nv = np.array([L], np.int32); lg = np.empty((1, small.text_config.vocab_size), np.float32)
    nb = m.lib.eilev_opt_workspace_bytes(C.byref(m.dims), 1, 1); ws = np.empty(nb // 4 + 1, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    t0 = time.perf_counter()
    for _ in range(2):
        m.lib.eilev_opt_decode_step(C.byref(m.dims), C.byref(m.pack.opt), P(tok), P(state), P(am), P(nv), 1, L, P(kv), L + 4,
                                    P(lg), P(fin), -1, 1, P(out), 8, P(ws), nb, None)
    t_dec1 = (time.perf_counter() - t0) / 2
    # scale: per sample = 17 clips x (39 ViT blocks + 6 Q-Former pairs) + 32 OPT blocks prefill + 31 decode steps x 32 blocks
    # (the lm_head inside t_pre1 / t_dec1 is counted 32x too often: a CPU-favourable... no, CPU-UNfavourable bias < 3 %)
    per_sample = 17 * (39 * t_vit1 + 6 * t_qf2) + 32 * t_pre1 + 31 * 32 * t_dec1
    return {"value": round(17.0 / per_sample, 5), "unit": "clips/s", "cores": cores, "kind": "port", "extrapolated": True,
            "sample": (f"oracle/libeilev_ref.so fp32, {cores} threads: 1 ViT-g block on 8 frames ({t_vit1:.2f}s), 2 Q-Former blocks "
                       f"on 1 clip ({t_qf2:.2f}s), 1 OPT-2.7B block prefill L={L} ({t_pre1:.2f}s), 1 block decode step "
                       f"({t_dec1:.3f}s); scaled to 17 clips x (39 ViT + 12 Q-Former blocks) + 32 blocks prefill + 31 x 32 decode")}


def reference_fixture_check(dev):
    """OUTSIDE the timed region: the full-depth fixtures made from the REFERENCE itself (fp32 and bf16 runs of ref:eilev/model/v2.py in the
    build container through 39 ViT-g + 12 Q-Former + 32 OPT-2.7B blocks at the real widths; weights by recipe, generated on the device in
    seconds) replayed on the HIP path — tests/golden/full_c1.npz (the C1 workload: 1 clip x 8 frames, L = 48) and, round 5,
    tests/golden/full_c2.npz (the HEADLINE shape: one 16-shot sample of 17 clips, L = 960, plus a shorter left-padded row).  Per fixture:
    distances of the last-row prefill logits HIP-vs-reference-fp32, reference-bf16-vs-fp32 (the yardstick) and HIP-vs-reference-bf16
    (what the north star's "within 1e-3 in bf16" is about), and the 32 greedy ids per row against the reference's (compared up to the
    first near-tie OF THE REFERENCE: oracle/parity.py).  Nothing under /root/reference is read: the fixtures are data."""
    import json as _json

    from eilev_amd.engine import HipEngine
    from eilev_amd.statedict import state_dict_shapes
    from eilev_amd.synth import synth_param_torch, synth_pixels
    from oracle.parity import greedy_ids_vs_reference  # the checker (outside the timed region)

    rr = lambda a, b: float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))
    ma = lambda a, b: float(np.abs(a - b).max())
    res, eng, built = {}, None, None
    for name, what in (("full_c1", "C1 workload: 1 clip x 8 frames, L = 48, 32 tokens"),
                       ("full_c2", "headline shape: 17 clips x 8 frames, L = 960 + a left-padded 3-clip row, 32 tokens each")):
        path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
        if not os.path.exists(path):
            continue
        t0 = time.perf_counter()
        g = np.load(path)
        meta = _json.loads(str(g["meta"]))
        cfg = blip2_config(meta["config"])
        key = (meta["config"], meta["weight_mode"], meta["weight_seed"])
        if built != key:  # (both fixtures use the same recipe and seed: one engine)
            del eng
            torch.cuda.empty_cache()
            sd = {k: synth_param_torch(k, shp, meta["weight_mode"], meta["weight_seed"], device=dev).to(torch.bfloat16) for k, shp in state_dict_shapes(cfg).items()}
            eng, built = HipEngine(cfg, sd, device=dev), key
            del sd
        nclips = sum(sum(c) for c, _ in meta["rows"])
        px = torch.from_numpy(synth_pixels(nclips, meta["frames"], cfg.vision_config.image_size)).to(dev)
        emb = eng.embed_scatter(torch.from_numpy(g["input_ids"]).to(dev), torch.from_numpy(g["video_input_mask"]).to(dev), eng.encode_clips(px))
        am = torch.from_numpy(g["attention_mask"]).to(dev)
        last, _, _ = eng.prefill(emb, am)
        ids = eng.greedy_decode(emb, am, meta["new_tokens"], eos_id=-1, use_graph=True).cpu().numpy()
        got, r32, r16 = last.float().cpu().numpy(), g["fp32_logits_last"], g["bf16_logits_last"]
        verdict = greedy_ids_vs_reference(ids, g)
        out = {"what": "tests/golden/%s.npz (reference fp32 / bf16 runs at full depth, %s) replayed on the HIP path: last-row prefill logits "
                       "(%d values, std %.2f) and greedy ids" % (name, what, r32.size, float(r32.std())),
               "logits_hip_vs_ref_fp32": {"rel_rms": round(rr(got, r32), 5), "max_abs": round(ma(got, r32), 4)},
               "logits_ref_bf16_vs_ref_fp32": {"rel_rms": round(rr(r16, r32), 5), "max_abs": round(ma(r16, r32), 4)},
               "logits_hip_vs_ref_bf16": {"rel_rms": round(rr(got, r16), 5), "max_abs": round(ma(got, r16), 4)},
               "greedy_ids_equal_reference": f"{int((ids == g['fp32_greedy_free']).sum())}/{ids.size}",
               "greedy_ids_vs_reference": verdict, "seconds": round(time.perf_counter() - t0, 1)}
        out["ok"] = bool(out["logits_hip_vs_ref_fp32"]["rel_rms"] <= 1.5 * out["logits_ref_bf16_vs_ref_fp32"]["rel_rms"] + 1e-3 and verdict["ok"] and
                         np.array_equal(got.argmax(-1), r32.argmax(-1)))
        res[name] = out
    del eng
    torch.cuda.empty_cache()
    if not res:
        return None
    top = dict(res.get("full_c1") or next(iter(res.values())))  # (the keys of rounds 3-4 stay at the top level: the C1 fixture)
    if "full_c2" in res:
        top["headline_shape"] = res["full_c2"]
    top["ok"] = all(r["ok"] for r in res.values())
    return top


def verify_against_oracle(cfg, eng, weights, px, ids, vm, am, new_tokens):  # weights: name -> fp32 numpy (host)
    """OUTSIDE the timed region: the kernels at the launch shapes the timed steps use, checked against the CPU oracle.

    (a) one clip end to end: pixels -> ViT-g (39 blocks, its frames taken from a bench-sized launch of 1088 frames) ->
        Q-Former -> projection; the clip's 32 projected query tokens against the oracle run on the same pixels;
    (b) one sample through the language model: the oracle prefills the SAME inputs_embeds (L = 960) and then decodes
        teacher-forced on the ids the HIP path generated (batch-32 prefill + hipGraph decode, as timed): last-row prefill
        logits, and per step the oracle's logit of the HIP token against the oracle's maximum.
    Bar (the one of tests/test_hip_stages.py): the HIP result must be as close to the fp32 oracle as a bf16-storage run of the SAME
    arithmetic is — distance <= 1.5 x (oracle with `emulate_bf16` vs oracle fp32) + 1e-3 in relative RMS.  Through 39 + 12 + 32
    blocks of random-init weights that noise floor is ~1e-2 (it is printed next to the HIP distance), so a fixed 1e-2 would be
    a coin flip.  A generated id may differ from the oracle's argmax only at a near-tie (margin <= 5 % of the logits' standard
    deviation)."""
    from oracle.runner import OracleModel

    t0 = time.perf_counter()
    host = lambda t: t.detach().float().cpu().numpy()
    ora = OracleModel(cfg, weights)                       # fp32 truth
    ora16 = OracleModel(cfg, weights, emulate_bf16=True)  # the same arithmetic with activations rounded to bf16 where HIP stores bf16
    chunk = px[: max(1, 1088 // FRAMES)]
    feats = eng.encode_clips(chunk)                                   # bench-shaped launch (M = 1088 x 257 rows in the ViT)
    nq = cfg.num_query_tokens
    px0 = host(px[:1])
    ref_q = ora.project(ora.qformer(ora.vit(px0)))                    # clip 0 on the CPU: 8 frames x 39 blocks + Q-Former
    ref_q16 = ora16.project(ora16.qformer(ora16.vit(px0)))
    got_q = host(feats[:nq])
    rr = lambda a, b: float(np.sqrt(((a - b) ** 2).mean()) / (np.sqrt((b ** 2).mean()) + 1e-30))
    q_rel, q_noise = rr(got_q, ref_q), rr(ref_q16, ref_q)
    n_clips = ids.shape[0] * (N_CTX + 1)
    all_feats = torch.cat([eng.encode_clips(px[i:i + chunk.shape[0]]) for i in range(0, n_clips, chunk.shape[0])])
    emb = eng.embed_scatter(ids, vm, all_feats)
    last, _, _ = eng.prefill(emb, am)
    out_ids = eng.greedy_decode(emb, am, new_tokens, eos_id=-1, pad_id=1, use_graph=True)
    torch.cuda.synchronize()
    L = ids.shape[1]
    hip_ids = out_ids[0].cpu().numpy()
    emb0, am0 = host(emb[:1]), np.ones((1, L), np.int32)
    ref_last, _, kv = ora.prefill(emb0, am0, kv_capacity=L + new_tokens, all_logits=False)
    ref_last16, _, _ = ora16.prefill(emb0, am0, kv_capacity=L, all_logits=False)
    p_rel, p_noise = rr(host(last[:1]), ref_last), rr(ref_last16, ref_last)
    d = ora.dims
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    state = np.array([1, 1], np.int32); fin = np.zeros(1, np.uint8); tok = np.zeros(1, np.int64)
    scratch = np.zeros((1, new_tokens), np.int64); nv = np.array([L], np.int32); lg = np.empty((1, d.vocab), np.float32)
    nb = ora.lib.eilev_opt_workspace_bytes(C.byref(d), 1, 1); ws = np.empty(nb // 4 + 1, np.float32)
    # Round 6: an id is REQUIRED to equal the oracle's argmax wherever the oracle's own top-2 margin exceeds what bf16 storage can move two
    # logits against each other: 4 x (measured bf16-storage noise of the prefill logits, relative RMS) x rms(logits).  Below that floor the
    # step is undecided (either of the tied ids is a correct greedy continuation of a bf16 run) and the HIP id's logit must lie within the floor.
    margins, exact, logits = [], 0, ref_last
    decided, decided_exact, undecided_steps = 0, 0, []
    for t in range(new_tokens):
        row = logits[0]
        margins.append(float((row.max() - row[hip_ids[t]]) / (row.std() + 1e-30)))
        exact += int(row.argmax() == hip_ids[t])
        top2 = np.partition(row, -2)[-2:]
        floor_t = 4.0 * p_noise * float(np.sqrt((row ** 2).mean()))
        if float(top2[1] - top2[0]) > floor_t:
            decided += 1
            decided_exact += int(row.argmax() == hip_ids[t])
        else:
            undecided_steps.append(t)
            if float(row.max() - row[hip_ids[t]]) > floor_t:  # a tie between OTHER ids: the HIP id is outside the floor -> a miss
                decided += 1
        if t + 1 == new_tokens:
            break
        tok[0] = hip_ids[t]                                            # teacher forcing: feed what the HIP path generated
        state[0] = t + 1
        rc = ora.lib.eilev_opt_decode_step(C.byref(d), C.byref(ora.pack.opt), P(tok), P(state), P(am0), P(nv), 1, L, P(kv), L + new_tokens,
                                           P(lg), P(fin), -1, 1, P(scratch), new_tokens, P(ws), nb, None)
        assert rc == 0, rc
        logits = lg
    ok = bool(q_rel <= 1.5 * q_noise + 1e-3 and p_rel <= 1.5 * p_noise + 1e-3 and decided_exact == decided)
    return ok, {"query_tokens_rel_rms_vs_fp32": round(q_rel, 5), "bf16_storage_noise_query_tokens": round(q_noise, 5),
                "prefill_logits_rel_rms_vs_fp32": round(p_rel, 5), "bf16_storage_noise_prefill_logits": round(p_noise, 5),
                "ids_equal_oracle_argmax": f"{exact}/{new_tokens}",
                "ids_exact_required": True,
                "ids_exact_at_decided_steps": f"{decided_exact}/{decided}", "undecided_steps": undecided_steps,
                "ids_exact_note": "exact wherever the fp32 oracle's top-2 margin exceeds the bf16 floor (4 x the measured bf16-storage noise x rms(logits)); at an "
                                  "undecided step (random-init weights at full depth give nearly flat logits) the HIP id's logit must lie within that floor of the "
                                  "maximum.  Exact greedy ids at THIS shape and depth (17 clips, L = 960, left padding, 39 / 12 / 32 blocks) are also pinned against "
                                  "the REFERENCE's own fp32 / bf16 runs by tests/golden/full_c2.npz, replayed in this run (`reference_parity.headline_shape`), and the "
                                  "timed decode step (32 rows x 975 keys, stream + row-block layouts, hipGraph) by tests/test_hip_real_shapes.py::test_decode_step_at_the_timed_bench_shape_vs_oracle",
                "max_margin_over_logit_std": round(max(margins), 5), "seconds": round(time.perf_counter() - t0, 1),
                "what": "oracle/libeilev_ref.so fp32 (and its bf16-storage emulation as the noise floor) on the same weights: clip 0 pixels -> projected query tokens (from a 1088-frame launch); "
                        "sample 0 inputs_embeds -> prefill last-row logits + teacher-forced decode on the HIP ids (batch-32 prefill, hipGraph decode)"}


def launch_ranks(n: int) -> int:
    """Start `n` copies of this script, one per GPU of this node, wired for torch.distributed (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR / MASTER_PORT): what `python -m torch.distributed.run --nproc-per-node n` does, without needing
    the launcher on the command line.  Rank 0 inherits stdout (it prints the JSON line); returns the worst exit code."""
    import socket
    import subprocess

    if torch.cuda.is_available() and torch.cuda.device_count() < n and "--share-gpu" not in sys.argv:
        print(f"bench.py: --gpus {n} but only {torch.cuda.device_count()} GPUs are visible", file=sys.stderr)
        return 2
    with socket.socket() as s:  # a free rendezvous port
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    codes = [None] * n
    while any(c is None for c in codes):  # a rank that dies would leave the others in a barrier forever: stop them
        for i, p in enumerate(procs):
            if codes[i] is None:
                codes[i] = p.poll()
        if any(c not in (None, 0) for c in codes):
            for i, p in enumerate(procs):
                if codes[i] is None:
                    p.terminate()
                    codes[i] = p.wait()
            break
        time.sleep(0.2)
    return max(abs(c) for c in codes)


def strong_scaling_phase(eng, cfg, world, rank, dev, exch_weak, is_t5, global_samples, steps=3, warmup=1):
    """SURVEY 8(d)'s configuration, measured in the same job right after the headline steps: `global_samples` (8) 16-shot samples per
    GLOBAL step whatever the rank count — 136 clips dealt round-robin (17 per GPU at N = 8), the language model data-parallel over
    samples (ONE sample per rank at N = 8: batch-1 prefill and decode).  Total work is fixed, so value(N) / value(1) is the
    strong-scaling speed-up.  Same barrier + synchronize bracket and max-over-ranks time as the headline number."""
    from eilev_amd.comm import ClipExchange
    from eilev_amd.sharding import my_samples

    nq, Dt = cfg.num_query_tokens, cfg.text_config.hidden_size
    cps = N_CTX + 1
    plan = ExchangePlan(global_samples, cps, world, rank, chunk_clips=max(1, 1088 // FRAMES))
    mine = my_samples(global_samples, world, rank)
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + rank)
    size = cfg.vision_config.image_size
    px = torch.randn((plan.n_local, 3, FRAMES, size, size), device=dev, generator=g).clamp_(-2.5, 2.5).to(torch.bfloat16)
    ids, vm = [], []
    for s_ in mine:
        i, m = synth_interleaved_ids([1] * cps, [24] * N_CTX + [14], nq, cfg.text_config.vocab_size, seed=100 + s_)
        ids.append(i)
        vm.append(m)
    if mine:
        ids = torch.from_numpy(np.stack(ids)).to(dev)
        vm = torch.from_numpy(np.stack(vm)).to(dev)
        am = torch.ones_like(ids, dtype=torch.int32)
    exch = ClipExchange(plan, nq, Dt, torch.bfloat16, dev, transport=exch_weak.transport if world > 1 else "local", comm=exch_weak.comm)

    seen = []  # the same (ids, vm) batch every step: its contract checks (two host syncs) run on the first submission only

    def step():
        feats = eng.encode_and_exchange(px, exch)
        if not mine:
            return None
        emb = eng.embed_scatter(ids, vm, feats, validated=bool(seen))
        seen.append(1)
        if is_t5:
            return eng.t5_greedy(emb, am, NEW_TOKENS, eos_id=-1, pad_id=0)[:, 1:]
        return eng.greedy_decode(emb, am, NEW_TOKENS, eos_id=-1, pad_id=1, use_graph=True)

    def sync():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device="cpu" if dist.get_backend() == "gloo" else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert out is None or out.shape == (len(mine), NEW_TOKENS)
    clips = global_samples * cps
    projection = None
    if world == 1 and not is_t5:
        # What ONE rank of an N-rank strong-scaling job would run, measured on this GPU: its dealt clips through ViT + Q-Former +
        # projection, then prefill + decode of its global_samples / N samples (N = 8: 17 clips, ONE sample, batch-1 decode).  The
        # exchange itself (2.8 MB per rank at N = 8, on a side stream under the next chunk's ViT) is not in it.  speedup = this job's
        # measured N = 1 step / that share: the strong-scaling curve the design predicts BEFORE multi-GPU hardware runs it.
        t1 = 1e3 * dt / steps
        projection = {"what": "one rank's share of the fixed global step, timed alone on this GPU (encode of its dealt clips + prefill and "
                              "decode of its samples; exchange excluded): projected speed-up = measured N=1 step / share", "n1_ms_per_step": round(t1, 3)}
        for n_ranks in (2, 4, 8):
            if global_samples % n_ranks:
                continue
            ns_, nc_ = global_samples // n_ranks, clips // n_ranks
            ids_n, vm_n, am_n, px_n = ids[:ns_], vm[:ns_], am[:ns_], px[:nc_]

            def share(first):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                feats = torch.cat([eng.encode_clips(px_n[i:i + 136]) for i in range(0, nc_, 136)])
                e1.record()
                emb = eng.embed_scatter(ids_n, vm_n, feats, validated=not first)
                eng.greedy_decode(emb, am_n, NEW_TOKENS, eos_id=-1, pad_id=1, use_graph=True)
                e2.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1), e1.elapsed_time(e2)

            share(True)
            runs = [share(False) for _ in range(3)]
            enc_ms, lm_ms = min(r[0] for r in runs), min(r[1] for r in runs)
            projection[f"N={n_ranks}"] = {"clips": nc_, "samples": ns_, "encode_ms": round(enc_ms, 2), "prefill_decode_ms": round(lm_ms, 2),
                                          "share_ms": round(enc_ms + lm_ms, 2), "projected_speedup": round(t1 / (enc_ms + lm_ms), 2)}
        if "N=8" in projection:
            projection["projected_speedup_at_8"] = projection["N=8"]["projected_speedup"]
    return {"projection": projection, "what": f"SURVEY 8(d): {global_samples} samples per GLOBAL step x {cps} clips = {clips} clips dealt over {world} rank(s), language model "
                    f"data-parallel over samples; fixed total work, same timing bracket as the headline number",
            "scaling": "strong", "global_samples": global_samples, "clips_per_step": clips, "steps": steps, "warmup": warmup,
            "value": round(clips * steps / dt, 3), "unit": "clips/s", "ms_per_step": round(1e3 * dt / steps, 3),
            "clips_encoded_rank0": plan.n_local, "samples_decoded_rank0": len(mine)}


def measure_traffic_pmc(shape: str = "fc1_ln", rows: int = 257 * 1088, kernel: str = "gemm_pp4"):
    """roofline.traffic measured in THIS run on THIS box: rocprofv3 --pmc around tools/gemm_probe.py launching the roofline kernel at the bench's
    launch shape (random bf16 operands, 12 launches), one counter per pass with --kernel-trace only (MI355X_MICROARCH.md: separate passes;
    FETCH_SIZE is doubled on gfx950, both are in KB).  Runs after the timed region, in a subprocess (the profiler attaches at process start).
    Returns ({"fetch_kb", "write_kb", "launches", "dur_us"}, None) or (None, reason)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_TOOL")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return None, "this process is itself being profiled"
    out = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="eilev_pmc_", dir="/tmp")
        try:
            env = dict(os.environ, PROBE_M=str(rows), TMPDIR="/tmp", EILEV_PROBE_ON_PRODUCT_LIB="1")  # the PRODUCT library's kernel, no switches
            r = subprocess.run([exe, "--kernel-trace", "--pmc", counter, "-d", tmp, "-o", "pm", "--", sys.executable,
                                os.path.join(ROOT, "tools", "gemm_probe.py"), "0", shape, "1"],
                               cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("_results.db")]
            if r.returncode != 0 or not dbs:
                return None, f"rocprofv3 --pmc {counter} failed (rc {r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
            rows_ = sqlite3.connect(dbs[0]).execute(
                "select dispatch_id, value, duration from counters_collection where counter_name = ? and kernel_name like ?",
                (counter, f"%{kernel}%")).fetchall()
            per, dur = {}, {}
            for did, v, d in rows_:  # summed over the XCDs / channels of a dispatch
                per[did] = per.get(did, 0.0) + v
                dur[did] = d
            if not per:
                return None, f"no {kernel} dispatch in the {counter} pass"
            out[counter] = sum(per.values()) / len(per)
            out["launches"] = len(per)
            out["dur_us"] = round(sum(dur.values()) / len(dur) / 1e3, 1)
        except Exception as e:  # noqa: BLE001 — a measurement aid: any failure falls back to the figure in profiles/
            return None, f"{type(e).__name__}: {e}"
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return {"fetch_kb": out["FETCH_SIZE"], "write_kb": out["WRITE_SIZE"], "launches": out["launches"], "dur_us": out["dur_us"]}, None


def dump_outputs(outdir, ids, feats, rank, world, budget=32 << 20):
    """--dump-outputs: what the last timed step computed, as DIR/<name>.npy — the generated ids (float64, exact) and a fixed, seeded sample
    of rows of the projected clip tokens (float32; the whole tensor is ~180 MB at the default size).  The same arguments give the same
    inputs and the same rows, so two builds compare output for output.  N > 1: every rank writes its own set (`_rank<r>`) within one budget."""
    os.makedirs(outdir, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    rows = feats.reshape(-1, feats.shape[-1])
    n = min(rows.shape[0], max(1, budget // world // (4 * rows.shape[1])))
    pick = np.sort(np.random.default_rng(0).choice(rows.shape[0], n, replace=False))
    arrays = {"generated_ids": ids.cpu().numpy().astype(np.float64),
              "clip_tokens_sample": rows[torch.from_numpy(pick).to(rows.device)].float().cpu().numpy(),
              "clip_tokens_sample_rows": pick.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(outdir, f"{name}{sfx}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=32, help="16-shot samples per GPU per step (<= 32: one decode batch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64): the "
                         "generated ids and a fixed, seeded row sample of the projected clip tokens (N > 1: one set per rank)")
    ap.add_argument("--full", action="store_true",
                    help="also run what takes work of its own after the timed steps: oracle verification + reference-fixture replay, "
                         "cpu_baseline, the strong-scaling phase, the live --pmc traffic measurement and (N > 1) sharded_check; the "
                         "--no-* options below switch single legs of it off")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-full", action="store_true", help="cpu_baseline from ONE complete 16-shot sample on the host cores (17 clips encoded + L = 960 prefill + 32 tokens: "
                    "~1.5-2 minutes of CPU) instead of the default bounded sample that is extrapolated")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling phase (SURVEY 8(d): 8 samples per GLOBAL step) that "
                    "runs after the headline weak-scaling steps and is reported as `strong_scaling` in the same JSON line")
    ap.add_argument("--strong-samples", type=int, default=8, help="samples per GLOBAL step of the strong-scaling phase")
    ap.add_argument("--no-pmc", action="store_true", help="do not re-measure roofline.traffic with rocprofv3 --pmc after the timed region (two short "
                    "profiled launches of the roofline kernel in a subprocess); the figure then comes from profiles/ and is labelled so")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle check of the timed kernels (outside the timed region)")
    ap.add_argument("--exchange", choices=["rccl", "torch"], default="rccl",
                    help="N > 1 transport of the clip tokens: rccl = eilev_exchange_clip_tokens (direct RCCL send/recv on a side "
                         "stream), torch = torch.distributed.all_to_all_single (also RCCL, through the process group)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal of the N-rank path on a box with ONE GPU: every rank uses cuda:0, the process group is gloo and the "
                         "exchange goes through torch.distributed (RCCL refuses two ranks on one device); the value it prints is not a "
                         "scaling number (`config.share_gpu` says so)")
    ap.add_argument("--lm", choices=["opt27", "t5xl", "opt67"], default="opt27",
                    help="opt27 = the headline configs[1]/[2]; informational: t5xl = BASELINE configs[3] (flan-t5-xl encoder-decoder LM), "
                         "opt67 = the OPT-6.7B backbone of configs[4] in bf16 (use --shots 32 for its 32-shot sequence)")
    ap.add_argument("--shots", type=int, default=16, help="in-context examples per sample (16 = the headline workload)")
    ap.add_argument("--lm-weights", choices=["bf16", "fp8", "fp8_mfma"], default="bf16",
                    help="fp8: e4m3 weights for the OPT linears, bf16 activations; fp8_mfma: e4m3 weights AND per-token e4m3 activations "
                         "on the fp8 MFMA in prefill (informational lines for configs[4]; the headline metric is bf16)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, RCCL)
        raise SystemExit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback on the product path)")
    if args.share_gpu:
        local = 0
        args.exchange = "torch"
    if local >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} needs GPU {local} but only {torch.cuda.device_count()} are visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        # a rank stuck in a collective (a peer that died, a fabric fault) would otherwise sit there until the caller's limit: give the
        # multi-rank run a wall-clock budget of its own and leave with a message instead
        import threading

        limit = float(os.environ.get("EILEV_BENCH_TIMEOUT_S", str(600 + 60 * (args.steps + args.warmup))))

        def _give_up():
            print(f"[rank {rank}] bench.py: no result after {limit:.0f} s with {world} ranks (stuck collective?); exiting", file=sys.stderr, flush=True)
            os._exit(124)

        wd = threading.Timer(limit, _give_up)
        wd.daemon = True
        wd.start()
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # backend "nccl" IS RCCL on ROCm

    from eilev_amd.engine import HipEngine

    global N_CTX
    N_CTX = args.shots
    cfg = blip2_config(args.lm)
    is_t5 = args.lm == "t5xl"
    seq_len = 1 + (N_CTX + 1) * 33 + N_CTX * 24 + 14
    weights = random_weights(cfg, dev)
    eng = HipEngine(cfg, weights, device=dev, lm_weights=args.lm_weights)
    do_verify = args.full and world == 1 and not args.no_verify and args.lm == "opt27" and args.lm_weights == "bf16"
    do_cpu = args.full and world == 1 and not args.no_cpu_baseline and args.lm == "opt27" and args.shots == 16
    if not (do_verify or do_cpu):
        del weights
    S = args.samples
    nq, Dt = cfg.num_query_tokens, cfg.text_config.hidden_size
    total_clips = world * S * (N_CTX + 1)
    # clips of the global step are dealt round-robin (clip c -> rank c % world); every rank materialises only ITS clips
    # (synthetic, so it just generates that many) and receives the projected tokens of the clips of ITS samples
    from eilev_amd.comm import ClipExchange

    plan = ExchangePlan(world * S, N_CTX + 1, world, rank, chunk_clips=max(1, 1088 // FRAMES))
    px, ids, vm, am = build_inputs(cfg, S, dev, seed=1234 + rank)
    assert px.shape[0] == plan.n_local and plan.n_consumed == S * (N_CTX + 1)
    transport = "torch" if args.share_gpu else args.exchange  # --share-gpu: N ranks on one device over gloo — RCCL cannot span them, by definition
    if world > 1 and transport == "rccl":
        # `--exchange rccl` (the default) means the direct RCCL communicator of csrc/comm.hip or NOTHING: a run that cannot build it must
        # say why and stop, not quietly time a different transport (VERDICT r4 item 8 — on first contact with N GPUs that fallback would
        # hide exactly the failure the run exists to find).  `--exchange torch` is the explicit way to time torch.distributed's RCCL.
        err = None
        try:
            exch = ClipExchange(plan, nq, Dt, torch.bfloat16, dev, transport="rccl")
        except (RuntimeError, OSError) as e:
            err = f"{type(e).__name__}: {e}"
            print(f"[rank {rank}] bench.py --exchange rccl: the direct RCCL communicator could not be created: {err}", file=sys.stderr, flush=True)
        ok = torch.tensor([0 if err else 1], device="cpu" if args.share_gpu else dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)  # every rank learns that some rank failed, so that all of them leave (no hung peer)
        if int(ok.item()) == 0:
            if rank == 0:
                print("bench.py: --exchange rccl failed on at least one rank (messages above); not falling back — rerun with "
                      "--exchange torch to time torch.distributed's all_to_all_single instead", file=sys.stderr, flush=True)
            dist.destroy_process_group()
            sys.exit(3)
    else:
        exch = ClipExchange(plan, nq, Dt, torch.bfloat16, dev, transport=transport)

    last = {}

    def stamp(name):
        if eng.timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            eng.timing.append((name, ev))

    seen = []  # the same (ids, vm) batch every step: its contract checks (two host syncs) run on the first (warm-up) submission only

    def step():
        stamp("step_begin")
        mine_f = last["feats"] = eng.encode_and_exchange(px, exch)  # chunks of 136 clips; each chunk's RCCL exchange runs under the next ViT
        emb = eng.embed_scatter(ids, vm, mine_f, validated=bool(seen))
        seen.append(1)
        stamp("encode_done")
        if is_t5:  # encoder-decoder LM: encoder + cross K/V take the place of the prefill
            out_ids = eng.t5_greedy(emb, am, NEW_TOKENS, eos_id=-1, pad_id=0)[:, 1:]
        else:
            out_ids = eng.greedy_decode(emb, am, NEW_TOKENS, eos_id=-1, pad_id=1, use_graph=True)  # stamps "prefill_done"
        stamp("step_end")
        return out_ids

    def sync():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        out = step()
    sync()
    eng.lib.eilev_prof_enable(1)
    eng.timing = []
    exch.timing = [] if world > 1 else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs:  # before anything else runs on the engine
        dump_outputs(args.dump_outputs, out, last["feats"], rank, world)
    # phase breakdown from events recorded on the launch stream inside the timed region (SURVEY §8d asks for these)
    phases = {"encode": 0.0, "prefill": 0.0, "decode": 0.0}
    marks = eng.timing
    eng.timing = None
    per = 5 if is_t5 else 4
    t5_enc_ms = 0.0
    for i in range(0, len(marks), per):
        if is_t5:  # T5: "prefill" = text encoder (24 blocks over L = 960) + cross K/V of the 24 decoder blocks
            (_, b0), (_, e1), (_, te), (_, p1), (_, s1) = marks[i:i + 5]
            t5_enc_ms += e1.elapsed_time(te)
        else:
            (_, b0), (_, e1), (_, p1), (_, s1) = marks[i:i + 4]
        phases["encode"] += b0.elapsed_time(e1)
        phases["prefill"] += e1.elapsed_time(p1)
        phases["decode"] += p1.elapsed_time(s1)
    assert out.shape == (S, NEW_TOKENS)
    sharded = None
    if world > 1:
        rdev = "cpu" if args.share_gpu else dev

        def over_ranks(x, op):
            t = torch.tensor([x], device=rdev, dtype=torch.float64)
            dist.all_reduce(t, op=op)
            return float(t.item())

        dt = over_ranks(dt, dist.ReduceOp.MAX)
        # every rank's own phase times (ms per step): one run locates an imbalance (a slow GPU, an exposed exchange, a rank with more clips)
        mine_ms = [phases["encode"] / args.steps, phases["prefill"] / args.steps, phases["decode"] / args.steps,
                   sum(m_[1].elapsed_time(m_[2]) for m_ in (exch.timing or []) if m_[0] == "wait") / args.steps]
        allp = torch.zeros(world, 4, dtype=torch.float64, device=rdev)
        allp[rank] = torch.tensor(mine_ms, dtype=torch.float64, device=rdev)
        dist.all_reduce(allp)
        per_rank_ms = [{"rank": r, "encode": round(float(allp[r, 0]), 2), "exchange_exposed": round(float(allp[r, 3]), 3),
                        "prefill": round(float(allp[r, 1]), 2), "decode": round(float(allp[r, 2]), 2)} for r in range(world)]
        if not is_t5 and args.full and not args.no_verify:
            # outside the timed region: every rank re-encodes the clips of ITS samples itself (the pixels of a peer are its seed
            # away) and the rows that came through the exchange must be those rows, the ids of its samples the same ids
            first, cps = rank * S * (N_CTX + 1), N_CTX + 1
            need = torch.arange(first, first + S * cps, device=dev)
            ref = torch.empty_like(last["feats"]).view(S * cps, nq, Dt)
            for q in range(world):
                sel = (need % world) == q
                if bool(sel.any()):
                    pq = px if q == rank else build_inputs(cfg, S, dev, seed=1234 + q)[0]
                    ref[sel] = eng.encode_clips(pq[need[sel] // world]).view(-1, nq, Dt)
                    del pq
            got_c, ref_c = last["feats"].float().view(S * cps, -1), ref.float().view(S * cps, -1)
            per_clip = (got_c - ref_c).pow(2).mean(1).sqrt() / ref_c.pow(2).mean(1).sqrt()   # a mis-routed clip reads ~1.4 here
            rel = float(((got_c - ref_c).pow(2).mean().sqrt() / ref_c.pow(2).mean().sqrt()).item())
            emb_ref = eng.embed_scatter(ids, vm, ref.view(-1, Dt))
            ids_ref = eng.greedy_decode(emb_ref, am, NEW_TOKENS, eos_id=-1, pad_id=1, use_graph=False)
            # first generated token, margin-aware: last-row prefill logits from the exchanged rows and from the locally encoded rows
            lg_x = eng.prefill(eng.embed_scatter(ids, vm, last["feats"], validated=True), am)[0].float()
            lg_r = eng.prefill(emb_ref, am)[0].float()
            lg_rel = float(((lg_x - lg_r).pow(2).mean().sqrt() / lg_r.pow(2).mean().sqrt()).item())
            top2 = lg_r.topk(2, dim=1).values
            near_tie = (top2[:, 0] - top2[:, 1]) <= 0.05 * lg_r.std(dim=1)
            first_ok = float(((lg_x.argmax(1) == lg_r.argmax(1)) | near_tie).float().mean().item())
            match = float((ids_ref == out).float().mean().item())
            first = float((ids_ref[:, 0] == out[:, 0]).float().mean().item())
            sharded = {"what": "per rank, after the timed steps: exchanged clip rows vs the same clips encoded locally (rel-RMS over all rows and the "
                               "WORST single clip, max over ranks; different launch compositions -> different tile / attention kernels -> bf16 "
                               "rounding; a mis-routed or stale clip reads ~1.4), last-row prefill logits from both row sets (rel-RMS, max over "
                               "ranks) and their argmax = the first generated token (equal, or the local logits' top-2 margin <= 5 % of their std: "
                               "min over ranks of the fraction of samples).  ids_match_min / first_token_match_min (greedy ids of all 32 tokens) are "
                               "informational: random-init weights put logits in near-ties and one flipped argmax changes the rest of its row",
                       "feat_rel_rms_max": round(over_ranks(rel, dist.ReduceOp.MAX), 6),
                       "worst_clip_rel_rms_max": round(over_ranks(float(per_clip.max().item()), dist.ReduceOp.MAX), 6),
                       "first_logits_rel_rms_max": round(over_ranks(lg_rel, dist.ReduceOp.MAX), 6),
                       "first_token_equal_or_near_tie_min": round(over_ranks(first_ok, dist.ReduceOp.MIN), 4),
                       "ids_match_min": round(over_ranks(match, dist.ReduceOp.MIN), 4),
                       "first_token_match_min": round(over_ranks(first, dist.ReduceOp.MIN), 4)}
            sharded["ok"] = (sharded["feat_rel_rms_max"] < 2e-2 and sharded["worst_clip_rel_rms_max"] < 3e-2 and
                             sharded["first_logits_rel_rms_max"] < 2e-2 and sharded["first_token_equal_or_near_tie_min"] == 1.0)

    # dominant kernel: the ViT GEMM family, timed with hipEvents on the launch stream during the timed region
    kinds = {1: "gemm_nt ViT fc1 (+bias+GELU) [gemm_pp4_kernel<1, false, 1, 1>: folded LayerNorm, 16x16x32 MFMAs; M x 6144 x 1408, M = 257 tokens x 1088 frames]", 2: "gemm_nt ViT fc2 (+bias+residual) [M x 1408 x 6144]",
             3: "gemm_nt ViT qkv (+bias) [M x 4224 x 1408]", 4: "gemm_nt ViT proj (+bias+residual) [M x 1408 x 1408]"}
    best = None
    tot_ms = 0.0
    per_kind = {}
    for kd, nm in kinds.items():
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        eng.lib.eilev_prof_collect(kd, C.byref(n), C.byref(ms), C.byref(fl))
        tot_ms += ms.value
        if n.value:
            per_kind[nm.split(" [")[0].replace("gemm_nt ViT ", "")] = [round(1e3 * ms.value / n.value, 1), round(fl.value / ms.value / 1e9, 1)]
        if n.value and (best is None or ms.value > best[2]):
            best = (nm, n.value, ms.value, fl.value)
    # the pixel read of the frame tensor (north star: "coalesced HBM loads of the frame tensor evidenced by achieved GB/s"): im2col_strip_kernel,
    # timed with hipEvents inside the timed region (prof kind 6: its "flops" field carries the pixel BYTES read)
    pixel_read = None
    n6, ms6, by6 = C.c_int64(), C.c_double(), C.c_double()
    eng.lib.eilev_prof_collect(6, C.byref(n6), C.byref(ms6), C.byref(by6))
    if n6.value and ms6.value > 0:
        rd = by6.value / (ms6.value * 1e-3) / 1e9
        wr = rd * (640.0 / 588.0)  # the patch rows it writes (K = 3 x 14 x 14 = 588 padded to 640 bf16), same element size as bf16 pixels
        pixel_read = {"kernel": "im2col_strip_kernel (frame tensor (N,3,T,224,224) -> patch rows; one workgroup per (frame, patch row), coalesced 16-byte loads)",
                      "launches": int(n6.value), "avg_launch_us": round(1e3 * ms6.value / n6.value, 1),
                      "pixel_bytes_per_launch": int(by6.value / n6.value), "achieved_read_GB_s": round(rd, 1),
                      "achieved_read_plus_write_GB_s": round(rd + wr, 1), "hbm_peak_GB_s": 8000.0,
                      "frac_of_hbm_peak_read_plus_write": round((rd + wr) / 8000.0, 4)}
    eng.lib.eilev_prof_enable(0)

    # the exchange of the timed steps: bytes, time on the side stream, and the part of it the ViT did not cover (rank 0's view)
    exchange_info = None
    if world > 1:
        marks_x = exch.timing or []
        rounds = [m_ for m_ in marks_x if m_[0] == "round"]
        waits = [m_ for m_ in marks_x if m_[0] == "wait"]
        exchange_info = {"rccl_ranks": int(getattr(getattr(exch, "comm", None), "world", dist.get_world_size())), "transport": exch.transport,
                         "rounds_per_step": len(rounds) // max(1, args.steps),
                         "sent_MB_per_step": round(sum(m_[3] for m_ in rounds) / args.steps / 1e6, 2),
                         "received_MB_per_step": round(sum(m_[4] for m_ in rounds) / args.steps / 1e6, 2),
                         "exchange_ms_per_step_side_stream": round(sum(m_[1].elapsed_time(m_[2]) for m_ in rounds) / args.steps, 3),
                         "exposed_ms_per_step": round(sum(m_[1].elapsed_time(m_[2]) for m_ in waits) / args.steps, 3),
                         "overlap": "every encode chunk's exchange runs on a side stream under the next chunk's ViT; exposed = the main stream's "
                                    "wait for the side stream before the language model"}
    exch.timing = None
    strong = None
    if args.full and not args.no_strong and args.shots == 16:
        strong = strong_scaling_phase(eng, cfg, world, rank, dev, exch, is_t5, args.strong_samples)

    if rank == 0:
        clips = world * S * (N_CTX + 1) * args.steps
        value = clips / dt
        res = {
            "metric": f"clips/sec (8-frame, {N_CTX} in-context) encode+generate, " +
                      {"t5xl": "eilev-blip2-flan-t5-xl", "opt27": "eilev-blip2-opt-2.7b", "opt67": "blip2-opt-6.7b backbone (bf16)"}[args.lm],
            "value": round(value, 3), "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": {"bf16": "bf16", "fp8": "bf16 activations, fp8 (e4m3) OPT weights",
                                          "fp8_mfma": "ViT / Q-Former bf16; OPT prefill linears fp8 e4m3 x e4m3 on the fp8 MFMA (fp32 accumulate), OPT decode bf16 x fp8 weights"}[args.lm_weights], "data": "synthetic",
            "config": {"workload": (f"configs[3]: eilev-blip2-flan-t5-xl (random-init), {S} samples/GPU/step x 17 clips x 8 frames "
                                    f"224x224, encoder L=960, 32 greedy decoder tokens (EOS off)") if is_t5 else
                                   (f"{'configs[1]: eilev-blip2-opt-2.7b' if args.lm == 'opt27' else ('configs[4] backbone blip2-opt-6.7b in bf16' if args.lm_weights == 'bf16' else ('configs[4] blip2-opt-6.7b, fp8 OPT weights' if args.lm_weights == 'fp8' else 'configs[4] blip2-opt-6.7b, fp8 MFMA (e4m3 weights + activations in prefill)'))} (random-init), "
                                    f"{S} samples/GPU/step x {N_CTX + 1} clips x 8 frames "
                                    f"224x224, L={seq_len} prefill, 32 greedy tokens (EOS off), clips dealt round-robin + "
                                    f"{('RCCL all-to-all of the clip tokens (' + exch.transport + ')') if world > 1 else 'no collective at N=1'}"),
                       **({"share_gpu": "all ranks on ONE GPU over gloo: a rehearsal of the N-rank path, not a scaling number"} if args.share_gpu else {}),
                       "samples_per_gpu": S, "clips_per_step": world * S * (N_CTX + 1), "seq_len": seq_len, "new_tokens": NEW_TOKENS},
            "whole_path_tflops": (round((74.75 if is_t5 else TFLOP_PER_SAMPLE) * world * S * args.steps / dt, 1)
                                  if N_CTX == 16 and args.lm != "opt67" else None),
            "phases_rank0": {"encode_ms_per_step": round(phases["encode"] / args.steps, 2),
                             "encode_only_clips_per_s": round(S * (N_CTX + 1) * args.steps / (phases["encode"] * 1e-3), 1),
                             "prefill_ms_per_step": round(phases["prefill"] / args.steps, 2),
                             # (OPT: the first token comes out of the prefill, 31 decode steps follow; T5: all 32 tokens are decoder steps)
                             "decode_ms_per_token": round(phases["decode"] / args.steps / (NEW_TOKENS if is_t5 else NEW_TOKENS - 1), 3),
                             "samples_per_s": round(world * S * args.steps / dt, 3)},
        }
        if best is not None:
            nm, n, ms, fl = best
            ach = fl / (ms * 1e-3) / 1e12
            traffic = tr = None
            try:  # PMC-measured HBM/fabric bytes per launch of this kernel (profiles/, collected with rocprofv3 --pmc)
                with open(os.path.join(ROOT, "profiles", "r05_gemm_traffic.json")) as fh:
                    tr = json.load(fh).get(nm.split(" [")[0].replace("gemm_nt ViT ", ""))
                if tr:  # measured on the bench's launch shape (1088 frames x 257 tokens per launch)
                    traffic = int((2 * tr["fetch_kb"] + tr["write_kb"]) * 1024)
            except OSError:
                pass
            live, why = (None, "re-measured with --full only") if not args.full else (None, "--no-pmc") if args.no_pmc else (None, "N > 1") if world > 1 else \
                (None, "not the fc1 roofline kernel / launch shape") if "fc1" not in nm or S * (N_CTX + 1) % 136 else measure_traffic_pmc()
            src = "profiles/r05_gemm_traffic.json (rocprofv3 --pmc FETCH_SIZE x 2 + WRITE_SIZE of this kernel at this launch shape; not re-measured in this run: " + str(why) + ")"
            if live:
                traffic = int((2 * live["fetch_kb"] + live["write_kb"]) * 1024)
                src = (f"measured in this run after the timed region: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one pass each) around "
                       f"PROBE_M=279616 tools/gemm_probe.py 0 fc1_ln 1 = {live['launches']} launches of this kernel at the bench launch shape "
                       f"({live['dur_us']} us each under the profiler); bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024 (gfx950 correction of MI355X_MICROARCH.md)")
            res["roofline"] = {"bound": "mfma", "kernel": nm, "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFLOPS,
                               "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                               "launches": int(n), "avg_launch_ms": round(ms / n, 4), "traffic_measured_in_run": bool(live),
                               "traffic_source": src, "algorithmic_bytes": int(2 * (257 * 1088 * 1408 + 6144 * 1408 + 257 * 1088 * 6144)) if "fc1" in nm else None,
                               "mfma_busy_frac_pmc": (tr or {}).get("mfma_busy_frac"), "effective_clock_ghz_pmc": (tr or {}).get("eff_clock_ghz"),
                               "vit_gemm_ms_per_step": round(tot_ms / args.steps, 2),
                               "vit_gemm_us_and_tflops": per_kind}
        if pixel_read is not None:
            res["pixel_read"] = pixel_read
        if not is_t5 and args.lm_weights == "bf16":
            # decode step against the HBM roofline: every token reads all block weights + the lm_head once and, per row, the K / V of its
            # prompt + the tokens generated so far (averaged over the NEW_TOKENS - 1 timed steps); bf16
            t = cfg.text_config
            Dt, Ft, Ll = t.hidden_size, t.ffn_dim, t.num_hidden_layers
            w_bytes = 2 * (Ll * (4 * Dt * Dt + 2 * Dt * Ft) + t.vocab_size * Dt)
            kv_bytes = 2 * 2 * Ll * Dt * S * (seq_len + NEW_TOKENS / 2.0)
            ms_tok = phases["decode"] / args.steps / (NEW_TOKENS - 1)
            ach = (w_bytes + kv_bytes) / (ms_tok * 1e-3) / 1e12
            res["decode"] = {"bound": "hbm", "rows": S, "ms_per_token": round(ms_tok, 3), "weight_bytes_per_token": int(w_bytes),
                             "kv_bytes_per_token": int(kv_bytes), "achieved": round(ach, 3), "peak": 8.0, "unit": "TB/s", "frac": round(ach / 8.0, 4)}
        # the language-model phase of THIS run against its rooflines (configs[3] / configs[4] need their own blocks):
        # prefill-like work (OPT prefill; T5 text encoder + cross K/V) = dense contractions -> MFMA peak of the operand type;
        # decode = weight + K/V streaming -> HBM
        t = cfg.text_config
        if is_t5:
            D_, I_, F_, Le, Ld = t.d_model, t.num_heads * t.d_kv, t.d_ff, t.num_layers, t.num_decoder_layers
            enc_tf = Le * (2 * seq_len * D_ * 3 * I_ + 2 * seq_len * I_ * D_ + 3 * 2 * seq_len * D_ * F_ + 4 * seq_len * seq_len * I_) / 1e12
            ckv_tf = Ld * 2 * 2 * seq_len * D_ * I_ / 1e12
            enc_ms, pre_ms = t5_enc_ms / args.steps, phases["prefill"] / args.steps
            ms_tok = phases["decode"] / args.steps / NEW_TOKENS
            w_bytes = 2 * (Ld * (6 * D_ * I_ + 3 * D_ * F_) + t.vocab_size * D_)
            kv_bytes = 2 * 2 * Ld * I_ * S * (seq_len + NEW_TOKENS / 2.0)  # cross K/V of the 960 encoder positions + the self-attention cache so far
            res["lm_phase"] = {
                "text_encoder": {"bound": "mfma", "tflop_per_sample": round(enc_tf, 3), "ms_per_step": round(enc_ms, 2),
                                 "achieved": round(enc_tf * S / (enc_ms * 1e-3), 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                                 "frac": round(enc_tf * S / (enc_ms * 1e-3) / MFMA_BF16_PEAK_TFLOPS, 4)},
                "cross_kv": {"tflop_per_sample": round(ckv_tf, 3), "ms_per_step": round(pre_ms - enc_ms, 2)},
                "decode": {"bound": "hbm", "rows": S, "ms_per_token": round(ms_tok, 3), "weight_bytes_per_token": int(w_bytes), "kv_bytes_per_token": int(kv_bytes),
                           "achieved": round((w_bytes + kv_bytes) / (ms_tok * 1e-3) / 1e12, 3), "peak": 8.0, "unit": "TB/s",
                           "frac": round((w_bytes + kv_bytes) / (ms_tok * 1e-3) / 1e12 / 8.0, 4),
                           "floor_ms_per_token_at_6.3TBs": round((w_bytes + kv_bytes) / 6.3e12 * 1e3, 3)}}
        else:
            Dt_, Ft_, Ll_ = t.hidden_size, t.ffn_dim, t.num_hidden_layers
            pre_tf = (Ll_ * (2 * seq_len * Dt_ * (4 * Dt_ + 2 * Ft_) + 2 * seq_len * seq_len * Dt_) + 2 * Dt_ * t.vocab_size) / 1e12  # causal attention halved; lm_head on the last row
            pre_ms = phases["prefill"] / args.steps
            peak = 5000.0 if args.lm_weights == "fp8_mfma" else MFMA_BF16_PEAK_TFLOPS
            res["lm_phase"] = {"prefill": {"bound": "mfma", "operands": "fp8 e4m3 x e4m3 (fp32 accumulate)" if args.lm_weights == "fp8_mfma" else "bf16",
                                           "tflop_per_sample": round(pre_tf, 3), "ms_per_step": round(pre_ms, 2),
                                           "achieved": round(pre_tf * S / (pre_ms * 1e-3), 1), "peak": peak, "unit": "TFLOP/s",
                                           "frac": round(pre_tf * S / (pre_ms * 1e-3) / peak, 4)}}
            if args.lm_weights != "bf16":  # (the bf16 decode block is `decode` above)
                wb = 1 if args.lm_weights in ("fp8", "fp8_mfma") else 2
                w_bytes = wb * Ll_ * (4 * Dt_ * Dt_ + 2 * Dt_ * Ft_) + 2 * t.vocab_size * Dt_
                kv_bytes = 2 * 2 * Ll_ * Dt_ * S * (seq_len + NEW_TOKENS / 2.0)
                ms_tok = phases["decode"] / args.steps / (NEW_TOKENS - 1)
                res["lm_phase"]["decode"] = {"bound": "hbm", "rows": S, "ms_per_token": round(ms_tok, 3), "weight_bytes_per_token": int(w_bytes),
                                             "kv_bytes_per_token": int(kv_bytes), "achieved": round((w_bytes + kv_bytes) / (ms_tok * 1e-3) / 1e12, 3),
                                             "peak": 8.0, "unit": "TB/s", "frac": round((w_bytes + kv_bytes) / (ms_tok * 1e-3) / 1e12 / 8.0, 4)}
        if sharded is not None:
            res["sharded_check"] = sharded
        if exchange_info is not None:
            exchange_info["per_rank_ms_per_step"] = per_rank_ms
            res["exchange"] = exchange_info
        if strong is not None:
            res["strong_scaling"] = strong
        if do_verify or do_cpu:  # fp32 host copy of the weights, shared by the oracle check and the stock-HF CPU baseline
            from oracle.hf_baseline import effective_cpus

            # the OpenMP pool (shared by torch's CPU ops and the oracle) sized to what the container may really use: a box that
            # reports 256 logical CPUs under a smaller quota runs 10-40x slower with 256 spinning threads
            torch.set_num_threads(max(1, min(effective_cpus(), 64)))
            host_w = {k: v.detach().float().cpu().numpy() for k, v in weights.items()}
        if do_verify:
            res["verified"], res["verification"] = verify_against_oracle(cfg, eng, host_w, px, ids, vm, am, NEW_TOKENS)
            ref_par = reference_fixture_check(dev)
            if ref_par is not None:
                res["reference_parity"] = ref_par
                res["verified"] = bool(res["verified"] and ref_par["ok"])
        if do_cpu:
            res["cpu_baseline"] = cpu_baseline(cfg, host_w, full_c2=args.cpu_full)
        print(json.dumps(res), flush=True)
    bad = None
    if world > 1 and rank == 0:
        # the N > 1 line is only valid if the exchange really spanned N ranks on the transport that was asked for and the rows that came
        # through it are the rows a rank computes itself; otherwise the JSON line above stands as the evidence and the run exits non-zero
        if exchange_info["rccl_ranks"] != world or exchange_info["transport"] != transport:
            bad = f"exchange ran on {exchange_info['rccl_ranks']} ranks over '{exchange_info['transport']}', expected {world} over '{transport}'"
        elif sharded is not None and not sharded["ok"]:
            bad = "sharded_check failed: " + json.dumps({k: v for k, v in sharded.items() if k != "what"})
        if bad:
            print("bench.py: INVALID multi-rank run — " + bad, file=sys.stderr, flush=True)
    if world > 1:
        flag = torch.tensor([1 if bad else 0], device="cpu" if args.share_gpu else dev)
        dist.broadcast(flag, 0)
        dist.destroy_process_group()
        if int(flag.item()):
            sys.exit(4)


if __name__ == "__main__":
    main()
