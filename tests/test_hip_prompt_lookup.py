"""-m gpu: prompt-lookup decoding (libeilev_hip_pld.so, include/eilev_pld.h; HipEngine.greedy_lookup_decode / t5_greedy_lookup;
generate(prompt_lookup_num_tokens=k)).

The draft and step kernels equal their restatement (eilev_amd/pld.py) bit for bit; end to end the ids equal the reference's fp32 greedy
ids (oracle/parity.py's near-tie rule where the fixture records the step logits, exact elsewhere) and the engine's plain greedy ids."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from eilev_amd import abi
from eilev_amd.pld import PldState, draft_ref, step_ref
from hip_utils import P, load_case, models, stream_ptr
from oracle.parity import greedy_ids_vs_reference

pytestmark = pytest.mark.gpu

KS = [1, 4, 10]


# ---- kernels against the restatement --------------------------------------------------------------------------------------------
def _device_state(st: PldState, corpus_cap: int, max_new: int):
    t = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    corpus = torch.zeros(corpus_cap, dtype=torch.int64, device="cuda")
    corpus[:len(st.corpus)] = t(st.corpus, torch.int64)
    out = torch.full((max_new,), -7, dtype=torch.int64, device="cuda")
    if st.out:
        out[:len(st.out)] = t(st.out, torch.int64)
    return dict(corpus=corpus, corpus_len=t([len(st.corpus)], torch.int32), window=t(st.window, torch.int64),
                state=t([st.status[0], 1], torch.int32), out=out, status=t(st.status, torch.int32))


def _params(st: PldState, corpus_cap: int):
    return abi.pld_params(st.k, st.ngram, st.max_new, st.slot_base, st.slot_limit, corpus_cap, st.eos)


def _check(st: PldState, dev: dict):
    n = len(st.corpus)
    assert dev["status"].tolist() == st.status
    assert int(dev["corpus_len"]) == n and dev["corpus"][:n].tolist() == st.corpus
    assert dev["window"][:1 + st.status[1]].tolist()[1:] == st.draft
    assert dev["out"][:len(st.out)].tolist() == st.out


def _random_state(rng, k, vocab):
    n = rng.randrange(2, 300)
    ids = [rng.randrange(min(vocab, rng.choice([4, 16, vocab]))) for _ in range(n)]
    for _ in range(3):  # planted repeats onto the tail
        seg = ids[rng.randrange(0, n):][:rng.randrange(1, 8)]
        ids[n - len(seg):] = seg
    max_new = rng.choice([1, 2, 3, k + 1, 64])
    c = rng.randrange(0, max_new)
    eos = rng.sample(ids, min(len(ids), rng.choice([0, 1, 2]))) if rng.random() < 0.5 else []
    st = PldState(k=k, ngram=rng.choice([1, 2, 3]), max_new=max_new, slot_base=rng.randrange(0, 50), slot_limit=10 ** 6, eos=eos, corpus=ids)
    st.slot_limit = st.slot_base + c + rng.choice([0, 1, 2, k, 10 ** 5])  # the window's room in the cache
    st.status[0] = c
    st.out = [rng.randrange(vocab) for _ in range(c)]
    st.window = [rng.randrange(vocab) for _ in range(k + 1)]
    return st


def test_draft_kernel_equals_restatement():
    pld = abi.load_pld()
    rng = random.Random(7)
    for trial in range(120):
        k = rng.choice([1, 4, 10, abi.PLD_MAX_K])
        st = _random_state(rng, k, 512)
        cap = len(st.corpus) + rng.choice([0, 5])  # a full corpus too
        dev = _device_state(st, cap, st.max_new)
        abi.check(pld.eilev_pld_draft(C.byref(_params(st, cap)), P(dev["corpus"]), P(dev["corpus_len"]), P(dev["window"]), P(dev["status"]),
                                      stream_ptr()), "eilev_pld_draft")
        draft_ref(st)
        torch.cuda.synchronize()
        _check(st, dev)


@pytest.mark.parametrize("vocab", [512, 50272])
def test_step_kernel_equals_restatement(vocab):
    pld = abi.load_pld()
    rng = random.Random(vocab)
    g = torch.Generator().manual_seed(vocab)
    seen = dict(full=0, partial=0, eos_stop=0, budget_stop=0, m_is_k=0)
    for trial in range(80):
        k = rng.choice([1, 4, 10])
        st = _random_state(rng, k, vocab)
        st.status[1] = m = rng.randrange(0, max(0, min(k, st.max_new - st.status[0] - 1)) + 1)
        seen["m_is_k"] += m == k
        if st.eos and m and rng.random() < 0.5:  # an EOS id inside the draft
            st.window[1 + rng.randrange(m)] = st.eos[0]
        logits = torch.randn((m + 1, vocab), generator=g)
        # rows agree with the draft up to a random point; some rows tie their maximum with a lower or a higher id
        agree = rng.randrange(0, m + 1)
        for i in range(m + 1):
            x = st.window[1 + i] if i < agree else rng.randrange(vocab)
            logits[i, x] = 9.0
            if rng.random() < 0.4:
                logits[i, rng.randrange(vocab)] = 9.0
        cap = len(st.corpus) + st.max_new
        dev = _device_state(st, cap, st.max_new)
        scratch = torch.empty(int(pld.eilev_pld_scratch_bytes(m + 1, vocab)), dtype=torch.uint8, device="cuda")
        lg = logits.cuda()
        abi.check(pld.eilev_pld_step(C.byref(_params(st, cap)), P(lg), m + 1, vocab, P(dev["corpus"]), P(dev["corpus_len"]), P(dev["window"]),
                                     P(dev["state"]), P(dev["out"]), P(dev["status"]), P(scratch), scratch.numel(), stream_ptr()), "eilev_pld_step")
        c0 = st.status[0]
        step_ref(st, logits)
        torch.cuda.synchronize()
        _check(st, dev)
        assert int(dev["window"][0]) == (st.out[-1] if st.status[0] > c0 else st.window[0])
        assert dev["state"].tolist() == [st.status[0], 1 - st.status[2]]
        seen["full"] += st.status[3] == m and m > 0
        seen["partial"] += 0 < st.status[3] < m
        seen["eos_stop"] += bool(st.status[2]) and st.out[-1] in st.eos
        seen["budget_stop"] += st.status[0] == st.max_new
    assert all(v > 0 for v in seen.values()), seen


# ---- OPT end to end --------------------------------------------------------------------------------------------------------------
def _opt_case(golden_dir, name):
    g, meta, px = load_case(golden_dir, name)
    cfg, oracle, eng = models(meta["config"], meta["weight_mode"], seed=meta.get("weight_seed", 0))
    feats = eng.encode_clips(torch.from_numpy(px).cuda())
    emb = eng.embed_scatter(torch.from_numpy(g["input_ids"]).cuda(), torch.from_numpy(g["video_input_mask"]).cuda(), feats)
    return g, meta, eng, emb, torch.from_numpy(g["attention_mask"]).cuda()


def _text(g, b):
    keep = (g["attention_mask"][b] != 0) & (g["video_input_mask"][b] == 0)
    return torch.from_numpy(g["input_ids"][b][keep]).cuda()


def _row(g, b):
    """The fixture's record of row b alone, in the layout oracle/parity.py reads."""
    out = {"fp32_greedy_free": g["fp32_greedy_free"][b:b + 1]}
    for key in ("fp32_step_logits_top8", "fp32_step_logits_top8_ids", "bf16_step_logits_top8", "bf16_step_logits_top8_ids"):
        out[key] = g[key][:, b:b + 1]
    return out


@pytest.mark.parametrize("name,row", [("mid_v1", 0), ("mid_v2", 0), ("mid_v2", 1), ("real_v1", 0)])
def test_opt_lookup_ids_equal_reference_and_greedy(golden_dir, name, row):
    g, meta, eng, emb, am = _opt_case(golden_dir, name)
    n = meta["new_tokens"]
    e, a = emb[row:row + 1], am[row:row + 1]  # mid_v2 row 1: the left-padded row, with its padding
    plain = eng.greedy_decode(e, a, n, eos_id=-1).cpu().numpy()
    for k in KS:
        ids = eng.greedy_lookup_decode(e, a, _text(g, row), n, k, 2, eos_id=-1).cpu().numpy()
        verdict = greedy_ids_vs_reference(ids, _row(g, row))
        assert verdict["ok"], (k, verdict)
        assert np.array_equal(ids, plain), (k, ids, plain)
        assert eng.pld_stats["verify"] + eng.pld_stats["single"] + 1 + eng.pld_stats["accepted"] == n


def test_opt_lookup_full_depth(golden_dir):
    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.synth import synth_param_torch, synth_pixels
    from oracle.runner import state_dict_shapes

    g = np.load(os.path.join(golden_dir, "full_c1.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = blip2_config(meta["config"])
    sd = {k: synth_param_torch(k, shp, meta["weight_mode"], meta["weight_seed"], device="cuda").to(torch.bfloat16)
          for k, shp in state_dict_shapes(cfg).items()}
    eng = HipEngine(cfg, sd, device="cuda")
    del sd
    px = synth_pixels(1, meta["frames"], cfg.vision_config.image_size)
    emb = eng.embed_scatter(torch.from_numpy(g["input_ids"]).cuda(), torch.from_numpy(g["video_input_mask"]).cuda(),
                            eng.encode_clips(torch.from_numpy(px).cuda()))
    am = torch.from_numpy(g["attention_mask"]).cuda()
    n = meta["new_tokens"]
    plain = eng.greedy_decode(emb, am, n, eos_id=-1).cpu().numpy()
    for k in KS:
        ids = eng.greedy_lookup_decode(emb, am, _text(g, 0), n, k, 2, eos_id=-1).cpu().numpy()
        verdict = greedy_ids_vs_reference(ids, _row(g, 0))
        assert verdict["ok"], (k, verdict)
        assert np.array_equal(ids, plain), (k, ids, plain)


def test_opt_lookup_drafts_are_accepted(golden_dir):
    """mid_b1's inputs and 'fanin' weights: the greedy continuation repeats, so the drafts found in it are accepted."""
    g, meta, eng, emb, am = _opt_case(golden_dir, "mid_b1")
    plain = eng.greedy_decode(emb, am, 32, eos_id=-1).cpu().numpy()
    for k in KS:
        ids = eng.greedy_lookup_decode(emb, am, _text(g, 0), 32, k, 2, eos_id=-1).cpu().numpy()
        assert np.array_equal(ids, plain), (k, ids, plain)
        st = eng.pld_stats
        assert st["verify"] + st["single"] + 1 + st["accepted"] == 32
        if k > 1:
            assert st["verify"] < 16 and st["accepted"] > 16, (k, st)


@pytest.mark.parametrize("name", ["mid_b1", "mid_b2"])
def test_opt_lookup_rows_equal_fixture(golden_dir, name):
    g, meta, eng, emb, am = _opt_case(golden_dir, name)
    n = g["fp32_greedy_free"].shape[1]
    for b in range(emb.shape[0]):
        for k in KS:
            ids = eng.greedy_lookup_decode(emb[b:b + 1], am[b:b + 1], _text(g, b), n, k, 2, eos_id=-1).cpu().numpy()
            assert np.array_equal(ids[0], g["fp32_greedy_free"][b]), (b, k, ids, g["fp32_greedy_free"][b])


@pytest.mark.parametrize("name", ["mid_b1", "mid_v1"])
def test_opt_lookup_eos(golden_dir, name):
    g, meta, eng, emb, am = _opt_case(golden_dir, name)
    n = int(meta["new_tokens"])
    eos = int(g["fp32_eos_id"])
    want = g["fp32_greedy_eos"][0]
    for k in KS:
        ids = eng.greedy_lookup_decode(emb, am, _text(g, 0), n, k, 2, eos_id=eos).cpu().numpy()[0]
        assert np.array_equal(ids, want), (k, ids, want)
        assert ids[-1] == eos and (ids[:-1] != eos).all()
        # EOS given as a list: the same ids
        assert np.array_equal(eng.greedy_lookup_decode(emb, am, _text(g, 0), n, k, 2, eos_id=[eos, 50271]).cpu().numpy()[0], want)


@pytest.mark.parametrize("name", ["mid_b1", "mid_v1"])
def test_opt_lookup_eos_anywhere_ends_the_output(golden_dir, name):
    """EOS = each id of the free continuation in turn: committed as the first id, by a single step or as the bonus id of a verify,
    the output ends at its first occurrence, like plain greedy's."""
    g, meta, eng, emb, am = _opt_case(golden_dir, name)
    free = eng.greedy_decode(emb, am, 24, eos_id=-1).cpu().numpy()[0]
    for j in sorted({int(np.flatnonzero(free == x)[0]) for x in free}):
        eos = int(free[j])
        want = free[:j + 1]
        for k in (4, 10):
            ids = eng.greedy_lookup_decode(emb, am, _text(g, 0), 24, k, 2, eos_id=eos).cpu().numpy()[0]
            assert np.array_equal(ids, want), (eos, k, ids, want)
            assert np.array_equal(eng.greedy_decode(emb, am, 24, eos_id=eos, poll_every=1).cpu().numpy()[0], want)


@pytest.mark.parametrize("name", ["mid_v1", "real_v1"])
def test_opt_lookup_without_match_is_plain_greedy_bit_for_bit(golden_dir, name):
    """No draft is ever found (an empty text corpus, and only the fixture's leading ids that do not repeat): every step is the plain
    decode step, so the ids AND each step's logits are bit-identical to an eager greedy loop over eilev_opt_decode_step with the same KV
    capacity."""
    g, meta, eng, emb, am = _opt_case(golden_dir, name)
    free = g["fp32_greedy_free"][0].tolist()
    n = next((i for i in range(1, len(free)) if free[i] in free[:i]), len(free))
    assert n >= 2
    k = 4
    trace = []
    ids = eng.greedy_lookup_decode(emb, am, torch.empty(0, dtype=torch.int64), n, k, 2, eos_id=-1, trace=trace).cpu().numpy()
    assert eng.pld_stats["verify"] == 0 and eng.pld_stats["single"] == n - 1
    # the eager reference loop: prefill at capacity L + n + k, then n - 1 decode steps
    lib, d = eng.lib, eng.dims
    L = emb.shape[1]
    cap = L + n + k
    kv = eng.new_kv_cache(1, cap)
    am32 = am.to(torch.int32).contiguous()
    last, _, _ = eng.prefill(emb, am32, kv_cache=kv, kv_capacity=cap)
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    fin = torch.zeros(1, dtype=torch.uint8, device="cuda")
    tok = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    lg = torch.empty((1, d.vocab), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.eilev_opt_workspace_bytes(C.byref(d), 1, 1)), dtype=torch.uint8, device="cuda")
    steps = [last.clone()]
    abi.check(lib.eilev_greedy_select(P(last), 1, d.vocab, P(state), P(fin), -1, 1, P(tok), P(out), n, stream_ptr()), "select")
    for _ in range(n - 1):
        abi.check(lib.eilev_opt_decode_step(C.byref(d), C.byref(eng.pack.opt), P(tok), P(state), P(am32), P(am32.sum(1, dtype=torch.int32)), 1, L,
                                            P(kv), cap, P(lg), P(fin), -1, 1, P(out), n, P(ws), ws.numel(), stream_ptr()), "decode_step")
        steps.append(lg.clone())
    assert np.array_equal(ids[0], out.cpu().numpy()), (ids, out)
    assert np.array_equal(ids[0], np.asarray(free[:n]))
    assert len(trace) == n
    for i in range(n):
        assert torch.equal(trace[i], steps[i]), i


# ---- flan-t5 ---------------------------------------------------------------------------------------------------------------------
def _t5_case(golden_dir, name):
    g, meta, px = load_case(golden_dir, name)
    cfg, oracle, eng = models(meta["config"])
    t = lambda a: torch.from_numpy(a).cuda()
    emb = eng.embed_scatter(t(g["input_ids"]), t(g["video_input_mask"]), eng.encode_clips(t(px)))
    return g, meta, eng, emb, t(g["attention_mask"])


@pytest.mark.parametrize("name", ["mid_t5_b1", "tiny_t5_b2"])
def test_t5_lookup_equals_t5_greedy(golden_dir, name):
    g, meta, eng, emb, am = _t5_case(golden_dir, name)
    n = int(meta["new_tokens"])
    for b in range(emb.shape[0]):
        for eos in (-1, int(g["fp32_eos_id"])):
            plain = eng.t5_greedy(emb[b:b + 1], am[b:b + 1], n, eos_id=eos).cpu().numpy()
            for k in KS:
                ids = eng.t5_greedy_lookup(emb[b:b + 1], am[b:b + 1], _text(g, b), n, k, 2, eos_id=eos).cpu().numpy()
                assert np.array_equal(ids, plain), (b, eos, k, ids, plain)
                assert ids[0, 0] == 0


def test_t5_lookup_eos_equals_reference(golden_dir):
    g, meta, eng, emb, am = _t5_case(golden_dir, "mid_t5_b1")
    eos = int(g["fp32_eos_id"])
    want = g["fp32_greedy_eos"]
    for k in KS:
        ids = eng.t5_greedy_lookup(emb, am, _text(g, 0), int(meta["new_tokens"]), k, 2, eos_id=eos).cpu().numpy()
        assert np.array_equal(ids, want), (k, ids, want)


# ---- the public interface ----------------------------------------------------------------------------------------------------------
def _model(meta, dtype):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration
    from oracle.runner import synth_state_dict

    cfg = blip2_config(meta["config"])
    m = VideoBlipForConditionalGeneration(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, meta["weight_mode"], meta.get("weight_seed", 0)).items()}
    if cfg.text_config.model_type == "t5":  # as tests/test_hip_t5.py loads it (the lm_head is tied to `shared`)
        m.load_state_dict(sd, strict=False)
    else:
        sd["language_model.lm_head.weight"] = sd["language_model.model.decoder.embed_tokens.weight"]
        m.load_state_dict(sd)
    return m.to(dtype).to("cuda")


def test_generate_prompt_lookup_opt(golden_dir):
    g, meta, px = load_case(golden_dir, "mid_v1")
    m = _model(meta, torch.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    kw = dict(input_ids=t(g["input_ids"]), pixel_values=t(px), video_input_mask=t(g["video_input_mask"]), attention_mask=t(g["attention_mask"]),
              max_new_tokens=int(meta["new_tokens"]), num_beams=1, do_sample=False)
    for k in KS:
        ids = m.generate(**kw, eos_token_id=int(g["fp32_eos_id"]), prompt_lookup_num_tokens=k).cpu().numpy()
        assert np.array_equal(ids, g["fp32_greedy_eos"]), (k, ids)
        ids = m.generate(**kw, eos_token_id=int(meta["never_id"]), prompt_lookup_num_tokens=k, max_matching_ngram_size=3).cpu().numpy()
        assert np.array_equal(ids, g["fp32_greedy_free"]), (k, ids)
    out = m.generate(**kw, eos_token_id=int(meta["never_id"]), prompt_lookup_num_tokens=4, return_dict_in_generate=True)
    assert np.array_equal(out.sequences.cpu().numpy(), g["fp32_greedy_free"])


def test_generate_prompt_lookup_t5(golden_dir):
    g, meta, px = load_case(golden_dir, "mid_t5_b1")
    m = _model(meta, torch.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    kw = dict(input_ids=t(g["input_ids"]), pixel_values=t(px), video_input_mask=t(g["video_input_mask"]), attention_mask=t(g["attention_mask"]),
              max_new_tokens=int(meta["new_tokens"]))
    plain = m.generate(**kw).cpu().numpy()
    for k in KS:
        ids = m.generate(**kw, prompt_lookup_num_tokens=k).cpu().numpy()
        assert np.array_equal(ids, plain), (k, ids, plain)
