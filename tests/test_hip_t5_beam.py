"""-m gpu: flan-t5 beam search on the device (include/eilev_t5beam.h, libeilev_hip_t5beam.so; HipEngine.t5_beam).

1. the shared-sample cross-attention kernel alone, on the case list of tests/t5beam_cases.py, against the float64 reference and the derived
   tolerance of tests/attn_decode_ref.py (tests/test_t5beam_ref.py holds the same list to the kernels' fp32 restatement on the CPU);
2. the decode step in the beam form = teacher forcing, under a scripted ancestry;
3. the loops: torch selection, the two selection kernels eager and captured, the old host loop;
4. the logits rules inside the device loop;  5. generate();  6. more than 32 rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attn_decode_ref as R
import t5beam_cases as cases
from hip_utils import host, load_case, models, rel_rms

pytestmark = pytest.mark.gpu

SENT32 = 0x7FA5A5A5  # poison of `part` (a NaN as float)
SENT16 = 0x7FA5      # poison of `out` (a NaN as bf16)
_WORST: dict = {}


def _tb():
    from eilev_amd import abi

    return abi.load_t5beam()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_bits(a):
    return torch.from_numpy(R.bf16_bits(a)).cuda().view(torch.bfloat16)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
def _run_cross(sp):
    """One case: every slot of [enc_len, cap) holds NaN bits, out and part are poisoned; launched in sample groups of at most 32 rows."""
    c = R.build_case(sp)
    ref, A = R.reference(c)
    n, d = sp.seq_len, c.d
    kc, vc = c.kc.copy(), c.vc.copy()
    kc[:, :, n:], vc[:, :, n:] = np.nan, np.nan
    q, K, V = _dev_bits(c.qkv), _dev_bits(kc), _dev_bits(vc)
    mask = torch.from_numpy(c.mask).cuda().contiguous() if c.mask is not None else None
    out = torch.full((sp.batch, d), SENT16, dtype=torch.int16, device="cuda")
    per = max(1, 32 // sp.beams)
    for s0 in range(0, c.srows, per):
        s1 = min(c.srows, s0 + per)
        rows = (s1 - s0) * sp.beams
        ns = -(-n // 128)
        words = rows * sp.heads * ns * (sp.hd + 2)
        part = torch.full((words + 64,), SENT32, dtype=torch.int32, device="cuda")
        rc = _tb().eilev_t5beam_cross_attention(
            q[s0 * sp.beams:].data_ptr(), c.ldq, K[s0:].data_ptr(), V[s0:].data_ptr(), None if mask is None else mask[s0:].data_ptr(), rows, sp.beams,
            sp.heads, sp.hd, n, sp.cap, out[s0 * sp.beams:].data_ptr(), part.data_ptr(), 4 * words, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (sp.name, rc)
        p = part.cpu().numpy()
        assert (p[:words] != SENT32).all() and (p[words:] == SENT32).all(), f"{sp.name}: the records of the 128-key ranges"
    got = R.bits_to_f32(out.cpu().numpy()).reshape(sp.batch, d)
    ratio = R.worst_ratio(got, ref, A)
    if not ratio <= 1.0:
        err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - ref) / R.tolerance(A)
        b, col = np.unravel_index(np.argmax(err), err.shape)
        pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at row {b} head {col // sp.hd} dim {col % sp.hd} (got {got[b, col]}, ref {ref[b, col]}); "
                    f"that head's spike at key {c.spike_pos[b, col // sp.hd]}")
    assert np.array_equal(R.bf16_bits(kc), K.view(torch.int16).cpu().numpy()) and np.array_equal(R.bf16_bits(vc), V.view(torch.int16).cpu().numpy())
    return ratio


@pytest.mark.parametrize("group", list(cases.GROUPS))
def test_shared_sample_cross_attention_against_float64(group):
    """Acceptance: err <= 1.0 tol on every element of every case (the project's derived bound).  A key dropped, doubled or paired with the
    wrong value moves its (row, head) by more than 10 tol on this list (tests/test_t5beam_ref.py)."""
    from hip_utils import record_parity

    try:
        for sp in cases.GROUPS[group]():
            ratio = _run_cross(sp)
            print(f"[cross] {sp.name}: {ratio:.3f} tol")
            _WORST[group] = max(_WORST.get(group, 0.0), ratio)
    finally:
        record_parity("t5beam_cross_attention", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element, no floor",
                      **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()})


# ---- 2. the step ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _xl_engine():
    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.statedict import state_dict_shapes
    from eilev_amd.synth import synth_param

    cfg = blip2_config("t5xl")
    cfg.text_config.num_layers = 2
    cfg.text_config.num_decoder_layers = 2
    named = {k: torch.from_numpy(synth_param(k, shp, "fanin")).to(torch.bfloat16).cuda()
             for k, shp in state_dict_shapes(cfg).items() if k.startswith("language_model")}
    return HipEngine(cfg, named, device="cuda", parts=("t5",))


STEP_BOUND = 1e-2  # rel_rms of the existing step test (test_t5_xl_widths_decode_equals_teacher_forcing)


@pytest.mark.parametrize("samples", [2, 6])
@pytest.mark.parametrize("model", ["mid_t5", "t5xl"])
def test_beam_step_equals_teacher_forcing_under_a_scripted_ancestry(model, samples):
    """6 steps on samples x 5 rows, L = 300, one sample right-padded: seeded random tokens, seeded random parents within each sample, the
    table gathered the way beam_decode's host `step` gathers it; the logits of row r = t5_forward on the hypothesis row r now holds.  The
    generation cache starts as NaN bits.  Control: against a hypothesis with ONE ancestor swapped the distance exceeds 5 x the bound."""
    from eilev_amd import abi

    eng = models("mid_t5")[2] if model == "mid_t5" else _xl_engine()
    d, tb = eng.t5dims, _tb()
    beams, L, steps, gen_cap = 5, 300, 6, 8
    B, Rr = samples, samples * 5
    g = torch.Generator().manual_seed(11 + samples)
    emb = (0.5 * torch.randn(B, L, d.d_model, generator=g)).to(torch.bfloat16).cuda()
    am = torch.ones(B, L, dtype=torch.int32, device="cuda")
    am[1, 250:] = 0
    enc = eng.t5_encode(emb, am)
    ckv = eng.t5_cross_kv(enc)
    kv_start = torch.empty(int(eng.lib.eilev_t5_self_kv_bytes(C.byref(d), B, 1)), dtype=torch.uint8, device="cuda")
    eng.t5_decode(torch.zeros(B, 1, dtype=torch.int64, device="cuda"), am, 0, kv_start, 1, ckv, L)
    kv_gen = torch.full((int(eng.lib.eilev_t5_self_kv_bytes(C.byref(d), Rr, gen_cap)) // 2,), R.NAN_BITS, dtype=torch.int16, device="cuda")
    anc = torch.zeros((gen_cap, Rr), dtype=torch.int32, device="cuda")
    ident = torch.arange(Rr, dtype=torch.int32, device="cuda")
    state = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    tokens = torch.zeros(Rr, dtype=torch.int64, device="cuda")
    logits = torch.empty((Rr, d.vocab), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(tb.eilev_t5beam_workspace_bytes(C.byref(d), Rr, beams, L, gen_cap)), dtype=torch.uint8, device="cuda")
    emb_r, am_r = emb.repeat_interleave(beams, dim=0), am.repeat_interleave(beams, dim=0)
    base = (torch.arange(Rr) // beams) * beams
    hyp = torch.zeros((Rr, 1), dtype=torch.int64)  # decoder ids of the hypothesis in row r, the start token in front
    fed = []                                        # fed[t][r]: the token that went to slot t of physical row r
    worst = 0.0
    for t in range(steps):
        toks = torch.randint(2, d.vocab, (Rr,), generator=g)
        parents = base + torch.randint(0, beams, (Rr,), generator=g)
        if t > 0:
            anc[:t] = anc[:t].index_select(1, parents.cuda())
        anc[t] = ident
        hyp = torch.cat((hyp[parents], toks[:, None]), dim=1)
        fed.append(toks)
        tokens.copy_(toks)
        abi.check(tb.eilev_t5beam_decode_step(C.byref(d), C.byref(eng.pack.t5), tokens.data_ptr(), state.data_ptr(), am.data_ptr(), Rr, beams,
                                              kv_start.data_ptr(), kv_gen.data_ptr(), gen_cap, anc.data_ptr(), ckv.data_ptr(), L, logits.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream()), "eilev_t5beam_decode_step")
        assert int(state[0]) == t + 2
        full, _ = eng.t5_forward(emb_r, am_r, hyp.cuda())
        dist = rel_rms(host(logits), host(full[:, -1]))
        print(f"[step] {model} {samples} x 5, step {t}: rel_rms {dist:.2e}")
        worst = max(worst, dist)
        assert dist <= STEP_BOUND, (t, dist)
    # control: slot g of every row's hypothesis taken from another row of its sample that was fed a different token there
    a = anc.cpu().long()
    gslot = steps // 2
    wrong = hyp.clone()
    for r in range(Rr):
        others = [o for o in range(int(base[r]), int(base[r]) + beams) if o != int(a[gslot, r]) and int(fed[gslot][o]) != int(hyp[r, 1 + gslot])]
        assert others
        wrong[r, 1 + gslot] = fed[gslot][others[0]]
    full, _ = eng.t5_forward(emb_r, am_r, wrong.cuda())
    ctrl = rel_rms(host(logits), host(full[:, -1]))
    print(f"[step] {model} {samples} x 5: worst {worst:.2e}, control {ctrl:.2e}")
    assert ctrl > 5 * STEP_BOUND, ctrl


# ---- 3. the loops -----------------------------------------------------------------------------------------------------------------------------
def _case(golden_dir, name):
    g, meta, px = load_case(golden_dir, name)
    _, _, eng = models(meta["config"])
    t = lambda a: torch.from_numpy(a).cuda()
    return g, meta, eng, eng.embed_scatter(t(g["input_ids"]), t(g["video_input_mask"]), eng.encode_clips(t(px))), t(g["attention_mask"])


class _Switches:
    """Engine switches for one block, put back afterwards."""

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        self.old = {k: getattr(self.eng, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.eng, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.eng, k, v)


def _score(eng, emb, am, rows, eos, lp):
    """Length-penalised score of each returned hypothesis under the engine's own teacher-forced log-probabilities (test_t5_beam_search's rule)."""
    out = []
    for b, row in enumerate(rows):
        toks = [int(x) for x in row[1:]]
        if eos >= 0 and eos in toks:
            toks = toks[: toks.index(eos) + 1]
        dec = torch.tensor([[0] + toks[:-1]], device="cuda")
        logits, _ = eng.t5_forward(emb[b:b + 1], am[b:b + 1], dec)
        lp_ = torch.log_softmax(logits[0].float(), -1)
        out.append(float(sum(lp_[i, tok] for i, tok in enumerate(toks))) / len(toks) ** lp)
    return np.array(out)


@pytest.mark.parametrize("nb,lp", [(5, -1.0), (3, 1.0)])
@pytest.mark.parametrize("name", ["mid_t5_b1", "mid_t5_b2"])
def test_device_loops_agree_and_match_the_host_loop(golden_dir, name, nb, lp):
    g, meta, eng, emb, am = _case(golden_dir, name)
    n, B = meta["new_tokens"], emb.shape[0]
    for eos in (int(g["fp32_eos_id"]), -1):
        call = lambda **kw: eng.t5_beam(emb, am, n, nb, lp, eos_id=eos, **kw)
        with _Switches(eng, beam_topk_kernel=False, beam_advance_kernel=False):
            eng.t5_beam_stats = None
            torch_sel = call(use_graph=False)
            assert eng.t5_beam_stats == dict(path="device", steps=torch_sel.shape[1] - 1)
        fused = call()
        assert eng.t5_beam_stats["path"] == "device"
        with _Switches(eng, beam_capture=True):
            captured = call()
            assert eng.t5_beam_stats["path"] == "device"
        assert torch.equal(torch_sel, fused) and torch.equal(fused, captured), (torch_sel.tolist(), fused.tolist(), captured.tolist())
        assert fused.shape[0] == B and bool((fused[:, 0] == 0).all())
        with _Switches(eng, beam_device_loop=False):
            old = call()
            assert eng.t5_beam_stats == dict(path="host", steps=old.shape[1] - 1)
        if not (old.shape == fused.shape and torch.equal(old, fused)):  # the two steps round differently: a tie under test_t5_beam_search's rule
            mine, theirs = _score(eng, emb, am, fused.tolist(), eos, lp), _score(eng, emb, am, old.tolist(), eos, lp)
            assert np.all(np.abs(mine - theirs) <= 2e-2 * np.abs(theirs) + 1e-3), (fused.tolist(), old.tolist(), mine, theirs)
        two = call(num_return_sequences=2)
        assert two.shape[0] == B * 2 and torch.equal(two[::2, : fused.shape[1]], fused[:, : two.shape[1]])


# ---- 4. rules on the device ---------------------------------------------------------------------------------------------------------------------
def _no_repeated_ngram(row, n):
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) == len(set(grams))


class _Never:
    """a stopping criterion that never fires"""

    def __call__(self, input_ids, scores, **kw):
        return torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)


@pytest.mark.parametrize("name,nb", [("mid_t5_b2", 3), ("mid_t5_b1", 5)])
def test_rules_run_inside_the_device_loop(golden_dir, name, nb):
    from transformers import LogitsProcessorList

    g, meta, eng, emb, am = _case(golden_dir, name)
    T = 8
    first = int(eng.t5_beam(emb, am, T, nb, 1.0, eos_id=-1)[0, 1])
    sets = [dict(eos=-1, min_new=0, rules=dict(no_repeat_ngram_size=2)),
            dict(eos=first, min_new=2, rules=dict(repetition_penalty=1.15, no_repeat_ngram_size=3)),
            dict(eos=-1, min_new=0, rules=dict(no_repeat_ngram_size=1))]
    for s in sets:
        call = lambda **more: eng.t5_beam(emb, am, T, nb, 1.0, eos_id=s["eos"], min_new_tokens=s["min_new"], rules=dict(s["rules"], **more))
        eng.t5_beam_stats = eng.rules_stats = None
        ids = call()
        assert eng.t5_beam_stats["path"] == "device" and eng.rules_stats["path"] == "device", s
        assert bool((ids[:, 0] == 0).all()) and ids.shape[0] == emb.shape[0]
        ngram = s["rules"]["no_repeat_ngram_size"]
        for row in ids.tolist():
            body = row[1:]
            if s["eos"] >= 0:
                assert s["eos"] not in body[: s["min_new"]], (s, row)
                if s["eos"] in body:
                    body = body[: body.index(s["eos"]) + 1]
            assert _no_repeated_ngram([row[0]] + body, ngram), (s, row)  # (the start token counts)
            if ngram == 1:
                assert 0 not in body
        with _Switches(eng, beam_capture=True):
            assert torch.equal(call(), ids)
        for more in (dict(processors=LogitsProcessorList([])), dict(stopping=_Never())):
            eng.t5_beam_stats = None
            call(**more)
            assert eng.t5_beam_stats["path"] == "host", (s, more)


# ---- 5. the model API -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(config_name):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration
    from eilev_amd.synth import synth_interleaved_ids, synth_pixels

    torch.manual_seed(0)
    cfg = blip2_config(config_name)
    model = VideoBlipForConditionalGeneration(cfg).to(torch.bfloat16).cuda().eval()
    nq, vocab = cfg.num_query_tokens, cfg.text_config.vocab_size
    ids, vm = zip(*[synth_interleaved_ids([1, 1], [5, 4], nq, vocab, seed=3 + s) for s in range(2)])
    px = torch.from_numpy(synth_pixels(4, 2, cfg.vision_config.image_size)).cuda()
    return model, dict(input_ids=torch.from_numpy(np.stack(ids)).cuda(), pixel_values=px, video_input_mask=torch.from_numpy(np.stack(vm)).cuda())


@pytest.mark.parametrize("config_name,path", [("mid_t5", "device"), ("tiny_t5", "host")])
def test_generate_takes_the_device_path_at_head_size_64(config_name, path):
    model, kw = _model(config_name)
    eng = model.engine()
    vocab = model.config.text_config.vocab_size
    for call in (dict(num_beams=3), dict(num_beams=3, no_repeat_ngram_size=2)):
        eng.t5_beam_stats = None
        out = model.generate(**kw, max_new_tokens=6, eos_token_id=None, **call)
        assert eng.t5_beam_stats is not None and eng.t5_beam_stats["path"] == path, (config_name, call)
        assert out.dtype == torch.int64 and out.shape[0] == 2 and out.shape[1] <= 7 and bool((out[:, 0] == 0).all()) and int(out.min()) >= 0 and int(out.max()) < vocab
        if "no_repeat_ngram_size" in call:
            assert all(_no_repeated_ngram(r, 2) for r in out.tolist())
        with _Switches(eng, beam_device_loop=False):  # the host loop: what the call returned before there was a device path
            old = model.generate(**kw, max_new_tokens=6, eos_token_id=None, **call)
            assert eng.t5_beam_stats["path"] == "host" and old.shape == out.shape and old.dtype == out.dtype
        if path == "host":
            assert torch.equal(old, out)


# ---- 6. more rows than one call takes ----------------------------------------------------------------------------------------------------------
def test_forty_rows_run_in_sample_groups():
    """8 samples x 5 beams: sample groups of 6 and 2; every row is the row of the same call made for its sample alone (up to the padding of
    a row that finished early)."""
    eng = models("mid_t5")[2]
    g = torch.Generator().manual_seed(5)
    B, L, T, nb = 8, 40, 6, 5
    emb = (0.5 * torch.randn(B, L, eng.t5dims.d_model, generator=g)).to(torch.bfloat16).cuda()
    am = torch.ones(B, L, dtype=torch.int32, device="cuda")
    am[3, 30:] = 0
    eos = int(eng.t5_beam(emb[:1], am[:1], T, nb, -1.0, eos_id=-1)[0, 3])
    eng.t5_beam_stats = None
    ids = eng.t5_beam(emb, am, T, nb, -1.0, eos_id=eos)
    assert eng.t5_beam_stats["path"] == "device" and ids.shape[0] == B
    for b in range(B):
        one = eng.t5_beam(emb[b:b + 1], am[b:b + 1], T, nb, -1.0, eos_id=eos)
        k = one.shape[1]
        assert torch.equal(ids[b, :k], one[0]) and bool((ids[b, k:] == eos).all()), (b, ids[b].tolist(), one[0].tolist())
