"""-m gpu: rows that continue one shared, prefilled prefix (include/eilev_prefix.h, libeilev_hip_prefix.so; HipEngine.prefill_context /
extend_shared / greedy_decode_context, model.encode_context / generate(context=) / classify(share_prompt_cache=True)).

1. the attention kernel alone, on the case list of tests/prefix_cases.py, against the float64 reference and the derived tolerance of
   tests/attn_decode_ref.py (tests/test_prefix_ref.py holds the same list to the kernel's fp32 restatement on the CPU);
2. extend_shared = one prefill over [prefix | new] of every row;
3. the decode wiring (eilev_opt_decode_step_beam + eilev_greedy_select after the extend) = teacher forcing;
4. generate(context=) on the goldens;  5. classify(share_prompt_cache=True) on the goldens."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prefix_cases as cases
from hip_utils import host, load_case, models, rel_rms

pytestmark = pytest.mark.gpu

_WORST: dict = {}


def _px():
    from eilev_amd import abi

    return abi.load_prefix()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(name):
    c = cases.build_case(cases.by_name(name))
    return (c, *cases.reference(c))


@pytest.mark.parametrize("sp", cases.CASES, ids=lambda sp: sp.name)
def test_prefix_attention_against_float64(sp):
    """Acceptance: err <= 1.0 tol on every element (the project's derived bound); the sentinel row behind the last query and the inputs
    (with their NaN guard rows and slots) are bit-unchanged.  Every mutation of tests/prefix_cases.py exceeds 1.0 tol on the cases it
    applies to (tests/test_prefix_ref.py)."""
    from hip_utils import record_parity

    c, ref, A = _built(sp.name)
    pk = cases.pack(c)
    dev = lambda a: torch.from_numpy(a).cuda()
    qkv, kp, vp, out = dev(pk.qkv), dev(pk.kp), dev(pk.vp), dev(pk.out)
    D = pk.D
    rc = _px().eilev_prefix_attention(qkv.data_ptr(), 3 * D, qkv.data_ptr() + 2 * D, 3 * D, qkv.data_ptr() + 4 * D, 3 * D, kp.data_ptr(), vp.data_ptr(),
                                      sp.P, sp.cap, sp.R, sp.n, sp.heads, sp.hd, float(c.scale), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (sp.name, rc)
    raw = out.cpu().numpy()
    assert (raw[c.S].view(np.uint16) == cases.SENT16).all(), f"{sp.name}: the row behind the last query was written"
    got = cases_bits_to_f32(raw[:c.S]).reshape(c.S, sp.heads, sp.hd)
    ratio = cases.worst_ratio(got, ref, A)
    print(f"[prefix attention] {sp.name}: {ratio:.3f} tol")
    group = f"hd{sp.hd}"
    _WORST[group] = max(_WORST.get(group, 0.0), ratio)
    record_parity("prefix_attention", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element, no floor",
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()})
    if not ratio <= 1.0:
        err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - ref) / cases.tolerance(A)
        s, h, e = np.unravel_index(np.argmax(err), err.shape)
        pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at stacked query {s} (row {s // sp.n}, position {s % sp.n}) head {h} dim {e} "
                    f"(got {got[s, h, e]}, ref {ref[s, h, e]}); its spike at key {c.spike_pos[h, s]}")
    for name, t, a in (("qkv", qkv, pk.qkv), ("k_prefix", kp, pk.kp), ("v_prefix", vp, pk.vp)):
        assert np.array_equal(t.cpu().numpy(), a), f"{sp.name}: {name} changed"


def cases_bits_to_f32(b):
    from attn_decode_ref import bits_to_f32

    return bits_to_f32(b)


# ---- 2. extend_shared = one prefill ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lm_engine(cfg_name):
    """mid, or the real OPT-2.7B / OPT-6.7B widths (hd 80 / 128, 32 heads, vocab 50272) with two layers, as test_extend_equals_full_prefill builds them."""
    if cfg_name == "mid":
        return models("mid")[2]
    from eilev_amd.configs import blip2_config
    from eilev_amd.engine import HipEngine
    from eilev_amd.statedict import state_dict_shapes
    from eilev_amd.synth import synth_param

    cfg = blip2_config(cfg_name[:5])
    cfg.text_config.num_hidden_layers = 2
    named = {k: torch.from_numpy(synth_param(k, shp, "fanin")).to(torch.bfloat16).cuda()
             for k, shp in state_dict_shapes(cfg).items() if k.startswith("language_model")}
    return HipEngine(cfg, named, device="cuda", parts=("opt",))


@pytest.mark.parametrize("cfg_name,P,n", [("mid", 70, 20), ("opt27_2l", 300, 40), ("opt67_2l", 300, 40)])
def test_extend_shared_equals_one_prefill(cfg_name, P, n):
    """Three rows with different new embeddings after the same prefix: the logits of every new position against the existing prefill over
    [prefix | new] of each row (rel-RMS <= 5e-3), the K / V written to kv_rows against that prefill's slots [P, P + n) (<= 3e-3) — the
    bounds of test_extend_equals_full_prefill, where the two paths likewise run different kernels; without kv_rows the same bits."""
    eng = _lm_engine(cfg_name)
    d = eng.dims
    R, D, cap = 3, d.t_hidden, n + 3
    g = torch.Generator().manual_seed(5)
    prefix = (0.5 * torch.randn(1, P, D, generator=g)).to(torch.bfloat16).cuda()
    new = (0.5 * torch.randn(R, n, D, generator=g)).to(torch.bfloat16).cuda()
    ctx = eng.prefill_context(prefix)
    assert ctx.P == P and ctx.last_logits.shape == (1, d.vocab)
    kv_rows = eng.new_kv_cache(R, cap)
    kv_rows.view(torch.int16).fill_(0x7FC0)  # NaN bits: what the call does not write stays recognisable
    ext = eng.extend_shared(ctx, new, kv_rows=kv_rows, cap=cap, all_logits=True)
    ext_none = eng.extend_shared(ctx, new, all_logits=True)
    last = eng.extend_shared(ctx, new, kv_rows=kv_rows, cap=cap)
    full_emb = torch.cat((prefix.expand(R, -1, -1), new), dim=1).contiguous()
    am = torch.ones(R, P + n, dtype=torch.int32, device="cuda")
    _, full, kv_full = eng.prefill(full_emb, am, kv_capacity=P + n, all_logits=True, last_logits=False)
    torch.cuda.synchronize()
    dist = rel_rms(host(ext), host(full[:, P:]))
    print(f"[extend_shared] {cfg_name}: logits rel-rms {dist:.2e}")
    assert dist <= 5e-3
    assert torch.equal(ext, ext_none)
    assert rel_rms(host(last), host(full[:, -1])) <= 5e-3
    planes, H, hd = 2 * d.t_layers, d.t_heads, D // d.t_heads
    a = kv_rows.view(torch.bfloat16).view(planes, R, H, cap, hd)
    b = kv_full.view(torch.bfloat16).view(planes, R, H, P + n, hd)[:, :, :, P:]
    assert rel_rms(host(a[:, :, :, :n].float()), host(b.float())) <= 3e-3
    assert bool((a[:, :, :, n:].contiguous().view(torch.int16) == 0x7FC0).all()), "slots behind new_len were written"
    # the first P slots of the full prefill's cache are the context's own
    c0 = ctx.kv.view(torch.bfloat16).view(planes, 1, H, P, hd)
    assert rel_rms(host(c0.float()), host(kv_full.view(torch.bfloat16).view(planes, R, H, P + n, hd)[:, :1, :, :P].float())) <= 3e-3


# ---- 3. the decode wiring -----------------------------------------------------------------------------------------------------------------------
STEP_BOUND = 1e-2  # the project's decode-step bound (test_hip_varied.py: rel-RMS of a step's logits)


@pytest.mark.parametrize("R", [3, 32])
@pytest.mark.parametrize("cfg_name,P,n", [("mid", 70, 12), ("opt27_2l", 300, 12)])
def test_decode_after_context_equals_teacher_forcing(cfg_name, P, n, R):
    """8 greedy tokens after extend_shared, eager with a trace; then ONE existing-route prefill with all logits over [prefix | new | the
    generated ids] of every row: every step's logits within the decode-step bound of it, the emitted id the arg-max of the step's own
    logits, the captured run the same ids, and an EOS id finishes its row and pads the rest.  A wrong position, KV slot or ancestor entry
    misses this by orders of magnitude."""
    eng = models("mid", "varied", seed=176)[2] if cfg_name == "mid" else _lm_engine(cfg_name)
    d = eng.dims
    D, T = d.t_hidden, 8
    g = torch.Generator().manual_seed(7 + R)
    prefix = (0.5 * torch.randn(1, P, D, generator=g)).to(torch.bfloat16).cuda()
    new = (0.5 * torch.randn(R, n, D, generator=g)).to(torch.bfloat16).cuda()
    ctx = eng.prefill_context(prefix)
    trace = []
    ids = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=False, trace=trace)
    assert ids.shape == (R, T) and len(trace) == T
    assert eng.context_stats == dict(path="shared", rows=R, prefix=P, new=n, steps=T)
    gen = eng.embed_scatter(ids[:, :T - 1], None, None)
    full_emb = torch.cat((prefix.expand(R, -1, -1), new, gen), dim=1).contiguous()
    L = P + n + T - 1
    _, full, _ = eng.prefill(full_emb, torch.ones(R, L, dtype=torch.int32, device="cuda"), all_logits=True, last_logits=False)
    torch.cuda.synchronize()
    worst = 0.0
    for k in range(T):
        step, ref = host(trace[k]), host(full[:, P + n - 1 + k])
        worst = max(worst, rel_rms(step, ref))
        assert np.array_equal(step[:, :d.vocab].argmax(-1), ids[:, k].cpu().numpy()), k
    print(f"[decode after context] {cfg_name} R={R}: worst step rel-rms {worst:.2e}")
    assert worst <= STEP_BOUND
    captured = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=True)
    assert torch.equal(captured, ids)
    again = eng.greedy_decode_context(ctx, new, T, eos_id=-1, use_graph=True)  # the cached graph, replayed
    assert torch.equal(again, ids)
    # EOS: the id row 0 emits at step 2 ends every row at its first occurrence; what follows is the pad id
    free = ids.cpu().numpy()
    eos, pad = int(free[0, 2]), 1
    want = free.copy()
    for r in range(R):
        hit = np.flatnonzero(free[r] == eos)
        if len(hit):
            want[r, hit[0] + 1:] = pad
    stop = max((np.flatnonzero(free[r] == eos)[0] + 1) if (free[r] == eos).any() else T for r in range(R))
    for use_graph in (False, True):
        got = eng.greedy_decode_context(ctx, new, T, eos_id=eos, pad_id=pad, use_graph=use_graph, poll_every=1).cpu().numpy()
        assert np.array_equal(got, want[:, :stop]), (use_graph, got, want)


# ---- 4. generate(context=) ------------------------------------------------------------------------------------------------------------------
def _build_model(meta):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration
    from oracle.runner import synth_state_dict

    cfg = blip2_config(meta["config"])
    m = VideoBlipForConditionalGeneration(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, meta.get("weight_mode", "fanin"), meta.get("weight_seed", 0)).items()}
    sd["language_model.lm_head.weight"] = sd["language_model.model.decoder.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to("cuda")


SPLIT = 29  # mid_b1 / mid_v1: BOS, two example clips with their texts, the separator | the query clip (8 slots) and its text


@pytest.mark.parametrize("name", ["mid_b1", "mid_v1"])
def test_generate_after_context_like_the_reference(golden_dir, name):
    """The golden prompt split at a clip boundary: encode_context on the two example clips, generate(context=) on the query clip and the
    question.  mid_v1 (ids that change from step to step, per-step logits in the fixture): oracle.parity.greedy_ids_vs_reference with its
    defaults.  mid_b1's fixture has no per-step logits for that function to judge a flip by, so its ids must EQUAL the reference's.  Then
    two rows of different visible length after one context: each row's ids are those of the row run alone."""
    from hip_utils import record_parity
    from oracle.parity import greedy_ids_vs_reference

    g, meta, px = load_case(golden_dir, name)
    m = _build_model(meta)
    t = lambda a: torch.from_numpy(a).cuda()
    ids, vm = t(g["input_ids"]), t(g["video_input_mask"])
    assert not bool(vm[0, SPLIT - 1]) and bool(vm[0, SPLIT]) and int(vm[0, :SPLIT].sum()) == 16
    n_new = meta["new_tokens"]
    ctx = m.encode_context(ids[:, :SPLIT], pixel_values=t(px[:2]), video_input_mask=vm[:, :SPLIT])
    assert ctx.P == SPLIT and torch.equal(ctx.input_ids, ids[:, :SPLIT])
    kw = dict(max_new_tokens=n_new, min_new_tokens=None, eos_token_id=meta.get("never_id", 511))
    out = m.generate(ids[:, SPLIT:], pixel_values=t(px[2:]), video_input_mask=vm[:, SPLIT:], context=ctx, **kw)
    got, ref = out.cpu().numpy(), g["fp32_greedy_free"]
    assert m.engine().context_stats == dict(path="shared", rows=1, prefix=SPLIT, new=ids.shape[1] - SPLIT, steps=n_new)
    exact = bool(np.array_equal(got, ref))
    record_parity(f"generate_context[{name}]", ids_equal_reference=float(exact))
    if "fp32_step_logits_top8" in g.files:
        verdict = greedy_ids_vs_reference(got, g)
        assert verdict["ok"], verdict
    else:
        assert exact, (got, ref)
    # max_length counts the context: the same budget gives the same ids
    again = m.generate(ids[:, SPLIT:], pixel_values=t(px[2:]), video_input_mask=vm[:, SPLIT:], context=ctx, max_length=ids.shape[1] + n_new,
                       eos_token_id=meta.get("never_id", 511))
    assert torch.equal(again, out)
    # two rows, the second two tokens shorter and left-padded
    S = ids.shape[1] - SPLIT
    row_a, vm_a = ids[0, SPLIT:], vm[0, SPLIT:]
    row_b = torch.cat((torch.full((2,), 1, dtype=ids.dtype, device="cuda"), ids[0, SPLIT:-2]))
    vm_b = torch.cat((torch.zeros(2, dtype=vm.dtype, device="cuda"), vm[0, SPLIT:-2]))
    am = torch.ones(2, S, dtype=torch.int64, device="cuda")
    am[1, :2] = 0
    px2 = t(np.concatenate([px[2:], px[2:]]))
    both = m.generate(torch.stack((row_a, row_b)), pixel_values=px2, video_input_mask=torch.stack((vm_a, vm_b)), attention_mask=am, context=ctx, **kw)
    assert m.engine().context_stats["path"] == "shared" and m.engine().context_stats["rows"] == 2
    alone_b = m.generate(ids[:, SPLIT:-2], pixel_values=t(px[2:]), video_input_mask=vm[:, SPLIT:-2], context=ctx, **kw)
    assert torch.equal(both[0], out[0]) and torch.equal(both[1], alone_b[0])
    # ... and the shorter row equals the existing route on its whole prompt
    whole_b = m.generate(ids[:, :-2], pixel_values=t(px), video_input_mask=vm[:, :-2], **kw)
    assert torch.equal(alone_b, whole_b)
    # a parameter update makes the context stale
    with torch.no_grad():
        m.language_model.model.decoder.final_layer_norm.bias.add_(0.5)
    with pytest.raises(ValueError, match="stale"):
        m.generate(ids[:, SPLIT:], pixel_values=t(px[2:]), video_input_mask=vm[:, SPLIT:], context=ctx, **kw)


# ---- 5. classify(share_prompt_cache=True) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["mid_b1", "mid_b2"])
def test_classify_with_a_shared_prompt_cache(golden_dir, name, dtype):
    """The assertion of test_classify_like_the_reference on the shared route; agreement with the default route within that test's
    max(2e-2, ulp), also in class chunks; and the shared call's peak memory lies below the default route's by at least (classes - 1) cache
    rows (the default route holds one copy of the prompt's cache per class)."""
    g, meta, px = load_case(golden_dir, name)
    m = _build_model(meta).to(dtype)
    t = lambda a: torch.from_numpy(a).cuda()
    kw = dict(prompt_attention_mask=t(g["attention_mask"]), pixel_values=t(px).to(dtype),
              prompt_video_input_mask=t(g["video_input_mask"]), class_attention_mask=t(g["class_attention_mask"]))
    args = (t(g["input_ids"]), t(g["class_input_ids"]))
    for share in (True, False):  # (first use of both routes: the engine, the kernels' modules and the workspaces, which the engine keeps)
        m.classify(*args, share_prompt_cache=share, **kw)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ll = m.classify(*args, share_prompt_cache=True, **kw)
    torch.cuda.synchronize()
    peak_shared = torch.cuda.max_memory_allocated() - base
    assert ll.dtype == dtype and ll.shape == g["fp32_classify"].shape
    truth, ref_bf16 = g["fp32_classify"], g["bf16_classify"]
    budget = 1.5 * np.abs(ref_bf16 - truth).max() + 2e-2
    assert np.abs(host(ll) - truth).max() <= budget, (host(ll), truth)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ll_default = m.classify(*args, **kw)
    torch.cuda.synchronize()
    peak_default = torch.cuda.max_memory_allocated() - base
    ulp = 2.0 ** -7 * np.abs(host(ll_default)).max() if dtype == torch.bfloat16 else 0.0
    assert np.abs(host(ll) - host(ll_default)).max() <= max(2e-2, ulp)
    ll2 = m.classify(*args, share_prompt_cache=True, class_batch_size=2, **kw)
    assert np.abs(host(ll2) - host(ll)).max() <= max(2e-2, ulp)
    eng = m.engine()
    n_cls, L = g["class_input_ids"].shape[0], g["input_ids"].shape[1]
    row = int(eng.lib.eilev_opt_kv_cache_bytes(C.byref(eng.dims), 1, L))
    print(f"[classify shared] {name} {dtype}: peak {peak_shared} B shared, {peak_default} B default, a cache row {row} B")
    assert peak_default - peak_shared >= (n_cls - 1) * row, (peak_default, peak_shared, row)
