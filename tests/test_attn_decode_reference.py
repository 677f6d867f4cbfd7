"""CPU checks of tests/attn_decode_ref.py — the float64 reference, the case builder and the derived tolerance that
test_hip_attn_decode.py holds the decode-attention kernels to — so that the GPU tests rest on a reference that was itself compared with
torch, on inputs an fp32 restatement of the kernels' arithmetic passes, and on cases that an index mistake of one key fails."""
import numpy as np
import pytest
import torch

import attn_decode_ref as R
from attn_decode_ref import Spec


def _sdpa(c, b):
    """torch float64 scaled_dot_product_attention(scale = 1) of row b on what the row attends to."""
    K, V, vis, bias = R.effective(c, b)
    q = torch.from_numpy(R._q(c, b).astype(np.float64))[:, None, :]
    m = torch.zeros(c.spec.heads, 1, c.n, dtype=torch.float64)
    if bias is not None:
        m += torch.from_numpy(bias)[:, None, :]
    m = m.masked_fill(~torch.from_numpy(vis)[None, None, :], float("-inf"))
    o = torch.nn.functional.scaled_dot_product_attention(q[None], torch.from_numpy(K.astype(np.float64))[None], torch.from_numpy(V.astype(np.float64))[None],
                                                         attn_mask=m[None], scale=1.0)
    return o[0, :, 0, :].numpy().reshape(-1)


@pytest.mark.parametrize("sp", [
    Spec("plain", "split", batch=3, heads=4, hd=80, seq_len=200, cap=260, n_gen=9, spikes="mix", stale="trap"),
    Spec("masked", "split", batch=8, heads=4, hd=80, seq_len=330, cap=400, n_gen=5, mask="mixed", spikes="mix", stale="nan"),
    Spec("biased-rel", "split", batch=2, heads=6, hd=64, seq_len=0, cap=150, n_gen=140, bias="rel", ldq_extra=128, spikes="mix"),
    Spec("biased-row", "split", batch=2, heads=6, hd=64, seq_len=77, cap=80, n_gen=None, fuse_new=0, ldq_extra=32, mask="ones", bias="row", spikes="mix"),
], ids=lambda s: s.name)
def test_reference_equals_torch_sdpa_in_float64(sp):
    c = R.build_case(sp)
    ref, A = R.reference(c)
    for b in range(sp.batch):
        _, _, vis, _ = R.effective(c, b)
        assert vis.any()
        np.testing.assert_allclose(ref[b], _sdpa(c, b), rtol=1e-12, atol=1e-13)
    assert (A >= np.abs(ref) - 1e-12).all()


def test_a_row_with_no_visible_key_is_zero():
    c = R.build_case(Spec("dead", "split", batch=4, heads=2, hd=64, seq_len=400, cap=400, n_gen=None, fuse_new=0, ldq_extra=64, mask="pad300+dead", spikes="mix"))
    ref, A = R.reference(c)
    assert not ref[3].any() and not A[3].any() and ref[:3].any(1).all()
    assert R.tolerance(A)[3].max() == R.TOL_FLOOR
    assert not R.merge_ref(R.partials_ref(c, 128))[3].any()


def test_spike_takes_half_the_weight_and_traps_are_invisible():
    sp = Spec("w", "split", batch=8, heads=4, hd=80, seq_len=530, cap=700, n_gen=3, mask="mixed", spikes="mix", stale="trap")
    c = R.build_case(sp)
    for b in range(sp.batch):
        K, V, vis, bias = R.effective(c, b)
        s = R.scores64(c, b, K, bias)
        assert np.abs(s[:, vis]).max() < 50.0
        p = np.exp(s[:, vis] - s[:, vis].max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        for h in range(sp.heads):
            j = c.spike_pos[b, h]
            assert vis[j] and abs(p[h, np.flatnonzero(vis).tolist().index(j)] - 0.5) < 0.02 and np.abs(V[h, j]).max() == 8.0
        masked = np.flatnonzero(~vis)
        if len(masked):  # a trap: 30 above the row's maximum, values of +-64
            assert (s[:, masked].min(1) > s[:, vis].max(1) + 29.0).all() and (np.abs(V[:, masked]) == 64.0).all()
        assert (np.abs(c.vc[b][:, c.n:]) == 64.0).all()
    nan = R.build_case(Spec("n", "split", batch=2, heads=2, hd=40, seq_len=20, cap=40, n_gen=3, stale="nan"))
    assert (R.bf16_bits(nan.kc[:, :, nan.n:]).view(np.uint16) == R.NAN_BITS).all() and np.isfinite(nan.kc[:, :, :nan.n]).all()


def test_seeds_differ_per_row_and_head():
    k = R.base_plane("k", 3, 4, 16, 8)
    flat = k.reshape(12, -1)
    assert len({row.tobytes() for row in flat}) == 12
    assert np.array_equal(R.base_plane("k", 3, 4, 9, 8), k[:, :, :9])


def test_beam_reference_equals_plain_reference_on_a_materialised_cache():
    sp = Spec("beam", "beam", batch=6, beams=3, heads=4, hd=80, seq_len=140, cap=140, cap_g=24, n_gen=17, spikes="beam", mask="mixed", mask_first=5, stale="trap")
    c = R.build_case(sp)
    assert ((c.anc // sp.beams) == (np.arange(sp.batch) // sp.beams)[None, :]).all() and (c.anc[16] == np.arange(6)).all()
    assert (c.anc[:16] != np.arange(6)[None, :]).any()
    ref, A = R.reference(c)
    # the same hypotheses with every row's keys copied into a cache of its own: a plain case
    plain = R.build_case(Spec("p", "split", batch=6, heads=4, hd=80, seq_len=140, cap=140 + 24, n_gen=17, spikes="none", mask="none", stale="rand"))
    plain.qkv = c.qkv.copy()
    plain.mask = np.repeat(c.mask, sp.beams, axis=0)
    for b in range(6):
        K, V, _, _ = R.effective(c, b)
        plain.kc[b, :, :c.n], plain.vc[b, :, :c.n] = K, V
    pref, pA = R.reference(plain)
    np.testing.assert_allclose(ref, pref, rtol=0, atol=0)
    np.testing.assert_allclose(A, pA, rtol=0, atol=0)
    kinds = {int(np.clip(j - sp.seq_len + 1, 0, 1)) + int(j == c.n - 1) for j in c.spike_pos.ravel()}
    assert kinds == {0, 1, 2}  # prompt keys, older generated keys, the newest key


@pytest.mark.parametrize("keys", [128, 256])
def test_float64_merge_of_partials_equals_the_unsplit_reference(keys):
    for sp in (Spec("m", "split", batch=8, heads=3, hd=80, seq_len=530, cap=1024, n_gen=3, mask="mixed", spikes="mix", stale="nan"),
               Spec("b", "beam", batch=5, beams=5, heads=3, hd=80, seq_len=420, cap=420, cap_g=40, n_gen=17, spikes="beam", mask="mixed", mask_first=5)):
        c = R.build_case(sp)
        part = R.partials_ref(c, keys)
        assert part.shape[2] == -(-(sp.cap if not sp.beams else sp.seq_len + sp.cap_g) // keys)
        empty = part[..., 1] == 0
        assert empty.any() and (part[..., 0][empty] == -1e30).all()
        part[..., 2:][empty] = np.nan  # what an empty range leaves in o is never read
        ref, A = R.reference(c)
        assert R.worst_ratio(R.merge_ref(part), ref, A) < 1e-9


def test_frag32_index_is_a_permutation_of_the_row_block():
    rows, cols = np.meshgrid(np.arange(32), np.arange(2560), indexing="ij")
    idx = R.frag32_index(rows, cols)
    assert sorted(idx.ravel().tolist()) == list(range(32 * 2560))
    assert R.frag32_index(5, 77) == 2 * 1024 + 5 * 32 + 13


# ---- the launches of the GPU tests: an fp32 restatement of the kernels' arithmetic passes them, an index mistake does not ----------------
_SPECS = R.all_specs()


def test_the_case_list_reaches_every_form_and_every_slot():
    forms = {sp.form for sp in _SPECS}
    assert forms == {"one80", "one64", "part128", "part256", "loop80", "loop64", "beam", "split"}
    names = [sp.name for sp in _SPECS]
    assert len(set(names)) == len(names)
    cover = {}
    for sp in R.cover_specs():
        form = sp.name.split("-")[1]
        got = cover.setdefault(form, (sp.cap, set()))[1]
        k = sp.spikes[1]
        got.update(range(k * sp.batch * sp.heads, min(sp.cap, (k + 1) * sp.batch * sp.heads)))
        assert R.kv_total_of(sp) == sp.cap
    for form, (cap, got) in cover.items():
        assert got == set(range(cap)), form
    c = R.build_case(R.cover_specs()[1])
    assert sorted(c.spike_pos.ravel().tolist()) == list(range(256, 512))
    for form in ("one80", "one64", "part128", "part256", "loop80", "loop64", "split"):
        G = R.FORMS[form]["G"]
        ns = {R.kv_total_of(sp) for sp in _SPECS if sp.name.startswith(f"sweep-{form}-")}
        want = {1, 2, G - 1, G, G + 1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024}
        if R.FORMS[form]["top"] >= 2048:
            want |= {1025, 2047, 2048}
        if R.FORMS[form]["top"] > 2048:
            want |= {2049}
        assert ns == want, form
        assert any(R.kv_total_of(sp) == sp.cap for sp in _SPECS if sp.name.startswith(f"sweep-{form}-"))


def _chunks(n):
    per = -(-len(_SPECS) // n)
    return [_SPECS[i * per:(i + 1) * per] for i in range(n)]


@pytest.mark.parametrize("chunk", range(8))
def test_fp32_restatement_of_the_range_loop_is_within_tol_on_every_gpu_case(chunk):
    worst = (0.0, "")
    for sp in _chunks(8)[chunk]:
        c = R.build_case(sp)
        ref, A = R.reference(c)
        r = R.worst_ratio(R.emulate_ranges(c, R.emu_keys(sp)), ref, A)
        worst = max(worst, (r, sp.name))
        assert r <= 1.0, (sp.name, r)
    print(f"chunk {chunk}: worst err/tol {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("mutate", ["drop", "double", "shift"])
def test_an_index_mistake_of_one_key_exceeds_tol_on_the_spiked_cases(mutate):
    """One key dropped, one key counted twice, or P paired with the neighbouring slot's V: each leaves tol far behind in EVERY (row, head)
    that carries a spike, so the GPU tests can fail."""
    picks = [sp for sp in _SPECS if sp.name in ("cover-one80-1", "cover-part128-3", "cover-loop64-2", "sweep-part256-257-seq-newest", "sweep-loop80-513-state-second",
                                                "mask-split-trap", "beam-beam-3x2-g17-trap", "t5-self-rel-g300-split")]
    assert len(picks) == 8
    for sp in picks:
        c = R.build_case(sp)
        ref, A = R.reference(c)
        err = np.abs(R.emulate_ranges(c, R.emu_keys(sp), mutate) - ref) / R.tolerance(A)
        per_head = err.reshape(sp.batch, sp.heads, sp.hd).max(-1)
        spiked = c.spike_pos >= 0
        assert spiked.any()
        print(f"{mutate} {sp.name}: err/tol min over spiked (row, head) {per_head[spiked].min():.1f}, median {np.median(per_head[spiked]):.1f}")
        assert (per_head[spiked] > 10.0).all(), (sp.name, mutate, per_head[spiked].min())


def test_probe_entry_exists_in_the_probe_build_only_and_refuses_a_stale_mirror():
    import ctypes
    import os

    from eilev_amd import abi
    from test_hip_attn_decode import AttnDecodeArgs

    assert ctypes.sizeof(AttnDecodeArgs) == 152 and AttnDecodeArgs.out_frag.offset == 148 and AttnDecodeArgs.part.offset == 80
    if os.path.exists(abi.HIP_LIB_PATH):
        assert not hasattr(ctypes.CDLL(abi.HIP_LIB_PATH), "eilev_debug_attn_decode")
    if not os.path.exists(abi.PROBES_LIB_PATH):
        pytest.skip("libeilev_hip_probes.so not built")
    fn = ctypes.CDLL(abi.PROBES_LIB_PATH).eilev_debug_attn_decode  # (loads without a GPU; these calls return before any HIP call)
    fn.argtypes = [ctypes.POINTER(AttnDecodeArgs), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    a = AttnDecodeArgs()
    assert fn(ctypes.byref(a), 144, 0, None, None) == -1 and fn(ctypes.byref(a), 160, 0, None, None) == -1
    assert fn(ctypes.byref(a), 152, 3, None, None) == -1 and fn(None, 152, 0, None, None) == -1
    assert fn(ctypes.byref(a), 152, 0, None, None) == -1  # out == nullptr and no nsplit: launch_attn_decode's own refusal
