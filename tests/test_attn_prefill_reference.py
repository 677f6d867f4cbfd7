"""CPU checks of tests/attn_prefill_ref.py, the reference of test_hip_attn_prefill.py: that an honest kernel stays inside the derived
tolerance on every launch of the GPU file (fp32 / bf16 numpy restatements of the four kernel families), that every planted key carries
the weight the derivation needs, and that every mistake the GPU tests are there to catch exceeds the tolerance at least four times.

Smallest err / tol per mutation over the cases it applies to (MUTATION_FLOOR below, from a run of this file; a kernel sitting a full tol off
the other way still fails by the factor less one): one key dropped 122, doubled 42, two keys' V swapped 201, all keys shifted 250, causal
limit + 1 / - 1 31 / 183, key mask ignored in one tile 770, one key past skv 1934, the next head's K 129, the next row's q 120, a skipped
rescale 12, position index + 1 / - 1 86 / 97, another head's table 71, scale dropped 65.  Where a mutation does not apply (attn_prefill_ref.
applies): the causal limit needs a row that sees a handful of keys (the left-padding cases), a skipped rescale needs a maximum that moves
late (the "rise" and "late" profiles), the next row's q is invisible in "late" (every row's output is the same two values)."""
import ctypes
import os

import numpy as np
import pytest

import attn_prefill_ref as R
from attn_prefill_ref import FRAME, FRAME3, V2, Spec
from eilev_amd import abi

# measured by test_every_mutation_exceeds_four_tol (rounded down, one less where the figure is a whole number): the inputs are deterministic, so a smaller figure means the cases changed
MUTATION_FLOOR = {"drop": 122, "double": 42, "swap_v": 201, "shift": 249, "causal+1": 31, "causal-1": 183, "mask_tile": 769, "past_skv": 1934,
                  "next_head_k": 129, "next_row_q": 120, "norescale": 12, "rel+1": 86, "rel-1": 97, "rel_head": 71, "scale_dropped": 64}


def form_of(sp: Spec) -> int:
    """launch_attention's route table restated (csrc/attention.hip), for a launch without hm and dropout."""
    force_v1, dbg = sp.force & 1, sp.force >> 1
    ld_same = sp.layout != "sep"  # (pack(): "sep" is the layout with ldk != ldv)
    if (not force_v1 and not dbg & 4 and not sp.rel and sp.hd == 88 and sp.sq == sp.skv and 256 < sp.sq <= 272 and not sp.causal and not sp.mask
            and ld_same):
        if sp.sq == 257 and not dbg & 32 and (dbg & (16 | 512) or sp.batch >= 512):
            return FRAME3
        return FRAME
    qt = -(-sp.sq // 32)
    if not force_v1 and sp.hd == 64 and sp.sq >= 128 and sp.skv >= 64:
        need = sp.sq + sp.skv - 1
        rel_off, rel_n = {"": (0, 0), "tight": (sp.skv - 1, need), "gap": (sp.skv + 2, need + 6), "n4096": (4096 - sp.sq - 1, 4096),
                          "n4097": (4097 - sp.sq - 1, 4097), "short": (sp.skv - 4, need - 7)}[sp.rel]
        if not sp.rel or (rel_n <= 4096 and rel_off >= sp.skv - 1 and rel_off + sp.sq <= rel_n):
            return V2(8 if qt >= 5 else 4, 2, int(bool(sp.rel)))
    if not force_v1 and not sp.rel and sp.hd == 128 and sp.sq >= 64 and sp.skv >= 64:
        return V2(4 if dbg & 64 else (8 if qt >= 5 else 4), 4)
    if not force_v1 and not sp.rel and sp.hd in (72, 80, 88) and sp.skv >= 32:
        return V2(9 if qt == 9 else (8 if qt >= 5 else (4 if qt >= 3 else 2)))
    return 64 if sp.hd <= 64 else (96 if sp.hd <= 96 else 128)


_SPECS = R.all_specs(256)
_LIGHT = [sp for sp in _SPECS if not sp.name.startswith(("frame-pairs", "frame3-pairs"))]
_case_cache: dict = {}


def _case(sp):
    """(case, reference, A): built once per spec and left unchanged."""
    got = _case_cache.get(sp.name)
    if got is None:
        c = R.build_case(sp)
        got = _case_cache[sp.name] = (c,) + R.reference(c)
        if sp.batch * sp.heads > 64:
            _case_cache.pop(sp.name)  # (the large frame launches are used once)
    return got


def test_names_are_unique_and_shapes_small():
    names = [sp.name for sp in _SPECS]
    assert len(set(names)) == len(names)
    for sp in _SPECS:
        if R.family(sp.form) in ("v1", "v2"):
            assert sp.batch <= 3 and sp.heads <= 3 and max(sp.sq, sp.skv) <= 704, sp.name


def test_route_restatement_agrees_with_every_case():
    for sp in _SPECS:
        assert form_of(sp) == sp.form, (sp.name, form_of(sp), sp.form)
        assert R._first_form(sp.hd, sp.sq, sp.skv, sp.force, sp.rel) == sp.form or R.family(sp.form) in ("frame", "frame3") or sp.name.startswith("route-"), sp.name


def test_every_form_and_boundary_of_the_table_is_a_case():
    forms = {sp.form for sp in _SPECS}
    assert forms == {64, 96, 128, V2(2), V2(4), V2(8), V2(9), V2(4, 2), V2(8, 2), V2(4, 2, 1), V2(8, 2, 1), V2(4, 4), V2(8, 4), FRAME, FRAME3}
    by = {}
    for sp in _SPECS:
        by.setdefault((sp.hd, bool(sp.force & 1)), set()).add((sp.sq, sp.skv, sp.form))
    hd80 = {sq: f for sq, skv, f in by[(80, False)] if sq == skv}
    assert [hd80[s] for s in (64, 65, 128, 129, 256, 257, 288, 289, 512, 513)] == [V2(2), V2(4), V2(4), V2(8), V2(8), V2(9), V2(9), V2(8), V2(8), V2(8)]
    assert {(127, 127, 64), (128, 128, V2(4, 2)), (128, 63, 64), (128, 64, V2(4, 2)), (160, 160, V2(8, 2)), (161, 161, V2(8, 2))} <= by[(64, False)]
    assert {(63, 63, 128), (64, 64, V2(4, 4)), (70, 63, 128), (70, 64, V2(4, 4)), (128, 128, V2(4, 4)), (129, 129, V2(8, 4))} <= by[(128, False)]
    for hd in (72, 80, 88):
        assert {(40, 31, 96), (40, 32, V2(2)), (17, 17, 96)} <= by[(hd, False)]
    assert {(n, n, FRAME) for n in (257, 258, 264, 272)} <= by[(88, False)]


def test_every_key_slot_is_some_rows_spike_in_one_shape_per_form():
    for form in R.V12_FORMS + (FRAME, FRAME3):
        done = False
        for sp in _LIGHT:
            if sp.form != form or sp.mask or done:
                continue
            c = _case(sp)[0]
            done = all(set(c.spike_pos[b, h]) >= set(range(sp.skv)) for b in range(sp.batch) for h in range(sp.heads))
        assert done, R.form_name(form)


def test_spike_positions_differ_per_head_and_batch_entry():
    c = _case(next(sp for sp in _SPECS if sp.name == "route-frame-257"))[0]
    first = {(b, h): int(c.spike_pos[b, h, 0]) for b in range(2) for h in range(3)}
    assert len(set(first.values())) == len(first)


@pytest.mark.parametrize("chunk", range(8))
def test_restatements_stay_within_tol_and_spikes_carry_their_weight(chunk):
    """Per launch of the GPU file: the spike weights (rows with company: inside [0.45, 0.5), so inside the issue's [0.25, 0.75]; rows
    with a single visible key: 1), the explicit fp32 bound <= 2^-11 A, and the family's fp32 / bf16 restatement within tol."""
    worst, worst_fp32 = {}, 0.0
    for sp in _SPECS[chunk::8]:
        c, ref, A = _case(sp)
        many, single = R.spike_weights(c)
        assert len(many) == 0 or (many.min() >= R.W_LO and many.max() < R.W_HI), (sp.name, many.min(), many.max())
        assert len(many) == 0 or (many.min() >= 0.25 and many.max() <= 0.75)
        assert (np.abs(single - 1.0) < 1e-12).all(), sp.name
        dead = R.dead_rows(c)
        assert (ref[dead.nonzero()[0], :, dead.nonzero()[1]] == 0).all()
        if sp.batch * sp.heads <= 64:
            t = R.fp32_term(c, A)
            worst_fp32 = max(worst_fp32, t)
            assert t <= 2.0 ** -11, (sp.name, t * 2 ** 11)
        emu = R.emulate(c)
        ratio = R.worst_ratio(emu, ref, A)
        assert ratio <= 1.0, (sp.name, ratio)
        assert (emu[dead.nonzero()[0], :, dead.nonzero()[1]] == 0).all()
        worst[R.form_name(sp.form)] = max(worst.get(R.form_name(sp.form), 0.0), ratio)
        if sp.profile == "lazy":  # both sides of v2's lazy-rescale threshold, decided by the one real row of the wave
            for b in range(sp.batch):
                for h in range(sp.heads):
                    rise = c.lazy_rise[b, h]
                    assert abs(rise - R.LAZY_RISE[(b * sp.heads + h) % len(R.LAZY_RISE)]) < 0.04 and abs(rise - 6.0) > 0.02
                    assert bool(c.emu_rescales[(b, h)][1, 0]) == (rise > 6.0), (sp.name, b, h, rise)
    print("restatement err/tol:", {k: round(v, 3) for k, v in worst.items()}, "fp32 term / 2^-11:", round(worst_fp32 * 2 ** 11, 3))


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_exceeds_four_tol(mut):
    floor, where, n = np.inf, "", 0
    for sp in _LIGHT:
        if mut in ("causal+1", "causal-1", "mask_tile") and not sp.mask or mut.startswith("rel") and not sp.rel:
            continue
        c, ref, A = _case(sp)
        if not R.applies(mut, c):
            continue
        ratio = R.worst_ratio(R.mutated(c, mut), ref, A)
        n += 1
        if ratio < floor:
            floor, where = ratio, sp.name
    print(f"mutation {mut}: smallest err/tol {floor:.1f} ({where}), {n} cases")
    assert n > 0 and floor >= 4.0, (mut, floor, where)
    assert floor >= MUTATION_FLOOR[mut], (mut, floor)
    if mut == "norescale":
        assert n >= 2 * len(R.V12_FORMS)


def test_packed_buffers_hold_the_case():
    for name in ("route-qformer-self", "route-qformer-cross", "keys-v1<96>-hd80-33", "route-hd88-272-ldk"):
        sp = next(sp for sp in _SPECS if sp.name == name)
        c = _case(sp)[0]
        P = R.pack(c)
        for which, src in (("q", c.Q), ("k", c.K), ("v", c.V)):
            buf, off = getattr(P, which)
            flat = P.bufs[buf].reshape(-1)
            ld, bs, hs = getattr(P, f"ld{which}"), getattr(P, f"{which}_bs"), getattr(P, f"{which}_hs")
            rows = sp.sq if which == "q" else sp.skv
            for b in range(sp.batch):
                for h in range(sp.heads):
                    idx = off + b * bs + h * hs + np.arange(rows)[:, None] * ld + np.arange(sp.hd)[None, :]
                    assert idx.max() < flat.size and np.array_equal(flat[idx], R.bf16_bits(src[b, h, :rows])), (name, which)
        for arr in P.bufs.values():
            assert all(v % 8 == 0 for v in (P.ldq, P.ldk, P.ldv, P.q_bs, P.k_bs, P.v_bs, P.q_hs, P.k_hs, P.o_ld))


def test_probe_entry_only_in_the_probe_library():
    if os.path.exists(abi.HIP_LIB_PATH):
        assert not hasattr(ctypes.CDLL(abi.HIP_LIB_PATH), "eilev_debug_attention")
    if not os.path.exists(abi.PROBES_LIB_PATH):
        return
    fn = ctypes.CDLL(abi.PROBES_LIB_PATH).eilev_debug_attention  # (loads without a GPU; these calls return before any HIP call)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(256)
    assert fn(None, 200, None, None) == -1 and fn(buf, 192, None, None) == -1 and fn(buf, 208, None, None) == -1
