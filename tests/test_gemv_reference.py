"""CPU: the wave-to-row deal, the cases, the route mirror and the bound of tests/gemv_ref.py (what tests/test_hip_gemv.py holds the M <= 8
row-dot decode kernels of csrc/gemv.hip to), and what planted mistakes cost against them.

emulate() below replays one launch through the kernels' own index maps in numpy: the prologue in fp32 with the staged rows rounded to bf16,
the product chunk by chunk of 512 (a lane's slice is 8 elements of a chunk, a sub-block SB or CPS chunks), the epilogue in the kernels' order
(bias, scale on the first scale_cols columns, ReLU, residual), the deal of the output rows to the waves with the 64-row flush of
gemv1_kernel / gemvm_kernel, and the store into a poisoned (or, in place, residual-holding) out allocation.  One mistake at a time is
planted.  The condition: on every spec the mistake can touch it is detected (an element it changes fails the check: unequal bits on the exact
family, err > tol on the bounded one), and of all the elements it changes — those that differ from the unmutated emulation — at most 1 % stay
inside the bound.  The unmutated emulation passes its own check.

  mistake                  what it plants
  slice_skipped            lane (11 c + 5) % 64 leaves out its 8 elements of the last 512-chunk c
  chunk_twice              chunk 1 is multiplied with the weights of chunk 0
  bias_row_plus1           bias[n + 1]
  scale_cols_plus1         one column more is scaled
  relu_after_resid         ReLU applied after the residual
  resid_row_plus1          the residual of row m + 1
  flush_wrong_lane         the 64-row flush stores `mine` of lane ^ 1
  last_subblock_next_row   the last sub-block of an output row is credited to the next row
  ln_var_uncentred         LayerNorm variance as E[x^2]
  merge_empty_weight       an empty range weighs in with exp(max_s - max) (a finite stale o)
  merge_max_live_only      the maximum over the live ranges, the weights over all"""
import ctypes

import numpy as np
import pytest

import gemm_ref as R
import gemv_ref as V
from eilev_amd.synth import round_bf16

NCU = 256
f32 = np.float32


# ---- the deal ----------------------------------------------------------------------------------------------------------------------------------

def test_wave_to_row_deal_is_a_partition():
    specs = V.route_specs() + [sp for sp, _ in V.refused_specs() if V.expected(sp, NCU)[0] == R.OK]
    extra = [V.GSpec("p", V.GEMV1, V.PRO_X, 1, n, 2560, grid=g) for n in (1, 2, 4, 5, 6, 39, 40, 41, 79, 1279, 1280, 1281, 50272) for g in (0, 1, 3, 8)]
    extra += [V.GSpec("p", V.ROWS, V.PRO_X, 3, n, 512) for n in (1, 2, 7, 8, 9, 2047, 4096, 4097, 50272)]
    for sp in specs + extra:
        for n_cu in (NCU, 304, 8):
            grid, rpw, kb = V.geometry(sp, n_cu)
            d = V.deal(sp, n_cu)
            assert grid >= 1 and len(d) == grid * (4 if sp.launcher == V.ROWS else 5)
            nxt = 0
            for r0, r1 in d:
                assert r0 == nxt and r1 >= r0
                nxt = r1
            assert nxt == sp.N, (sp.name, n_cu)
            if sp.launcher != V.ROWS:
                assert grid <= V.eff_cus(sp, n_cu) and (grid * 5 <= sp.N or grid == (sp.N + 4) // 5)
                if grid * 5 > sp.N:  # the clamped grid: zero-row waves at the end, one row each before them
                    assert rpw == 0 and kb == sp.N and sum(1 for r0, r1 in d if r1 == r0) == grid * 5 - sp.N


def test_the_cases_reach_the_paths_they_are_named_for():
    by = {sp.name: sp for sp in V.route_specs()}
    rows = lambda name: sorted({r1 - r0 for r0, r1 in V.deal(by[name], NCU)})
    assert rows("gemv1-x-12x2560-x") == [0, 1] and rows("gemv1-x-640x2560-x") == [16] and rows("gemv1-x-702x2560-x") == [17, 18]
    assert rows("gemv1-x-930x2560-x") == [23, 24] and rows("gemv1-x-2650x2560-x") == [66, 67] and rows("gemv1-x-46x10240-x") == [1, 2]
    assert rows("gemv1-ln-320x2560-b") == [8] and rows("gemv1-ln-382x2560-b") == [9, 10] and rows("gemv1-ln-450x2560-f32-b") == [11, 12]
    assert rows("gemv1-merge-12-ns5-x") == [0, 1] and rows("gemvm-x-5x12-x") == [0, 1]
    assert V.geometry(by["rows-x-1x4100x512-x"], NCU)[1] == 3 and V.geometry(by["rows-x-2x6x512-x"], NCU)[0] == 1
    assert V.ring(by["gemv1-x-46x10240-x"]) == (5, 4, 4) and V.ring(by["gemv1-x-126x4096-x"]) == (8, 1, 4) and V.ring(by["gemv1-ln-320x2560-b"]) == (5, 1, 4)
    assert V.ring(by["gemvm-x-2x638-x"]) == (5, 1, 8) and V.ring(by["gemvm-x-3x318-x"]) == (5, 1, 4) and V.ring(by["gemvm-ln-2x318-b"]) == (5, 1, 4)
    # the LONG threshold of gemvm_kernel from both sides; below it the short form still meets waves of exactly 2 RB rows
    assert V.instance_name(V.expected(by["gemvm-x-2x638-x"], NCU)[1]) == "gemvm-x-m2-short" and max(rows("gemvm-x-2x638-x")) == 16
    assert V.instance_name(V.expected(by["gemvm-x-2x640-x"], NCU)[1]) == "gemvm-x-m2-long"
    assert V.instance_name(V.expected(by["gemvm-ln-8x318-b"], NCU)[1]) == "gemvm-ln-m8-short" and max(rows("gemvm-ln-8x318-b")) == 8
    assert V.instance_name(V.expected(by["gemvm-ln-8x320-b"], NCU)[1]) == "gemvm-ln-m8-long"
    # the natural-grid cases are short on any device with at least 64 CUs
    for n_cu in (64, 256, 304):
        assert V.families(by["gemv1-x-natural-x"], n_cu) == ["gemv1-x-5-short"]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------

def test_exact_family_results_are_bf16_values():
    specs = [sp for sp in V.route_specs() if sp.family == "exact"]
    assert len(specs) > 100
    for sp in specs:
        c = V.build_case(sp)
        y, S, D = V.reference(c)
        assert R.is_bf16(y) and np.abs(y).max() <= 128, sp.name
        x, d = V.prologue(c)
        assert R.is_bf16(x) and np.abs(x).max() <= 1, sp.name
        if sp.pro == V.PRO_MERGE:  # weights 1, the sums add up to 4 (or the row is dead)
            l = c.part[..., 1].sum(-1)
            assert set(np.unique(l)) <= {0.0, 4.0} and len({v for v in np.unique(c.part[..., 0]) if v > -1e29}) == 1


def test_guards_are_where_build_case_says():
    by = {sp.name: sp for sp in V.route_specs()}
    for name in ("rows-x-3x1001x512-b", "rows-x-8x1001x512-x", "gemvm-ln-4x342-b", "gemv1-x-126x2560-b", "rows-merge-2x40-32x80-ns8-b", "gemv1-merge-126-dead-x"):
        sp = by[name]
        c = V.build_case(sp)
        ldx, ldr, ldo = V.strides(sp)
        M, N, K = sp.M, sp.N, sp.K
        assert (c.ldx, c.ldr, c.ldo) == (ldx, ldr, ldo) and c.W_buf.shape == (N + 2, K) and (np.abs(c.W_buf[N:]) == R.TRAP).all()
        assert (ldx, ldo) == ((K, N) if sp.launcher == V.GEMV1 else (K + 8, N + 8)) and (sp.resid != 2 or ldr == ldo)
        if sp.pro != V.PRO_MERGE:
            assert c.x_buf.shape == (M + 2, ldx) and (np.abs(c.x_buf[M:]) == R.TRAP).all() and (np.abs(c.x_buf[:M, K:]) == R.TRAP).all()
        if sp.bias:
            assert (c.bias[N:] == R.TRAP).all() and np.abs(c.bias[:N]).max() < 16
        if sp.resid:
            assert c.resid_buf.shape == (M + 2, ldr) and (np.abs(c.resid_buf[M:]) == R.TRAP).all() and (np.abs(c.resid_buf[:M, N:]) == R.TRAP).all()
        if sp.pro == V.PRO_MERGE:
            assert c.part.shape == (M, sp.heads, sp.nsplit, sp.hd + 2) and np.array_equal(c.live, c.part[..., 1] > 0)
            o = c.part[..., 2:]
            assert np.isnan(o[~c.live]).all() and (o[~c.live].view(np.uint32) == V.SENT32).all() and np.isfinite(o[c.live]).all()
            if sp.nsplit >= 5 and not (sp.dead_row and M == 1):   # empty ranges at the front, in the middle (with a stale finite maximum) and at the end
                assert not c.live[0, 1, 0] and not c.live[0, 1, 1] and not c.live[0, 2, sp.nsplit // 2] and not c.live[0, 3, sp.nsplit - 1] and c.live[0, 0].all()
                assert c.part[0, 1, 0, 0] == np.float32(V.EMPTY_MAX) and abs(c.part[0, 2, sp.nsplit // 2, 0]) <= 4.0
            if sp.dead_row:
                assert not c.live[M - 1].any()
                y = V.reference(c)[0]
                want = c.bias[:N].astype(np.float64) if sp.bias else np.zeros(N)   # bias (ReLU) plus residual, nothing else
                want = (np.maximum(want, 0.0) if sp.epi == 2 else want) + (c.resid[M - 1] if sp.resid else 0.0)
                assert np.array_equal(y[M - 1], want)


def test_route_mirror_is_self_consistent():
    for n_cu in (256, 304, 64):
        specs = V.route_specs()
        names = [sp.name for sp in specs]
        assert len(set(names)) == len(names)
        seen = set()
        for sp in specs:
            rc, code = V.expected(sp, n_cu)
            assert rc == R.OK and code // 100000 == sp.launcher + 1, sp.name
            seen.update(V.families(sp, n_cu))
            if sp.grid:
                assert V.expected(sp, n_cu) == V.expected(sp, 256) and V.families(sp, n_cu) == V.families(sp, 256)
        assert not [f for f in V.REQUIRED if f not in seen], [f for f in V.REQUIRED if f not in seen]
    for sp, rc in V.refused_specs():
        assert V.expected(sp, NCU) == (rc, 0), sp.name
    assert V.instance(3, 5, 5, 1, 1) == 350511 and V.instance_name(350511) == "gemvm-ln-m5-long" and V.instance_name(212000) == "gemv1-x-20"
    assert V.instance_name(180820) == "rows-merge-m8-cps8" and V.instance_name(0) == "none"
    assert [V.rows_cps(k) for k in (512, 1024, 2560, 4096, 5120, 10240, 16384)] == [1, 1, 5, 8, 5, 5, 8]


def test_addition_count_and_constants_of_the_bound():
    sp = V.GSpec("t", V.ROWS, V.PRO_X, 1, 40, 2560)
    assert V.n_adds(sp) == 2560 + 8 and R.ACC_C == 1.0 and V.EXPF_TERM == 2.0 ** -20
    assert 8 * 1.4427 * 2.0 ** -24 + 2.0 ** -23 < V.EXPF_TERM   # the rounding of d log2(e) for |d| <= 8 plus a unit of v_exp_f32 at a result <= 1
    # the merge term: e_m of the magnitudes, plus half a bf16 unit
    msp = V.GSpec("t", V.GEMV1, V.PRO_MERGE, 1, 12, 2560, heads=32, hd=80, nsplit=5, family="bounded")
    c = V.build_case(msp)
    x, d = V.merged_x(c)
    assert (d >= R.half_ulp(x, 8)).all() and (d <= R.half_ulp(x, 8) + ((2 * 5 + 8) * 2.0 ** -24 + 2.0 ** -20) * 12.5).all()


def test_probe_entry_refuses_a_stale_struct_without_a_gpu():
    """eilev_debug_gemv exists in the probe library only; a wrong struct size comes back as EILEV_E_BADARG before any HIP call."""
    import os

    from eilev_amd import abi

    assert os.path.exists(abi.PROBES_LIB_PATH), "libeilev_hip_probes.so is not built: build() makes it next to the product library (a failed probe build must not pass)"
    if os.path.exists(abi.HIP_LIB_PATH):
        assert not hasattr(ctypes.CDLL(abi.HIP_LIB_PATH), "eilev_debug_gemv")
    fn = ctypes.CDLL(abi.PROBES_LIB_PATH).eilev_debug_gemv
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(512)
    inst = ctypes.c_int(-1)
    for size in (144, 148, 160, 0):
        for launcher in (0, 1, 2):
            assert fn(buf, ctypes.c_size_t(size), launcher, ctypes.byref(inst), None) == R.E_BADARG
    assert fn(None, ctypes.c_size_t(152), 0, ctypes.byref(inst), None) == R.E_BADARG
    assert fn(buf, ctypes.c_size_t(152), 3, ctypes.byref(inst), None) == R.E_BADARG and fn(buf, ctypes.c_size_t(152), -1, ctypes.byref(inst), None) == R.E_BADARG
    assert inst.value == -1


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------------

def _staged(c, mut):
    """The activation rows as the kernels stage them: fp32 arithmetic, rounded to bf16.  float64 [M, K]."""
    sp = c.spec
    if sp.pro == V.PRO_X:
        return c.x.astype(np.float64)
    if sp.pro == V.PRO_LN:
        x = c.x.astype(f32)
        mean = (x.sum(1, dtype=f32) / f32(sp.K)).astype(f32)[:, None]
        cen = x if mut == "ln_var_uncentred" else (x - mean).astype(f32)
        var = ((cen * cen).sum(1, dtype=f32) / f32(sp.K)).astype(f32)[:, None]
        rstd = (f32(1.0) / np.sqrt(var + f32(c.eps))).astype(f32)
        return round_bf16(((x - mean) * rstd * c.gamma[None, :] + c.beta[None, :]).astype(f32)).astype(np.float64)
    p = c.part.copy()
    live = c.live
    if mut in ("merge_empty_weight", "merge_max_live_only"):
        p[..., 2:] = np.where(live[..., None], p[..., 2:], f32(V.STALE_O))   # a finite stale o
    else:
        p[..., 2:] = np.where(live[..., None], p[..., 2:], f32(0.0))         # (the guarded select)
    mx_all = p[..., 0].max(-1, keepdims=True)
    mx_live = np.where(live, p[..., 0], f32(-1e30)).max(-1, keepdims=True)
    mx = mx_live if mut == "merge_max_live_only" else mx_all
    weigh = np.ones_like(live) if mut in ("merge_empty_weight", "merge_max_live_only") else live
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):   # (a dead row under a planted mistake: exp(stale max + 1e30) * 0)
        w = np.where(weigh, np.exp((p[..., 0] - mx).astype(f32)), f32(0.0)).astype(f32)
        l = (w * p[..., 1]).sum(-1, dtype=f32)
        o = (w[..., None] * p[..., 2:]).sum(-2, dtype=f32)
    x = np.where(l[..., None] > 0, o / np.where(l > 0, l, f32(1.0))[..., None], f32(0.0)).astype(f32)
    return round_bf16(x.reshape(sp.M, sp.K)).astype(np.float64)


def _round_out(sp, v):
    return v.astype(f32).astype(np.float64) if sp.out_f32 else round_bf16(v.astype(f32)).astype(np.float64)


def out_alloc(c):
    """The out allocation before the launch, as float64 with NaN for the sentinel: (M + 2, ldo)."""
    sp = c.spec
    if sp.resid == 2:
        return c.resid_buf.astype(np.float64).copy()
    return np.full((sp.M + 2, c.ldo), np.nan)


def applies(mut, sp, n_cu=NCU):
    _, ipr, _ = V.ring(sp) if sp.launcher != V.ROWS else (0, (sp.K >> 9) // V.rows_cps(sp.K), 0)
    some_x = not (sp.pro == V.PRO_MERGE and sp.dead_row and sp.M == 1)   # (a launch whose only row is dead multiplies zeros)
    return {"slice_skipped": some_x,
            "chunk_twice": sp.K >= 1024 and some_x,
            "bias_row_plus1": sp.bias,
            "scale_cols_plus1": sp.scale_cols < sp.N and sp.scale != 1.0,
            "relu_after_resid": sp.epi == 2 and sp.resid != 0,
            "resid_row_plus1": sp.resid != 0,
            "flush_wrong_lane": sp.launcher != V.ROWS and any(r1 - r0 >= 64 for r0, r1 in V.deal(sp, n_cu)),
            "last_subblock_next_row": ipr >= 2 and sp.N >= 2 and some_x,
            "ln_var_uncentred": sp.pro == V.PRO_LN,
            "merge_empty_weight": sp.pro == V.PRO_MERGE and sp.nsplit >= 2 and some_x,
            "merge_max_live_only": sp.pro == V.PRO_MERGE and sp.nsplit >= 2 and some_x}[mut]


MUTATIONS = ["slice_skipped", "chunk_twice", "bias_row_plus1", "scale_cols_plus1", "relu_after_resid", "resid_row_plus1", "flush_wrong_lane",
             "last_subblock_next_row", "ln_var_uncentred", "merge_empty_weight", "merge_max_live_only"]


def emulate(c, n_cu=NCU, mut=None):
    sp = c.spec
    M, N, K = sp.M, sp.N, sp.K
    nch = K >> 9
    xs = _staged(c, mut)
    W = c.W.astype(np.float64)
    sub = (V.rows_cps(K) if sp.launcher == V.ROWS else V.ring(sp)[0]) * 512   # elements per sub-block
    if mut == "last_subblock_next_row":
        head, last = xs[:, :K - sub] @ W[:, :K - sub].T, xs[:, K - sub:] @ W[:, K - sub:].T
        acc = head
        acc[:, 1:] += last[:, :-1]
    else:
        acc = xs @ W.T
    if mut == "slice_skipped":
        ch = nch - 1
        k0 = ch * 512 + 8 * ((11 * ch + 5) % 64)
        acc = acc - xs[:, k0:k0 + 8] @ W[:, k0:k0 + 8].T
    if mut == "chunk_twice":
        acc = acc - xs[:, 512:1024] @ W[:, 512:1024].T + xs[:, 512:1024] @ W[:, 0:512].T
    if c.bias is not None:
        sh = 1 if mut == "bias_row_plus1" else 0
        acc = acc + c.bias[sh:sh + N].astype(np.float64)[None, :]
    sc = sp.scale_cols + (1 if mut == "scale_cols_plus1" else 0)
    acc[:, :sc] *= sp.scale
    if sp.epi == 2 and mut != "relu_after_resid":
        acc = np.maximum(acc, 0.0)
    if sp.resid:
        sh = 1 if mut == "resid_row_plus1" else 0
        acc = acc + c.resid_buf[sh:sh + M, :N].astype(np.float64)
    if sp.epi == 2 and mut == "relu_after_resid":
        acc = np.maximum(acc, 0.0)
    vals = _round_out(sp, acc)
    flat = out_alloc(c)
    for r0, r1 in V.deal(sp, n_cu):   # the stores, wave by wave
        cols = np.arange(r0, r1)
        src = cols.copy()
        if mut == "flush_wrong_lane" and r1 - r0 >= 64:
            src[:64] = r0 + (np.arange(64) ^ 1)
        flat[:M, cols] = vals[:, src]
    return flat


def judge(c, flat, clean=None):
    """(elements of the output that the mistake changes — that differ from the unmutated emulation `clean`, or without one from the reference's
    rounding —, how many of those stay inside the bound, True iff every word outside the output is as it was)."""
    sp = c.spec
    y, S, D = V.reference(c)
    got = flat[:sp.M, :sp.N]
    base = _round_out(sp, y) if clean is None else clean[:sp.M, :sp.N]
    before = out_alloc(c)
    rest = np.ones(flat.shape, bool)
    rest[:sp.M, :sp.N] = False
    intact = bool(((flat == before) | (np.isnan(flat) & np.isnan(before)))[rest].all())
    changed = ~((got == base) & ~np.isnan(got))
    if sp.family == "exact":   # (the check is equality with the reference: every changed element is outside it)
        assert clean is None or np.array_equal(clean[:sp.M, :sp.N], _round_out(sp, y))
        return int(changed.sum()), 0, intact
    inside = R.ratio(np.abs(got - y), V.tol(c, y, S, D)) <= 1.0
    return int(changed.sum()), int((changed & inside).sum()), intact


_cases: dict = {}


def _case(sp):
    if sp.name not in _cases:
        _cases[sp.name] = V.build_case(sp)
    return _cases[sp.name]


def test_the_unmutated_emulation_passes_its_own_check():
    for sp in V.route_specs():
        c = _case(sp)
        flat = emulate(c)
        y, S, D = V.reference(c)
        n, _, intact = judge(c, flat)
        assert intact, sp.name
        if sp.family == "exact":
            assert n == 0, sp.name
        else:
            assert float(R.ratio(np.abs(flat[:sp.M, :sp.N] - y), V.tol(c, y, S, D)).max()) <= 1.0, sp.name


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_planted_mistake_is_detected(mut):
    """On every spec the mistake can touch it changes at least one element and at least one changed element is outside the bound; of all the
    elements it changes over all specs, at most 1 % stay inside."""
    specs = [sp for sp in V.route_specs() if applies(mut, sp)]
    assert specs, mut
    changed = inside = 0
    for sp in specs:
        c = _case(sp)
        n, n_in, _ = judge(c, emulate(c, NCU, mut), emulate(c, NCU))
        assert n >= 1, f"{mut} on {sp.name}: no output element changes"
        assert n_in < n, f"{mut} on {sp.name}: all {n} elements it changes stay inside the bound"
        changed, inside = changed + n, inside + n_in
    print(f"{mut:24s} {len(specs):4d} specs, {changed:8d} elements changed, {inside:6d} of them inside the bound ({inside / changed:.3%})")
    assert inside <= 0.01 * changed, f"{mut}: {inside} of the {changed} elements it changes stay inside the bound"
