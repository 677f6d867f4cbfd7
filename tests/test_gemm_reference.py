"""CPU: the cases, the float64 reference, the bound and the route mirror of tests/gemm_ref.py (what tests/test_hip_gemm_wide.py holds the wide
GEMM kernels to), and what planted mistakes cost against them.

The mutation table: a numpy emulation of one launch (emulate below: the epilogue order of csrc/gemm_common.h in float64, the output rounded as
the kernel rounds it, written into a poisoned allocation at gemm_ref.out_index) is given one mistake at a time.  On the exact family a mistake must
change at least one word of C / stat_out; on the bounded family it must cost err / tol >= 4.  Measured (words changed on the exact family,
worst err / tol on the bounded family; "-" = the mistake cannot act on that family):

  mistake              exact: words  bounded: err/tol
  drop_k32                      723           9.5e+03
  drop_k64                      847          1.14e+04
  double_k64                    853          9.04e+03
  ktail_zero                  17687          1.06e+04
  pad_col                      1024          3.12e+12
  bias_shift4                 38250          2.21e+08
  bias_shift8                 38550          2.44e+08
  resid_row1                  38391          2.58e+08
  resid_coltile               38414          4.89e+04
  half_swap                   18382          5.77e+04
  tail_row_prev                5652          6.41e+04
  relu_before_bias            23158          2.39e+04
  resid_before_act            25368               503
  scale_cols_off16             2255               440
  scale_before_bias           12900          9.43e+04
  patch_cls_off                9967 inf (a word outside the output)
  patch_pos_no_plus1           9324          1.02e+05
  hm_swap_blocks             109615           1.8e+05
  ascale_by_col               15231          2.27e+04
  wscale_after_bias           26250          2.36e+04
  ln_plus_mean                28677          4.16e+04
  stat_slot_shift              1298 inf (a word outside the output)
  stat_rounded                    -               524
  splitk_overlap                896              13.5
"""
import ctypes

import numpy as np
import pytest

import gemm_ref as R
from gemm_ref import Spec
from eilev_amd.synth import round_bf16


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------------

def _round_out(sp, v):
    return v.astype(np.float32).astype(np.float64) if sp.out_f32 else round_bf16(v.astype(np.float32)).astype(np.float64)


def emulate(c, mut=None):
    """(flat C allocation with NaN where nothing was written, stat_out [slots + 2, M, 2] with NaN likewise or None)."""
    sp = c.spec
    M, N, K = sp.M, sp.N, sp.K
    A, W = c.A.astype(np.float64), c.W.astype(np.float64)
    acc = A @ W.T
    rb, cb = slice(0, min(M, 32)), slice(0, min(N, 32))  # one 32 x 32 block: what a single wave's mistake reaches

    def step(k0, k1, rows=rb, cols=cb):
        return c.A_buf[rows, k0:k1].astype(np.float64) @ c.W_buf[cols, k0:k1].astype(np.float64).T

    if mut == "drop_k32":
        acc[rb, cb] -= step(32, 64)
    elif mut == "drop_k64":
        acc[rb, cb] -= step(64, 128)
    elif mut == "double_k64":
        acc[rb, cb] += step(0, 64)
    elif mut == "ktail_zero":
        assert K % 64
        acc -= step(K - K % 64, K, slice(0, M), slice(0, N))
    elif mut == "pad_col":
        assert c.lda > K and c.ldw > K
        acc[rb, cb] += step(K, K + 1)
    elif mut == "splitk_overlap":
        k_slice = R.split_k_slices(sp)[1]
        acc += step(k_slice * 64, k_slice * 64 + 64, slice(0, M), slice(0, N))
    if sp.lnfold:
        nm, cs = c.ln_rows[:, 1].astype(np.float64)[:, None], c.ln_csum.astype(np.float64)[None, :]
        acc = (acc - nm * cs if mut == "ln_plus_mean" else acc + nm * cs) * c.ln_rows[:, 0].astype(np.float64)[:, None]
    ws = None if c.wscale is None else c.wscale.astype(np.float64)[None, :]
    if ws is not None and mut != "wscale_after_bias":
        acc = acc * ws
    if c.ascale is not None:
        acc = acc * (c.ascale.astype(np.float64)[np.arange(N) % M][None, :] if mut == "ascale_by_col" else c.ascale.astype(np.float64)[:, None])
    v = acc
    if mut == "relu_before_bias":
        assert sp.epi == 2
        v = np.maximum(v, 0.0)
    shift = {"bias_shift4": 4, "bias_shift8": 8}.get(mut, 0)
    b = 0.0 if c.bias is None else c.bias[shift:shift + N].astype(np.float64)[None, :]
    sc = sp.scale_cols + (16 if mut == "scale_cols_off16" else 0)
    if mut == "scale_before_bias":
        v = v.copy()
        v[:, :sc] *= sp.scale
        v = v + b
    else:
        v = v + b
        v[:, :sc] *= sp.scale
    if ws is not None and mut == "wscale_after_bias":
        v = v * ws
    r = None
    if c.resid_buf is not None:
        rbuf = c.resid_buf.astype(np.float64)
        rows = np.arange(M)
        if sp.patch_group:
            rows = rows % sp.patch_group + (0 if mut == "patch_pos_no_plus1" else 1)
        if mut == "resid_row1":
            rows = rows + 1
        r = rbuf[rows][:, :N]
        if mut == "resid_coltile":
            r = r[:, (np.arange(N) + 128) % N]
    if mut == "resid_before_act":
        assert r is not None and sp.epi
        v, r = v + r, None
    if sp.epi == 1:
        v = R.gelu_exact(v)
    elif sp.epi == 2 and mut != "relu_before_bias":
        v = np.maximum(v, 0.0)
    if r is not None:
        v = v + r
    if mut == "half_swap":
        n0 = N // 256 * 256
        assert N - n0 == 128
        v = v.copy()
        v[:, n0:n0 + 64], v[:, n0 + 64:n0 + 128] = v[:, n0 + 64:n0 + 128].copy(), v[:, n0:n0 + 64].copy()
    if mut == "tail_row_prev":
        tail = M % 128
        assert tail and M > 128
        v = v.copy()
        v[M - tail:] = v[M - tail - 128:M - 128]
    stat = None
    if sp.stats:
        slots = (N + 63) // 64
        stat = np.full((c.stat_slots, M, 2), np.nan)
        sv = _round_out(sp, v) if mut == "stat_rounded" else v.astype(np.float32).astype(np.float64)
        for s in range(slots):
            blk = sv[:, 64 * s:64 * s + 64]
            to = s + 1 if mut == "stat_slot_shift" else s
            stat[to, :, 0], stat[to, :, 1] = blk.sum(1), (blk * blk).sum(1)
    out = _round_out(sp, v)
    idx = R.out_index(c, hm_swapped=(mut == "hm_swap_blocks"))
    if mut == "patch_cls_off":
        idx = idx - c.ldc
    flat = np.full(R.c_words(c), np.nan)
    flat[idx.ravel()] = out.ravel()
    return flat, stat


def _judge(c, flat, stat):
    """(words that differ from the reference allocation, worst err / tol) of an emulated launch."""
    sp = c.spec
    y, S, _ = R.reference(c)
    form = R.expected(sp, 256)[1] or 2040
    ref_flat = np.full(R.c_words(c), np.nan)
    tol_flat = np.zeros(R.c_words(c))
    idx = R.out_index(c).ravel()
    ref_flat[idx] = _round_out(sp, y).ravel()
    tol_flat[idx] = R.tol(c, y, S, form).ravel()
    same = (flat == ref_flat) | (np.isnan(flat) & np.isnan(ref_flat))
    words = int((~same).sum())
    y_flat = np.full(R.c_words(c), np.nan)
    y_flat[idx] = y.ravel()
    err = np.abs(flat - y_flat)
    written = ~np.isnan(y_flat)
    ratio = R.ratio(err[written], tol_flat[written]).max()
    if (~np.isnan(flat[~written])).any():  # a word outside the output
        ratio = np.inf
    if stat is not None:
        sref, stol = R.stat_ref(c, y, S)
        full = np.full(stat.shape, np.nan)
        full[:sref.shape[0]] = sref
        sm = (stat.astype(np.float32) == full.astype(np.float32)) | (np.isnan(stat) & np.isnan(full))
        words += int((~sm).sum())
        ratio = max(ratio, R.ratio(np.abs(stat[:sref.shape[0]] - sref), stol).max())
        if (~np.isnan(stat[sref.shape[0]:])).any():
            ratio = np.inf
    return words, float(ratio)


BASE = dict(M=150, N=264, K=136, resid=True)
MUTATIONS = {  # name: (spec fields, families the mistake can act on)
    "drop_k32": (BASE, "xb"),
    "drop_k64": (BASE, "xb"),
    "double_k64": (BASE, "xb"),
    "ktail_zero": (BASE, "xb"),
    "pad_col": (BASE, "xb"),
    "bias_shift4": (BASE, "xb"),
    "bias_shift8": (BASE, "xb"),
    "resid_row1": (BASE, "xb"),
    "resid_coltile": (BASE, "xb"),
    "half_swap": (dict(M=150, N=384, K=128), "xb"),
    "tail_row_prev": (BASE, "xb"),
    "relu_before_bias": (dict(M=150, N=264, K=136, epi=2), "xb"),
    "resid_before_act": (dict(M=150, N=264, K=136, epi=2, resid=True), "xb"),
    "scale_cols_off16": (dict(M=150, N=264, K=136, scale_cols=88, scale=0.125), "xb"),
    "scale_before_bias": (dict(M=150, N=264, K=136, scale_cols=88, scale=0.125), "xb"),
    "patch_cls_off": (dict(M=48, N=200, K=72, patch_group=16, resid=True), "xb"),
    "patch_pos_no_plus1": (dict(M=48, N=200, K=72, patch_group=16, resid=True), "xb"),
    "hm_swap_blocks": (dict(M=258, N=3 * 2 * 72, K=64, lnfold=True, hm=(129, 2, 72)), "xb"),
    "ascale_by_col": (dict(M=130, N=200, K=128, a8=True), "xb"),
    "wscale_after_bias": (dict(M=150, N=264, K=136, wscale=True), "xb"),
    "ln_plus_mean": (dict(M=150, N=264, K=128, lnfold=True), "xb"),
    "stat_slot_shift": (dict(M=130, N=200, K=64, stats=True, resid=True, resid_gain=8.0), "xb"),
    # integers are bf16 values: rounding before summing changes nothing on the exact family
    "stat_rounded": (dict(M=130, N=200, K=64, stats=True, resid=True, resid_gain=8.0), "b"),
    "splitk_overlap": (dict(M=100, N=120, K=8192, bias=False, out_f32=True), "xb"),
}


def mutation_table():
    table = {}
    for name, (kw, fams) in MUTATIONS.items():
        words = ratio = None
        if "x" in fams:
            c = R.build_case(Spec(name, family="exact", **kw))
            words = _judge(c, *emulate(c, name))[0]
        if "b" in fams:
            c = R.build_case(Spec(name, family="bounded", **kw))
            ratio = _judge(c, *emulate(c, name))[1]
        table[name] = (words, ratio)
    return table


def test_every_planted_mistake_is_detected():
    table = mutation_table()
    for name, (words, ratio) in table.items():
        print(f"{name:20s} {'-' if words is None else words:>8} {'-' if ratio is None else format(ratio, '.3g'):>10}")
    for name, (words, ratio) in table.items():
        assert words is None or words >= 1, f"{name}: no word changes on the exact family"
        assert ratio is None or ratio >= 4.0, f"{name}: costs only {ratio:.3g} tol on the bounded family"
    assert sum(1 for w, r in table.values() if w is None or r is None) == 1  # stat_rounded, as listed


def test_the_unmutated_emulation_passes_its_own_check():
    """No mistake: bit equality on the exact family, err / tol <= 1 on the bounded one (so the table above measures the mistakes alone)."""
    seen = set()
    for name, (kw, fams) in MUTATIONS.items():
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key in seen:
            continue
        seen.add(key)
        c = R.build_case(Spec(name, family="exact", **kw))
        assert _judge(c, *emulate(c))[0] == 0, name
        c = R.build_case(Spec(name, family="bounded", **kw))
        assert _judge(c, *emulate(c))[1] <= 1.0, name


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------

def _small(specs, limit=3e8):
    return [sp for sp in specs if sp.M * sp.N * sp.K <= limit]


def test_exact_family_is_exact_in_fp32_in_any_order_and_in_bf16():
    """The float64 reference of every exact case (the large lean / A3 ones by their bound: |partial sum| <= K < 2^24 with operands in {-1, 0, 1})
    equals a float32 evaluation in three summation orders, and every output value survives a bf16 round trip."""
    specs = [sp for sp in R.route_specs(256) if sp.family == "exact"]
    assert len(specs) > 60
    for sp in specs:
        assert sp.K < 2 ** 24
    for sp in _small(specs):
        c = R.build_case(sp)
        y = R.reference(c)[0]
        assert R.is_bf16(y), sp.name
        assert np.abs(y).max() <= 256, sp.name
        if sp.lnfold or sp.a8 or sp.wscale or sp.w8:
            continue  # (scaled sums: the products below are the unscaled ones, checked on the plain cases)
        A, W = c.A, c.W
        plain = (A.astype(np.float64) @ W.astype(np.float64).T)
        fwd = np.zeros((sp.M, sp.N), np.float32)
        for k0 in range(0, sp.K, 32):
            fwd += A[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T
        rev = np.zeros((sp.M, sp.N), np.float32)
        for k0 in reversed(range(0, sp.K, 8)):
            rev += A[:, k0:k0 + 8] @ W[:, k0:k0 + 8].T
        halves = (A[:, ::2] @ W[:, ::2].T).astype(np.float32) + (A[:, 1::2] @ W[:, 1::2].T).astype(np.float32)
        for other in (fwd, rev, halves):
            assert np.array_equal(other.astype(np.float64), plain), sp.name


def test_exact_scaled_cases_round_trip_through_the_emulation():
    """The scaled exact cases (fp8 scales, folded LayerNorm, statistics): the float32 emulation of the epilogue order equals the float64 reference
    bit for bit, statistics included."""
    for sp in _small([sp for sp in R.route_specs(256) if sp.family == "exact" and (sp.lnfold or sp.a8 or sp.wscale or sp.w8 or sp.stats)]):
        c = R.build_case(sp)
        assert _judge(c, *emulate(c))[0] == 0, sp.name


def test_traps_and_sentinels_are_where_build_case_says():
    for sp in (Spec("t", 150, 264, 136, resid=True), Spec("t8", 130, 200, 128, a8=True, resid=True), Spec("tb", 150, 264, 136, resid=True, family="bounded"),
               Spec("tp", 48, 200, 72, patch_group=16, resid=True), Spec("tw", 70, 136, 64, w8=True, resid=True, family="bounded")):
        c = R.build_case(sp)
        M, N, K = sp.M, sp.N, sp.K
        assert c.A_buf.shape == (M + 2, c.lda) and c.W_buf.shape == (N + 2, c.ldw)
        fixed_a, fixed_w = sp.a8, sp.a8 or sp.w8
        assert (c.lda == K) == fixed_a and (c.ldw == K) == fixed_w and c.lda % 8 == 0 and c.ldw % 8 == 0 and c.ldc == N + 8 and c.ldr == N + 16
        trap_a = 448.0 if sp.a8 else R.TRAP
        trap_w = 448.0 if fixed_w else R.TRAP
        assert (np.abs(c.A_buf[M:]) == trap_a).all() and (np.abs(c.A_buf[:M, K:]) == R.TRAP).all()
        assert (np.abs(c.W_buf[N:]) == trap_w).all() and (np.abs(c.W_buf[:N, K:]) == R.TRAP).all()
        assert np.abs(c.A).max() < 64 and np.abs(c.W).max() < 64
        assert R.is_bf16(c.A_buf) and R.is_bf16(c.W_buf) and R.is_bf16(c.bias) and R.is_bf16(c.resid_buf)
        assert (c.bias[N:] == R.TRAP).all()
        rows = 1 + sp.patch_group if sp.patch_group else M
        assert c.resid_buf.shape == (rows + 2, c.ldr) and (np.abs(c.resid_buf[rows:]) == R.TRAP).all() and (np.abs(c.resid_buf[:rows, N:]) == R.TRAP).all()
        if sp.a8:
            assert np.array_equal(R.e4m3_table()[c.A8], c.A_buf) and c.A8.dtype == np.uint8
        if fixed_w:
            assert np.array_equal(R.e4m3_table()[c.W8], c.W_buf)
        idx = R.out_index(c)
        assert idx.shape == (M, N) and len(np.unique(idx)) == M * N and idx.max() < R.c_words(c) - 2 * c.ldc + c.ldc
        if sp.patch_group:  # the CLS rows are not output
            cls_rows = np.arange(M // sp.patch_group) * (sp.patch_group + 1)
            assert not np.isin(idx // c.ldc, cls_rows).any() and c.out_rows == M + M // sp.patch_group
    assert np.isnan(R.bits_to_f32(np.array([R.SENT16], np.uint16)))[0]
    assert np.isnan(np.array([R.SENT16 << 16 | R.SENT16], np.uint32).view(np.float32))[0]


def test_head_major_index_is_the_layout_of_common_h():
    """[frame][q|k|v][head] blocks of tok * hd elements, each [token][64] followed by [token][hd - 64]; weight rows ordered, per third of N, as the
    first 64 dims of every head and then the rest of every head."""
    tok, nh, hd = 17, 2, 72
    c = R.build_case(Spec("hm", 34, 3 * nh * hd, 64, lnfold=True, hm=(tok, nh, hd)))
    idx = R.out_index(c)
    assert c.ldc == c.spec.N and sorted(idx.ravel()) == list(range(34 * c.spec.N))
    d3 = nh * hd
    for (m, n) in ((0, 0), (18, 5), (3, 64 + 7), (20, 2 * 64 + 3), (33, d3 + 2 * 64 + 7), (16, 2 * d3 + 64), (17, 2 * 64 + 8 + 1)):
        f, t, plane, rr = m // tok, m % tok, n // d3, n % d3
        if rr < nh * 64:
            head, dim = rr // 64, rr % 64
        else:
            head, dim = (rr - nh * 64) // (hd - 64), 64 + (rr - nh * 64) % (hd - 64)
        block = ((f * 3 + plane) * nh + head) * tok * hd
        want = block + (t * 64 + dim if dim < 64 else tok * 64 + t * (hd - 64) + dim - 64)
        assert idx[m, n] == want, (m, n)


def test_route_mirror_is_self_consistent():
    """Every spec names a launch the dispatch accepts, every form of the issue's table is reached at 256 CUs and at 304 and 120, the forced
    routes do not depend on the CU count, and each predicate is approached from both sides."""
    for n_cu in (256, 304, 120):
        specs = R.route_specs(n_cu)
        names = [sp.name for sp in specs]
        assert len(set(names)) == len(names)
        forms = {}
        for sp in specs:
            rc, form = R.expected(sp, n_cu)
            assert rc == R.OK and form, sp.name
            forms.setdefault(R.family_of(form), []).append(sp)
        assert not [f for f in R.REQUIRED if f not in forms], [f for f in R.REQUIRED if f not in forms]
        for fam in ("pp4-lean16ht", "pp4-a3", "pp4-f8", "pp4-lnfold-lean16", "pp4-stats-lean16ht"):  # the product's instances: dbg == 0
            assert all(sp.flags == 0 for sp in forms[fam]), fam
        for sp in specs:
            if sp.flags & (15 << R.FORCE_SHIFT) and not sp.name.startswith(("w6-", "lnout-rms-w6")):
                assert R.expected(sp, n_cu) == R.expected(sp, 256), sp.name
        by = {sp.name: R.form_name(R.expected(sp, n_cu)[1]) for sp in specs}
        assert by["t64-96tiles-x"].startswith("glds-128x128") and by["t64-94tiles-x"].startswith("glds-64x128")
        assert by["t64-m64-x"].startswith("glds-128x128") and by["t64-m65-x"].startswith("glds-64x128")
        assert by["splitk-refused-by-bias"].startswith("glds-") and by["splitk-short-k"].startswith("glds-")
        assert by["w6-refuses-resid-relu-x"].startswith("glds-") and by["w6-refuses-k192-x"].startswith("glds-")
        assert [n for n in by if n.startswith("a3-off")] and all(by[n] == "pp4-lean16ht-epi0" for n in by if n.startswith("a3-off"))
        assert by["lnf-lean-300x384x128-x"] == "pp4-lnfold-lean16-epi0" and by["lnf-general-300x328x128-x"] == "pp4-lnfold-general-epi0"
    # slice counts where nk / slices is not whole
    assert R.split_k_slices(Spec("s", 200, 264, 8512))[0] == 15 and (8512 // 64) % 15 != 0
    assert R.form_name(4110 | R.W8_EXPANDED) == "pp4-lnfold-lean16-epi0+w8x" and R.form_name(3016) == "splitk-16slices"


def test_gelu_forms_are_measured_from_the_header():
    e = R.gelu_forms()
    assert set(e) == {"deg12", "phi", "deg8"}
    assert 0 < e["deg12"] < 4e-6 and 5e-5 < e["phi"] < 2.5e-4 and 5e-5 < e["deg8"] < 2.5e-4, e  # (sanity: a misparsed coefficient gives 1e-1)
    print(e)


def test_half_unit_of_the_output_formats():
    assert R.half_ulp(1.0, 8) == 2.0 ** -8 and R.half_ulp(1.99, 8) == 2.0 ** -8 and R.half_ulp(2.0, 8) == 2.0 ** -7 and R.half_ulp(0.0, 8) == 0
    x = np.linspace(0.5, 4.0, 100001)
    assert (np.abs(round_bf16(x.astype(np.float32)).astype(np.float64) - x.astype(np.float32)) <= R.half_ulp(x.astype(np.float32), 8)).all()
    assert (np.abs(round_bf16(x.astype(np.float32)).astype(np.float64) - x.astype(np.float32)) > 2.0 ** -9 * x).any()  # why the flat 2^-9 |y| is not the bound


def test_probe_entry_refuses_a_stale_struct_without_a_gpu():
    """eilev_debug_gemm exists in the probe library only, and a wrong struct size comes back as EILEV_E_BADARG before any HIP call."""
    import os

    from eilev_amd import abi

    if not os.path.exists(abi.PROBES_LIB_PATH):
        pytest.skip("libeilev_hip_probes.so not built")
    if os.path.exists(abi.HIP_LIB_PATH):
        assert not hasattr(ctypes.CDLL(abi.HIP_LIB_PATH), "eilev_debug_gemm")
    fn = ctypes.CDLL(abi.PROBES_LIB_PATH).eilev_debug_gemm
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(512)
    form = ctypes.c_int(-1)
    assert fn(buf, ctypes.c_size_t(216), ctypes.byref(form), None) == R.E_BADARG
    assert fn(buf, ctypes.c_size_t(232), ctypes.byref(form), None) == R.E_BADARG
    assert fn(None, ctypes.c_size_t(224), ctypes.byref(form), None) == R.E_BADARG
