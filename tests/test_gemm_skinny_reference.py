"""CPU: the route mirror, the K partition, the row deal, the layouts and the bound of tests/gemm_skinny_ref.py (what tests/test_hip_gemm_skinny.py
holds the M <= 32 GEMM kernels to), and what planted mistakes cost against them.

emulate() below replays one launch through the kernels' own index maps in numpy: the K range of every (split, wave) as the kernels compute it, the
partial planes [ks][mr][N] in a poisoned scratch, the reduce over the planes, the epilogue order of skinny_epilogue, the stream layout read back
with the kernel's fragment stride, the row-block layout of A / C / ln_out, and the store into a poisoned C allocation.  One mistake at a time is
planted; on the exact family it must change at least one word, on the bounded family it must cost err / tol >= 4 (or write outside the output).
Measured (words changed on the exact family, worst err / tol on the bounded family):

  mistake                 exact: words  bounded: err/tol
  plane_off_mr                    4789               inf   (rows 16..31 of the second plane are read where nothing was written)
  plane_not_summed                4146               585
  bias_col_plus1                  4791          9.57e+06
  scale_cols_one_block             386               315
  stream_nv16                      987          2.16e+03
  frag_halves_swapped             6968               inf   (rows 25..31 of the A buffer hold NaN)
  frag_rows16_from_row0           2461          1.43e+03
  store_into_ldc_padding             1               inf
"""
import ctypes

import numpy as np

import gemm_ref as R
import gemm_skinny_ref as S
from eilev_amd.synth import round_bf16


# ---- the K partition and the row deal ---------------------------------------------------------------------------------------------------------

def _partition(units, ks):
    """Tiles per (y, wave) of one launch; asserts that they cover [0, units) exactly once."""
    count = np.zeros(units, int)
    sizes = []
    for y in range(ks):
        for w in range(4):
            beg, end = S.wave_range(units, ks, y, w)
            assert beg >= 0 and (end == beg or end <= units)   # (an idle wave's empty range may start past the end)
            count[beg:end] += 1
            sizes.append(end - beg)
    assert (count == 1).all(), (units, ks, count)
    return sizes


def test_k_partition_of_the_dma_nb_w8_and_plain_kernels_is_a_partition():
    pairs = {(sp.K // 256, S.plan(sp, 256)[2]) for sp in S.route_specs(256) if sp.K % 256 == 0 and (S.plan(sp, 256)[1] & 0xFFFF) // 100 != 63}
    pairs |= {(kt, ks) for kt in range(1, 81) for ks in range(1, 17)}
    for kt, ks in sorted(pairs):
        sizes = _partition(kt, max(ks, 1))
        if S.pre_rule(kt * 256, max(ks, 1)):
            assert max(sizes) <= 3, (kt, ks, sizes)   # the preloaded forms hold three tiles of activations per wave
    # the plain kernel: the same rule in steps of 32 over ceil(K / 32)
    for K in (72, 264, 2056, 512, 8, 40):
        for ks in (1, 2, 3):
            _partition((K + 31) // 32, ks)
    # the launch's own ks leaves every wave >= 8 steps of 32: ks <= ksteps / 32
    for sp in S.route_specs(256):
        rc, form, ks, _ = S.plan(sp, 256)
        if (form & 0xFFFF) // 100 != 63 and ks > 1:
            assert ks <= (sp.K + 31) // 32 // 32, sp.name


def test_rows32_k_slices_are_a_partition():
    """gemm_rows32_kernel: wave w of split y owns columns [(8 y + w) KS 32, + KS 32): 8 ks KS 32 == K for every planned shape."""
    for K in range(256, 256 * 81, 256):
        for n_cu in (8, 64, 120, 256, 304):
            for N in (16, 320, 4096, 20000):
                for ff in (False, True):
                    shape = S.rows32_shape(N, K, n_cu, ff)
                    if shape:
                        k5, ksteps, grid_x = shape
                        assert 8 * k5 * ksteps * 32 == K and ksteps in (5, 8, 10) and 1 <= grid_x <= max(n_cu, 1) and grid_x <= (N + 15) // 16


def test_row_deal_is_a_partition():
    for N in list(range(1, 70)) + [200, 637, 1027, 4095, 20736]:
        for grid in (1, 2, 3, 7, 8, 13, 64, 255, 256):
            if grid > (N + 15) // 16:
                continue
            nxt = 0
            for x in range(grid):
                r0, cnt = S.rows32_rows(N, grid, x)
                assert r0 == nxt and cnt >= 0
                nxt = r0 + cnt
            assert nxt == N


def test_stream_layout_is_a_permutation_and_matches_the_restatement_of_the_pack_test():
    for N, K, grid in ((811, 64, 8), (320, 96, 20), (37, 32, 3), (771, 64, 8)):
        W = np.arange(N * K, dtype=np.int64).reshape(N, K)
        idx = S.stream_index(N, K, grid)
        assert sorted(idx.ravel()) == list(range(N * K))
        Wp = S.stream_pack(W, grid)
        assert np.array_equal(S.stream_read(Wp, N, K, grid), W)
        # the restatement of tests/test_hip_stream_layout.py (blocks as reshapes), stated again here
        out = np.empty(N * K, np.int64)
        per, rem = divmod(N, grid)
        for x in range(grid):
            r0, cnt = x * per + min(x, rem), per + (1 if x < rem else 0)
            for j in range((cnt + 15) // 16):
                nv = min(16, cnt - 16 * j)
                out[(r0 + 16 * j) * K:(r0 + 16 * j + nv) * K] = W[r0 + 16 * j:r0 + 16 * j + nv].reshape(nv, K // 32, 4, 8).transpose(1, 0, 2, 3).reshape(-1)
        assert np.array_equal(out, Wp)


def test_frag32_index():
    r, c = np.arange(32)[:, None], np.arange(96)[None, :]
    idx = S.frag32_index(r, c)
    assert sorted(idx.ravel()) == list(range(32 * 96))
    assert idx[0, 0] == 0 and idx[1, 0] == 32 and idx[0, 31] == 31 and idx[0, 32] == 1024 and idx[16, 0] == 512 and idx[31, 95] == 2 * 1024 + 31 * 32 + 31
    buf = S.to_frag32(np.ones((25, 64), np.float32), 64)
    assert np.isnan(buf).sum() == 7 * 64 and np.isnan(buf[S.frag32_index(np.arange(25, 32)[:, None], np.arange(64)[None, :])]).all()


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------------

def _round_out(sp, v):
    return v.astype(np.float32).astype(np.float64) if sp.out_f32 else round_bf16(v.astype(np.float32)).astype(np.float64)


def _k_slices(sp, form, ks):
    """Per split y: the K columns its workgroups accumulate."""
    K = sp.K
    if (form & 0xFFFF) // 100 == 63:
        KS = (form & 0xFFFF) % 100
        return [np.arange(y * 8 * KS * 32, (y + 1) * 8 * KS * 32) for y in range(ks)]
    unit = 256 if (form & 0xFFFF) // 100 != 60 else 32
    units = -(-K // unit)
    out = []
    for y in range(ks):
        cols = [np.arange(b * unit, min(e * unit, K)) for b, e in (S.wave_range(units, ks, y, w) for w in range(4)) if e > b]
        out.append(np.concatenate(cols) if cols else np.arange(0))
    return out


def c_words(c):
    sp = c.spec
    return 32 * sp.N if sp.c_frag else (sp.M + 2) * c.ldc


def out_index(c):
    sp = c.spec
    m, n = np.arange(sp.M)[:, None], np.arange(sp.N)[None, :]
    return S.frag32_index(m, n) if sp.c_frag else m * c.ldc + n


def emulate(c, n_cu, mut=None):
    sp = c.spec
    rc, form, ks, grid_x = S.plan(sp, n_cu)
    assert rc == R.OK
    ks = max(ks, 1)
    M, N, K = sp.M, sp.N, sp.K
    mr = 16 if M <= 16 else 32
    A, W = c.A.astype(np.float64), c.W.astype(np.float64)
    if form & S.STREAM:
        W = S.stream_read(S.stream_pack(W, grid_x), N, K, grid_x, (lambda nv: 16) if mut == "stream_nv16" else None)
    if sp.a_frag:
        buf = S.to_frag32(c.A, K).astype(np.float64)
        rows = np.arange(M)
        if mut == "frag_halves_swapped":
            rows = (rows + 16) % 32
        elif mut == "frag_rows16_from_row0":
            rows = np.where(rows >= 16, 0, rows)
        A = buf[S.frag32_index(rows[:, None], np.arange(K)[None, :])]
    # partial planes in a poisoned scratch
    scratch = np.full((ks + S.GUARD_PLANES) * mr * N, np.nan)
    stride_w = (48 - mr) if mut == "plane_off_mr" else mr
    rows, cols = np.arange(M)[:, None], np.arange(N)[None, :]
    for y, kc in enumerate(_k_slices(sp, form, ks)):
        scratch[(y * stride_w + rows) * N + cols] = A[:, kc] @ W[:, kc].T
    acc = np.zeros((M, N))
    for s in range(ks - 1 if mut == "plane_not_summed" else ks):
        acc = acc + scratch[(s * mr + rows) * N + cols]
    if c.wscale is not None:
        acc = acc * c.wscale.astype(np.float64)[None, :]
    if c.bias is not None:
        sh = 1 if mut == "bias_col_plus1" else 0
        acc = acc + c.bias[sh:sh + N].astype(np.float64)[None, :]
    sc = sp.scale_cols + (16 if mut == "scale_cols_one_block" else 0)
    acc[:, :sc] *= sp.scale
    if sp.epi == 1:
        acc = R.gelu_exact(acc)
    elif sp.epi == 2:
        acc = np.maximum(acc, 0.0)
    if c.resid is not None:
        acc = acc + c.resid.astype(np.float64)
    flat = np.full(c_words(c), np.nan)
    flat[out_index(c).ravel()] = _round_out(sp, acc).ravel()
    if mut == "store_into_ldc_padding":
        flat[N] = 1.0
    return flat


def judge(c, flat, n_cu=256):
    """(words that differ from the reference allocation, worst err / tol; inf for a word outside the output or a NaN inside)."""
    sp = c.spec
    y, Sm, _ = R.reference(c)
    _, form, ks, _ = S.plan(sp, n_cu)
    idx = out_index(c).ravel()
    ref = np.full(c_words(c), np.nan)
    ref[idx] = _round_out(sp, y).ravel()
    same = (flat == ref) | (np.isnan(flat) & np.isnan(ref))
    ratio = float(R.ratio(np.abs(flat[idx] - y.ravel()), S.tol(c, y, Sm, form, ks).ravel()).max())
    written = np.zeros(flat.size, bool)
    written[idx] = True
    if (~np.isnan(flat[~written])).any():
        ratio = np.inf
    return int((~same).sum()), ratio


NCU = 256
MUTATIONS = {  # name: the spec (by name, both families) the mistake acts on
    "plane_off_mr": "dma-25x200x2048-split",
    "plane_not_summed": "dma-25x200x2048-split",
    "bias_col_plus1": "r32epi-bias-relu",
    "scale_cols_one_block": "r32epi-scale16",
    "stream_nv16": "ring-1280-short-25x1067",
    "frag_halves_swapped": "frag-a-25x296x1280",
    "frag_rows16_from_row0": "frag-a-25x296x1280",
    "store_into_ldc_padding": "dma-3x200x512",
}


def _spec(name):
    return next(sp for sp in S.route_specs(NCU) if sp.name == name)


def test_every_planted_mistake_is_detected():
    table = {}
    for mut, base in MUTATIONS.items():
        cx, cb = S.build_case(_spec(base + "-x")), S.build_case(_spec(base + "-b"))
        table[mut] = (judge(cx, emulate(cx, NCU, mut))[0], judge(cb, emulate(cb, NCU, mut))[1])
    for mut, (words, ratio) in table.items():
        print(f"{mut:24s} {words:>8} {ratio:>12.3g}")
    for mut, (words, ratio) in table.items():
        assert words >= 1, f"{mut}: no word changes on the exact family"
        assert ratio >= 4.0, f"{mut}: costs only {ratio:.3g} tol on the bounded family"


def test_the_unmutated_emulation_passes_its_own_check():
    """Every kind of launch once, through the index maps: bit equality on the exact family, err / tol <= 1 on the bounded one."""
    names = set(MUTATIONS.values()) | {"plain-16x40x2056-split", "nb7-32x200x2048-split", "r32-5-split4-32x320x5120", "stream-split-32x320x2560",
                                       "frag-ac-17x288x1280", "w8-17x200x2048-split", "ring-2560-uneven-32x771", "reduce-ks3-scale", "plain-3x1001x264-f32"}
    for base in sorted(names):
        cx, cb = S.build_case(_spec(base + "-x")), S.build_case(_spec(base + "-b"))
        assert judge(cx, emulate(cx, NCU))[0] == 0, base
        assert judge(cb, emulate(cb, NCU))[1] <= 1.0, base


# ---- the cases and the mirror ------------------------------------------------------------------------------------------------------------------

def test_exact_family_results_are_bf16_values():
    specs = [sp for sp in S.route_specs(NCU) if sp.family == "exact" and sp.M * sp.N * sp.K <= 3e8]
    assert len(specs) > 100
    for sp in specs:
        c = S.build_case(sp)
        y = R.reference(c)[0]
        assert R.is_bf16(y) and np.abs(y).max() <= 256, sp.name


def test_guards_are_where_build_case_says():
    for sp in (_spec("dma-25x200x2048-split-x"), _spec("ring-1280-short-25x1067-b"), _spec("w8-17x200x512-b")):
        c = S.build_case(sp)
        lda, ldw, ldr, ldc = S.strides(sp)
        assert (c.lda, c.ldw, c.ldr, c.ldc) == (lda, ldw, ldr, ldc) and c.W_buf.shape == (sp.N + 2, ldw) and c.A_buf.shape == (sp.M + 2, lda)
        assert (ldw == sp.K) == bool(sp.dense_w or sp.w8) and lda == sp.K + 8 and ldc == sp.N + 8
        assert (np.abs(c.A_buf[sp.M:]) == R.TRAP).all() and (np.abs(c.A_buf[:sp.M, sp.K:]) == R.TRAP).all()
        assert (np.abs(c.W_buf[sp.N:]) == (448.0 if sp.w8 else R.TRAP)).all() and (np.abs(c.W_buf[:sp.N, sp.K:]) == R.TRAP).all()
        assert (c.bias[sp.N:] == R.TRAP).all()


def test_route_mirror_is_self_consistent():
    """Every form of the issue's table is reached by name on 256, 304 and 120 CUs; the flag-forced routes and the grid-override routes do not
    depend on the CU count; each predicate is approached from both sides."""
    for n_cu in (256, 304, 120):
        specs = S.route_specs(n_cu)
        names = [sp.name for sp in specs]
        assert len(set(names)) == len(names)
        seen = set()
        for sp in specs:
            rc, form, ks = S.expected(sp, n_cu)
            assert rc == R.OK and form and (form & 0xFFFF) // 1000 == 6 and ks >= 1, sp.name
            assert bool(form & S.SPLIT_K) == (ks > 1), sp.name
            seen.add(S.family_of(form))
            seen.add(S.reduce_name(form, ks))
            if sp.grid == 8 or (sp.flags and not sp.name.startswith("r32")):
                assert S.expected(sp, n_cu) == S.expected(sp, 256), sp.name
        assert not [f for f in S.REQUIRED if f not in seen], [f for f in S.REQUIRED if f not in seen]
        by = {sp.name: S.form_name(S.expected(sp, n_cu)[1]) for sp in specs}
        assert by["dma-16x200x2048-split-x"] == "dma-1-pre+split" and by["dma-16x200x2048-fallback-x"] == "dma-1-pre"
        assert by["dma-16x200x2048-short-scratch-x"] == "dma-1-pre"
        assert by["r32-5-split2-25x320x2560-x"] == "rows32-5+split" and by["r32-nosplit-25x320x2560-x"] == "dma-2-pre"
        assert by[f"r32-8-17x{16 * n_cu - 1}x2048-x"] == "rows32-8" and by[f"r32-8-refused-17x{16 * n_cu - 16}x2048-x"] == "dma-2-pre"
        assert by["stream-25x296x1280-x"] == "rows32-5+stream" and by["stream-off-ldw-x"] == "rows32-5" and by["stream-off-flag-x"] == "rows32-5"
        assert by["rln-ks2-ln-320"].endswith("+split+ln") and by["rln-two-launch-relu"].endswith("+split")
        assert by["rln-unfused-flag"].endswith("+split") and by["w8-16x40x272-expanded-x"] == "plain+w8x"
        ring = S.natural_ring_spec(n_cu)
        rc, form, ks, grid_x = S.plan(ring, n_cu)
        assert S.form_name(form) == "rows32-10+stream" and grid_x == n_cu and all(S.rows32_rows(ring.N, grid_x, x)[1] == 81 for x in range(grid_x))
    # the ring cases cross 2 RB blocks per workgroup from both sides (RB = 4 for KS = 5, 3 for KS = 8 / 10) and deal uneven shares
    for sp in S.ring_specs():
        rc, form, ks, grid_x = S.plan(sp, 256)
        assert grid_x == 8 and sp.N % 8
    blocks = {(sp.K, max((S.rows32_rows(sp.N, 8, x)[1] + 15) // 16 for x in range(8))) for sp in S.ring_specs()}
    for K, RB in ((1280, 4), (2560, 3), (2048, 3)):
        assert {(K, 2 * RB - 1), (K, 2 * RB), (K, 2 * RB + 1), (K, 3 * RB + 1)} <= blocks
    sp = next(sp for sp in S.ring_specs() if "uneven" in sp.name)
    assert len({(S.rows32_rows(sp.N, 8, x)[1] + 15) // 16 for x in range(8)}) == 2
    # refusals the mirror knows
    assert S.expected(S.SSpec("r", 25, 296, 1280, c_frag=True), 256)[0] == R.E_UNSUPPORTED            # N % 32
    assert S.expected(S.SSpec("r", 25, 320, 1280, c_frag=True, resid=True), 256)[0] == R.E_UNSUPPORTED
    assert S.expected(S.SSpec("r", 16, 320, 1280, a_frag=True), 256)[0] == R.E_UNSUPPORTED             # M <= 16: not rows32
    assert S.expected(S.SSpec("r", 25, 320, 768, a_frag=True), 256)[0] == R.E_UNSUPPORTED              # no rows32 shape
    assert S.expected(S.SSpec("r", 25, 320, 2560, ln_frag=True, scratch=S.scr(320)), 256)[0] == R.E_UNSUPPORTED   # no ln_out
    assert S.expected(S.SSpec("r", 25, 320, 2560, c_frag=True, scratch=S.scr(320)), 256)[0] == R.E_UNSUPPORTED    # a split
    assert S.expected(S.SSpec("r", 16, 4104, 2048, ln_out=1, scratch=S.scr(4104)), 256) == (R.E_UNSUPPORTED, 0, 0)  # ln_out nobody can write
    assert S.expected(S.SSpec("r", 16, 40, 264, w8=True), 256)[0] == R.E_BADARG and S.expected(S.SSpec("r", 16, 40, 68), 256)[0] == R.E_UNSUPPORTED
    assert S.form_name(6228 | S.SPLIT_K) == "nb-2-8+split" and S.form_name(6310 | S.STREAM) == "rows32-10+stream" and S.form_name(6000) == "plain"
    assert S.form_name(6411) == "w8-1-pre" and S.form_name(6120) == "dma-2-rolled" and S.family_of(6305 | S.SPLIT_K | S.REDUCE_LN) == "rows32-5"


def test_addition_count_of_the_bound():
    sp = S.SSpec("t", 16, 200, 2048)
    assert S.n_adds(sp, 6111, 1) == 2048 + 8 and S.n_adds(sp, 6111 | S.SPLIT_K, 2) == 2048 + 4 + 2 + 3 and S.n_adds(sp, 6310, 1) == 2048 + 8 + 1 + 3
    assert R.ACC_C == 1.0


def test_skinny_probe_entry_refuses_a_stale_struct_without_a_gpu():
    """eilev_debug_gemm_skinny exists in the probe library only; a wrong struct size comes back as EILEV_E_BADARG before any HIP call."""
    import os

    from eilev_amd import abi

    assert os.path.exists(abi.PROBES_LIB_PATH), "libeilev_hip_probes.so is not built: build() makes it next to the product library (a failed probe build must not pass)"
    if os.path.exists(abi.HIP_LIB_PATH):
        assert not hasattr(ctypes.CDLL(abi.HIP_LIB_PATH), "eilev_debug_gemm_skinny")
    fn = ctypes.CDLL(abi.PROBES_LIB_PATH).eilev_debug_gemm_skinny
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(512)
    form, ks = ctypes.c_int(-1), ctypes.c_int(-1)
    for size in (224, 256, 260, 272):
        assert fn(buf, ctypes.c_size_t(size), ctypes.byref(form), ctypes.byref(ks), None) == R.E_BADARG
    assert fn(None, ctypes.c_size_t(264), ctypes.byref(form), ctypes.byref(ks), None) == R.E_BADARG
    assert form.value == -1 and ks.value == -1
