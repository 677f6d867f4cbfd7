"""Every M <= 32 (decode) GEMM kernel of csrc/gemm_skinny.h and the two reduce kernels behind a K split (skinny_reduce_kernel, norm.hip
reduce_ln_wg_kernel), launched on their own through the probe entry eilev_debug_gemm_skinny (one launch_gemm on explicit arguments, with the
split-K scratch, the stream-layout copy of W and the row-block switches that eilev_debug_gemm cannot pass; it reports the kernel instance and
the K slices) and compared with the float64 reference of tests/gemm_ref.py under the bound of tests/gemm_skinny_ref.py.

Every launch is judged as in test_hip_gemm_wide.py: the return code; form and ks equal to gemm_skinny_ref.expected (a Python mirror of
launch_skinny, rows32_plan and skinny_reduce); every output element within tol (derived, no floor, no max|ref| term) and BIT FOR BIT on the
exact family (+-0 are one value); every word outside the defined output still on its NaN sentinel — the ldc padding, the guard rows, rows
M.. of ln_out, rows M..mr - 1 of every used scratch plane and every plane behind the ks used ones.  On the exact family the used planes must
also add up to A W^T exactly (a partial in the wrong plane or a K slice read twice cannot hide behind the reduce).  The operands carry
+-2^14 traps in their padding columns and in the two rows after the last; rows M..31 of a row-block A buffer hold NaN.

instance (gemm_skinny_ref.family_of)   route (gemm_skinny_ref.route_specs)
plain                  K % 256 != 0 or DBG_GEMM_SKINNY_NO_DMA, M <= 16: 40 x 72, 1001 x 264 (ragged N, the kin tail), 40 x 2056 with scratch (ks = 2)
dma-{1,2}-pre          200 x 512 (three idle waves), 200 x 768, 24 x 3072 (3 tiles per wave), 200 x 2048 with scratch (split), without and with
                       a scratch one word short (fallback)
dma-{1,2}-rolled       DBG_GEMM_SKINNY_NO_PRELOAD; naturally 200 x 3328 (4 tiles per wave)
nb-{1,2}-{2,4,8}       DBG_GEMM_NB_SHIFT 2 / 4 / 7: 200 x 768 (13 blocks: a short last workgroup, a clamped last block), 16 x 256 (total = 1), split
rows32-{5,8,10}        K = 1280 / 2048 / 2560: N = 200, 1000, 16 n_cu +- 16; 320 x 2560 / 5120 split in 2 / 4; 16 n_cu rows; the per_wave == 8 refusal;
                       grid override 8: 2 RB - 1, 2 RB, 2 RB + 1, 3 RB + 1 blocks per workgroup, short last blocks, uneven shares; ONE natural-grid
                       ring case (N = 81 n_cu, K = 2560); plain and general epilogues; stream layout on / ignored; row-block A, C and ln_out
w8-{1,2}-{pre,rolled}  e4m3 weights with wscale: 200 x 512, 200 x 2048 split, 200 x 768 rolled; K = 272 takes the expansion and the plain kernel
skinny_reduce          ks = 2, 3, 4 x ReLU, GELU, fp32 + residual, scale_cols, wscale
reduce_ln-{2,4,0}      N = 320 and 4096, LayerNorm and RMS, wscale, ln_frag; epi != 0 and the switch take the two-launch form; N = 4104 (no
                       LayerNorm kernel takes more than 4096 columns) is refused before anything runs

Measured on the device: profiles/parity_r06.json, section gemm_skinny."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gemm_ref as R
import gemm_skinny_ref as S
from gemm_skinny_ref import SSpec

pytestmark = pytest.mark.gpu


class GemmArgs(C.Structure):
    """ctypes mirror of EilevDebugGemmArgs (csrc/gemm.hip, probe build), as in test_hip_gemm_wide.py."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("W", C.c_void_p), ("ldw", C.c_int64),
                ("bias", C.c_void_p), ("resid", C.c_void_p), ("ldr", C.c_int64), ("C", C.c_void_p), ("ldc", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epi", C.c_int32), ("out_f32", C.c_int32),
                ("scale", C.c_float), ("scale_cols", C.c_int32), ("patch_group", C.c_int32),
                ("hm_tok", C.c_int32), ("hm_heads", C.c_int32), ("hm_hd", C.c_int32), ("pad0", C.c_int32),
                ("wscale", C.c_void_p), ("W8", C.c_void_p), ("w8_scratch", C.c_void_p), ("A8", C.c_void_p),
                ("ascale", C.c_void_p), ("ln_rows", C.c_void_p), ("ln_csum", C.c_void_p),
                ("stat_out", C.c_void_p), ("stat_ld", C.c_int64),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out", C.c_void_p), ("ln_eps", C.c_float), ("pad1", C.c_int32)]


class SkinnyArgs(C.Structure):
    """ctypes mirror of EilevDebugSkinnyArgs (csrc/gemm.hip, probe build): EilevDebugGemmArgs followed by the six decode-only fields."""
    _fields_ = [("g", GemmArgs), ("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64), ("Wp", C.c_void_p),
                ("a_frag", C.c_int32), ("c_frag", C.c_int32), ("ln_frag", C.c_int32), ("pad2", C.c_int32)]


SENT32 = (R.SENT16 << 16) | R.SENT16
_WORST: dict = {}
_FIRST_FAIL: dict = {}
_SECONDS: dict = {}
_SEEN: set = set()
_case_cache: dict = {}


def _entry(lib):
    fn = lib.eilev_debug_gemm_skinny
    fn.argtypes = [C.POINTER(SkinnyArgs), C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
    fn.restype = C.c_int
    return fn


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case(sp):
    got = _case_cache.get(sp.name)
    if got is None:
        c = S.build_case(sp)
        y, Sm, _ = R.reference(c)
        got = (c, y, Sm)
        if sp.N * sp.K <= 1 << 21:
            _case_cache[sp.name] = got
    return got


def _dev_bf16(x):
    return torch.from_numpy(R.bf16_bits(x).view(np.int16)).cuda()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _poison16(n):
    return torch.full((n,), int(np.uint16(R.SENT16).view(np.int16)), dtype=torch.int16, device="cuda")


def _poison32(n):
    return torch.full((n,), int(np.uint32(SENT32).view(np.int32)), dtype=torch.int32, device="cuda")


def _same_bits(got, ref32):
    """Equal as numbers and no NaN: +0 and -0 are one value."""
    return (got == ref32) & ~np.isnan(got)


def _sent(t):
    r = t.cpu().numpy()
    return (r.view(np.uint32) == SENT32) if r.dtype == np.int32 else (r.view(np.uint16) == R.SENT16)


class Launch:
    """The device buffers of one case, every output poisoned."""

    def __init__(self, lib, c, n_cu, pack=True):
        sp = self.sp = c.spec
        self.c, self.lib = c, lib
        self.plan = S.plan(sp, n_cu)
        a = self.args = SkinnyArgs()
        g, k = a.g, {}
        self.keep = k
        M, N, K = sp.M, sp.N, sp.K
        k["A"] = _dev_bf16(S.to_frag32(c.A, K)) if sp.a_frag else _dev_bf16(c.A_buf)
        g.A = k["A"].data_ptr()
        if sp.w8:
            k["W"] = _dev(c.W8)
            g.W8 = k["W"].data_ptr()
        else:
            k["W"] = _dev_bf16(c.W_buf)
            g.W = k["W"].data_ptr()
        g.lda, g.ldw, g.ldr, g.ldc = c.lda, c.ldw, c.ldr, c.ldc
        if c.bias is not None:
            k["bias"] = _dev_bf16(c.bias)
            g.bias = k["bias"].data_ptr()
        if c.resid_buf is not None:
            k["resid"] = _dev_bf16(c.resid_buf)
            g.resid = k["resid"].data_ptr()
        self.words = 32 * N if sp.c_frag else (M + 2) * c.ldc
        self.out = _poison32(self.words) if sp.out_f32 else _poison16(self.words)
        g.C = self.out.data_ptr()
        g.M, g.N, g.K, g.epi, g.out_f32 = M, N, K, sp.epi, int(sp.out_f32)
        g.scale, g.scale_cols = float(sp.scale), sp.scale_cols
        if c.wscale is not None:
            k["wscale"] = _dev(c.wscale.astype(np.float32))
            g.wscale = k["wscale"].data_ptr()
        self.w8x = None
        if sp.w8 and K % 256:
            self.w8x = _poison16((N + 2) * K)
            g.w8_scratch = self.w8x.data_ptr()
        self.ln = None
        if sp.ln_out:
            self.ln = _poison16(32 * N if sp.ln_frag else (M + 2) * N)
            k["gamma"] = _dev_bf16(c.gamma)
            g.ln_gamma, g.ln_out, g.ln_eps = k["gamma"].data_ptr(), self.ln.data_ptr(), c.ln_eps
            if c.beta is not None:
                k["beta"] = _dev_bf16(c.beta)
                g.ln_beta = k["beta"].data_ptr()
        self.scratch = None
        if sp.scratch:
            self.scratch = _poison32(sp.scratch // 4 + S.GUARD_PLANES * 32 * N)
            a.scratch, a.scratch_bytes = self.scratch.data_ptr(), sp.scratch
        a.a_frag, a.c_frag, a.ln_frag = int(sp.a_frag), int(sp.c_frag), int(sp.ln_frag)
        if sp.stream and pack:
            self._pack(n_cu)
        self.form, self.ks = C.c_int(-1), C.c_int(-1)

    def _pack(self, n_cu):
        """Wp from eilev_stream_layout_pack under the case's grid override; it must be the index function's permutation, with nothing behind it."""
        sp, c = self.sp, self.c
        N, K = sp.N, sp.K
        bits = R.bf16_bits(np.ascontiguousarray(c.W))
        src = torch.from_numpy(bits.view(np.int16)).cuda()
        dst = _poison16((N + 2) * K)
        try:
            self.lib.eilev_debug_grid_cus(sp.grid)
            rc = self.lib.eilev_stream_layout_pack(C.c_void_p(src.data_ptr()), N, K, C.c_void_p(dst.data_ptr()), _stream())
        finally:
            self.lib.eilev_debug_grid_cus(0)
        torch.cuda.synchronize()
        assert rc == R.OK, (sp.name, rc)
        grid_x = S.rows32_shape(N, K, S.eff_cus(sp, n_cu))[2]
        got = dst.cpu().numpy().view(np.uint16)
        assert (got[N * K:] == R.SENT16).all(), f"{sp.name}: the pack wrote behind the matrix"
        assert np.array_equal(got[:N * K], S.stream_pack(bits, grid_x)), f"{sp.name}: the packed copy is not the stream layout of {grid_x} workgroups"
        self.keep["Wp"] = dst
        self.args.Wp = dst.data_ptr()

    def launch(self, struct_bytes=None, flags=None):
        lib = self.lib
        try:
            lib.eilev_debug_gemm_flags(self.sp.flags if flags is None else flags)
            lib.eilev_debug_grid_cus(self.sp.grid)
            rc = _entry(lib)(C.byref(self.args), C.sizeof(SkinnyArgs) if struct_bytes is None else struct_bytes, C.byref(self.form), C.byref(self.ks), _stream())
        finally:
            lib.eilev_debug_gemm_flags(0)
            lib.eilev_debug_grid_cus(0)
        torch.cuda.synchronize()
        return rc

    def output(self):
        """(values at the logical [M, N] positions, True iff every other word of C holds the sentinel)."""
        sp, c = self.sp, self.c
        raw = self.out.cpu().numpy()
        if sp.out_f32:
            vals, sent = raw.view(np.float32), (raw.view(np.uint32) == SENT32).copy()
        else:
            vals, sent = R.bits_to_f32(raw.view(np.uint16)), (raw.view(np.uint16) == R.SENT16).copy()
        m, n = np.arange(sp.M)[:, None], np.arange(sp.N)[None, :]
        idx = S.frag32_index(m, n) if sp.c_frag else m * c.ldc + n
        got = vals[idx]
        sent[idx.ravel()] = True
        return got, bool(sent.all())

    def untouched(self):
        return all(bool(_sent(t).all()) for t in (self.out, self.ln, self.scratch, self.w8x) if t is not None)


def _note(fam, name, ratio, where=None):
    _WORST[fam] = max(_WORST.get(fam, 0.0), float(ratio))
    if where is not None and fam not in _FIRST_FAIL:
        _FIRST_FAIL[fam] = f"{name} {where}"


def _check_scratch(L, c, ks, y_exact):
    sp = c.spec
    if L.scratch is None:
        return
    mr, N = (16 if sp.M <= 16 else 32), sp.N
    raw = L.scratch.cpu().numpy()
    sent = raw.view(np.uint32) == SENT32
    used = ks * mr * N if ks > 1 else 0
    assert sent[used:].all(), f"{sp.name}: a scratch word behind the {ks if ks > 1 else 0} used planes was written"
    if not used:
        return
    planes = raw.view(np.float32)[:used].reshape(ks, mr, N)
    s3 = sent[:used].reshape(ks, mr, N)
    assert s3[:, sp.M:].all(), f"{sp.name}: rows past M of a partial plane were written"
    assert not s3[:, :sp.M].any() and np.isfinite(planes[:, :sp.M]).all(), f"{sp.name}: a partial of rows < M is missing"
    if y_exact is not None:
        assert np.array_equal(planes[:, :sp.M].astype(np.float64).sum(0), y_exact), f"{sp.name}: the {ks} partial planes do not add up to A W^T"


def _check_ln_out(L, c, got_c):
    sp = c.spec
    raw = L.ln.cpu().numpy().view(np.uint16)
    if sp.ln_frag:
        m, n = np.arange(sp.M)[:, None], np.arange(sp.N)[None, :]
        idx = S.frag32_index(m, n)
        rest = np.ones(raw.size, bool)
        rest[idx.ravel()] = False
        assert (raw[rest] == R.SENT16).all(), f"{sp.name}: ln_out rows past M of the row-block buffer were written"
        got = R.bits_to_f32(raw[idx]).astype(np.float64)
    else:
        raw = raw.reshape(sp.M + 2, sp.N)
        assert (raw[sp.M:] == R.SENT16).all(), f"{sp.name}: ln_out rows past M were written"
        got = R.bits_to_f32(raw[:sp.M]).astype(np.float64)
    ref, t = R.ln_out_ref(c, got_c)
    rt = R.ratio(np.abs(got - ref), t)
    worst = float(rt.max())
    print(f"{sp.name}: ln_out err/tol {worst:.3f}")
    i, j = np.unravel_index(np.argmax(rt), rt.shape)
    _note("ln_out", sp.name, worst, None if worst <= 1 else f"[{i}, {j}]")
    assert worst <= 1.0, f"{sp.name}: ln_out err/tol {worst:.3g} at [{i}, {j}]: got {got[i, j]}, ref {ref[i, j]}"


def run_case(lib, sp, n_cu, keep=None):
    """One launch, every check.  Returns the Launch."""
    c, y, Sm = _case(sp)
    want_rc, want_form, want_ks, _ = S.plan(sp, n_cu)
    assert want_rc == R.OK, sp.name
    L = Launch(lib, c, n_cu)
    rc = L.launch()
    assert rc == want_rc, (sp.name, rc)
    assert (L.form.value, L.ks.value) == (want_form, want_ks), \
        f"{sp.name}: launched {S.form_name(L.form.value)} ks {L.ks.value}, the dispatch mirror says {S.form_name(want_form)} ks {want_ks}"
    fam, red = S.family_of(want_form), S.reduce_name(want_form, want_ks)
    got, intact = L.output()
    assert intact, f"{sp.name} ({fam}): a write outside the rows and columns of the output"
    exact = sp.family == "exact"
    for key in (fam, red):
        if key is None:
            continue
        if exact:
            ref32 = y.astype(np.float32)
            same = _same_bits(got, ref32)
            if not same.all():
                i, j = np.argwhere(~same)[0]
                _note(key, sp.name, np.inf, f"[{i}, {j}]")
                pytest.fail(f"{sp.name} ({S.form_name(want_form)}): {int((~same).sum())} of {same.size} elements differ on the exact family, first at "
                            f"[{i}, {j}]: got {got[i, j]}, ref {ref32[i, j]}")
            _note(key + "/exact", sp.name, 0.0)
        else:
            t = S.tol(c, y, Sm, want_form, want_ks)
            rt = R.ratio(np.abs(got.astype(np.float64) - y), t)
            worst = float(rt.max())
            if key == fam:
                print(f"{sp.name}: {S.form_name(want_form)} err/tol {worst:.3f}")
            if not worst <= 1.0:
                i, j = np.unravel_index(np.argmax(rt), rt.shape)
                _note(key, sp.name, worst, f"[{i}, {j}]")
                pytest.fail(f"{sp.name} ({S.form_name(want_form)}): err/tol {worst:.3g} at [{i}, {j}] (got {got[i, j]}, ref {y[i, j]}, tol {t[i, j]:.3g}); "
                            f"{int((rt > 1).sum())} of {rt.size} elements beyond tol")
            _note(key, sp.name, worst)
        _SEEN.add(key)
    _check_scratch(L, c, want_ks, c.A.astype(np.float64) @ c.W.astype(np.float64).T if exact and want_ks > 1 else None)
    if sp.ln_out:
        _check_ln_out(L, c, got)
    if L.w8x is not None:
        raw = L.w8x.cpu().numpy().view(np.uint16).reshape(sp.N + 2, sp.K)
        assert want_form & R.W8_EXPANDED and (raw[sp.N:] == R.SENT16).all(), f"{sp.name}: the expansion wrote past N rows"
        assert np.array_equal(raw[:sp.N], R.bf16_bits(c.W_buf[:sp.N])), f"{sp.name}: the scratch is not the e4m3 decode"
    if want_form & S.STREAM:  # the same launch on the checkpoint layout: same bits, the form bit clear
        L2 = Launch(lib, c, n_cu, pack=False)
        assert L2.launch() == R.OK and L2.form.value == want_form & ~S.STREAM, (sp.name, S.form_name(L2.form.value))
        got2, intact2 = L2.output()
        assert intact2 and np.array_equal(got2.view(np.uint32), got.view(np.uint32)), f"{sp.name}: the stream layout changes the result"
    if keep is not None:
        keep[sp.name] = got
    return L


def _record():
    from hip_utils import record_parity

    record_parity("gemm_skinny",
                  tol="half a unit of the output format at y + (K + waves + ks + 3) 2^-24 S_ij (x 1.13 for GELU) + the GELU polynomial's measured error; "
                      "exact family: equality; ACC_C = %g" % R.ACC_C,
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()}, **{f"first_failing_{k}": v for k, v in _FIRST_FAIL.items()},
                  **{f"seconds_{k}": v for k, v in _SECONDS.items()}, seconds_total=sum(_SECONDS.values()))


def _run_all(lib, specs, label, keep=None):
    assert specs
    n_cu = _num_cu()
    t0 = time.time()
    try:
        for sp in specs:
            run_case(lib, sp, n_cu, keep)
    finally:
        _SECONDS[label] = _SECONDS.get(label, 0.0) + time.time() - t0
        _record()


def test_plain_kernel(probes):
    _run_all(probes, S.plain_specs(), "plain")


def test_dma_kernels_preloaded_and_rolled(probes):
    _run_all(probes, S.dma_specs(), "dma")


@pytest.mark.parametrize("v", [2, 4, 7])
def test_nb_kernels(probes, v):
    """DBG_GEMM_NB_SHIFT 2 / 4 / 7: nb<1, 2>, <2, 2>; <1, 4>, <2, 4>; <1, 4> (8 is M > 16 only), <2, 8>."""
    _run_all(probes, [sp for sp in S.nb_specs() if sp.name.startswith(f"nb{v}-")], f"nb-{v}")


def test_rows32_natural_grid(probes):
    _run_all(probes, S.rows32_specs(_num_cu()), "rows32")


@pytest.mark.parametrize("K", [1280, 2048, 2560])
def test_rows32_ring_tail_and_uneven_deal(probes, K):
    """Grid override 8: the steady loop (nblk >= 2 RB), its tail, the short form below it, short last blocks and shares of different block counts."""
    _run_all(probes, [sp for sp in S.ring_specs() if sp.name.startswith(f"ring-{K}-")], f"ring-{K}")


def test_rows32_ring_at_the_natural_grid(probes):
    _run_all(probes, [S.natural_ring_spec(_num_cu())], "ring-natural")


def test_rows32_epilogues(probes):
    _run_all(probes, S.rows32_epilogue_specs(), "rows32-epilogues")


def test_stream_layout_used_and_ignored(probes):
    _run_all(probes, S.stream_specs(), "stream")


def test_row_block_layouts(probes):
    _run_all(probes, S.frag_specs(), "frag")


def test_fp8_weight_kernels(probes):
    _run_all(probes, S.w8_specs(), "w8")


def test_skinny_reduce_kernel(probes):
    _run_all(probes, S.reduce_specs(), "skinny_reduce")


def test_reduce_ln_kernels(probes):
    _run_all(probes, S.reduce_ln_specs(), "reduce_ln")


def test_fused_reduce_gives_the_bits_of_the_two_launches(probes):
    """DBG_GEMM_NO_REDUCE_LN: C agrees bit for bit with the fused launch (ln_out need not: its statistics are summed in another order, and both
    are held to the LayerNorm reference above)."""
    n_cu = _num_cu()
    fused = [sp for sp in S.reduce_ln_specs() + S.frag_specs() if S.plan(sp, n_cu)[1] & S.REDUCE_LN and not sp.ln_frag]
    assert len(fused) >= 8
    for sp in fused:
        c = _case(sp)[0]
        La = Launch(probes, c, n_cu)
        assert La.launch() == R.OK and La.form.value & S.REDUCE_LN
        two = R.replace(sp, flags=sp.flags | S.NO_REDUCE_LN)
        Lb = Launch(probes, c, n_cu)
        assert Lb.launch(flags=two.flags) == R.OK and Lb.form.value == La.form.value & ~S.REDUCE_LN, sp.name
        (ga, ia), (gb, ib) = La.output(), Lb.output()
        assert ia and ib and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), f"{sp.name}: fused and unfused C differ"
        _check_ln_out(Lb, c, gb)


def test_every_instance_of_the_table_was_reached_by_name(probes):
    """(Runs after the tests above in file order.)  What they recorded covers gemm_skinny_ref.REQUIRED; without them this test launches one case each."""
    n_cu = _num_cu()
    for key in S.REQUIRED:
        if key not in _SEEN:
            sp = next(sp for sp in S.route_specs(n_cu) if key in (S.family_of(S.plan(sp, n_cu)[1]), S.reduce_name(*S.plan(sp, n_cu)[1:3])))
            _run_all(probes, [sp], "coverage")
    assert not [k for k in S.REQUIRED if k not in _SEEN]


def test_refusals_launch_nothing(probes):
    """Each refusal returns its code, reports no form and leaves C, ln_out, the scratch and the expansion scratch on their sentinels."""
    n_cu = _num_cu()

    def call(sp, want, struct_bytes=None, top=None, **fields):
        L = Launch(probes, _case(sp)[0], n_cu)
        for k, v in fields.items():
            setattr(L.args.g, k, v)
        for k, v in (top or {}).items():
            setattr(L.args, k, v)
        rc = L.launch(struct_bytes)
        assert L.untouched(), (sp.name, fields, top)
        assert L.form.value in (0, -1), (sp.name, fields, top, L.form.value)
        assert rc == want, (sp.name, fields, top, rc, want)

    assert C.sizeof(SkinnyArgs) == 264 and C.sizeof(GemmArgs) == 224
    base = SSpec("refuse", 25, 320, 1280, grid=8)
    assert S.expected(base, n_cu)[0] == R.OK
    call(base, R.E_BADARG, struct_bytes=224)
    call(base, R.E_BADARG, struct_bytes=256)
    call(base, R.E_BADARG, struct_bytes=272)
    # any *_frag on a launch rows32 does not plan
    norows = SSpec("refuse-768", 25, 320, 768)
    for f in (dict(a_frag=1), dict(c_frag=1), dict(ln_frag=1)):
        call(norows, R.E_UNSUPPORTED, top=f)
    call(SSpec("refuse-m16", 16, 320, 1280, grid=8), R.E_UNSUPPORTED, top=dict(a_frag=1))
    call(R.replace(base, name="refuse-norows32", flags=S.NO_ROWS32), R.E_UNSUPPORTED, top=dict(a_frag=1))
    # c_frag with a residual, with a split, with N % 32 != 0, with fp32 output
    call(R.replace(base, name="refuse-cres", resid=True), R.E_UNSUPPORTED, top=dict(c_frag=1))
    split = SSpec("refuse-split", 25, 320, 2560, grid=64, scratch=S.scr(320), resid=False)
    assert S.expected(split, n_cu)[2] == 2
    call(split, R.E_UNSUPPORTED, top=dict(c_frag=1))
    call(SSpec("refuse-n296", 25, 296, 1280, grid=8), R.E_UNSUPPORTED, top=dict(c_frag=1))
    call(R.replace(base, name="refuse-cf32", out_f32=True), R.E_UNSUPPORTED, top=dict(c_frag=1))
    # ln_frag without a split, without ln_out
    call(R.replace(base, name="refuse-ln-nosplit", ln_out=1), R.E_UNSUPPORTED, top=dict(ln_frag=1))
    call(split, R.E_UNSUPPORTED, top=dict(ln_frag=1))
    # ln_out that neither the fused reduce nor a LayerNorm launch can write (N > 4096, fp32 output): refused before the GEMM
    wide_ln = SSpec("refuse-ln-4104", 16, 4104, 2048, family="bounded", scratch=S.scr(4104), ln_out=1, resid=True)
    assert S.expected(wide_ln, n_cu) == (R.E_UNSUPPORTED, 0, 0)
    call(wide_ln, R.E_UNSUPPORTED)
    call(SSpec("refuse-ln-f32", 16, 320, 2048, family="bounded", scratch=S.scr(320), ln_out=1), R.E_UNSUPPORTED, out_f32=1)
    # W8 without wscale, with ldw != K, with K % 16 != 0; K % 8 != 0; null operands
    w8 = SSpec("refuse-w8", 16, 200, 512, w8=True)
    call(w8, R.E_BADARG, wscale=None)
    call(w8, R.E_BADARG, ldw=520)
    call(w8, R.E_BADARG, K=264, ldw=264)
    call(SSpec("refuse-k", 16, 200, 72), R.E_UNSUPPORTED, K=68)
    call(SSpec("refuse-k", 16, 200, 72), R.E_UNSUPPORTED, lda=76)
    for f in (dict(A=None), dict(W=None), dict(C=None), dict(N=0)):
        call(SSpec("refuse-k", 16, 200, 72), R.E_BADARG, **f)


_product = None


def test_product_library_gives_the_same_bits(probes):
    """The public entry points of the PRODUCT library on one dma, one rows32 and one split shape (eilev_linear_w8 is the public call that passes
    a split-K scratch): bit-identical to the probe launch, and the product exports no probe entry."""
    from eilev_amd import abi

    global _product
    if _product is None:
        _product = abi.load_library(abi.HIP_LIB_PATH)
    assert not hasattr(_product, "eilev_debug_gemm_skinny") and not hasattr(_product, "eilev_debug_grid_cus")
    n_cu = _num_cu()
    for sp, want in ((SSpec("product-dma", 16, 200, 512, epi=2, resid=True, family="bounded", pad=False), "dma-1-pre"),
                     (SSpec("product-rows32", 32, 1000, 1280, epi=1, family="bounded", pad=False), "rows32-5"),
                     (SSpec("product-w8-split", 25, 200, 2048, w8=True, resid=True, family="bounded", pad=False, scratch=S.scr(200)), "w8-2-pre+split")):
        assert S.form_name(S.plan(sp, n_cu)[1]) == want
        keep = {}
        run_case(probes, sp, n_cu, keep)
        L = Launch(probes, _case(sp)[0], n_cu)
        a, g = L.args, L.args.g
        if sp.w8:
            rc = _product.eilev_linear_w8(C.c_void_p(g.A), C.c_void_p(g.W8), C.c_void_p(g.wscale), C.c_void_p(g.bias), C.c_void_p(g.resid), C.c_void_p(g.C),
                                          sp.M, sp.N, sp.K, sp.epi, 0, C.c_void_p(a.scratch), a.scratch_bytes, _stream())
        else:
            rc = _product.eilev_linear(C.c_void_p(g.A), C.c_void_p(g.W), C.c_void_p(g.bias), C.c_void_p(g.resid), C.c_void_p(g.C), sp.M, sp.N, sp.K, sp.epi, 0,
                                       _stream())
        torch.cuda.synchronize()
        assert rc == R.OK, (sp.name, rc)
        got, intact = L.output()
        assert intact and np.array_equal(got.view(np.uint32), keep[sp.name].view(np.uint32)), f"{sp.name}: product and probe library differ"


@pytest.mark.parametrize("B", [16, 32])
def test_product_decode_step_runs_the_fused_reduce_with_the_probe_builds_bits(probes, B):
    """reduce_ln_wg_kernel is reached by the product only inside a decode step (out_proj and fc2 of an OPT block: K split, + residual, the next
    LayerNorm in the same launch).  (a) The two launches as the step makes them — M = B rows, 2560 x 2560 and 2560 x 10240, dense strides, the
    step's 16 MiB scratch, residual, ln_out — take the fused reduce in the probe build (form bit, asserted against the mirror) and pass every
    check of run_case.  (b) One eilev_opt_decode_step at OPT-2.7B widths (one block) through the PRODUCT library and through the probe library,
    same weights, prefilled cache and workspace contents: identical fp32 logits, ids and cache."""
    from eilev_amd import abi
    from hip_utils import P, models, stream_ptr

    global _product
    if _product is None:
        _product = abi.load_library(abi.HIP_LIB_PATH)
    n_cu = _num_cu()
    cfg, _, eng = models("real_1l")
    d = eng.dims
    D, F = d.t_hidden, d.t_ffn
    for name, k in (("out_proj", D), ("fc2", F)):
        sp = SSpec(f"step-{name}-{B}x{D}x{k}", B, D, k, family="exact", pad=False, resid=True, ln_out=1, scratch=16 << 20)
        rc, form, ks, _ = S.plan(sp, n_cu)
        assert rc == R.OK and form & S.SPLIT_K and form & S.REDUCE_LN and ks >= 2, (sp.name, S.form_name(form))
        run_case(probes, sp, n_cu)
    rng = np.random.default_rng(17)
    L, cap = 40, 44
    ids = torch.from_numpy(rng.integers(4, 50000, size=(B, L + 1)).astype(np.int64)).cuda()
    am = torch.ones((B, L), dtype=torch.int32, device="cuda")
    am[1, :7] = 0
    emb = eng.embed_scatter(ids, None, None)
    kv0 = eng.new_kv_cache(B, cap)
    eng.prefill(emb[:, :L].contiguous(), am, kv_cache=kv0, kv_capacity=cap)
    n_valid = am.sum(dim=1).to(torch.int32).contiguous()
    nbytes = max(int(lib.eilev_opt_workspace_bytes(C.byref(d), B, 1)) for lib in (_product, probes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = []
    for lib in (_product, probes):
        kv = kv0.clone()
        state = torch.tensor([1, B], dtype=torch.int32, device="cuda")
        tokens = ids[:, L].contiguous()
        finished = torch.zeros(B, dtype=torch.uint8, device="cuda")
        out = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        logits = torch.empty((B, d.vocab), dtype=torch.float32, device="cuda")
        ws.fill_(0x7f)
        rc = lib.eilev_opt_decode_step(C.byref(d), C.byref(eng.pack.opt), P(tokens), P(state), P(am), P(n_valid), B, L, P(kv), cap, P(logits),
                                       P(finished), -1, 1, P(out), 4, P(ws), ws.numel(), stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        res.append((logits.cpu().numpy(), out[:, 1].cpu().numpy(), kv))
    assert np.isfinite(res[0][0]).all()
    assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32)), "product and probe decode step: logits differ"
    assert np.array_equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
