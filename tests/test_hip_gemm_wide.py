"""Every wide (M > 32) GEMM kernel of csrc/gemm.hip, gemm_tiled.h, gemm_pp4.h, gemm_pp4_ext.hip and gemm_w6.h, launched on its own through the probe
entry eilev_debug_gemm (one launch_gemm on explicit arguments; it reports the kernel instance that was launched) and compared with the float64
reference of tests/gemm_ref.py.

Why this is tighter than test_hip_kernels.py::_lin_case (max|err| <= 1e-2 max|ref| on dense operands through eilev_linear): there a wrong bias
column, a residual row of the neighbouring tile, a scale_cols boundary one block off or a statistics slot past N sit inside the bound or outside
what is inspected, strides are always K / N, and the kernel that ran is a comment.  Here every launch is judged on four counts: the return code;
form == gemm_ref.expected (a Python mirror of the dispatch, so a retuned threshold moves the case list with it or fails the assertion); every
output element within gemm_ref.tol (derived from the arithmetic, no floor, no max|ref| term) and BIT FOR BIT on the exact family (integer
operands: every partial sum is exact in fp32 in any order, split-K atomics included; +-0 are one value); and every word of C, stat_out,
ln_out and the fp8 scratch outside the defined output still holding its NaN sentinel, with +-2^14 traps in the padding columns and rows of the
operands.  What each planted mistake costs against these checks is measured on the CPU by test_gemm_reference.py.

form (gemm_ref.family_of)        route (gemm_ref.route_specs; each boundary from both sides where the shape stays small)
nt-<tile>                        DBG_GEMM_NO_DMA + force 1-4: (300, 200, 72), (257, 528, 176), (520, 1536, 128), the half column tile, fp32 output
glds-<tile>, glds-64x128         force 1-4 / 13 and natural: the same with K % 64 == 0, scale_cols, DBG_GEMM_NO_HALF_TILES; M = 65, 64 + 128 n (+ 1);
                                 t64x128_takes at 94 / 96 tiles and M = 64 / 65
splitk                           natural (K >= 8192, 1 / 2 / ragged tiles, 15 and 16 slices with nk / slices not whole) and force 15; a bias and
                                 K = 8128 stay off it
pp4-general                      FORCE_PP4: (520, 640, 128), (1000, 1408, 256) GELU + residual, N % 128 != 0, one K-step, fp32, scale_cols, wscale, patch
pp4-lean16ht, pp4-a3             dbg == 0, natural, the smallest row counts the dispatch sends there on this device (gemm_ref.smallest_m): plain, ReLU +
                                 residual, an M tail, scale_cols = 16 and N / 3, N = 2176 (half tile), K = 5120 (A3) and 5056 (not); exact family, whose
                                 float32 BLAS reference is exact, and one bounded case
w6                               FORCE_W6: K = 256 / 320, N = 128 .. 1408, M tails 1 / 37 / 255, residual with epi 0; residual + ReLU and K = 192 are
                                 rerouted to a per-tile kernel (asserted); natural at N = 2048
pp4-lnfold-lean16 / -general     ln_rows (natural): N % 128 == 0 / != 0, x GELU; a large row mean and an outlier channel; the head-major q|k|v scatter
                                 (hm_tok 257 x hd 88 and 129 x 72) element by element against the layout of common.h
pp4-stats-lean16ht / -general    stat_out: N = 1408 (22 slots, half tile), 192, 1280, 200 (tail slot); slots past N and rows past M stay poisoned
pp4-f8                           A8: K = 128 / 256 / 384, tails, epi 0 / 2, bf16 / fp32, exact family with power-of-two scales
+w8x                             W8 with M > 32: the scratch equals the e4m3 decode, the result equals the bf16 launch on it bit for bit
ln_out                           LayerNorm / RMSNorm rows after a wide GEMM against the reference on the bf16 rows of C the device wrote

Measured on the device (profiles/parity_r06.json, section gemm_wide: worst err / tol per form, the first failing index if any, the wall time, and
the GELU polynomial errors measured on the CPU): bit equality on the exact family for every form; on the bounded family 0.988 .. 0.9995 for every
bf16 form (a result that rounds from just short of a tie sits at the half unit: the bound cannot be tighter), 3e-5 for split-K (fp32 output),
0.03 for stat_out, 0.9999 for ln_out.  The (K + 8) 2^-24 constant was NOT widened (ACC_C = 1).  One term was added to the derivation: the split
rank-1 term of the folded LayerNorm (gemm_ref's docstring; without it one element of 1.3 M reached 1.05 at K = 64).  The whole file: 5 s."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import Spec

pytestmark = pytest.mark.gpu


class GemmArgs(C.Structure):
    """ctypes mirror of EilevDebugGemmArgs (csrc/gemm.hip, probe build): GemmArgs without dbg, trace, trace_tiles and k_slice."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("W", C.c_void_p), ("ldw", C.c_int64),
                ("bias", C.c_void_p), ("resid", C.c_void_p), ("ldr", C.c_int64), ("C", C.c_void_p), ("ldc", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epi", C.c_int32), ("out_f32", C.c_int32),
                ("scale", C.c_float), ("scale_cols", C.c_int32), ("patch_group", C.c_int32),
                ("hm_tok", C.c_int32), ("hm_heads", C.c_int32), ("hm_hd", C.c_int32), ("pad0", C.c_int32),
                ("wscale", C.c_void_p), ("W8", C.c_void_p), ("w8_scratch", C.c_void_p), ("A8", C.c_void_p),
                ("ascale", C.c_void_p), ("ln_rows", C.c_void_p), ("ln_csum", C.c_void_p),
                ("stat_out", C.c_void_p), ("stat_ld", C.c_int64),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out", C.c_void_p), ("ln_eps", C.c_float), ("pad1", C.c_int32)]


SENT32 = (R.SENT16 << 16) | R.SENT16
_WORST: dict = {}
_FIRST_FAIL: dict = {}
_SECONDS: dict = {}
_case_cache: dict = {}


def _entry(lib):
    fn = lib.eilev_debug_gemm
    fn.argtypes = [C.POINTER(GemmArgs), C.c_size_t, C.POINTER(C.c_int), C.c_void_p]
    fn.restype = C.c_int
    return fn


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(sp):
    """(case, y, S) built once per spec and left unchanged."""
    got = _case_cache.get(sp.name)
    if got is None:
        c = R.build_case(sp)
        y, S, _ = R.reference(c)
        got = (c, y, S)
        if sp.M * sp.N <= 1 << 20:
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


class Launch:
    """The device buffers of one case, every output poisoned; launch() runs the probe entry under the spec's switch value."""

    def __init__(self, c):
        sp = self.sp = c.spec
        self.c = c
        a = self.args = GemmArgs()
        k = self.keep = {}
        if sp.a8:
            k["A"] = _dev(c.A8)
            a.A8 = k["A"].data_ptr()
        else:
            k["A"] = _dev_bf16(c.A_buf)
            a.A = k["A"].data_ptr()
        if sp.a8 or sp.w8:
            k["W"] = _dev(c.W8)
            a.W8 = k["W"].data_ptr()
        else:
            k["W"] = _dev_bf16(c.W_buf)
            a.W = k["W"].data_ptr()
        a.lda, a.ldw, a.ldr, a.ldc = c.lda, c.ldw, c.ldr, c.ldc
        if c.bias is not None:
            k["bias"] = _dev_bf16(c.bias)
            a.bias = k["bias"].data_ptr()
        if c.resid_buf is not None:
            k["resid"] = _dev_bf16(c.resid_buf)
            a.resid = k["resid"].data_ptr()
        self.words = R.c_words(c)
        self.out = _poison32(self.words) if sp.out_f32 else _poison16(self.words)
        a.C = self.out.data_ptr()
        a.M, a.N, a.K, a.epi, a.out_f32 = sp.M, sp.N, sp.K, sp.epi, int(sp.out_f32)
        a.scale, a.scale_cols, a.patch_group = float(sp.scale), sp.scale_cols, sp.patch_group
        if sp.hm:
            a.hm_tok, a.hm_heads, a.hm_hd = sp.hm
        for name in ("wscale", "ascale", "ln_rows", "ln_csum"):
            v = getattr(c, name)
            if v is not None:
                k[name] = _dev(v.astype(np.float32))
                setattr(a, name, k[name].data_ptr())
        self.scratch = None
        if sp.w8:
            self.scratch = _poison16((sp.N + 2) * sp.K)
            a.w8_scratch = self.scratch.data_ptr()
        self.stat = None
        if sp.stats:
            self.stat = _poison32(c.stat_slots * c.stat_ld * 2)
            a.stat_out, a.stat_ld = self.stat.data_ptr(), c.stat_ld
        self.ln = None
        if sp.ln_out:
            self.ln = _poison16((sp.M + 2) * sp.N)
            k["gamma"] = _dev_bf16(c.gamma)
            a.ln_gamma, a.ln_out, a.ln_eps = k["gamma"].data_ptr(), self.ln.data_ptr(), c.ln_eps
            if c.beta is not None:
                k["beta"] = _dev_bf16(c.beta)
                a.ln_beta = k["beta"].data_ptr()
        self.form = C.c_int(-1)

    def launch(self, lib, struct_bytes=None):
        try:
            lib.eilev_debug_gemm_flags(self.sp.flags)
            rc = _entry(lib)(C.byref(self.args), C.sizeof(GemmArgs) if struct_bytes is None else struct_bytes, C.byref(self.form),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
        finally:
            lib.eilev_debug_gemm_flags(0)
        torch.cuda.synchronize()
        return rc

    def output(self):
        """(values at the logical [M, N] positions as float64 (fp32 output) / float32 of bf16, True iff every other word holds the sentinel)."""
        sp, c = self.sp, self.c
        raw = self.out.cpu().numpy()
        if sp.out_f32:
            vals, sent = raw.view(np.float32), raw.view(np.uint32) == SENT32
        else:
            vals, sent = R.bits_to_f32(raw.view(np.uint16)), raw.view(np.uint16) == R.SENT16
        if sp.hm:
            idx = R.out_index(c)
            written = np.zeros(self.words, bool)
            written[idx.ravel()] = True
            return vals[idx], bool(sent[~written].all())
        v2, s2 = vals.reshape(-1, c.ldc), sent.reshape(-1, c.ldc).copy()
        rows = np.arange(sp.M)
        orow = rows + rows // sp.patch_group + 1 if sp.patch_group else rows
        got = v2[orow, :sp.N]
        s2[orow, :sp.N] = True
        return got, bool(s2.all())

    def untouched(self):
        raw = self.out.cpu().numpy()
        ok = (raw.view(np.uint32) == SENT32).all() if self.sp.out_f32 else (raw.view(np.uint16) == R.SENT16).all()
        for t in (self.stat, self.ln, self.scratch):
            if t is not None:
                r = t.cpu().numpy()
                ok = ok and ((r.view(np.uint32) == SENT32).all() if r.dtype == np.int32 else (r.view(np.uint16) == R.SENT16).all())
        return bool(ok)


def _note(fam, name, ratio, where=None):
    _WORST[fam] = max(_WORST.get(fam, 0.0), float(ratio))
    if where is not None and fam not in _FIRST_FAIL:
        _FIRST_FAIL[fam] = f"{name} {where}"


def _same_bits(got, ref32):
    """Equal as numbers and no NaN: +0 and -0 are one value (an accumulator that starts from -0 is not a mistake)."""
    return (got == ref32) & ~np.isnan(got)


def run_case(lib, sp, n_cu, keep=None):
    """One launch, every check."""
    c, y, S = _case(sp)
    want_rc, want_form = R.expected(sp, n_cu)
    assert want_rc == R.OK, sp.name
    L = Launch(c)
    rc = L.launch(lib)
    assert rc == R.OK, (sp.name, rc)
    assert L.form.value == want_form, f"{sp.name}: launched {R.form_name(L.form.value)}, the dispatch mirror says {R.form_name(want_form)}"
    fam = R.family_of(want_form)
    got, intact = L.output()
    assert intact, f"{sp.name} ({fam}): a write outside the rows and columns of the output"
    if sp.family == "exact":
        ref32 = y.astype(np.float32)
        same = _same_bits(got, ref32)
        if not same.all():
            i, j = np.argwhere(~same)[0]
            _note(fam, sp.name, np.inf, f"[{i}, {j}]")
            pytest.fail(f"{sp.name} ({fam}): {int((~same).sum())} of {same.size} elements differ on the exact family, first at [{i}, {j}]: "
                        f"got {got[i, j]}, ref {ref32[i, j]}")
        _note(fam + "/exact", sp.name, 0.0)
    else:
        t = R.tol(c, y, S, want_form)
        rt = R.ratio(np.abs(got.astype(np.float64) - y), t)
        worst = float(rt.max())
        print(f"{sp.name}: {R.form_name(want_form)} err/tol {worst:.3f}")
        if not worst <= 1.0:
            i, j = np.unravel_index(np.argmax(rt), rt.shape)
            _note(fam, sp.name, worst, f"[{i}, {j}]")
            pytest.fail(f"{sp.name} ({fam}): err/tol {worst:.3g} at [{i}, {j}] (got {got[i, j]}, ref {y[i, j]}, tol {t[i, j]:.3g}); "
                        f"{int((rt > 1).sum())} of {rt.size} elements beyond tol")
        _note(fam, sp.name, worst)
    if sp.stats:
        _check_stats(L, c, y, S, fam)
    if sp.ln_out:
        _check_ln_out(L, c, got, fam)
    if sp.w8:
        _check_w8(lib, L, c, got, want_form, n_cu)
    if keep is not None:
        keep[sp.name] = got


def _check_stats(L, c, y, S, fam):
    sp = c.spec
    raw = L.stat.cpu().numpy().reshape(c.stat_slots, c.stat_ld, 2)
    sent = raw.view(np.uint32) == SENT32
    slots = (sp.N + 63) // 64
    assert sent[slots:].all() and sent[:, sp.M:].all(), f"{sp.name}: a statistics slot at or past N, or a row past M, was written"
    got = raw.view(np.float32)[:slots, :sp.M].astype(np.float64)
    ref, t = R.stat_ref(c, y, S)
    if sp.family == "exact":
        assert np.array_equal(got, ref.astype(np.float32).astype(np.float64)), f"{sp.name}: statistics differ on the exact family"
        return
    rt = R.ratio(np.abs(got - ref), t)
    worst = float(rt.max())
    print(f"{sp.name}: stat_out err/tol {worst:.3f}")
    s, i, k = np.unravel_index(np.argmax(rt), rt.shape)
    _note("stat_out", sp.name, worst, None if worst <= 1 else f"slot {s} row {i} [{k}]")
    assert worst <= 1.0, f"{sp.name}: stat_out err/tol {worst:.3g} at slot {s} row {i} [{k}]: got {got[s, i, k]}, ref {ref[s, i, k]}"


def _check_ln_out(L, c, got_c, fam):
    sp = c.spec
    raw = L.ln.cpu().numpy().view(np.uint16).reshape(sp.M + 2, sp.N)
    assert (raw[sp.M:] == R.SENT16).all(), f"{sp.name}: ln_out rows past M were written"
    got = R.bits_to_f32(raw[:sp.M]).astype(np.float64)
    ref, t = R.ln_out_ref(c, got_c)
    rt = R.ratio(np.abs(got - ref), t)
    worst = float(rt.max())
    print(f"{sp.name}: ln_out err/tol {worst:.3f}")
    i, j = np.unravel_index(np.argmax(rt), rt.shape)
    _note("ln_out", sp.name, worst, None if worst <= 1 else f"[{i}, {j}]")
    assert worst <= 1.0, f"{sp.name}: ln_out err/tol {worst:.3g} at [{i}, {j}]: got {got[i, j]}, ref {ref[i, j]}"


def _check_w8(lib, L, c, got, form, n_cu):
    """The scratch holds the e4m3 decode exactly (and nothing behind it); the bf16 launch on the scratch gives the same bits."""
    sp = c.spec
    assert form & R.W8_EXPANDED
    raw = L.scratch.cpu().numpy().view(np.uint16).reshape(sp.N + 2, sp.K)
    assert (raw[sp.N:] == R.SENT16).all(), f"{sp.name}: the expansion wrote past N rows"
    assert np.array_equal(raw[:sp.N], R.bf16_bits(c.W_buf[:sp.N])), f"{sp.name}: the scratch is not the e4m3 decode"
    L2 = Launch(c)
    L2.args.W8, L2.args.w8_scratch, L2.args.W, L2.args.ldw = None, None, L.scratch.data_ptr(), sp.K
    assert L2.launch(lib) == R.OK and L2.form.value == form & ~R.W8_EXPANDED, (sp.name, R.form_name(L2.form.value))
    got2, intact = L2.output()
    assert intact and np.array_equal(got2.view(np.uint32), got.view(np.uint32)), f"{sp.name}: the bf16 launch on the expanded weights differs"


def _record():
    from hip_utils import record_parity

    record_parity("gemm_wide",
                  tol="half a unit of the output format at y + (K + 8) 2^-24 S_ij (x 1.13 for GELU) + the GELU polynomial's measured error; "
                      "exact family: equality; ACC_C = %g" % R.ACC_C,
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()}, **{f"first_failing_{k}": v for k, v in _FIRST_FAIL.items()},
                  **{f"gelu_max_abs_err_{k}": v for k, v in R.gelu_forms().items()},
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


@pytest.mark.parametrize("cfg", [1, 2, 3, 4], ids=["256x256", "256x128", "256x128-1stage", "128x128"])
def test_per_tile_kernels(probes, cfg):
    """gemm_nt_kernel (NO_DMA, K % 64 != 0 too) and gemm_glds_kernel in one tile configuration: tails in M, N and K, the half column tile with
    and without its path, every epilogue, bias on and off, residual, fp32 output, scale_cols."""
    _run_all(probes, [sp for sp in R.tiled_specs() if sp.name.startswith((f"nt{cfg}-", f"glds{cfg}-"))], f"tiled-{cfg}")


def test_64x128_kernel_and_its_predicate(probes):
    _run_all(probes, [sp for sp in R.tiled_specs() if sp.name.startswith(("glds64-", "t64-"))], "tiled-64x128")


def test_split_k_is_bit_exact_and_leaves_the_padding_alone(probes):
    """Atomics over 15 / 16 slices: bit equality on the exact family; C has ldc > N, so the zero-fill must cover the M x N output only."""
    _run_all(probes, R.split_k_specs(), "splitk")


def test_pp4_general_epilogue(probes):
    _run_all(probes, R.pp4_general_specs(), "pp4-general")


@pytest.mark.parametrize("which", range(11))
def test_pp4_lean_and_a3_at_dbg_0(probes, which):
    """The product's 16 x 16 instances, reached without any probe flag (asserted by the form)."""
    specs = R.lean_specs(_num_cu())
    assert len(specs) == 11 and all(sp.flags == 0 for sp in specs)
    _run_all(probes, specs[which:which + 1], "pp4-lean")


def test_w6_kernel_and_what_it_refuses(probes):
    _run_all(probes, R.w6_specs(_num_cu()), "w6")


def test_folded_layernorm_and_head_major_scatter(probes):
    _run_all(probes, R.lnfold_specs(_num_cu()), "lnfold")


def test_statistics_producers(probes):
    _run_all(probes, R.stats_specs(_num_cu()), "stats")


def test_fp8_mfma_instances(probes):
    _run_all(probes, R.a8_specs(), "a8w8")


def test_fp8_weights_expanded_for_wide_launches(probes):
    _run_all(probes, R.w8_specs(), "w8")


def test_patch_embedding_row_remap(probes):
    """patch_group 256 and 16, 1 and 3 frames: the CLS rows keep the sentinel, the residual is the position table row 1 + row % group."""
    _run_all(probes, R.patch_specs(), "patch")


def test_ln_out_after_a_wide_gemm(probes):
    _run_all(probes, R.ln_out_specs(), "ln_out")


def test_every_form_of_the_table_was_reached_by_name(probes):
    """(Runs last in file order.)  The forms recorded by the tests above cover gemm_ref.REQUIRED; without them this test launches one case each."""
    n_cu = _num_cu()
    seen = {k.split("/")[0] for k in _WORST}
    for fam in R.REQUIRED:
        if fam not in seen:
            sp = next(sp for sp in R.route_specs(n_cu) if R.family_of(R.expected(sp, n_cu)[1]) == fam)
            _run_all(probes, [sp], "coverage")
    assert not [f for f in R.REQUIRED if f not in {k.split("/")[0] for k in _WORST}]


def test_refusals_launch_nothing(probes):
    """Each EILEV_E_UNSUPPORTED / EILEV_E_BADARG / EILEV_E_WORKSPACE branch of check_args, launch_a8w8, w8_check, hm_takes and launch_pp4_ext: the
    code comes back, no form is reported and every output buffer keeps its sentinel."""
    n_cu = _num_cu()

    def call(sp, struct_bytes=None, want=None, **fields):
        c = _case(sp)[0]
        L = Launch(c)
        for k, v in fields.items():
            setattr(L.args, k, v)
        rc = L.launch(probes, struct_bytes)
        assert L.untouched(), (sp.name, fields)
        assert L.form.value in (0, -1), (sp.name, fields, L.form.value)
        if want is not None:
            assert rc == want, (sp.name, fields, rc, want)
        return rc

    base = Spec("refuse", 70, 136, 64, resid=True, stats=False)
    assert C.sizeof(GemmArgs) == 224
    call(base, struct_bytes=216, want=R.E_BADARG)
    call(base, struct_bytes=232, want=R.E_BADARG)
    # check_args
    for f in (dict(A=None), dict(W=None), dict(C=None), dict(N=0), dict(K=0)):
        call(base, want=R.E_BADARG, **f)
    for f in (dict(K=60), dict(lda=76), dict(ldw=84), dict(ldc=140), dict(N=134), dict(ldr=156), dict(hm_tok=70, hm_heads=1, hm_hd=72)):
        call(base, want=R.E_UNSUPPORTED, **f)
    c = _case(base)[0]
    L = Launch(c)
    call(base, want=R.E_UNSUPPORTED, A=L.keep["A"].data_ptr() + 2)
    call(base, want=R.E_UNSUPPORTED, bias=L.keep["bias"].data_ptr() + 2)
    assert call(base, M=0) == R.OK
    # ln_fold launches: fp32, scale_cols, patch, wscale, K % 64; launch_pp4_ext: ReLU, a residual with ln_rows, statistics without one
    lnf = Spec("refuse-lnf", 70, 128, 64, lnfold=True)
    for f in (dict(out_f32=1), dict(scale_cols=16), dict(patch_group=10), dict(K=56), dict(epi=2), dict(ln_csum=None)):
        call(lnf, want=R.E_UNSUPPORTED, **f)
    rl = Launch(_case(base)[0])
    call(lnf, want=R.E_UNSUPPORTED, resid=rl.keep["resid"].data_ptr(), ldr=rl.c.ldr)
    st = Spec("refuse-st", 70, 128, 64, stats=True, resid=True)
    for f in (dict(resid=None), dict(epi=1), dict(stat_ld=69)):
        call(st, want=R.E_UNSUPPORTED, **f)
    # hm_takes: tokens per frame below a wave's 128 rows, a head size of 64, N that is not 3 heads hd, M that is no whole number of frames
    hm = Spec("refuse-hm", 258, 3 * 16 * 72, 64, lnfold=True, hm=(129, 16, 72))
    assert R.expected(hm, n_cu)[0] == R.OK
    for f in (dict(hm_tok=86), dict(hm_hd=64), dict(hm_heads=8), dict(M=200), dict(epi=1), dict(ln_rows=None)):
        call(hm, want=R.E_UNSUPPORTED, **f)
    # launch_a8w8
    a8 = Spec("refuse-a8", 70, 128, 128, a8=True, resid=True)
    for f in (dict(W8=None), dict(wscale=None), dict(ascale=None), dict(C=None)):
        call(a8, want=R.E_BADARG, **f)
    for f in (dict(K=64), dict(lda=136), dict(ldw=136), dict(patch_group=10), dict(ldc=132), dict(epi=1), dict(hm_tok=35, hm_heads=1, hm_hd=72)):
        call(a8, want=R.E_UNSUPPORTED, **f)
    # w8_check
    w8 = Spec("refuse-w8", 70, 136, 64, w8=True, family="bounded")
    for f in (dict(wscale=None), dict(ldw=72), dict(K=56), dict(A=None)):
        call(w8, want=R.E_BADARG, **f)
    call(w8, want=R.E_WORKSPACE, w8_scratch=None)
    # ln_out after a launch that cannot have one
    lo = Spec("refuse-lnout", 70, 136, 64, ln_out=1, family="bounded", out_f32=True)
    c = _case(lo)[0]
    L = Launch(c)
    assert L.launch(probes) == R.E_UNSUPPORTED and (L.ln.cpu().numpy().view(np.uint16) == R.SENT16).all()


_product = None


def test_product_library_gives_the_same_bits(probes):
    """The public eilev_linear of the PRODUCT library (dense strides: what it can express) on one lean, one w6 and one per-tile shape: bit-identical
    to the probe library's launch of the same operands, and the product exports no probe entry."""
    from eilev_amd import abi

    global _product
    if _product is None:
        _product = abi.load_library(abi.HIP_LIB_PATH)
    assert not hasattr(_product, "eilev_debug_gemm")
    n_cu = _num_cu()
    lean = next(sp for sp in R.lean_specs(n_cu) if sp.name.startswith("lean-relu-resid"))
    w6 = next(sp for sp in R.w6_specs(n_cu) if sp.name.startswith("w6-natural"))
    for sp in (R.replace(lean, pad=False, name="product-lean"), R.replace(w6, pad=False, name="product-w6"),
               Spec("product-tiled", 300, 200, 72, epi=1, resid=True, family="bounded", pad=False)):
        keep = {}
        run_case(probes, sp, n_cu, keep)
        c = _case(sp)[0]
        L = Launch(c)
        a = L.args
        rc = _product.eilev_linear(C.c_void_p(a.A), C.c_void_p(a.W), C.c_void_p(a.bias), C.c_void_p(a.resid), C.c_void_p(a.C), sp.M, sp.N, sp.K, sp.epi, 0,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == R.OK, (sp.name, rc)
        got, intact = L.output()
        assert intact and np.array_equal(got.view(np.uint32), keep[sp.name].view(np.uint32)), f"{sp.name}: product and probe library differ"
