"""Every M <= 8 row-dot decode kernel of csrc/gemv.hip (gemv_rows_kernel, gemv1_kernel, gemvm_kernel x the plain, LayerNorm and merge
prologues), launched on its own through the probe entry eilev_debug_gemv (ONE call of launch_gemv_rows / launch_gemv1 / launch_gemvm on
explicit arguments; it reports the kernel instance) and compared with the float64 reference of tests/gemv_ref.py under its per-element bound.

Every launch is judged as in test_hip_gemm_skinny.py: the return code and the instance equal gemv_ref.expected (a Python mirror of the three
launchers); every output element within tol (derived, no floor, no max|ref| term) and BIT FOR BIT on the exact family (+-0 are one value);
every word outside the defined output untouched — the ldo padding and the two guard rows on their NaN sentinel, or, with the residual in
place (out IS the residual buffer, as in every product call), on the residual's +-2^14 traps.  The operands carry traps in their padding and
in the two rows after the last; the o words of empty merge ranges hold NaN bits.

template          route (gemv_ref.route_specs)
gemv_rows_kernel  PRO_X M = 1..8 x K = 512 / 1024 / 2560 / 4096 / 5120 (CPS 1, 1 x 2, 5, 8, 5 x 2); N = 1001 (ragged), 6 (three waves out of
                  range), 4100 (3 rows per wave); fp32 / bf16, ReLU, own and in-place residual, scale 2^-3 on 0, 1, N / 3, N columns;
                  PRO_LN M = 1, 4, 5, 8 x K = 512 / 2560 / 4096; PRO_MERGE M = 1, 2 x 32 x 80 / 8 x 64 heads x nsplit 1, 3, 8, dead rows
gemv1_kernel      grid override 8 (40 waves): PRO_X K = 2560 N = 12 (clamped grid, zero-row waves), 126, 640 (2 RB), 702, 930 (tails),
                  2650 (the 64-row flush); K = 4096 and 10240 short and long; PRO_LN short, 2 RB, tails, fp32, q scaling; PRO_MERGE nsplit
                  1, 2, 5, 8, N = 12, a long N, a dead row; one natural-grid case per prologue at N = 2560
gemvm_kernel      the same grid: M = 2..8 x PRO_X / PRO_LN at N = 40 * 2 RB - 2 (short form, waves of 2 RB rows), 40 * 2 RB (LONG), + 22
                  (uneven), N = 12 (clamped), 126
refusals          PRO_LN K = 4608, PRO_MERGE M = 3, M = 8 x K = 10240 (LDS), nsplit = 9, gemvm K = 5120, odd N with a bias or a residual
                  (launch_gemv1 / launch_gemvm fetch them as 32-bit pairs): the code, instance 0, every word intact
row independence  row 0 of an M-row launch equals the one-row launch bit for bit (gemvm_kernel against gemv1_kernel, gemv_rows_kernel
                  against itself)

Measured on the device: profiles/parity_r06.json, section gemv."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gemm_ref as R
import gemv_ref as V

pytestmark = pytest.mark.gpu


class GemvArgs(C.Structure):
    """ctypes mirror of EilevDebugGemvArgs (csrc/gemv.hip, probe build)."""
    _fields_ = [("pro", C.c_int32), ("pad0", C.c_int32), ("x", C.c_void_p), ("ldx", C.c_int64), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("eps", C.c_float), ("pad1", C.c_int32), ("part", C.c_void_p), ("heads", C.c_int32), ("hd", C.c_int32), ("nsplit", C.c_int32),
                ("pad2", C.c_int32), ("W", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p), ("ldr", C.c_int64), ("out", C.c_void_p),
                ("ldo", C.c_int64), ("out_f32", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epi", C.c_int32),
                ("scale", C.c_float), ("scale_cols", C.c_int32), ("pad3", C.c_int32)]


_WORST: dict = {}
_FIRST_FAIL: dict = {}
_SECONDS: dict = {}
_SEEN: set = set()
_case_cache: dict = {}


def _entry(lib):
    fn = lib.eilev_debug_gemv
    fn.argtypes = [C.POINTER(GemvArgs), C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    fn.restype = C.c_int
    return fn


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case(sp):
    got = _case_cache.get(sp.name)
    if got is None:
        c = V.build_case(sp)
        got = (c,) + V.reference(c)
        if sp.N * sp.K <= 1 << 21:
            _case_cache[sp.name] = got
    return got


def _dev_bf16(x):
    return torch.from_numpy(R.bf16_bits(x).view(np.int16)).cuda()


def _dev_bits32(x):
    """float32 to the device by its bits (NaN payloads survive)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32).view(np.int32)).cuda()


class Launch:
    """The device buffers of one case; out poisoned, or holding the residual when it is in place."""

    def __init__(self, lib, c):
        sp = self.sp = c.spec
        self.c, self.lib = c, lib
        a = self.args = GemvArgs()
        k = self.keep = {}
        M, N, K = sp.M, sp.N, sp.K
        a.pro = sp.pro
        if c.x_buf is not None:
            k["x"] = _dev_bf16(c.x_buf)
            a.x = k["x"].data_ptr()
        a.ldx, a.ldr, a.ldo = c.ldx, c.ldr, c.ldo
        if c.gamma is not None:
            k["gamma"], k["beta"] = _dev_bf16(c.gamma), _dev_bf16(c.beta)
            a.gamma, a.beta = k["gamma"].data_ptr(), k["beta"].data_ptr()
        a.eps = c.eps
        if c.part is not None:
            k["part"] = _dev_bits32(c.part)
            a.part, a.heads, a.hd, a.nsplit = k["part"].data_ptr(), sp.heads, sp.hd, sp.nsplit
        k["W"] = _dev_bf16(c.W_buf)
        a.W = k["W"].data_ptr()
        if c.bias is not None:
            k["bias"] = _dev_bf16(c.bias)
            a.bias = k["bias"].data_ptr()
        words = (M + 2) * c.ldo
        if sp.resid == 2:
            self.before = R.bf16_bits(c.resid_buf).ravel()
            assert self.before.size == words
        elif sp.out_f32:
            self.before = np.full(words, V.SENT32, np.uint32)
        else:
            self.before = np.full(words, R.SENT16, np.uint16)
        self.out = torch.from_numpy(self.before.view(np.int32 if sp.out_f32 else np.int16).copy()).cuda()
        a.out = self.out.data_ptr()
        if sp.resid == 1:
            k["resid"] = _dev_bf16(c.resid_buf)
            a.resid = k["resid"].data_ptr()
        elif sp.resid == 2:
            a.resid = a.out
        a.out_f32, a.M, a.N, a.K, a.epi = int(sp.out_f32), M, N, K, sp.epi
        a.scale, a.scale_cols = float(sp.scale), sp.scale_cols
        self.instance = C.c_int(-1)

    def launch(self, struct_bytes=None, launcher=None):
        lib = self.lib
        try:
            lib.eilev_debug_grid_cus(self.sp.grid)
            rc = _entry(lib)(C.byref(self.args), C.sizeof(GemvArgs) if struct_bytes is None else struct_bytes,
                             self.sp.launcher if launcher is None else launcher, C.byref(self.instance), _stream())
        finally:
            lib.eilev_debug_grid_cus(0)
        torch.cuda.synchronize()
        return rc

    def raw(self):
        r = self.out.cpu().numpy()
        return r.view(np.uint32) if self.sp.out_f32 else r.view(np.uint16)

    def output(self):
        """(values at the logical [M, N] positions, True iff every other word of out holds what it held before the launch)."""
        sp, c = self.sp, self.c
        raw = self.raw()
        vals = raw.view(np.float32) if sp.out_f32 else R.bits_to_f32(raw)
        idx = (np.arange(sp.M)[:, None] * c.ldo + np.arange(sp.N)[None, :])
        same = raw == self.before
        same[idx.ravel()] = True
        return vals[idx], bool(same.all())

    def untouched(self):
        return bool((self.raw() == self.before).all())


def _note(fam, name, ratio, where=None):
    _WORST[fam] = max(_WORST.get(fam, 0.0), float(ratio))
    if where is not None and fam not in _FIRST_FAIL:
        _FIRST_FAIL[fam] = f"{name} {where}"


def _same_bits(got, ref32):
    return (got == ref32) & ~np.isnan(got)


def run_case(lib, sp, n_cu, keep=None):
    c, y, Sm, Dm = _case(sp)
    want_rc, want_inst = V.expected(sp, n_cu)
    assert want_rc == R.OK, sp.name
    L = Launch(lib, c)
    rc = L.launch()
    assert rc == want_rc, (sp.name, rc)
    assert L.instance.value == want_inst, f"{sp.name}: launched {V.instance_name(L.instance.value)}, the mirror says {V.instance_name(want_inst)}"
    fams = V.families(sp, n_cu)
    got, intact = L.output()
    assert intact, f"{sp.name} ({fams[0]}): a write outside the rows and columns of the output"
    if sp.family == "exact":
        ref32 = y.astype(np.float32)
        same = _same_bits(got, ref32)
        if not same.all():
            i, j = np.argwhere(~same)[0]
            for f in fams:
                _note(f + "/exact", sp.name, np.inf, f"[{i}, {j}]")
            pytest.fail(f"{sp.name} ({fams[0]}): {int((~same).sum())} of {same.size} elements differ on the exact family, first at [{i}, {j}]: "
                        f"got {got[i, j]}, ref {ref32[i, j]}")
        for f in fams:
            _note(f + "/exact", sp.name, 0.0)
    else:
        t = V.tol(c, y, Sm, Dm)
        rt = R.ratio(np.abs(got.astype(np.float64) - y), t)
        worst = float(rt.max())
        print(f"{sp.name}: {fams[0]} err/tol {worst:.3f}")
        if not worst <= 1.0:
            i, j = np.unravel_index(np.argmax(rt), rt.shape)
            for f in fams:
                _note(f, sp.name, worst, f"[{i}, {j}]")
            pytest.fail(f"{sp.name} ({fams[0]}): err/tol {worst:.3g} at [{i}, {j}] (got {got[i, j]}, ref {y[i, j]}, tol {t[i, j]:.3g}); "
                        f"{int((rt > 1).sum())} of {rt.size} elements beyond tol, {int(np.isnan(got).sum())} NaN")
        for f in fams:
            _note(f, sp.name, worst)
    _SEEN.update(fams)
    if keep is not None:
        keep[sp.name] = got
    return L


def _record():
    from hip_utils import record_parity

    record_parity("gemv",
                  tol="half a unit of the output format at y + (K + 8) 2^-24 S_ij + sum_k |w_jk| d_ik (d: 0, the LayerNorm bound, or half a bf16 unit "
                      "+ ((2 nsplit + 8) 2^-24 + %g) sum_s w_s |o_s| / l); exact family: equality; ACC_C = %g" % (V.EXPF_TERM, R.ACC_C),
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


@pytest.mark.parametrize("m", range(1, 9))
def test_rows_kernel_plain(probes, m):
    _run_all(probes, [sp for sp in V.rows_x_specs() if sp.M == m], f"rows-x-m{m}")


def test_rows_kernel_layernorm(probes):
    _run_all(probes, V.rows_ln_specs(), "rows-ln")


def test_rows_kernel_merge(probes):
    _run_all(probes, V.rows_merge_specs(), "rows-merge")


def test_gemv1_kernel_plain(probes):
    _run_all(probes, V.gemv1_x_specs(), "gemv1-x")


def test_gemv1_kernel_layernorm(probes):
    _run_all(probes, V.gemv1_ln_specs(), "gemv1-ln")


def test_gemv1_kernel_merge_with_nan_in_the_empty_ranges(probes):
    """Every o word of an empty range holds NaN bits: unwritten workspace, as attn_decode_part_kernel leaves it on every early step."""
    _run_all(probes, V.gemv1_merge_specs(), "gemv1-merge")


def test_gemv1_kernel_at_the_natural_grid(probes):
    _run_all(probes, V.gemv1_natural_specs(), "gemv1-natural")


@pytest.mark.parametrize("pro", [V.PRO_X, V.PRO_LN])
def test_gemvm_kernel(probes, pro):
    _run_all(probes, [sp for sp in V.gemvm_specs() if sp.pro == pro], f"gemvm-{V.PRO_NAME[pro]}")


def _one_row(sp, launcher):
    return V.replace(sp, name=sp.name + "-row0", launcher=launcher, M=1)


def test_row_zero_does_not_depend_on_the_rows_that_share_the_launch(probes):
    """Row 0 of an M-row launch equals the one-row launch of the same operands bit for bit: gemvm_kernel against gemv1_kernel (the same
    lane tree and chunk order), gemv_rows_kernel against itself."""
    n_cu = _num_cu()
    pairs = [(sp, V.GEMV1) for sp in V.gemvm_specs() if sp.family == "bounded" and sp.M in (2, 5, 8) and sp.N > 12]
    pairs += [(sp, V.ROWS) for sp in V.rows_x_specs() + V.rows_ln_specs() if sp.family == "bounded" and sp.M in (2, 5, 8) and sp.N in (40, 1001)]
    assert len(pairs) >= 30
    for sp, launcher in pairs:
        one = _one_row(sp, launcher)
        cm, c1 = _case(sp)[0], _case(one)[0]
        assert np.array_equal(cm.x[0], c1.x[0]) and np.array_equal(cm.W, c1.W), sp.name     # (the generators are indexed by element: row 0 is shared)
        assert (cm.bias is None or np.array_equal(cm.bias, c1.bias)) and (cm.resid is None or np.array_equal(cm.resid[0], c1.resid[0])), sp.name
        Lm, L1 = Launch(probes, cm), Launch(probes, c1)
        assert Lm.launch() == R.OK and L1.launch() == R.OK, sp.name
        assert Lm.instance.value == V.expected(sp, n_cu)[1] and L1.instance.value == V.expected(one, n_cu)[1], sp.name
        (gm, im), (g1, i1) = Lm.output(), L1.output()
        assert im and i1, sp.name
        assert np.array_equal(gm[0].view(np.uint32), g1[0].view(np.uint32)), f"{sp.name}: row 0 of {sp.M} rows differs from the one-row launch"


def test_every_instance_family_was_reached_by_name(probes):
    """(Runs after the tests above in file order.)  What they recorded covers gemv_ref.REQUIRED; without them this test launches one case each."""
    n_cu = _num_cu()
    for key in V.REQUIRED:
        if key not in _SEEN:
            sp = next(sp for sp in V.route_specs() if key in V.families(sp, n_cu))
            _run_all(probes, [sp], "coverage")
    assert not [k for k in V.REQUIRED if k not in _SEEN]


def test_refusals_launch_nothing(probes):
    """Each refusal returns its code, reports no instance and leaves every word of out as it was."""
    n_cu = _num_cu()

    def call(sp, want, struct_bytes=None, launcher=None, **fields):
        L = Launch(probes, _case(sp)[0])
        for k, v in fields.items():
            setattr(L.args, k, v)
        rc = L.launch(struct_bytes, launcher)
        assert L.untouched(), (sp.name, fields)
        assert L.instance.value in (0, -1), (sp.name, fields, L.instance.value)
        assert rc == want, (sp.name, fields, rc, want)

    assert C.sizeof(GemvArgs) == 152
    for sp, want in V.refused_specs():
        assert V.expected(sp, n_cu) == (want, 0), sp.name
        call(sp, want)
    base = V.GSpec("refuse-base", V.GEMVM, V.PRO_X, 3, 126, 2560, grid=V.G, resid=2)
    assert V.expected(base, n_cu)[0] == R.OK
    for size in (144, 148, 160):
        call(base, R.E_BADARG, struct_bytes=size)
    call(base, R.E_BADARG, launcher=3)
    call(base, R.E_BADARG, launcher=1)        # launch_gemv1 takes one row
    call(base, R.E_UNSUPPORTED, N=125)        # odd N with a bias and a residual: before anything runs
    call(base, R.E_UNSUPPORTED, W=None)
    call(base, R.E_UNSUPPORTED, ldx=2564)
    call(base, R.E_BADARG, ldr=135)
    one = V.GSpec("refuse-one", V.GEMV1, V.PRO_X, 1, 126, 2560, grid=V.G, resid=2)
    call(one, R.E_UNSUPPORTED, N=125)
    call(one, R.E_UNSUPPORTED, x=None)
    call(one, R.E_UNSUPPORTED, K=3072)
    rows = V.GSpec("refuse-rows", V.ROWS, V.PRO_X, 3, 40, 512, resid=2)
    call(rows, R.E_UNSUPPORTED, M=9)
    call(rows, R.E_UNSUPPORTED, K=520)
    call(rows, R.E_BADARG, ldx=516)
    call(rows, R.E_BADARG, x=None)
    call(V.GSpec("refuse-rows-merge", V.ROWS, V.PRO_MERGE, 2, 40, 512, heads=8, hd=64, nsplit=3), R.E_BADARG, heads=7)
