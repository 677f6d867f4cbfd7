"""Every prefill attention kernel of csrc/attention.hip and attn_frame3.h, launched on its own through the probe entry
eilev_debug_attention (one launch_attention on explicit arguments; it reports the kernel instance that was launched) and compared
with the float64 reference of tests/attn_prefill_ref.py.

Why this is tighter than test_hip_kernels.py (1e-2..2e-2 max|ref| on random q / k / v): there a dropped, doubled or mis-addressed key moves
a row by ~1/N of a value and disappears in the bound, as do a causal limit or a relative-position index that is off by one, a key mask
ignored in one tile, a read one row past skv, a skipped rescale.  Here the bound is derived from the kernels' own arithmetic —
tol_i = (2^-8 + 2^-11) A_i, A_i = sum_j p_j |v_ji| / sum_j p_j, no absolute floor — every row owns a planted key of softmax weight
~0.48 and values +-8, and every key that must not be seen (mask == 0, the row behind skv, stale cache slots) is a finite trap 30 above
the launch's maximum with values +-64; memory that must not be touched holds NaN bits, the output sentinels.  What each mistake costs
in tol is measured on the CPU by test_attn_prefill_reference.py (>= 4 for every one, mostly > 100).

form            route (each boundary from both sides: attn_prefill_ref.route_specs)
v1<64>          hd 64 with sq < 128 or skv < 64 (Q-Former self 32 x 32; cross 32 x 257 in k|v rows); hd 32 / 48; hd 64 with a position table
                that does not cover the launch (v1 clamps the index) or is longer than 4096
v1<96>          hd 72 / 80 / 88 with skv < 32 (17 x 17); hd 96
v1<128>         hd 128 with sq < 64 or skv < 64; hd 104 / 120
v1, any shape   eilev_debug_attn_v1(1): multi-tile causal + mask + position bias at hd 64 / 80 / 128, and every sweep below
v2<2|4|8|9>     hd 72 / 80 / 88, skv >= 32; ceil(sq / 32) = 1-2 | 3-4 | 5-8, 10-16, > 16 | 9; hd 88 with 257..272 rows that the frame route refuses
v2<4|8,2>(,rel) hd 64, sq >= 128, skv >= 64; sq 128 | 129..; table tight (rel_off = skv - 1, rel_n = sq + skv - 1), with a gap, rel_n = 4096
v2<4|8,4>       hd 128, sq >= 64, skv >= 64; sq 64..128 | 129..
frame<88,17>    hd 88, unmasked, sq = skv in 257, 258, 264, 272, fused q|k|v rows; pair counts below, at and above the CU count
frame3<88,17>   flag 16, S = 257; 1 and 3 frames, a pair count above the CU count; patch rows bit-equal to frame<88,17>

Every v1 / v2 form: the key-count sweep (guards and stale slots trapped), left padding on both sides of every 32- and 64-key boundary
(causal off = 0, causal off > 0, not causal), other masks incl. a batch entry without a visible key, ragged query counts, the three
layouts (fused ld 3D, k|v ld 2D, cache planes with 1 / 5 / 33 rows), both scales, and the online-softmax profiles (rising, falling, one
late key, a fully masked first tile; for v2 the lazy-rescale threshold from both sides).

Measured worst err / tol per form and the wall time: profiles/parity_r06.json, section attn_prefill (record_parity)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import attn_prefill_ref as R
from attn_prefill_ref import FRAME, FRAME3
from eilev_amd import abi

pytestmark = pytest.mark.gpu

EILEV_OK, EILEV_E_BADARG = 0, -1


class AttnArgs(C.Structure):
    """ctypes mirror of EilevDebugAttnArgs (csrc/attention.hip, probe build): AttnArgs without hm and dropout."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
                ("q_bs", C.c_int64), ("k_bs", C.c_int64), ("v_bs", C.c_int64), ("o_bs", C.c_int64),
                ("q_hs", C.c_int64), ("k_hs", C.c_int64), ("v_hs", C.c_int64), ("o_hs", C.c_int64),
                ("ldq", C.c_int64), ("ldk", C.c_int64), ("ldv", C.c_int64), ("ldo", C.c_int64),
                ("batch", C.c_int32), ("heads", C.c_int32), ("sq", C.c_int32), ("skv", C.c_int32), ("hd", C.c_int32),
                ("scale", C.c_float), ("causal", C.c_int32), ("pad0", C.c_int32),
                ("key_mask", C.c_void_p), ("mask_ld", C.c_int64), ("rel_tab", C.c_void_p), ("rel_hs", C.c_int64),
                ("rel_off", C.c_int32), ("rel_n", C.c_int32)]


_WORST: dict = {}
_FIRST: dict = {}
_SECONDS: dict = {}
_case_cache: dict = {}


def _entry(lib):
    fn = lib.eilev_debug_attention
    fn.argtypes = [C.POINTER(AttnArgs), C.c_size_t, C.POINTER(C.c_int), C.c_void_p]
    fn.restype = C.c_int
    return fn


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(sp):
    """(case, reference, A), built once per spec and left unchanged (the product block and the frame3 cross-check reuse them)."""
    got = _case_cache.get(sp.name)
    if got is None:
        c = R.build_case(sp)
        got = (c,) + R.reference(c)
        if sp.batch * sp.heads <= 64:
            _case_cache[sp.name] = got
    return got


class Launch:
    """The device buffers of one case (attn_prefill_ref.pack), the output poisoned; launch() runs the probe entry under the case's switch."""

    def __init__(self, c):
        sp = self.sp = c.spec
        P = self.P = R.pack(c)
        self.bufs = {n: torch.from_numpy(a).cuda() for n, a in P.bufs.items()}
        self.mask = None
        if c.mask is not None:  # (batch, skv + 3): the 3 words behind a row say "visible" — over a trap
            m = np.ones((sp.batch, sp.skv + 3), np.int32)
            m[:, :sp.skv] = c.mask
            self.mask = torch.from_numpy(m).cuda()
        self.rel = torch.from_numpy(c.rel_flat).cuda() if c.rel_tab is not None else None
        self.out = torch.full((sp.batch * P.o_rows * P.o_ld,), np.int16(np.uint16(R.SENT16).view(np.int16)).item(), dtype=torch.int16, device="cuda")
        a = self.args = AttnArgs()
        for n in ("q", "k", "v"):
            buf, off = getattr(P, n)
            setattr(a, n, self.bufs[buf].data_ptr() + 2 * off)
        a.o = self.out.data_ptr()
        a.q_bs, a.k_bs, a.v_bs, a.o_bs = P.q_bs, P.k_bs, P.v_bs, P.o_rows * P.o_ld
        a.q_hs, a.k_hs, a.v_hs, a.o_hs = P.q_hs, P.k_hs, P.v_hs, sp.hd
        a.ldq, a.ldk, a.ldv, a.ldo = P.ldq, P.ldk, P.ldv, P.o_ld
        a.batch, a.heads, a.sq, a.skv, a.hd = sp.batch, sp.heads, sp.sq, sp.skv, sp.hd
        a.scale, a.causal = float(c.scale), sp.causal
        if self.mask is not None:
            a.key_mask, a.mask_ld = self.mask.data_ptr(), sp.skv + 3
        if self.rel is not None:
            a.rel_tab, a.rel_hs, a.rel_off, a.rel_n = self.rel.data_ptr() + 4 * c.rel_lead, c.rel_hs, c.rel_off, c.rel_n
        self.form = C.c_int(-1)

    def launch(self, lib):
        try:
            lib.eilev_debug_attn_v1(self.sp.force)
            return _entry(lib)(C.byref(self.args), C.sizeof(AttnArgs), C.byref(self.form), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        finally:
            lib.eilev_debug_attn_v1(0)


def run_case(lib, sp, keep=None):
    """One launch, every check; returns the worst err / tol."""
    c, ref, A = _case(sp)
    L = Launch(c)
    rc = L.launch(lib)
    torch.cuda.synchronize()
    assert rc == EILEV_OK, (sp.name, rc)
    assert L.form.value == sp.form, f"{sp.name}: launched {R.form_name(L.form.value)}, the table says {R.form_name(sp.form)}"
    obits = L.out.cpu().numpy()
    got, intact = R.unpack_out(c, obits)
    assert intact, f"{sp.name}: a write outside the rows and columns of the output"
    dead = R.dead_rows(c)
    if dead.any():
        b, i = dead.nonzero()
        assert (got[b, :, i] == 0).all(), f"{sp.name}: a row without a visible key is not exact zeros"
    ratio = R.worst_ratio(got, ref, A)
    name = R.form_name(sp.form)
    print(f"{sp.name}: {name} err/tol {ratio:.3f}")
    _WORST[name] = max(_WORST.get(name, 0.0), ratio)
    _FIRST.setdefault(name, sp.name)
    if not ratio <= 1.0:
        err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - ref) / R.tolerance(A)
        b, h, i, d = np.unravel_index(np.argmax(err), err.shape)
        pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at batch {b} head {h} row {i} dim {d} (got {got[b, h, i, d]}, ref {ref[b, h, i, d]}); that row's spike at key "
                    f"{c.spike_pos[b, h, i]}, visible keys {int(R.visible(c, b)[i].sum())}; rows beyond tol: {int((err.max(-1) > 1).sum())} of {err[..., 0].size}")
    if keep is not None:
        keep[sp.name] = got
    return ratio


def _record():
    from hip_utils import record_parity

    record_parity("attn_prefill", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element, no floor",
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()}, **{f"first_case_{k}": v for k, v in _FIRST.items()},
                  **{f"seconds_{k}": v for k, v in _SECONDS.items()}, seconds_total=sum(_SECONDS.values()))


def _run_all(lib, specs, label, keep=None):
    assert specs
    t0 = time.time()
    try:
        for sp in specs:
            run_case(lib, sp, keep)
    finally:
        _SECONDS[label] = _SECONDS.get(label, 0.0) + time.time() - t0
        _record()


def test_route_boundaries_report_the_form_of_the_table(probes):
    """Both sides of every boundary of launch_attention's route: the form comes from the probe entry, the numbers are held to tol."""
    _run_all(probes, R.route_specs(), "route")


@pytest.mark.parametrize("form", R.V12_FORMS, ids=R.form_name)
def test_key_count_sweep(probes, form):
    """skv = 32, 33, 63..65, 95..97, 127..129, 191..193, 255..257, 511..513 (cut to what the route admits), hd 80 and one other where the form
    takes two; the row behind skv and the stale cache slots are traps; the layouts and the two scales alternate."""
    _run_all(probes, R.sweep_specs(form), f"keys-{R.form_name(form)}")


@pytest.mark.parametrize("form", R.V12_FORMS, ids=R.form_name)
def test_left_padding_and_the_causal_diagonal(probes, form):
    """L = 0, 1, 31..33, 63..65, 127..129, 300: behind the padding one row sees exactly one key, the rows before it none (exact zeros)."""
    _run_all(probes, R.pad_specs(form), f"pad-{R.form_name(form)}")


@pytest.mark.parametrize("form", R.V12_FORMS, ids=R.form_name)
def test_masks_cache_planes_and_online_softmax(probes, form):
    """Holes, right padding, a batch entry without a visible key, a first tile fully masked; cache planes with 1, 5 and 33 query rows; scores
    that rise and fall tile by tile and one late dominant key over ten key tiles."""
    _run_all(probes, R.mask_specs(form) + R.cache_specs(form) + R.online_specs(form), f"mask-{R.form_name(form)}")


def test_v2_lazy_rescale_threshold_from_both_sides(probes):
    """One real row per wave whose maximum rises by 5.5 .. 6.5 (and 3, 9, 12) base-2 units from key tile 0 to key tile 1."""
    _run_all(probes, R.lazy_specs(), "lazy")


@pytest.mark.parametrize("which", range(3))
def test_frame_kernel_pair_counts(probes, which):
    """(frame, head) pairs below, at and above the CU count (a ragged last round of the persistent walk)."""
    _run_all(probes, [sp for sp in R.frame_specs(_num_cu()) if sp.form == FRAME][which:which + 1], "frame")


@pytest.mark.parametrize("which", range(3))
def test_frame3_kernel_and_its_cross_check(probes, which):
    """1 and 3 frames and a pair count above the CU count; the same inputs through attn_frame_kernel: patch rows bit-equal, the CLS row
    (eight partial softmaxes merged) within tol of the reference in both."""
    sp = [sp for sp in R.frame_specs(_num_cu()) if sp.form == FRAME3][which]
    keep = {}
    _run_all(probes, [sp, R.replace(sp, name=sp.name + "-frame", form=FRAME, force=0)], "frame3", keep)
    a, b = keep[sp.name], keep[sp.name + "-frame"]
    assert np.array_equal(R.bf16_bits(a[:, :, :256]), R.bf16_bits(b[:, :, :256])), "patch rows differ between the two frame kernels"


_product = None


def test_product_library_gives_the_same_bits(probes):
    """One case per form through the public eilev_attention / eilev_attention_rel of the PRODUCT library (dense output, one batch entry: the
    public entry has no batch stride): bit-identical to the probe library's launch of the same case, so what is tested is what ships."""
    global _product
    if _product is None:
        _product = abi.load_library(abi.HIP_LIB_PATH)
    assert not hasattr(_product, "eilev_debug_attention")
    by_name = {sp.name: sp for sp in R.route_specs()}
    seen = set()
    for name in R.PRODUCT_CASES:
        sp = R.replace(by_name[name], batch=1, name=name + "-b1")
        keep = {}
        run_case(probes, sp, keep)
        c = _case(sp)[0]
        L = Launch(c)
        D = sp.heads * sp.hd
        out = torch.full((sp.sq * D,), 0x7FA5, dtype=torch.int16, device="cuda")
        a = L.args
        common = (a.q, a.k, a.v, out.data_ptr(), 1, sp.heads, sp.sq, sp.skv, sp.hd, a.ldq, a.ldk, a.ldv, float(c.scale), sp.causal, a.key_mask)
        assert L.mask is None or a.mask_ld == sp.skv + 3  # (one batch entry: the row stride of the mask is never used)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if c.rel_tab is not None:
            rc = _product.eilev_attention_rel(*common, a.rel_tab, a.rel_hs, a.rel_off, a.rel_n, stream)
        else:
            rc = _product.eilev_attention(*common, stream)
        torch.cuda.synchronize()
        assert rc == EILEV_OK, (name, rc)
        got = R.bits_to_f32(out.cpu().numpy()).reshape(sp.sq, sp.heads, sp.hd).transpose(1, 0, 2)
        assert np.array_equal(R.bf16_bits(got), R.bf16_bits(keep[sp.name][0])), f"{name}: product and probe library differ"
        seen.add(sp.form)
    assert seen == set(R.V12_FORMS) | {FRAME}


def test_refusals_launch_nothing(probes):
    """Host-side refusals: the code comes back, the form is 0 and the output is untouched."""
    sp = R.Spec("refuse", 96, batch=1, heads=2, hd=80, sq=17, skv=17)
    c = _case(sp)[0]

    def call(struct_bytes=None, **fields):
        L = Launch(c)
        for k, v in fields.items():
            setattr(L.args, k, v)
        if struct_bytes is None:
            rc = L.launch(probes)
        else:
            rc = _entry(probes)(C.byref(L.args), struct_bytes, C.byref(L.form), None)
        torch.cuda.synchronize()
        assert (L.out.cpu().numpy().view(np.uint16) == R.SENT16).all()
        return rc, L.form.value

    assert call(hd=136) == (-2, 0) and call(hd=12) == (-2, 0) and call(ldk=L_odd(c)) == (-2, 0)
    assert call(q=None) == (EILEV_E_BADARG, 0) and call(skv=0) == (EILEV_E_BADARG, 0)
    assert call(batch=0) == (EILEV_OK, 0)
    assert call(struct_bytes=C.sizeof(AttnArgs) - 8)[0] == EILEV_E_BADARG and call(struct_bytes=C.sizeof(AttnArgs) + 8)[0] == EILEV_E_BADARG
    assert C.sizeof(AttnArgs) == 200


def L_odd(c):
    return R.pack(c).ldk + 4
