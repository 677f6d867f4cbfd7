"""Cases, float64 reference, per-element bound and expected route of the wide (M > 32) bf16 GEMM family of csrc/gemm.hip.  CPU only, numpy.

A Spec names one launch_gemm call field by field (GemmArgs of csrc/common.h) plus the probe switch value (eilev_debug_gemm_flags).  build_case
makes its operands with guards, reference evaluates it in float64, tol gives the bound every output element is held to, expected names the
return code and the kernel instance (common.h GEMM_FORM) that launch_gemm must reach on a device of n_cu compute units, route_specs lists the
launches of tests/test_hip_gemm_wide.py.  tests/test_gemm_reference.py checks all of this on the CPU and measures what planted mistakes cost.

Guards (build_case): A and W are allocated with lda > K and ldw > K wherever the route accepts it (launch_a8w8, w8_check and the head-major
output need == K / have no stride), the padding columns hold finite traps of +-2^14, two trap rows follow row M - 1 of A and of the residual
and row N - 1 of W; C has ldc > N and two guard rows, all NaN bits (0x7FA5 per half word), as are stat_out, ln_out and the fp8 scratch.

Families: "exact" — A and W in {-1, 0, 1} thinned so that results stay below 2^6, integer bias / residual, power-of-two scales: every partial
sum is an integer below 2^24 (exact in fp32 in any order) and every result is a bf16 value, so a kernel must match BIT FOR BIT;
"bounded" — dense asymmetric normals (det_normal), for GELU, real scales, the folded LayerNorm with a large row mean and the statistics.

tol, per element, no floor and no max|ref| term:
  output rounding    half a unit in the last place of the output format AT y: 2^(floor(log2 |y|) - 8) for bf16, ... - 24 for fp32.  (bf16 keeps 8
                     significant bits, so round-to-nearest errs by up to 2^-8 |y| at the bottom of a binade and 2^-9 |y| only at its top: a flat
                     2^-9 |y| would fail correctly rounded results.  The exact half unit is what the format guarantees, and it is never wider.)
  fp32 accumulation  ACC_C * (K + 8) * 2^-24 * S_ij * slope, S_ij = sum_k |a_ik w_jk| (+ |mean_i csum_j| for the folded LayerNorm) with the same
                     scales as y, slope 1 (none / ReLU) or 1.13 (GELU).  ACC_C = 1 unless a measurement on the device widens it (see there).
  GELU               + the measured max abs error of the polynomial the instance evaluates (gelu_forms: replayed in fp32 from common.h)
  folded LayerNorm   + 3 * 2^-18 rstd_i |mean_i csum_j|: gemm_pp4.h feeds -mean and csum to one short MFMA as two bf16 pieces each
                     (m = mh + ml, c = ch + cl) and leaves out ml * cl; a piece pair misses its number by <= 2^-18 of it (2^-9 * 2^-9) and the
                     omitted product is <= 2^-18 |m c|, three such terms in all.  (K + 8) 2^-24 (S + |mean csum|) alone is below this for K < 256:
                     measured on the device at K = 64, one element of 1.3 M reached 1.05 of the bound without the term while the exact family
                     matched bit for bit.  (LN-fold cases only; scales with the GELU slope.)
stat_out and ln_out: stat_ref / ln_out_ref below."""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, replace  # noqa: F401  (replace: for the tests)

import numpy as np

from eilev_amd.synth import det_normal, round_bf16

OK, E_BADARG, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3
SENT16 = 0x7FA5        # a NaN as bf16; 0x7FA57FA5 is one as fp32
TRAP = 16384.0         # 2^14: finite, bf16-exact, far above any output
ACC_C = 1.0            # multiplier of the (K + 8) 2^-24 constant (the issue: widen to twice the measured ratio if the MFMA needs it)

# dbg bits / force values of csrc/common.h (an interface: numbers)
NO_DMA, NO_WIDE, NO_HALF, WIDE_TILED, NO_W6 = 1 << 2, 1 << 14, 1 << 19, 1 << 20, 1 << 21
FORCE_SHIFT = 4
FORCE_PP4, FORCE_W6, FORCE_64x128, FORCE_128x128, FORCE_SPLIT_K = 9, 12, 13, 14, 15
ROW_CHUNKS, W8_EXPANDED = 1 << 16, 1 << 17
BK = 64
OFFSET_LIMIT = 0x7FFF0000
A3_MIN_K = 5120


def force(v):
    return v << FORCE_SHIFT


@dataclass(frozen=True)
class Spec:
    name: str
    M: int
    N: int
    K: int
    epi: int = 0              # 0 none, 1 GELU, 2 ReLU
    bias: bool = True
    resid: bool = False
    out_f32: bool = False
    scale_cols: int = 0
    scale: float = 1.0
    patch_group: int = 0      # > 0: M = frames * group rows, the output has a CLS row in front of every frame
    hm: tuple = ()            # (hm_tok, hm_heads, hm_hd)
    wscale: bool = False
    w8: bool = False          # weights as e4m3 bytes (expanded into the scratch for M > 32)
    a8: bool = False          # e4m3 activations and weights with ascale / wscale
    lnfold: bool = False      # ln_rows + ln_csum
    stats: bool = False       # stat_out
    ln_out: int = 0           # 1 LayerNorm (gamma, beta), 2 RMSNorm (gamma)
    family: str = "exact"
    flags: int = 0            # eilev_debug_gemm_flags
    pad: bool = True          # lda / ldw / ldr / ldc wider than the matrix where the route takes it
    seed: int = 0
    resid_gain: float = 1.0   # bounded family: the residual's scale (a residual stream that dominates what is added to it)


@dataclass
class Case:
    spec: Spec
    lda: int
    ldw: int
    ldr: int
    ldc: int
    out_rows: int
    A_buf: np.ndarray = None      # float32 (M + 2, lda), bf16-exact; a8: the decoded e4m3 values (M + 2, K)
    W_buf: np.ndarray = None      # float32 (N + 2, ldw); w8 / a8: the decoded values
    A8: np.ndarray = None         # uint8 bytes
    W8: np.ndarray = None
    bias: np.ndarray = None       # float32 (N + 8), the tail trapped
    resid_buf: np.ndarray = None  # float32 (rows + 2, ldr)
    wscale: np.ndarray = None
    ascale: np.ndarray = None
    ln_rows: np.ndarray = None    # (M, 2): rstd, -mean
    ln_csum: np.ndarray = None
    gamma: np.ndarray = None
    beta: np.ndarray = None
    stat_ld: int = 0
    stat_slots: int = 0           # allocated, two more than ceil(N / 64)
    ln_eps: float = 1e-5
    ln_split: object = 0.0        # reference() leaves the bound of the folded LayerNorm's split rank-1 term here (tol adds it)

    @property
    def A(self):
        return self.A_buf[:self.spec.M, :self.spec.K]

    @property
    def W(self):
        return self.W_buf[:self.spec.N, :self.spec.K]

    @property
    def resid(self):
        rows = 1 + self.spec.patch_group if self.spec.patch_group else self.spec.M
        return None if self.resid_buf is None else self.resid_buf[:rows, :self.spec.N]


# ---- number formats --------------------------------------------------------------------------------------------------------------------------

def bf16_bits(x):
    """bf16-exact float32 -> uint16 bit patterns."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bits_to_f32(b):
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def is_bf16(x):
    x32 = np.asarray(x, np.float32)
    return bool(np.array_equal(x32.astype(np.float64), np.asarray(x, np.float64)) and np.array_equal(round_bf16(x32), x32))


def half_ulp(y, bits):
    """Half a unit in the last place of a format with `bits` significant bits at |y| (0 at y = 0)."""
    y = np.abs(np.asarray(y, np.float64))
    e = np.floor(np.log2(np.where(y > 0, y, 1.0)))
    return np.where(y > 0, np.exp2(e - bits), 0.0)


_E4M3 = None


def e4m3_table():
    """The 256 OCP e4m3 values (0x7F / 0xFF are NaN: never generated)."""
    global _E4M3
    if _E4M3 is None:
        t = np.zeros(256, np.float32)
        for c in range(256):
            s, e, m = c >> 7, (c >> 3) & 15, c & 7
            v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
            t[c] = -v if s else v
        t[0x7F] = t[0xFF] = np.nan
        _E4M3 = t
    return _E4M3


# ---- the GELU forms the kernels evaluate (csrc/common.h), replayed in fp32 ---------------------------------------------------------------------

def _coeffs(name):
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eilev_amd", "csrc", "common.h")).read()
    body = re.search(r"#define " + name + r"\s*\\\s*\n\s*\{([^}]*)\}", h).group(1)
    return np.array([float(t.strip().rstrip("f")) for t in body.replace("\\", " ").split(",")], np.float32)


def _horner(c, t):
    p = np.full_like(t, c[-1])
    for k in range(len(c) - 2, -1, -1):
        p = (p * t + c[k]).astype(np.float32)
    return p


def gelu_deg12(x):
    """gelu_erf / gelu_erf_pk: the per-tile kernels (gemm_nt_kernel, gemm_glds_kernel)."""
    x = np.asarray(x, np.float32)
    u = np.minimum(np.abs(x), np.float32(5.0))
    t = (u * np.float32(0.4) - np.float32(1.0)).astype(np.float32)
    return (np.maximum(x, 0) - u * _horner(_coeffs("EILEV_GELU12_COEFFS"), t)).astype(np.float32)


def gelu_phi(x):
    """gelu_erf_n with EILEV_GELU_PHI (the default): every instance of gemm_pp4_kernel, lean and general epilogue."""
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eilev_amd", "csrc", "common.h")).read()
    c = np.float32(re.search(r"#define EILEV_GELU_PHI_C ([0-9.]+)f", h).group(1))
    x = np.asarray(x, np.float32)
    xc = np.clip(x, -c, c).astype(np.float32)
    p = _horner(_coeffs("EILEV_GELU_PHI_COEFFS"), (xc * xc).astype(np.float32))
    return (x * (xc * p + np.float32(0.5)).astype(np.float32)).astype(np.float32)


def gelu_deg8(x):
    """The degree-8 form (EILEV_GELU_COEFFS) that gemm_w6_kernel evaluates in its chunked epilogue."""
    x = np.asarray(x, np.float32)
    u = np.minimum(np.abs(x), np.float32(4.0))
    t = (u * np.float32(0.5) - np.float32(1.0)).astype(np.float32)
    return (np.maximum(x, 0) - _horner(_coeffs("EILEV_GELU_COEFFS"), t)).astype(np.float32)


def erf64(x):
    x = np.asarray(x, np.float64)
    return np.vectorize(math.erf, otypes=[np.float64])(x) if x.size else x


def gelu_exact(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf64(x / math.sqrt(2.0)))


GELU_RANGE = 16.0  # the pre-activations of every GELU case stay inside (build_case asserts it)
_gelu_err = {}


def gelu_forms():
    """{form name: measured max |polynomial - exact erf GELU| on [-GELU_RANGE, GELU_RANGE]} — measured here, never taken from a device."""
    if not _gelu_err:
        x = np.linspace(-GELU_RANGE, GELU_RANGE, 640001)
        ex = gelu_exact(x)
        for name, f in (("deg12", gelu_deg12), ("phi", gelu_phi), ("deg8", gelu_deg8)):
            _gelu_err[name] = float(np.abs(f(x).astype(np.float64) - ex).max())
    return dict(_gelu_err)


def gelu_form_of(form):
    """Which polynomial the kernel instance `form` evaluates."""
    fam = (form & 0xFFFF) // 1000
    return {1: "deg12", 2: "deg12", 3: "deg12", 4: "phi", 5: "deg8"}[fam]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------

def _strides(sp):
    pad = sp.pad
    a_fixed = sp.a8
    w_fixed = sp.a8 or sp.w8
    lda = sp.K + (8 if pad and not a_fixed else 0)
    ldw = sp.K + (16 if pad and not w_fixed else 0)
    ldr = sp.N + (16 if pad else 0)
    ldc = sp.N + (8 if pad and not sp.hm else 0)
    return lda, ldw, ldr, ldc


def _trap_fill(buf, rows, cols, salt):
    """Everything outside [:rows, :cols] becomes +-TRAP in a checkerboard (so that a sum of traps does not cancel by accident)."""
    r, c = np.indices(buf.shape)
    sign = np.where(((r * 3 + c + salt) % 5) < 3, 1.0, -1.0).astype(np.float32)
    out = (r >= rows) | (c >= cols)
    buf[out] = (sign * np.float32(TRAP))[out]


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _ternary(rng, shape, density):
    return (rng.integers(0, 2, size=shape, dtype=np.int8) * 2 - 1).astype(np.float32) * (rng.random(shape, dtype=np.float32) < density) + np.float32(0.0)  # (no -0)


def _pow2(rng, n, exps):
    return np.exp2(rng.choice(np.asarray(exps, np.float64), size=n)).astype(np.float32)


def _encode_e4m3(x):
    """Nearest e4m3 code of values that ARE e4m3 values (exact family / decoded tables): by lookup."""
    t = e4m3_table()
    order = np.argsort(np.where(np.isnan(t), np.inf, t), kind="stable")
    vals = t[order]
    idx = np.searchsorted(vals[:254], x.ravel())
    codes = order[np.clip(idx, 0, 253)].astype(np.uint8).reshape(x.shape)
    codes[x == 0] = 0  # (+0, not -0)
    assert np.array_equal(t[codes], x), "not an e4m3 value"
    return codes


def build_case(sp: Spec) -> Case:
    M, N, K = sp.M, sp.N, sp.K
    lda, ldw, ldr, ldc = _strides(sp)
    rng = np.random.default_rng([sp.seed, M, N, K, sp.epi, int(sp.family == "exact")])
    exact = sp.family == "exact"
    assert not (exact and sp.epi == 1), "GELU has no exact family"
    frames = M // sp.patch_group if sp.patch_group else 0
    assert not sp.patch_group or M == frames * sp.patch_group
    out_rows = frames * (sp.patch_group + 1) if sp.patch_group else M
    c = Case(sp, lda, ldw, ldr, ldc, out_rows)
    fp8 = sp.a8 or sp.w8
    A_buf = np.zeros((M + 2, lda), np.float32)
    W_buf = np.zeros((N + 2, ldw), np.float32)
    if exact:
        d = min(0.5, math.sqrt(12.0 / K))  # K d^2 = 12 nonzero products per element: |sum| stays below 2^5
        A_buf[:M, :K] = _ternary(rng, (M, K), d)
        W_buf[:N, :K] = _ternary(rng, (N, K), d)
        if sp.lnfold:  # thinner weights: csum stays small, so that mean * csum does
            W_buf[:N, :K] *= rng.random((N, K), dtype=np.float32) < 0.5
    elif sp.a8:
        t = e4m3_table()
        ca = (rng.integers(0, 2, (M, K)) << 7 | rng.integers(4, 9, (M, K)) << 3 | rng.integers(0, 8, (M, K))).astype(np.uint8)   # |a| in [2^-3, 3.75)
        cw = (rng.integers(0, 2, (N, K)) << 7 | rng.integers(2, 7, (N, K)) << 3 | rng.integers(0, 8, (N, K))).astype(np.uint8)   # |w| in [2^-5, 0.94)
        A_buf[:M, :K], W_buf[:N, :K] = t[ca], t[cw]
    else:
        a = det_normal(f"gw-A{sp.seed}", (M, K), sp.seed)
        if sp.lnfold:  # a raw residual stream: a large row mean and one outlier channel
            a = a + 3.0 + 0.5 * det_normal("gw-rowmean", (M, 1), sp.seed)
            a[:, 5] *= 12.0
        A_buf[:M, :K] = round_bf16(a)
        w = det_normal(f"gw-W{sp.seed}", (N, K), sp.seed) / np.sqrt(K)
        if sp.w8:
            t = e4m3_table()
            cw = (rng.integers(0, 2, (N, K)) << 7 | rng.integers(1, 6, (N, K)) << 3 | rng.integers(0, 8, (N, K))).astype(np.uint8)
            w = t[cw]
        W_buf[:N, :K] = round_bf16(w)
    _trap_fill(A_buf, M, K, 0)
    _trap_fill(W_buf, N, K, 1)
    if sp.a8:  # byte operands: the trap rows are the largest e4m3 value
        A_buf[M:] = np.sign(A_buf[M:]) * 448.0
        c.A8 = _encode_e4m3(A_buf)
    if fp8:
        W_buf[N:] = np.sign(W_buf[N:]) * 448.0
        c.W8 = _encode_e4m3(W_buf)
    c.A_buf, c.W_buf = A_buf, W_buf
    if sp.bias:
        b = np.full(N + 8, TRAP, np.float32)
        b[:N] = _ints(rng, N, -8, 8) if exact else round_bf16(0.5 * det_normal("gw-b", (N,), sp.seed))
        c.bias = b
    if sp.resid:
        rows = 1 + sp.patch_group if sp.patch_group else M
        r = np.zeros((rows + 2, ldr), np.float32)
        r[:rows, :N] = _ints(rng, (rows, N), -16, 16) if exact else round_bf16(sp.resid_gain * det_normal("gw-r", (rows, N), sp.seed))
        _trap_fill(r, rows, N, 2)
        c.resid_buf = r
    if sp.wscale or fp8:
        c.wscale = _pow2(rng, N, [-2, -1, 0]) if exact else (0.02 + 0.05 * rng.random(N)).astype(np.float32)
    if sp.a8:
        c.ascale = _pow2(rng, M, [-1, 0, 1]) if exact else (0.5 + rng.random(M)).astype(np.float32)
    if sp.lnfold:
        ln = np.zeros((M, 2), np.float32)
        if exact:
            ln[:, 0] = _pow2(rng, M, [-2, -1, 0])
            ln[:, 1] = -_ints(rng, M, -3, 3)
        else:  # the row's own LayerNorm statistics, as ln_finalize_kernel leaves them
            a64 = c.A.astype(np.float64)
            ln[:, 0] = 1.0 / np.sqrt(a64.var(1) + 1e-5)
            ln[:, 1] = -a64.mean(1)
        c.ln_rows = ln
        c.ln_csum = c.W.astype(np.float64).sum(1).astype(np.float32)
        if exact:
            assert np.array_equal(c.ln_csum.astype(np.float64), c.W.astype(np.float64).sum(1)) and np.abs(c.ln_csum).max() <= 256
    if sp.stats:
        c.stat_ld = M + 8
        c.stat_slots = (N + 63) // 64 + 2
    if sp.ln_out:
        c.gamma = round_bf16(1.0 + 0.1 * det_normal("gw-g", (N,), sp.seed))
        c.beta = round_bf16(0.1 * det_normal("gw-be", (N,), sp.seed)) if sp.ln_out == 1 else None
    return c


# ---- reference -------------------------------------------------------------------------------------------------------------------------------

def _matmul(c: Case, big=1 << 31):
    """(A W^T, |A| |W|^T) in float64; a large exact-family product in float32 BLAS, which is exact there (integer partial sums below 2^24)."""
    sp = c.spec
    A, W = c.A, c.W
    if sp.family == "exact" and not sp.a8 and sp.M * sp.N * sp.K >= big:
        y = np.empty((sp.M, sp.N), np.float64)
        Wt = np.ascontiguousarray(W.T)
        for r0 in range(0, sp.M, 512):
            y[r0:r0 + 512] = A[r0:r0 + 512] @ Wt
        return y, np.zeros_like(y)  # (no bound is evaluated on these: the comparison is bit for bit)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    return A64 @ W64.T, np.abs(A64) @ np.abs(W64).T


def reference(c: Case):
    """(y, S, pre) in float64 on the logical [M, N] output: the value, the magnitude sum its fp32 accumulation is bounded with, and the
    pre-activation (GELU cases: its range is asserted)."""
    sp = c.spec
    M, N = sp.M, sp.N
    y, S = _matmul(c)
    split = 0.0  # (see tol: the folded LayerNorm's rank-1 term)
    if sp.lnfold:
        rstd, nm = c.ln_rows[:, 0].astype(np.float64)[:, None], c.ln_rows[:, 1].astype(np.float64)[:, None]
        cs = c.ln_csum.astype(np.float64)[None, :]
        y = rstd * (y + nm * cs)
        S = np.abs(rstd) * (S + np.abs(nm * cs))
        split = 3 * 2.0 ** -18 * np.abs(rstd * nm * cs)
    if c.wscale is not None:
        y, S = y * c.wscale.astype(np.float64)[None, :], S * c.wscale.astype(np.float64)[None, :]
    if c.ascale is not None:
        y, S = y * c.ascale.astype(np.float64)[:, None], S * c.ascale.astype(np.float64)[:, None]
    if c.bias is not None:
        y = y + c.bias[:N].astype(np.float64)[None, :]
    if sp.scale_cols:
        y[:, :sp.scale_cols] *= sp.scale
        S[:, :sp.scale_cols] *= abs(sp.scale)
    c.ln_split = split * (1.13 if sp.epi == 1 else 1.0)
    pre = y
    if sp.epi == 1:
        assert np.abs(y).max() < GELU_RANGE
        y = gelu_exact(y)
    elif sp.epi == 2:
        y = np.maximum(y, 0.0)
    if c.resid is not None:
        r = c.resid.astype(np.float64)
        y = y + (r[1 + np.arange(M) % sp.patch_group] if sp.patch_group else r)
    return y, S, pre


def tol(c: Case, y, S, form):
    sp = c.spec
    t = half_ulp(y, 24 if sp.out_f32 else 8)
    t = t + ACC_C * (sp.K + 8) * 2.0 ** -24 * S * (1.13 if sp.epi == 1 else 1.0)
    if sp.epi == 1:
        t = t + gelu_forms()[gelu_form_of(form)]
    if sp.lnfold:
        t = t + c.ln_split
    return t


def ratio(err, t):
    """err / tol per element: NaN in the output counts as infinite, an exact zero held to a zero bound as 0."""
    err, t = np.asarray(err, np.float64), np.asarray(t, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(t > 0, err / t, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def out_index(c: Case, hm_swapped=False):
    """Flat element index into the C allocation of every logical (row, column): row-major with ldc, the patch remap (a CLS row in front of
    every frame), or the head-major q|k|v scatter exactly as GemmArgs::hm_tok describes it (csrc/common.h)."""
    sp = c.spec
    m, n = np.arange(sp.M, dtype=np.int64)[:, None], np.arange(sp.N, dtype=np.int64)[None, :]
    if sp.hm:
        tok, nh, hd = sp.hm
        d3 = sp.N // 3
        f, t = m // tok, m % tok
        plane, rr = n // d3, n % d3
        first = rr < nh * 64
        # per third of N: [head h dims 0..63] for all heads, then [head h dims 64..hd-1] for all heads
        head = np.where(first, rr // 64, (rr - nh * 64) // (hd - 64))
        dim = np.where(first, rr % 64, (rr - nh * 64) % (hd - 64))
        # every (frame, plane, head) owns tok * hd elements: [token][64] followed by [token][hd - 64]
        block = f * tok * sp.N + (plane * nh + head) * tok * hd
        if hm_swapped:  # (a planted mistake of test_gemm_reference.py: the two parts of a block exchanged)
            return block + np.where(first, tok * (hd - 64) + t * 64 + dim, t * (hd - 64) + dim)
        return block + np.where(first, t * 64 + dim, tok * 64 + t * (hd - 64) + dim)
    orow = m + m // sp.patch_group + 1 if sp.patch_group else m
    return orow * c.ldc + n


def c_words(c: Case):
    """Elements of the C allocation: the output rows plus two guard rows (head-major: M * N + 2 * N)."""
    return (c.out_rows + 2) * (c.spec.N if c.spec.hm else c.ldc)


def stat_ref(c: Case, y, S):
    """stat_out as gemm_epilogue / the lean epilogue of gemm_pp4_kernel write it: per 64-column slot and row the (sum, sum of squares) of the
    fp32 values BEFORE their bf16 rounding (residual included), over the columns < N.  Returns (ref [slots, M, 2], tol [slots, M, 2]): the
    element errors d_ij <= ACC_C (K + 8) 2^-24 S_ij add up over the slot, and summing 64 fp32 numbers in any order adds (64 + 8) 2^-24 sum |v|;
    for the squares d(v^2) = 2 |v| d."""
    sp = c.spec
    slots = (sp.N + 63) // 64
    ref = np.zeros((slots, sp.M, 2))
    tl = np.zeros((slots, sp.M, 2))
    d = ACC_C * (sp.K + 8) * 2.0 ** -24 * S + 3 * 2.0 ** -24 * np.abs(y)  # (+ the bias, activation and residual additions: one rounding each)
    for s in range(slots):
        v, dv = y[:, 64 * s:64 * s + 64], d[:, 64 * s:64 * s + 64]
        ref[s, :, 0], ref[s, :, 1] = v.sum(1), (v * v).sum(1)
        tl[s, :, 0] = dv.sum(1) + 72 * 2.0 ** -24 * np.abs(v).sum(1)
        tl[s, :, 1] = (2 * np.abs(v) * dv + dv * dv).sum(1) + 72 * 2.0 ** -24 * (v * v).sum(1)
    return ref, tl


def ln_out_ref(c: Case, rows_bf16):
    """(ref, tol) of GemmArgs::ln_out on the bf16 rows of C that the device wrote (float array [M, N]): norm.hip layernorm_kernel /
    rmsnorm_kernel in float64.  eps_n = (N + 16) 2^-24 bounds the fp32 sums (mean, variance: N additions each) and the rsqrt.
    LayerNorm: y = (x - mean) rstd g + b: d <= eps_n (|x| + |mean|) rstd |g| (the mean's error and the difference's) + eps_n |y - b| (rstd,
    products) + half a bf16 unit at y.  RMSNorm: y = g * bf16(x rs): the inner rounding may fall either way when x rs (1 +- eps_n) straddles
    a tie, so the bound is the larger distance to the two results of rounding x rs (1 - eps_n) and x rs (1 + eps_n), + half a unit at y."""
    sp = c.spec
    x = np.asarray(rows_bf16, np.float64)
    g = c.gamma.astype(np.float64)[None, :]
    eps_n = (sp.N + 16) * 2.0 ** -24
    if sp.ln_out == 1:
        mean = x.mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + c.ln_eps)
        b = c.beta.astype(np.float64)[None, :]
        y = (x - mean) * rstd * g + b
        t = eps_n * (np.abs(x) + np.abs(mean)) * rstd * np.abs(g) + eps_n * np.abs(y - b) + half_ulp(y, 8) + 2.0 ** -24 * np.abs(y)
        return y, t
    rs = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + c.ln_eps)
    inner = x * rs
    mid = round_bf16(inner.astype(np.float32)).astype(np.float64)
    lo = round_bf16((inner * (1 - eps_n)).astype(np.float32)).astype(np.float64)
    hi = round_bf16((inner * (1 + eps_n)).astype(np.float32)).astype(np.float64)
    y = g * mid
    t = np.abs(g) * np.maximum(np.abs(lo - mid), np.abs(hi - mid)) + half_ulp(y, 8) + np.abs(g) * half_ulp(mid, 8) * 2.0 ** -12
    return y, t


# ---- the route: a mirror of launch_gemm_core / launch_wide / launch_pp4 / launch_pp4_ext (csrc/gemm.hip, gemm_pp4_ext.hip) ---------------------------

def _cdiv(a, b):
    return -(-a // b)


def _fits(rows, ld):
    return rows * ld * 2 < OFFSET_LIMIT


def pp4_all_lean(sp, dbg):
    scale_ok = sp.scale_cols == 0 or (sp.scale_cols % 16 == 0 and sp.epi == 0 and not sp.resid and not sp.lnfold and not sp.stats)
    return sp.N % 128 == 0 and not sp.out_f32 and sp.patch_group == 0 and scale_ok and not (sp.wscale or sp.w8 or sp.a8) and not dbg


def hm_takes(sp, dbg):
    tok, nh, hd = sp.hm
    return (tok >= 128 and nh > 0 and hd > 64 and hd % 8 == 0 and sp.N == 3 * nh * hd and sp.lnfold and sp.epi == 0 and not sp.resid and not sp.stats
            and not sp.scale_cols and pp4_all_lean(sp, dbg) and sp.N % 64 == 0 and sp.M % tok == 0 and sp.M * sp.N * 2 < 0xFFFFFFF0)


def tile_cfg(sp):
    tm256 = _cdiv(sp.M, 256)
    if tm256 * _cdiv(sp.N, 256) >= 256 and sp.N >= 2048:
        return 1
    if tm256 * _cdiv(sp.N, 128) >= 512:
        return 3
    if tm256 * _cdiv(sp.N, 128) >= 192:
        return 2
    return 4


def w6_ok(sp, lda, ldw, ldr, ldc):
    return (sp.K % 64 == 0 and sp.K >= 256 and sp.N % 128 == 0 and (not sp.resid or (sp.epi == 0 and ldr % 8 == 0)) and not sp.out_f32
            and sp.patch_group == 0 and sp.scale_cols == 0 and not (sp.wscale or sp.w8) and _fits(sp.M, lda) and _fits(sp.N, ldw) and ldc % 8 == 0)


def w6_pick(sp, n_cu):
    tm256 = _cdiv(sp.M, 256)
    tiles256 = tm256 * _cdiv(sp.N, 256)
    q = n_cu // 8 * 8
    fill = lambda t: t / (_cdiv(t, q) * q)
    return 1.06 * fill(tiles256) < fill(tm256 * _cdiv(sp.N, 128)) if sp.N % 256 == 0 else tiles256 < 1024


def split_k_takes(sp, lda, ldw):
    return (sp.out_f32 and not sp.bias and not sp.resid and sp.epi == 0 and not (sp.wscale or sp.w8) and sp.scale_cols == 0 and sp.patch_group == 0
            and sp.K % BK == 0 and sp.K >= 8192 and _cdiv(sp.M, 128) * _cdiv(sp.N, 128) <= 128 and _fits(sp.M, lda) and _fits(sp.N, ldw))


def split_k_slices(sp):
    tiles, nk = _cdiv(sp.M, 128) * _cdiv(sp.N, 128), sp.K // BK
    slices = min(max(512 // tiles, 2), 16)
    if slices > nk // 8:
        slices = nk // 8 if nk // 8 > 1 else 1
    k_slice = _cdiv(nk, slices)
    return _cdiv(nk, k_slice), k_slice


def _tiled(sp, shape, dbg, lda, ldw):
    fast = sp.K % BK == 0 and not (dbg & NO_DMA) and _fits(sp.M, lda) and _fits(sp.N, ldw)
    epi = sp.epi if sp.epi in (1, 2) else 0
    return (2000 if fast else 1000) + 10 * shape + epi


def _pp4(sp, dbg):
    if sp.a8 or sp.lnfold or sp.stats:
        if sp.a8 and sp.hm:
            return E_UNSUPPORTED, 0
        if sp.a8:
            return (E_UNSUPPORTED, 0) if sp.epi == 1 else (OK, 4040 + (2 if sp.epi == 2 else 0))
        if sp.hm and not hm_takes(sp, dbg):
            return E_UNSUPPORTED, 0
        if sp.epi == 2 or sp.out_f32 or (sp.lnfold and (sp.resid or sp.stats)) or (sp.stats and (not sp.resid or sp.epi != 0)):
            return E_UNSUPPORTED, 0
        lean = pp4_all_lean(sp, dbg)
        if sp.stats:
            return OK, 4220 if lean else 4200
        return OK, (4110 if lean else 4100) + (1 if sp.epi == 1 else 0)
    if pp4_all_lean(sp, dbg) and sp.epi != 1:
        if sp.epi == 0 and sp.K >= A3_MIN_K:
            return OK, 4030
        return OK, 4020 + (2 if sp.epi == 2 else 0)
    return OK, 4000 + (sp.epi if sp.epi in (1, 2) else 0)


def expected(sp: Spec, n_cu: int):
    """(return code, form) of launch_gemm on this spec, as build_case lays it out."""
    lda, ldw, ldr, ldc = _strides(sp)
    dbg = sp.flags
    M, N, K = sp.M, sp.N, sp.K
    if M <= 0:
        return OK, 0
    bits = 0
    if sp.a8:
        if K % 128 or sp.patch_group:
            return E_UNSUPPORTED, 0
        if not sp.out_f32 and (ldc % 8 or N % 4 or (sp.resid and ldr % 8)):
            return E_UNSUPPORTED, 0
        return _pp4(sp, dbg)
    if sp.w8:
        if K % 16:
            return E_BADARG, 0
        assert M > 32, "the fp8 weight stream of M <= 32 belongs to the skinny family"
        bits |= W8_EXPANDED
    if K % 8 or lda % 8 or ldw % 8:
        return E_UNSUPPORTED, 0
    if sp.hm and not hm_takes(sp, dbg):
        return E_UNSUPPORTED, 0
    ln_fold = sp.lnfold or sp.stats
    if ln_fold and (sp.w8 or sp.wscale or sp.out_f32 or sp.patch_group or sp.scale_cols or K % BK or not _fits(N, ldw)):
        return E_UNSUPPORTED, 0
    skinny = (M <= 16 or (M <= 32 and K % 256 == 0)) and sp.patch_group == 0 and not ln_fold
    assert not skinny, "the skinny family is not covered here"
    if not sp.out_f32 and (ldc % 8 or N % 4 or (sp.resid and ldr % 8)):
        return E_UNSUPPORTED, 0
    assert _fits(M, lda), "row-chunked launches keep their own test"
    if ln_fold:
        rc, form = _pp4(sp, dbg)
        return rc, (form | bits if rc == OK else 0)
    # launch_wide
    frc = (dbg >> FORCE_SHIFT) & 15
    no_dma = bool(dbg & NO_DMA)
    cfg = tile_cfg(sp)
    promoted = False
    ok6 = w6_ok(sp, lda, ldw, ldr, ldc)
    if cfg == 3 and K % BK == 0 and not (dbg & NO_WIDE):
        cfg, promoted = 1, True
    if cfg == 2 and ok6 and frc == 0 and not (dbg & (NO_WIDE | NO_W6 | NO_DMA)):
        cfg, promoted = 1, True
    if frc == FORCE_PP4:
        cfg = 1
    if frc in (FORCE_64x128, FORCE_128x128, FORCE_SPLIT_K):
        cfg = 4
    elif 1 <= frc <= 4:
        cfg = frc
    if ok6 and (frc == FORCE_W6 or (frc == 0 and cfg == 1 and w6_pick(sp, n_cu) and not (dbg & (NO_W6 | NO_DMA)))):
        return OK, bits | (5000 + (sp.epi if sp.epi in (1, 2) else 0))
    if cfg == 1:
        if not (promoted and dbg & WIDE_TILED) and frc in (0, FORCE_PP4) and not no_dma and K % BK == 0 and _fits(N, ldw):
            rc, form = _pp4(sp, dbg)
            return rc, (form | bits if rc == OK else 0)
        return OK, bits | _tiled(sp, 1, dbg, lda, ldw)
    if cfg == 3:
        return OK, bits | _tiled(sp, 3, dbg, lda, ldw)
    if cfg == 2:
        return OK, bits | _tiled(sp, 2, dbg, lda, ldw)
    if split_k_takes(sp, lda, ldw) and frc in (0, FORCE_SPLIT_K) and not no_dma:
        return OK, bits | (3000 + split_k_slices(sp)[0])
    t64 = _cdiv(M, 128) * _cdiv(N, 128) < 96 and M > 64
    if (frc == FORCE_64x128 or (frc == 0 and t64)) and M > 64 and not no_dma:
        return OK, bits | _tiled(sp, 5, dbg, lda, ldw)
    return OK, bits | _tiled(sp, 4, dbg, lda, ldw)


def form_name(form):
    if form == 0:
        return "none"
    low, out = form & 0xFFFF, ""
    fam, rest = low // 1000, low % 1000
    shapes = {1: "256x256", 2: "256x128", 3: "256x128-1stage", 4: "128x128", 5: "64x128"}
    if fam in (1, 2):
        out = f"{'nt' if fam == 1 else 'glds'}-{shapes[rest // 10]}-epi{rest % 10}"
    elif fam == 3:
        out = f"splitk-{rest}slices"
    elif fam == 4:
        inst = {0: "general", 1: "lean16", 2: "lean16ht", 3: "a3", 4: "f8"}[rest % 100 // 10]
        out = f"pp4-{('', 'lnfold-', 'stats-')[rest // 100]}{inst}-epi{rest % 10}"
    elif fam == 5:
        out = f"w6-epi{rest}"
    return out + ("+chunks" if form & ROW_CHUNKS else "") + ("+w8x" if form & W8_EXPANDED else "")


def family_of(form):
    """The row of the coverage table a form belongs to (what the parity record is keyed by)."""
    low = form & 0xFFFF
    fam, rest = low // 1000, low % 1000
    if fam in (1, 2):
        return ("nt-" if fam == 1 else "glds-") + {1: "256x256", 2: "256x128", 3: "256x128-1stage", 4: "128x128", 5: "64x128"}[rest // 10]
    if fam == 3:
        return "splitk"
    if fam == 5:
        return "w6"
    return "pp4-" + ("", "lnfold-", "stats-")[rest // 100] + {0: "general", 1: "lean16", 2: "lean16ht", 3: "a3", 4: "f8"}[rest % 100 // 10]


# ---- the launches of tests/test_hip_gemm_wide.py ---------------------------------------------------------------------------------------------

def _both(name, M, N, K, **kw):
    """The spec in both families (GELU: bounded only)."""
    out = [Spec(name + "-b", M, N, K, family="bounded", **kw)]
    if kw.get("epi", 0) != 1:
        out.append(Spec(name + "-x", M, N, K, family="exact", **kw))
    return out


def tiled_specs():
    """gemm_nt_kernel / gemm_glds_kernel, the four configurations (force 1-4) and 64 x 128 (force 13)."""
    S = []
    shapes = [(300, 200, 72), (257, 528, 176), (520, 1536, 128)]  # tails in M, N (N % 8 = 0, N % 128 != 0; 1536 % 256 = 0), K % 64 != 0 for nt
    for cfg in (1, 2, 3, 4):
        for i, (m, n, k) in enumerate(shapes):
            epi = (cfg + i) % 3
            S += _both(f"nt{cfg}-{m}x{n}x{k}", m, n, k, epi=epi, bias=(i != 1), resid=(i != 0), flags=NO_DMA | force(cfg))
            k64 = _cdiv(k, 64) * 64
            S += _both(f"glds{cfg}-{m}x{n}x{k64}", m, n, k64, epi=(epi + 1) % 3, bias=(i != 2), resid=(i != 1), flags=force(cfg))
        # the half column tile (N % 256 <= 128) and fp32 output
        S += _both(f"nt{cfg}-half", 260, 384, 136, epi=2, resid=True, flags=NO_DMA | force(cfg))
        S += _both(f"glds{cfg}-half", 260, 384, 128, epi=0, resid=True, flags=force(cfg))
        S += _both(f"glds{cfg}-half-off", 260, 384, 128, epi=0, resid=True, flags=force(cfg) | NO_HALF)
        S += _both(f"nt{cfg}-f32", 150, 202, 72, out_f32=True, bias=True, resid=True, flags=NO_DMA | force(cfg))
        S += _both(f"glds{cfg}-f32", 150, 202, 64, out_f32=True, epi=1, flags=force(cfg))
        S += _both(f"glds{cfg}-scale", 140, 264, 64, scale_cols=88, scale=0.125, flags=force(cfg))
    for m in (65, 64 + 128, 64 + 128 * 2 + 1, 130):
        S += _both(f"glds64-m{m}", m, 200, 128, epi=m % 3, resid=True, flags=force(FORCE_64x128))
    # t64x128_takes from both sides: 95 / 96 tiles of 128 x 128 (natural), M = 64 / 65
    S += _both("t64-96tiles", 129, 128 * 47 + 8, 64, bias=False)         # 2 x 48 = 96 tiles of 128 x 128 -> not taken ...
    S += _both("t64-94tiles", 129, 128 * 47, 64, bias=False)             # ... 2 x 47 = 94 -> 64 x 128
    S += _both("t64-m64", 64, 256, 64)                                    # M = 64 -> 128 x 128
    S += _both("t64-m65", 65, 256, 64)
    return S


def split_k_specs():
    S = []
    for m, n, k in ((100, 120, 8192), (128, 256, 8192), (200, 264, 8192 + 64 * 5), (700, 392, 8192 + 64 * 3)):
        S.append(Spec(f"splitk-{m}x{n}x{k}", m, n, k, bias=False, out_f32=True))
        S.append(Spec(f"splitk-{m}x{n}x{k}-b", m, n, k, bias=False, out_f32=True, family="bounded"))
    S.append(Spec("splitk-forced", 300, 200, 8192, bias=False, out_f32=True, flags=force(FORCE_SPLIT_K)))
    S.append(Spec("splitk-refused-by-bias", 100, 120, 8192, bias=True, out_f32=True))  # the predicate's other side: a per-tile kernel
    S.append(Spec("splitk-short-k", 100, 120, 8128, bias=False, out_f32=True))
    return S


def pp4_general_specs():
    S = []
    S += _both("pp4g-520x640x128", 520, 640, 128, epi=0, resid=True, flags=force(FORCE_PP4))            # N % 256 = 128: half tile; M tail
    S += _both("pp4g-1000x1408x256", 1000, 1408, 256, epi=1, resid=True, flags=force(FORCE_PP4))        # GELU + residual
    S += _both("pp4g-300x328x64", 300, 328, 64, epi=2, flags=force(FORCE_PP4))                          # N % 128 != 0, one K-step
    S += _both("pp4g-513x776x192", 513, 776, 192, epi=1, bias=False, flags=force(FORCE_PP4))            # odd step count
    S += _both("pp4g-260x520x128-f32", 260, 520, 128, out_f32=True, resid=True, flags=force(FORCE_PP4))
    S += _both("pp4g-scale", 300, 768, 128, scale_cols=256, scale=0.25, flags=force(FORCE_PP4))
    S += _both("pp4g-nohalf", 300, 640, 128, epi=2, resid=True, flags=force(FORCE_PP4) | NO_HALF)
    S += _both("pp4g-wscale", 300, 640, 128, wscale=True, flags=force(FORCE_PP4))
    return S


def smallest_m(n_cu, want, N, K, **kw):
    """The smallest row count (a multiple of 256) at which launch_gemm reaches the form `want` naturally (no probe flag) for this N, K and
    epilogue: the lean 16 x 16 instances need >= 256 tiles of 256 x 256 and a tile count that w6_pick leaves to the ping-pong kernel, both
    of which follow the device's CU count (256 CUs, N = 4096: M = 4096)."""
    for m in range(1024, 65537, 256):
        if expected(Spec("probe", m, N, K, **kw), n_cu) == (OK, want) and expected(Spec("probe", m - 19, N, K, **kw), n_cu) == (OK, want):
            return m
    raise AssertionError(("no natural route", want, N, K, kw))


def lean_specs(n_cu):
    """The product's 16 x 16 instances at dbg == 0: plain, ReLU, residual, an M tail, the q pre-scaling of a fused q|k|v projection (16 columns
    and N / 3), N = 256 n + 128 (a half tile; with scale_cols, which keeps the shape off w6 below 1024 tiles), A3 (K >= 5120) and K = 5056 just
    below it.  All in the exact family (a float32 BLAS product is the exact reference) but one bounded case."""
    S = []
    n = 4096
    for tag, want, kw in (("plain", 4020, {}), ("relu-resid", 4022, dict(epi=2, resid=True)), ("resid", 4020, dict(resid=True)),
                          ("scale16", 4020, dict(scale_cols=16, scale=0.125)), (f"scale{n // 3 // 16 * 16}", 4020, dict(scale_cols=n // 3 // 16 * 16, scale=0.125))):
        m = smallest_m(n_cu, want, n, 256, **kw)
        S.append(Spec(f"lean-{tag}-{m}x{n}", m, n, 256, **kw))
    m = smallest_m(n_cu, 4022, n, 256, epi=2)
    S.append(Spec(f"lean-tail-{m - 19}x{n}", m - 19, n, 256, epi=2))
    m = smallest_m(n_cu, 4020, 2048, 256)
    S.append(Spec(f"lean-nobias-{m}x2048", m, 2048, 256, bias=False))
    m = smallest_m(n_cu, 4020, 2048 + 128, 256, scale_cols=16, scale=0.125)
    S.append(Spec(f"lean-half-{m - 19}x2176", m - 19, 2048 + 128, 256, scale_cols=16, scale=0.125))
    m = smallest_m(n_cu, 4020, n, 256, resid=True, family="bounded")
    S.append(Spec(f"lean-bounded-{m - 19}x{n}", m - 19, n, 256, resid=True, family="bounded"))
    m = smallest_m(n_cu, 4030, n, 5120)
    S.append(Spec(f"a3-{m - 19}x{n}x5120", m - 19, n, 5120))
    S.append(Spec(f"a3-off-{m}x{n}x5056", m, n, 5056))
    return S


def w6_specs(n_cu):
    S = []
    for k in (256, 320):
        for m in (257, 256 + 37, 255):
            n = 128 if m == 255 else 1408 - 128 * (m % 3)
            S += _both(f"w6-{m}x{n}x{k}", m, n, k, epi=(m + k // 64) % 3, flags=force(FORCE_W6))
    S += _both("w6-resid", 300, 384, 256, epi=0, resid=True, flags=force(FORCE_W6))
    S += _both("w6-nobias", 513, 256, 384, epi=2, bias=False, flags=force(FORCE_W6))
    # residual + activation: w6_ok is false, the force is ignored and the shape's per-tile kernel runs
    S += _both("w6-refuses-resid-relu", 300, 384, 256, epi=2, resid=True, flags=force(FORCE_W6))
    S += _both("w6-refuses-k192", 300, 384, 192, flags=force(FORCE_W6))
    # natural: the smallest row count at N = 2048 that w6_pick takes
    for m in range(2048, 32769, 256):
        sp = Spec(f"w6-natural-{m}x2048", m - 5, 2048, 256, epi=2)
        if expected(sp, n_cu)[1] == 5002:
            S.append(sp)
            break
    return S


def lnfold_specs(n_cu):
    S = []
    S += _both("lnf-lean-300x384x128", 300, 384, 128, lnfold=True)                      # N % 128 = 0: 16 x 16 instance, half-valid last tile run whole
    S += _both("lnf-lean-gelu", 520, 512, 192, lnfold=True, epi=1)
    S += _both("lnf-general-300x328x128", 300, 328, 128, lnfold=True)                    # N % 128 != 0: 32 x 32 instance
    S += _both("lnf-general-gelu-half", 513, 392, 256, lnfold=True, epi=1)
    S += _both("lnf-hm", 257 * 2, 3 * 16 * 88, 128, lnfold=True, hm=(257, 16, 88))
    S += _both("lnf-hm-tok129", 129 * 3, 3 * 16 * 72, 64, lnfold=True, hm=(129, 16, 72))  # every wave's 128 rows cross a frame boundary
    return S


def stats_specs(n_cu):
    S = []
    for m, n, k in ((300, 1408, 128), (520, 192, 64), (260, 1280, 192), (130, 200, 64)):
        S.append(Spec(f"stats-{m}x{n}x{k}-x", m, n, k, stats=True, resid=True))
        S.append(Spec(f"stats-{m}x{n}x{k}-b", m, n, k, stats=True, resid=True, family="bounded", resid_gain=8.0))
    return S


def a8_specs():
    S = []
    for m, n, k, epi, f32 in ((300, 512, 128, 0, False), (130, 200, 384, 2, False), (513, 392, 128, 0, True), (40, 384, 128, 2, True),
                              (260, 640, 256, 0, False)):
        S += _both(f"a8-{m}x{n}x{k}", m, n, k, a8=True, epi=epi, out_f32=f32, resid=(epi == 0))
    return S


def patch_specs():
    S = []
    for group, frames in ((256, 1), (256, 3), (16, 1), (16, 3)):
        m = group * frames
        S += _both(f"patch-g{group}-f{frames}-nt", m, 200, 72, patch_group=group, resid=True, flags=NO_DMA)
        S += _both(f"patch-g{group}-f{frames}-glds", m, 264, 128, patch_group=group, resid=True)
    S += _both("patch-pp4", 768, 640, 128, patch_group=256, resid=True, flags=force(FORCE_PP4))
    return S


def ln_out_specs():
    return [Spec("lnout-ln", 300, 264, 128, ln_out=1, family="bounded", resid=True),
            Spec("lnout-rms", 130, 512, 64, ln_out=2, family="bounded", bias=False),
            Spec("lnout-rms-w6", 300, 384, 256, ln_out=2, family="bounded", bias=False, flags=force(FORCE_W6)),
            Spec("lnout-ln-x", 70, 136, 64, ln_out=1, family="exact")]


def w8_specs():
    return [Spec("w8x-300x264x128", 300, 264, 128, w8=True, family="bounded"),
            Spec("w8x-130x384x256-x", 130, 384, 256, w8=True, family="exact", epi=2)]


def route_specs(n_cu):
    return (tiled_specs() + split_k_specs() + pp4_general_specs() + lean_specs(n_cu) + w6_specs(n_cu) + lnfold_specs(n_cu) + stats_specs(n_cu)
            + a8_specs() + patch_specs() + ln_out_specs() + w8_specs())


# forms the table of the issue asks for, by family_of(): every one must be reached by route_specs on any CU count
REQUIRED = (["nt-" + s for s in ("256x256", "256x128", "256x128-1stage", "128x128")]
            + ["glds-" + s for s in ("256x256", "256x128", "256x128-1stage", "128x128", "64x128")]
            + ["splitk", "w6", "pp4-general", "pp4-lean16ht", "pp4-a3", "pp4-lnfold-lean16", "pp4-lnfold-general", "pp4-stats-lean16ht",
               "pp4-stats-general", "pp4-f8"])
