"""Cases, float64 reference, per-element bound and expected route of the M <= 8 row-dot decode kernels of csrc/gemv.hip (gemv_rows_kernel,
gemv1_kernel, gemvm_kernel, each with the plain, LayerNorm and flash-decoding-merge prologue).  CPU only, numpy.

A GSpec names ONE call of a launcher (0 launch_gemv_rows, 1 launch_gemv1, 2 launch_gemvm) field by field plus the grid override of the probe
build (eilev_debug_grid_cus, which launch_gemv1 / launch_gemvm follow).  build_case makes its operands with guards, reference evaluates it in
float64, tol gives the bound every output element is held to, expected names the return code and the kernel instance, route_specs lists the
launches of tests/test_hip_gemv.py.  tests/test_gemv_reference.py checks all of this on the CPU and measures what planted mistakes cost.

Guards (build_case): x has ldx = K + 8 (launcher 1 passes no stride: K) with +-2^14 traps in the padding and in two rows after row M - 1; the
same for a residual that is not in place (ldr = N + 16); W is dense (the kernels have no ldw) with two trap rows behind row N - 1; bias has
eight trap elements behind N; out has ldo = N + 8 (launcher 1: N) and two guard rows, all on the NaN sentinel.  An IN-PLACE residual (what
every product call passes: b.h as residual and output) IS the out buffer: ldr == ldo, its padding and guard rows hold the residual's traps
and must come back bit for bit.  The merge partials are (M, heads, nsplit, hd + 2) floats [max, sum, o[hd]]; every o word of an empty range
(sum == 0) holds NaN bits, empty ranges stand at the front, in the middle and at the end, `dead_row` empties every range of the last row
(its output is bias + residual alone).  Empty ranges carry max = -1e30 as attn_decode_part_kernel writes it, except the middle ones, which
carry a STALE finite maximum inside the window of the live ones: a merge that weighs a range by its maximum alone must not pass.

Families: "exact" — x and W in {-1, 0, 1} thinned so that results stay below 2^6, integer bias / residual, scale 2^-3: every partial sum is
exact in fp32 in any order and every result is a bf16 value, so a kernel must match BIT FOR BIT.  For the merge prologue every live range
shares one maximum (weights __expf(0) = 1), the sums add up to 4 and the o_s are small integers with sum o = 4 x.  PRO_LN has no exact family.
"bounded" — dense normals with, per 512-chunk c, one outlier channel k_out(c) (x = 12, w = +-16 / sqrt(K), the sign per output row), bias
+-1.5 alternating by column and residual +-2 alternating by row under the noise: a dropped 8-element slice, a neighbour's bias or a
neighbour's residual row then moves an element by far more than the bound, however the noise falls (test_gemv_reference.py measures it).
LayerNorm rows have mean 3 and the same outliers.

tol, per element, no floor and no max|ref| term:
  output rounding    half a unit of the output format at y (gemm_ref.half_ulp: bf16 8 bits, fp32 24)
  fp32 accumulation  ACC_C * n_adds * 2^-24 * S_ij, S_ij = sum_k |x_ik w_jk| (scaled like y), n_adds = K + 8: K products, 6 steps of the lane
                     tree, + bias, + residual (the scale is a power of two).  ACC_C = gemm_ref.ACC_C.
  staged activation  sum_k |w_jk| d_ik: d = 0 (PRO_X); the LayerNorm bound of gemm_ref.ln_out_ref with K columns, which contains the half
                     bf16 unit of the staging (PRO_LN); half a bf16 unit at the merged value + e_m sum_s w_s |o_s| / l (PRO_MERGE),
                     e_m = (2 nsplit + 8) 2^-24 + EXPF_TERM: nsplit products and additions above and below the division, the division, and
                     __expf of an argument in [-8, 0] (one unit of v_exp_f32 plus the rounding of d log2(e): 8 * 1.4427 * 2^-24 < 2^-20).
                     build_case asserts the window of 8."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace  # noqa: F401
from types import SimpleNamespace

import numpy as np

import gemm_ref as R
from attn_decode_ref import merge_ref
from gemm_ref import OK, E_BADARG, E_UNSUPPORTED, SENT16, TRAP, _ints, _ternary, bf16_bits, half_ulp, ratio  # noqa: F401
from eilev_amd.synth import det_normal, round_bf16

PRO_X, PRO_LN, PRO_MERGE = 0, 1, 2
ROWS, GEMV1, GEMVM = 0, 1, 2
PRO_NAME = {PRO_X: "x", PRO_LN: "ln", PRO_MERGE: "merge"}
SENT32 = (SENT16 << 16) | SENT16
EXPF_TERM = 2.0 ** -20   # __expf on [-8, 0] (module docstring); widened only to twice a device measurement of __expf against float64 exp
EMPTY_MAX = -1e30        # what attn_decode_part_kernel stores as the maximum of an empty range
STALE_O = 1000.0         # the finite stale o of the merge mistakes planted by test_gemv_reference.py (the device cases hold NaN bits)


@dataclass(frozen=True)
class GSpec:
    name: str
    launcher: int
    pro: int
    M: int
    N: int
    K: int
    epi: int = 0              # 0 none, 2 ReLU
    bias: bool = True
    resid: int = 0            # 0 none, 1 its own buffer (ldr = N + 16), 2 in place (the out buffer, ldr == ldo)
    out_f32: bool = False
    scale_cols: int = 0
    scale: float = 1.0
    family: str = "exact"
    grid: int = 0             # eilev_debug_grid_cus (launchers 1 and 2)
    heads: int = 0            # PRO_MERGE: heads * hd == K
    hd: int = 0
    nsplit: int = 0
    dead_row: bool = False    # PRO_MERGE: every range of row M - 1 is empty
    seed: int = 0


@dataclass
class Case:
    spec: GSpec
    ldx: int
    ldr: int
    ldo: int
    x_buf: np.ndarray = None      # float32 (M + 2, ldx), bf16-exact (None for PRO_MERGE)
    W_buf: np.ndarray = None      # float32 (N + 2, K)
    bias: np.ndarray = None       # float32 (N + 8)
    resid_buf: np.ndarray = None  # float32 (M + 2, ldr); in place: the initial content of out
    gamma: np.ndarray = None
    beta: np.ndarray = None
    part: np.ndarray = None       # float32 (M, heads, nsplit, hd + 2)
    live: np.ndarray = None       # bool (M, heads, nsplit)
    eps: float = 1e-5

    @property
    def x(self):
        return self.x_buf[:self.spec.M, :self.spec.K]

    @property
    def W(self):
        return self.W_buf[:self.spec.N]

    @property
    def resid(self):
        return None if self.resid_buf is None else self.resid_buf[:self.spec.M, :self.spec.N]


def strides(sp):
    """(ldx, ldr, ldo).  launch_gemv1 takes no strides (one row)."""
    if sp.launcher == GEMV1:
        return sp.K, sp.N, sp.N
    ldo = sp.N + 8
    return sp.K + 8, (ldo if sp.resid == 2 else sp.N + 16), ldo


def k_out(K):
    """The outlier channel of every 512-chunk c: lane (11 c + 5) % 64, element c % 8."""
    c = np.arange(K // 512)
    return c * 512 + 8 * ((11 * c + 5) % 64) + c % 8


def row_sign(N):
    n = np.arange(N)
    return np.where((n * 7) % 3 == 0, -1.0, 1.0).astype(np.float32)


def empty_ranges(h, ns):
    """The empty ranges of head h: none / front / middle / end by h % 4 (front: two ranges when nsplit >= 5).  One range stays live."""
    kind = h % 4
    if ns < 2 or kind == 0:
        return []
    if kind == 1:
        return [0, 1] if ns >= 5 else [0]
    if kind == 2:
        return [ns // 2]
    return [ns - 1]


def stale_max_ranges(h, ns):
    """Empty ranges that hold a stale finite maximum: the middle ones."""
    return [ns // 2] if ns >= 2 and h % 4 == 2 else []


def _build_part(sp, rng, exact):
    M, H, ns, hd, K = sp.M, sp.heads, sp.nsplit, sp.hd, sp.K
    assert H * hd == K and hd % 8 == 0 and ns >= 1
    part = np.zeros((M, H, ns, hd + 2), np.float32)
    live = np.ones((M, H, ns), bool)
    for h in range(H):
        live[:, h, empty_ranges(h, ns)] = False
    if sp.dead_row:
        live[M - 1] = False
    ko = k_out(K)
    if exact:
        d = min(0.5, math.sqrt(12.0 / K))
        target = _ternary(rng, (M, K), d)
        target[:, ko] = 1.0
        target = target.reshape(M, H, hd)
        mx = np.full((M, H, ns), 1.5, np.float32)
        for m in range(M):
            for h in range(H):
                idx = np.flatnonzero(live[m, h])
                if not idx.size:
                    continue
                part[m, h, idx, 1] = 0.5
                part[m, h, idx[-1], 1] = 4.0 - 0.5 * (idx.size - 1)
                o = _ints(rng, (idx.size, hd), -3, 3)
                o[-1] = 4.0 * target[m, h] - o[:-1].sum(0)
                part[m, h, idx, 2:] = o
    else:
        mx = (8.0 * rng.random((M, H, ns)) - 4.0).astype(np.float32)
        l = (1.0 + 39.0 * rng.random((M, H, ns))).astype(np.float32)
        v = det_normal(f"gv-part{sp.seed}", (M, ns, K), sp.seed)
        v[:, :, ko] = 12.0
        v = v.reshape(M, ns, H, hd).transpose(0, 2, 1, 3)
        part[..., 1] = l
        part[..., 2:] = l[..., None] * v
    part[..., 0] = mx
    stale = np.zeros((M, H, ns), bool)
    for h in range(H):
        stale[:, h, stale_max_ranges(h, ns)] = True
    part[..., 0] = np.where(live | stale, part[..., 0], np.float32(EMPTY_MAX))
    part[..., 1] = np.where(live, part[..., 1], np.float32(0.0))
    nan32 = np.array([SENT32], np.uint32).view(np.float32)[0]
    part[..., 2:] = np.where(live[..., None], part[..., 2:], nan32)
    finite = part[..., 0] > -1e29
    if finite.any():
        assert part[..., 0][finite].max() - part[..., 0][finite].min() <= 8.0, "the range maxima must lie within a window of 8 (EXPF_TERM)"
    return part, live


def build_case(sp: GSpec) -> Case:
    M, N, K = sp.M, sp.N, sp.K
    ldx, ldr, ldo = strides(sp)
    exact = sp.family == "exact"
    assert not (exact and sp.pro == PRO_LN), "PRO_LN has no exact family"
    assert not (sp.resid == 2 and sp.out_f32), "a bf16 residual cannot be an fp32 output"
    assert K % 512 == 0 and K >= 512
    rng = np.random.default_rng([sp.seed, M, N, K, sp.pro, sp.launcher, int(exact)])
    c = Case(sp, ldx, ldr, ldo)
    ko, sgn = k_out(K), row_sign(N)
    W_buf = np.zeros((N + 2, K), np.float32)
    d = min(0.5, math.sqrt(12.0 / K))
    if exact:
        W_buf[:N] = _ternary(rng, (N, K), d)
        W_buf[:N, ko] = sgn[:, None]
    else:
        w = det_normal(f"gv-W{sp.seed}", (N, K), sp.seed) / np.sqrt(K)
        w[:, ko] = sgn[:, None] * 16.0 / np.sqrt(K)
        W_buf[:N] = round_bf16(w.astype(np.float32))
    R._trap_fill(W_buf, N, K, 1)
    c.W_buf = W_buf
    if sp.pro == PRO_MERGE:
        c.part, c.live = _build_part(sp, rng, exact)
    else:
        x_buf = np.zeros((M + 2, ldx), np.float32)
        if exact:
            x_buf[:M, :K] = _ternary(rng, (M, K), d)
            x_buf[:M, ko] = 1.0
        else:
            a = det_normal(f"gv-x{sp.seed}", (M, K), sp.seed)
            if sp.pro == PRO_LN:  # a raw residual stream: a large row mean
                a = a + 3.0 + 0.5 * det_normal("gv-rowmean", (M, 1), sp.seed)
                a[:, ko] += 12.0
            else:
                a[:, ko] = 12.0
            x_buf[:M, :K] = round_bf16(a.astype(np.float32))
        R._trap_fill(x_buf, M, K, 0)
        c.x_buf = x_buf
    if sp.pro == PRO_LN:
        c.gamma = round_bf16(1.0 + 0.1 * det_normal("gv-g", (K,), sp.seed))
        c.beta = round_bf16(0.1 * det_normal("gv-be", (K,), sp.seed))
    if sp.bias:
        b = np.full(N + 8, TRAP, np.float32)
        b[:N] = _ints(rng, N, -8, 8) if exact else round_bf16((1.5 * (1 - 2 * (np.arange(N) % 2)) + 0.5 * det_normal("gv-b", (N,), sp.seed)).astype(np.float32))
        c.bias = b
    if sp.resid:
        r = np.zeros((M + 2, ldr), np.float32)
        alt = (2.0 * (1 - 2 * (np.arange(M) % 2)))[:, None]
        r[:M, :N] = _ints(rng, (M, N), -16, 16) if exact else round_bf16((alt + det_normal("gv-r", (M, N), sp.seed)).astype(np.float32))
        R._trap_fill(r, M, N, 2)
        c.resid_buf = r
    return c


# ---- reference -------------------------------------------------------------------------------------------------------------------------------

def merged_x(c: Case):
    """(x, d) of the merge prologue in float64: the merged rows (attn_decode_ref.merge_ref) and the bound of their staged bf16 values."""
    sp = c.spec
    x = merge_ref(c.part)
    with np.errstate(invalid="ignore"):
        p = np.asarray(c.part, np.float64)
    live = c.live
    mx, l = p[..., 0], p[..., 1]
    m = np.where(live, mx, -np.inf).max(-1, keepdims=True)
    w = np.where(live, np.exp(np.where(live, mx, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
    lsum = (w * np.where(live, l, 0.0)).sum(-1)
    oabs = (w[..., None] * np.where(live[..., None], np.abs(p[..., 2:]), 0.0)).sum(-2)
    mag = np.where(lsum[..., None] > 0, oabs / np.where(lsum > 0, lsum, 1.0)[..., None], 0.0).reshape(sp.M, sp.K)
    e_m = (2 * sp.nsplit + 8) * 2.0 ** -24 + EXPF_TERM
    return x, half_ulp(x, 8) + e_m * mag


def ln_x(c: Case):
    """(x, d) of the LayerNorm prologue: gemm_ref.ln_out_ref on K columns."""
    sp = c.spec
    shim = SimpleNamespace(spec=SimpleNamespace(N=sp.K, ln_out=1), gamma=c.gamma, beta=c.beta, ln_eps=c.eps)
    return R.ln_out_ref(shim, c.x.astype(np.float64))


def prologue(c: Case):
    sp = c.spec
    if sp.pro == PRO_LN:
        return ln_x(c)
    if sp.pro == PRO_MERGE:
        return merged_x(c)
    return c.x.astype(np.float64), np.zeros((sp.M, sp.K))


def reference(c: Case):
    """(y, S, D) in float64 on the logical [M, N] output: the value, sum_k |x_ik w_jk| and sum_k |w_jk| d_ik, both scaled like y."""
    sp = c.spec
    x, d = prologue(c)
    W = c.W.astype(np.float64)
    y, S, D = x @ W.T, np.abs(x) @ np.abs(W).T, d @ np.abs(W).T
    if c.bias is not None:
        y = y + c.bias[:sp.N].astype(np.float64)[None, :]
    if sp.scale_cols:
        y[:, :sp.scale_cols] *= sp.scale
        S[:, :sp.scale_cols] *= abs(sp.scale)
        D[:, :sp.scale_cols] *= abs(sp.scale)
    if sp.epi == 2:
        y = np.maximum(y, 0.0)
    if c.resid is not None:
        y = y + c.resid.astype(np.float64)
    return y, S, D


def n_adds(sp):
    """fp32 additions that reach one output: K products, 6 steps of the lane tree, + bias, + residual."""
    return sp.K + 6 + 2


def tol(c: Case, y, S, D):
    sp = c.spec
    return half_ulp(y, 24 if sp.out_f32 else 8) + R.ACC_C * n_adds(sp) * 2.0 ** -24 * S + D


# ---- the route: a mirror of launch_gemv_rows / launch_gemv1 / launch_gemvm ---------------------------------------------------------------------

def instance(tmpl, mr, geo, pro, lng=0):
    """GEMV_INSTANCE of csrc/gemv.hip."""
    return tmpl * 100000 + mr * 10000 + geo * 100 + pro * 10 + lng


def gemv_rows_ok(M, N, K):
    return 1 <= M <= 8 and K % 512 == 0 and K >= 512 and N >= 1 and M * K * 2 <= 150 * 1024


def gemv1_ok(N, K, pro):
    nch = K >> 9
    if K % 512 or N < 1:
        return False
    if pro == PRO_LN:
        return nch == 5
    return pro == PRO_X and nch in (5, 8, 20)


def gemvm_ok(M, N, K, pro):
    if M < 2 or M > 8 or K % 512 or N < 1 or M * K * 2 > 150 * 1024:
        return False
    return (K >> 9) == 5 and pro in (PRO_X, PRO_LN)


def eff_cus(sp, n_cu):
    return sp.grid if 0 < sp.grid < n_cu else n_cu


def rows_cps(K):
    nch = K >> 9
    return 8 if nch % 8 == 0 else 5 if nch % 5 == 0 else 1


def ring(sp):
    """(SB, IPR, RB) of gemv1_kernel / gemvm_kernel for this launch."""
    nch = sp.K >> 9
    if sp.launcher == GEMVM:
        return 5, nch // 5, (4 if sp.pro == PRO_LN or sp.M >= 3 else 8)
    sb = 5 if nch % 5 == 0 else 8
    ipr = nch // sb
    ln = sp.pro == PRO_LN
    rb = ((4 if ln else 8) if sb == 5 else (2 if ln else 4)) if ipr == 1 else 4
    return sb, ipr, rb


def geometry(sp, n_cu):
    """(grid, rows_per_wave, KB): what the launcher puts into GemvArgs."""
    if sp.launcher == ROWS:
        rpw = max(2, -(-sp.N // 2048))
        return -(-sp.N // (4 * rpw)), rpw, sp.K
    grid = eff_cus(sp, n_cu)
    if grid * 5 > sp.N:
        grid = (sp.N + 4) // 5
    return grid, sp.N // (grid * 5), sp.N % (grid * 5)


def deal(sp, n_cu):
    """[(r0, r1)] per wave, as the kernels compute it (gemv_rows_kernel: clamped to N)."""
    grid, rpw, kb = geometry(sp, n_cu)
    if sp.launcher == ROWS:
        return [(min(w * rpw, sp.N), min((w + 1) * rpw, sp.N)) for w in range(grid * 4)]
    out = []
    for w in range(grid * 5):
        r0 = w * rpw + min(w, kb)
        out.append((r0, r0 + rpw + (1 if w < kb else 0)))
    return out


def expected(sp, n_cu):
    """(return code, instance) of eilev_debug_gemv on this spec, as build_case lays it out (aligned, non-null operands)."""
    M, N, K, pro = sp.M, sp.N, sp.K, sp.pro
    paired = (sp.bias or sp.resid) and N % 2 == 1
    if sp.launcher == ROWS:
        if not gemv_rows_ok(M, N, K):
            return E_UNSUPPORTED, 0
        if pro == PRO_MERGE and (sp.heads * sp.hd != K or sp.hd % 8):
            return E_BADARG, 0
        if pro == PRO_LN and K > 4096:
            return E_UNSUPPORTED, 0
        if pro == PRO_MERGE and M > 2:
            return E_UNSUPPORTED, 0
        return OK, instance(1, M, rows_cps(K), pro)
    if sp.launcher == GEMV1:
        if M != 1:
            return E_BADARG, 0
        if pro == PRO_MERGE:
            if not 1 <= sp.nsplit <= 8 or sp.heads * sp.hd != K or sp.hd % 8 or (K >> 9) != 5 or K % 512:
                return E_UNSUPPORTED, 0
        elif not gemv1_ok(N, K, pro):
            return E_UNSUPPORTED, 0
        if N < 1 or paired:
            return E_UNSUPPORTED, 0
        return OK, instance(2, 1, K >> 9, pro)
    if not gemvm_ok(M, N, K, pro) or paired:
        return E_UNSUPPORTED, 0
    _, ipr, rb = ring(sp)
    return OK, instance(3, M, K >> 9, pro, int(geometry(sp, n_cu)[1] * ipr >= 2 * rb))


def instance_name(code):
    if code == 0:
        return "none"
    tmpl, mr, geo, pro, lng = code // 100000, code // 10000 % 10, code // 100 % 100, code // 10 % 10, code % 10
    if tmpl == 1:
        return f"rows-{PRO_NAME[pro]}-m{mr}-cps{geo}"
    if tmpl == 2:
        return f"gemv1-{PRO_NAME[pro]}-{geo}"
    return f"gemvm-{PRO_NAME[pro]}-m{mr}-{'long' if lng else 'short'}"


def families(sp, n_cu):
    """The coverage keys of one launch: its instance, and for gemv1_kernel the run-time paths its waves take (short / long waves, the 64-row
    flush, zero-row waves)."""
    rc, code = expected(sp, n_cu)
    if rc != OK:
        return []
    name = instance_name(code)
    if sp.launcher != GEMV1:
        return [name]
    _, ipr, rb = ring(sp)
    rows = [r1 - r0 for r0, r1 in deal(sp, n_cu)]
    out = []
    if any(0 < r * ipr < 2 * rb for r in rows):
        out.append(name + "-short")
    if any(r * ipr >= 2 * rb for r in rows):
        out.append(name + "-long")
    if any(r > 64 for r in rows):
        out.append(name + "-flush64")
    if any(r == 0 for r in rows):
        out.append(name + "-zero")
    return out


REQUIRED = ([f"rows-x-m{m}-cps{c}" for m in range(1, 9) for c in (1, 5, 8)] + [f"rows-ln-m{m}-cps{c}" for m in (1, 4, 5, 8) for c in (1, 5, 8)]
            + [f"rows-merge-m{m}-cps{c}" for m in (1, 2) for c in (1, 5)]
            + [f"gemv1-x-{g}-{p}" for g in (5, 8, 20) for p in ("short", "long")] + ["gemv1-x-5-flush64", "gemv1-x-5-zero"]
            + ["gemv1-ln-5-short", "gemv1-ln-5-long", "gemv1-merge-5-short", "gemv1-merge-5-long", "gemv1-merge-5-zero"]
            + [f"gemvm-{p}-m{m}-{l}" for p in ("x", "ln") for m in range(2, 9) for l in ("short", "long")])


# ---- the launches of tests/test_hip_gemv.py ----------------------------------------------------------------------------------------------------

def both(name, launcher, pro, M, N, K, **kw):
    out = [GSpec(name + "-b", launcher, pro, M, N, K, family="bounded", **kw)]
    if pro != PRO_LN:
        out.append(GSpec(name + "-x", launcher, pro, M, N, K, family="exact", **kw))
    return out


def _epilogue(i, N, f32_ok=True):
    """A rotation of epilogues by case number: fp32 / bf16, ReLU, no / own / in-place residual, q scaling."""
    kw = [dict(resid=2), dict(epi=2, resid=1), dict(out_f32=True, resid=1), dict(scale_cols=N // 3, scale=0.125), dict(epi=2, resid=2),
          dict(out_f32=True, epi=2, bias=False), dict(resid=2, scale_cols=N, scale=0.125), dict(bias=False, resid=1)][i % 8]
    if not f32_ok and kw.get("out_f32"):
        kw = dict(resid=2)
    return kw


def rows_x_specs():
    S = []
    for m in range(1, 9):
        for j, K in enumerate((512, 1024, 2560, 4096, 5120)):
            S += both(f"rows-x-{m}x40x{K}", ROWS, PRO_X, m, 40, K, **_epilogue(m + j, 40))
    S += both("rows-x-3x1001x512", ROWS, PRO_X, 3, 1001, 512, epi=2, resid=2)      # ragged: the clamped weight row of the last wave
    S += both("rows-x-8x1001x512", ROWS, PRO_X, 8, 1001, 512, out_f32=True, resid=1)
    S += both("rows-x-2x6x512", ROWS, PRO_X, 2, 6, 512, resid=2)                   # one workgroup, three waves out of range
    S += both("rows-x-7x6x512", ROWS, PRO_X, 7, 6, 512, epi=2)
    S += both("rows-x-1x4100x512", ROWS, PRO_X, 1, 4100, 512, resid=2)             # rows_per_wave = 3
    S += both("rows-x-6x4100x512", ROWS, PRO_X, 6, 4100, 512, epi=2, resid=1)
    for sc in (0, 1, 13, 40):
        S += both(f"rows-x-2x40x512-scale{sc}", ROWS, PRO_X, 2, 40, 512, scale_cols=sc, scale=0.125)
    return S


def rows_ln_specs():
    S = []
    for i, m in enumerate((1, 4, 5, 8)):  # M >= 5: the second row pass of a wave
        for j, K in enumerate((512, 2560, 4096)):
            S += both(f"rows-ln-{m}x40x{K}", ROWS, PRO_LN, m, 40, K, **_epilogue(i + j, 40))
    S += both("rows-ln-5x1001x512", ROWS, PRO_LN, 5, 1001, 512, out_f32=True)
    return S


def rows_merge_specs():
    S = []
    for m in (1, 2):
        for heads, hd in ((32, 80), (8, 64)):
            for ns in (1, 3, 8):
                S += both(f"rows-merge-{m}x40-{heads}x{hd}-ns{ns}", ROWS, PRO_MERGE, m, 40, heads * hd, heads=heads, hd=hd, nsplit=ns,
                          dead_row=(m == 2), resid=2 if ns != 3 else 1, epi=2 if ns == 8 else 0)
    S += both("rows-merge-1x40-dead", ROWS, PRO_MERGE, 1, 40, 2560, heads=32, hd=80, nsplit=3, dead_row=True, resid=2)
    return S


G = 8  # the grid override of the gemv1 / gemvm cases: 40 waves


def gemv1_x_specs():
    S = []
    for i, n in enumerate((12, 126, 640, 40 * 17 + 22, 40 * 23 + 10, 2650)):
        # clamped grid with zero-row waves; short uneven; exactly 2 RB; long with a tail of 1 and 2 items; a tail of RB - 1; the 64-row flush
        S += both(f"gemv1-x-{n}x2560", GEMV1, PRO_X, 1, n, 2560, grid=G, **_epilogue(i, n))
    S += both("gemv1-x-126x4096", GEMV1, PRO_X, 1, 126, 4096, grid=G, resid=2)
    S += both("gemv1-x-366x4096", GEMV1, PRO_X, 1, 366, 4096, grid=G, epi=2, resid=1)       # 9 and 10 rows: long (RB 4)
    S += both("gemv1-x-46x10240", GEMV1, PRO_X, 1, 46, 10240, grid=G, resid=2)              # IPR = 4: one row short, two rows long
    S += both("gemv1-x-126x10240", GEMV1, PRO_X, 1, 126, 10240, grid=G, out_f32=True)
    return S


def gemv1_ln_specs():
    S = []
    S += both("gemv1-ln-126x2560", GEMV1, PRO_LN, 1, 126, 2560, grid=G, epi=2)                 # short: 3 and 4 rows
    S += both("gemv1-ln-320x2560", GEMV1, PRO_LN, 1, 320, 2560, grid=G, resid=2)               # exactly 2 RB
    S += both("gemv1-ln-382x2560", GEMV1, PRO_LN, 1, 382, 2560, grid=G, resid=1)               # 9 and 10 rows: tails of 1 and 2
    S += both("gemv1-ln-450x2560-f32", GEMV1, PRO_LN, 1, 450, 2560, grid=G, out_f32=True, bias=False)   # the lm_head form; tails of 3 and 0
    S += both("gemv1-ln-384x2560-q", GEMV1, PRO_LN, 1, 384, 2560, grid=G, scale_cols=128, scale=0.125)  # q|k|v
    return S


def gemv1_merge_specs():
    S = []
    for ns in (1, 2, 5, 8):
        S += both(f"gemv1-merge-126-ns{ns}", GEMV1, PRO_MERGE, 1, 126, 2560, grid=G, heads=32, hd=80, nsplit=ns, resid=2)
    S += both("gemv1-merge-12-ns5", GEMV1, PRO_MERGE, 1, 12, 2560, grid=G, heads=32, hd=80, nsplit=5, resid=1)   # zero-row waves meet the barrier
    S += both("gemv1-merge-702-ns8", GEMV1, PRO_MERGE, 1, 702, 2560, grid=G, heads=32, hd=80, nsplit=8, resid=2)
    S += both("gemv1-merge-126-dead", GEMV1, PRO_MERGE, 1, 126, 2560, grid=G, heads=32, hd=80, nsplit=5, dead_row=True, resid=2)
    S += both("gemv1-merge-126-40x64", GEMV1, PRO_MERGE, 1, 126, 2560, grid=G, heads=40, hd=64, nsplit=3, epi=2)
    return S


def gemv1_natural_specs():
    return (both("gemv1-x-natural", GEMV1, PRO_X, 1, 2560, 2560, resid=2) + both("gemv1-ln-natural", GEMV1, PRO_LN, 1, 2560, 2560, epi=2)
            + both("gemv1-merge-natural", GEMV1, PRO_MERGE, 1, 2560, 2560, heads=32, hd=80, nsplit=8, resid=2))


def gemvm_specs():
    S = []
    for pro in (PRO_X, PRO_LN):
        for m in range(2, 9):
            rb = 4 if pro == PRO_LN or m >= 3 else 8
            tag = PRO_NAME[pro]
            below, at = 40 * 2 * rb - 2, 40 * 2 * rb  # rows_per_wave = 2 RB - 1 with 38 waves of 2 RB rows (short form) / 2 RB (long form)
            S += both(f"gemvm-{tag}-{m}x{below}", GEMVM, pro, m, below, 2560, grid=G, **_epilogue(m, below))
            S += both(f"gemvm-{tag}-{m}x{at}", GEMVM, pro, m, at, 2560, grid=G, **_epilogue(m + 3, at))
            S += both(f"gemvm-{tag}-{m}x{at + 22}", GEMVM, pro, m, at + 22, 2560, grid=G, **_epilogue(m + 5, at + 22))  # long, uneven: tails of 0 and 1
        S += both(f"gemvm-{PRO_NAME[pro]}-5x12", GEMVM, pro, 5, 12, 2560, grid=G, resid=2)        # clamped grid, zero-row waves
        S += both(f"gemvm-{PRO_NAME[pro]}-3x126", GEMVM, pro, 3, 126, 2560, grid=G, epi=2, resid=1)
    return S


def refused_specs():
    """(spec, return code): refused before anything runs."""
    return [(GSpec("refuse-rows-ln-4608", ROWS, PRO_LN, 2, 40, 4608, family="bounded"), E_UNSUPPORTED),
            (GSpec("refuse-rows-merge-m3", ROWS, PRO_MERGE, 3, 40, 512, heads=8, hd=64, nsplit=3), E_UNSUPPORTED),
            (GSpec("refuse-rows-8x10240", ROWS, PRO_X, 8, 40, 10240), E_UNSUPPORTED),
            (GSpec("refuse-gemv1-ns9", GEMV1, PRO_MERGE, 1, 126, 2560, grid=G, heads=32, hd=80, nsplit=9), E_UNSUPPORTED),
            (GSpec("refuse-gemv1-ln-4096", GEMV1, PRO_LN, 1, 126, 4096, grid=G, family="bounded"), E_UNSUPPORTED),
            (GSpec("refuse-gemv1-odd-bias", GEMV1, PRO_X, 1, 127, 2560, grid=G), E_UNSUPPORTED),
            (GSpec("refuse-gemv1-odd-resid", GEMV1, PRO_X, 1, 127, 2560, grid=G, bias=False, resid=2), E_UNSUPPORTED),
            (GSpec("refuse-gemv1-odd-merge", GEMV1, PRO_MERGE, 1, 127, 2560, grid=G, heads=32, hd=80, nsplit=3, resid=2), E_UNSUPPORTED),
            (GSpec("refuse-gemvm-5120", GEMVM, PRO_X, 2, 126, 5120, grid=G), E_UNSUPPORTED),
            (GSpec("refuse-gemvm-odd-bias", GEMVM, PRO_X, 3, 127, 2560, grid=G), E_UNSUPPORTED),
            (GSpec("refuse-gemvm-odd-resid", GEMVM, PRO_LN, 3, 127, 2560, grid=G, bias=False, resid=1, family="bounded"), E_UNSUPPORTED)]


def route_specs():
    return (rows_x_specs() + rows_ln_specs() + rows_merge_specs() + gemv1_x_specs() + gemv1_ln_specs() + gemv1_merge_specs() + gemv1_natural_specs()
            + gemvm_specs())
