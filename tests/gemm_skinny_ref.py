"""Cases, bound, layouts and expected route of the M <= 32 (decode) GEMM family of csrc/gemm_skinny.h and its two reduce kernels.  CPU only, numpy.

Everything that is not particular to the family comes from tests/gemm_ref.py: Spec (extended here), build_case with its guards (lda / ldw / ldr /
ldc wider than the matrix, +-2^14 traps in the padding columns and in the two rows behind the last, NaN sentinels in every output), the float64
reference, half_ulp, ratio and ln_out_ref.  SSpec adds what only a decode launch passes: the split-K scratch (bytes offered), the stream-layout
copy of W (Wp), the three row-block switches and the grid override of the probe build (eilev_debug_grid_cus, which skinny_n_cu follows there).

expected(sp, n_cu) -> (rc, form, ks) mirrors w8_streams, check_args, skinny_takes, launch_skinny (the ks rule with its scratch fallback, the pre
rule, skinny_nbsel), rows32_shape / rows32_plan and the fused-LayerNorm predicate of skinny_reduce, every constant read off csrc/gemm.hip and
csrc/gemm_skinny.h.  Form codes (csrc/common.h): 6000 plain, 6100 + 10 MB + PRE dma, 6200 + 10 MB + NB nb, 6300 + KS rows32, 6400 + 10 MB + PRE w8;
bits SPLIT_K, REDUCE_LN (the reduce wrote the LayerNorm rows too), STREAM (Wp was read).

tol, per element, no floor and no max|ref| term: gemm_ref.tol with its (K + 8) replaced by the number of fp32 additions that reach one output,
counted from the code (n_adds):
    K          products accumulated by the MFMAs of one wave chain (a wave's slice) and across the chains
  + 4 or 8     wave partials summed through LDS (gemm_rows32_kernel: 8 waves; every other kernel: 4)
  + ks         split planes summed by skinny_reduce_kernel / reduce_ln_wg_kernel (1 when there is no split)
  + 3          epilogue operations: x wscale, + bias, x scale (or + residual)
i.e. K + 8 for an unsplit four-wave launch, as in the wide family.  ACC_C stays gemm_ref.ACC_C (1 unless a device measurement widens it)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import gemm_ref as R
from gemm_ref import OK, E_BADARG, E_UNSUPPORTED, Spec  # noqa: F401

# dbg bits of csrc/common.h (an interface: numbers)
SKINNY_NO_DMA, NO_PRELOAD, NO_STREAM, FIRST_FIT, NO_ROWS32, NO_REDUCE_LN, NB_BLOCKS_ONLY = 1 << 3, 1 << 7, 1 << 15, 1 << 27, 1 << 28, 1 << 29, 1 << 30
NB_SHIFT = 26
SPLIT_K, REDUCE_LN, STREAM = 1 << 18, 1 << 19, 1 << 20
GUARD_PLANES = 2  # poisoned planes behind the scratch that is offered


def nb_flag(v):
    """(dbg >> 26) & 7: 2 / 4 / 7 (= 8) weight blocks per workgroup.  The field shares bits 27 and 28 with FIRST_FIT and NO_ROWS32."""
    return v << NB_SHIFT


@dataclass(frozen=True)
class SSpec(Spec):
    scratch: int = 0      # bytes of split-K scratch offered (0: none)
    stream: bool = False  # pack W for the launch's grid and pass it as Wp
    dense_w: bool = False  # ldw == K (what Wp needs); w8 always has it
    a_frag: bool = False  # A in the row-block layout (32 rows whatever M is; rows M..31 NaN)
    c_frag: bool = False
    ln_frag: bool = False
    grid: int = 0         # eilev_debug_grid_cus


def scr(N, planes=8):
    """Scratch bytes for `planes` split planes of 32 rows."""
    return planes * 32 * N * 4


def strides(sp):
    lda, ldw, ldr, ldc = R._strides(sp)
    if getattr(sp, "dense_w", False) or sp.w8:
        ldw = sp.K
    return lda, ldw, ldr, ldc


def build_case(sp):
    c = R.build_case(sp)
    if strides(sp)[1] != c.ldw:
        c.W_buf = np.ascontiguousarray(c.W_buf[:, :sp.K])
        c.ldw = sp.K
    return c


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------

def frag32_index(row, col):
    """csrc/common.h frag32_index: element (row, col) of up to 32 rows at (col / 32) * 1024 + row * 32 + col % 32."""
    return (np.asarray(col, np.int64) >> 5) * 1024 + np.asarray(row, np.int64) * 32 + (np.asarray(col, np.int64) & 31)


def to_frag32(x, cols, fill=np.nan):
    """[M, cols] -> the 32 x cols row-block buffer (flat), rows M..31 = fill.  cols % 32 == 0."""
    assert cols % 32 == 0
    out = np.full(32 * cols, fill, np.float32)
    m = x.shape[0]
    out[frag32_index(np.arange(m)[:, None], np.arange(cols)[None, :])] = x[:, :cols]
    return out


def rows32_rows(N, grid_x, x):
    """gemm_skinny.h rows32_rows: (r0, cnt) of workgroup x."""
    per, rem = divmod(N, grid_x)
    return x * per + min(x, rem), per + (1 if x < rem else 0)


def stream_index(N, K, grid_x, nv_of=None):
    """Flat destination of every element (n, k) in the stream layout (stream_pack_kernel): workgroup x keeps its rows [r0, r0 + cnt) together at
    r0 K; 16-row block j (nv rows) at + 16 j K holds per k-step of 32 the nv x 32 fragment as one piece, element (l15, chunk lg) at (l15 4 + lg) 8."""
    idx = np.empty((N, K), np.int64)
    k = np.arange(K)
    kstep, lg, e = k // 32, (k // 8) % 4, k % 8
    for x in range(grid_x):
        r0, cnt = rows32_rows(N, grid_x, x)
        for j in range((cnt + 15) // 16):
            nv = min(16, cnt - 16 * j)
            nvs = nv if nv_of is None else nv_of(nv)
            for l15 in range(nv):
                idx[r0 + 16 * j + l15] = (r0 + 16 * j) * K + kstep * (nvs * 32) + (l15 * 4 + lg) * 8 + e
    return idx


def stream_pack(W, grid_x):
    N, K = W.shape
    out = np.empty(N * K, W.dtype)
    out[stream_index(N, K, grid_x).ravel()] = W.ravel()
    return out


def stream_read(Wp, N, K, grid_x, nv_of=None):
    """What gemm_rows32_kernel's load_block reads back from a packed copy, as [N, K] (nv_of: a planted fragment stride)."""
    idx = stream_index(N, K, grid_x, nv_of)
    return Wp[np.clip(idx, 0, Wp.size - 1)]


# ---- the K partition of the dma / nb / w8 kernels (units: tiles of 256) and of the plain kernel (units: steps of 32) -----------------------------

def wave_range(units, ks, y, wid):
    """[beg, end) of wave wid of workgroup row y: per_wg = ceil(units / ks), per_w = ceil(len / 4)."""
    per_wg = -(-units // ks)
    wg_beg = y * per_wg
    wg_end = min(units, wg_beg + per_wg)
    per_w = (max(wg_end - wg_beg, 0) + 3) // 4
    beg = wg_beg + wid * per_w
    return beg, max(beg, min(wg_end, beg + per_w))


def pre_rule(K, ks, dbg=0):
    return -(-(-(-(K // 256) // ks)) // 4) <= 3 and not dbg & NO_PRELOAD


# ---- the route -------------------------------------------------------------------------------------------------------------------------------

def rows32_shape(N, K, n_cu, first_fit=False):
    """(ks, ksteps, grid_x) or None."""
    if K % 256 or N < 1:
        return None
    nb, pw, k5 = (N + 15) // 16, K // 256, 0
    for c in (1, 2, 4, 8):
        if pw % c == 0 and (pw // c in (10, 5) or (pw // c == 8 and c == 1)):
            k5 = c
            if nb * c >= n_cu or pw // c == 5 or first_fit:
                break
    if not k5:
        return None
    cus = max(n_cu // k5, 1) if k5 > 1 else n_cu
    return k5, pw // k5, min(nb, cus)


def rows32_plan(sp, nb, n_cu, mr):
    shape = rows32_shape(sp.N, sp.K, n_cu, bool(sp.flags & FIRST_FIT))
    if shape is None:
        return None
    k5, ksteps, grid_x = shape
    wscale = sp.wscale or sp.w8
    if sp.c_frag and (k5 > 1 or sp.out_f32 or wscale or sp.resid or sp.N & 31):
        return None
    if sp.ln_frag and (k5 == 1 or not sp.ln_out):
        return None
    if k5 == 1 and nb < n_cu and sp.ln_out:
        return None
    if sp.K // 256 == 8 and nb < n_cu:
        return None
    if k5 > 1 and sp.flags & FIRST_FIT:
        return None
    if k5 > 1 and (not sp.scratch or k5 * mr * sp.N * 4 > sp.scratch):
        return None
    return k5, ksteps, grid_x


def skinny_nbsel(sp, nb, ks, w8):
    dbg = sp.flags
    nbsel = (dbg >> NB_SHIFT) & 7
    if nbsel == 0 and sp.M > 16:
        wgs = nb if dbg & NB_BLOCKS_ONLY else nb * ks
        nbsel = 8 if wgs >= 8 * 240 else 4 if wgs >= 4 * 240 else 2 if wgs >= 2 * 240 else 1
    if nbsel == 7:
        nbsel = 8
    if nbsel not in (2, 4, 8):
        nbsel = 1
    if nbsel == 8 and sp.M <= 16:
        nbsel = 4
    return 1 if w8 else nbsel


def eff_cus(sp, n_cu):
    return sp.grid if 0 < sp.grid < n_cu else n_cu


def fused_ln(sp, ldr, ldc):
    return bool(sp.ln_out and not sp.flags & NO_REDUCE_LN and not sp.out_f32 and sp.epi == 0 and sp.scale_cols == 0 and sp.N % 8 == 0 and sp.N <= 4096
                and ldc % 8 == 0 and (not sp.resid or ldr % 8 == 0))


def plan(sp, n_cu):
    """(rc, form, ks, grid_x): expected() plus the rows32 grid (0 for every other kernel)."""
    lda, ldw, ldr, ldc = strides(sp)
    dbg, M, N, K = sp.flags, sp.M, sp.N, sp.K
    cus = eff_cus(sp, n_cu)
    assert 0 < M <= 32 and not sp.a8 and not sp.patch_group and not sp.lnfold and not sp.stats and not sp.hm
    if sp.ln_out and (sp.out_f32 or N % 8 or ldc % 8 or N > 4096):
        return E_UNSUPPORTED, 0, 0, 0  # launch_gemm: no reduce and no LayerNorm launch (norm.hip: cols <= 4096) can write these rows; nothing runs
    bits, w8 = 0, False
    if sp.w8:
        if K % 16:
            return E_BADARG, 0, 0, 0
        if K % 256 == 0:  # w8_streams
            w8 = True
        else:
            bits |= R.W8_EXPANDED
    if K % 8 or lda % 8 or ldw % 8:
        return E_UNSUPPORTED, 0, 0, 0
    dma_ok = K % 256 == 0 and (not dbg & SKINNY_NO_DMA or w8)
    assert M <= 16 or dma_ok, "17..32 rows with K % 256 != 0 (or the no-DMA switch) belong to the wide family"
    mr, nb = (16 if M <= 16 else 32), (N + 15) // 16
    ks = 1 if nb >= 384 else (512 + nb - 1) // nb
    ksteps = (K + 31) // 32
    if ks > ksteps // 32:
        ks = max(ksteps // 32, 1)
    if ks > 1 and (not sp.scratch or ks * mr * N * 4 > sp.scratch):
        ks = 1
    pre = pre_rule(K, ks, dbg)
    nbsel = skinny_nbsel(sp, nb, ks, w8)
    r32 = None
    if not w8 and M > 16 and not dbg & NO_ROWS32:
        r32 = rows32_plan(sp, nb, cus, mr)
    if (sp.a_frag or sp.c_frag or sp.ln_frag) and r32 is None:
        return E_UNSUPPORTED, 0, 0, 0
    m32, grid_x = M > 16, 0
    if w8:
        form = 6400 + (20 if m32 else 10) + int(pre)
    elif r32 is not None:
        ks, ks32, grid_x = r32
        form = 6300 + ks32
        if sp.stream and ldw == K and not dbg & (NO_STREAM | FIRST_FIT):
            bits |= STREAM
    elif dma_ok and pre and nbsel > 1:
        form = 6200 + (20 if m32 else 10) + nbsel
    elif dma_ok:
        form = 6100 + (20 if m32 else 10) + int(pre)
    else:
        form = 6000
    if ks > 1:
        bits |= SPLIT_K
        if fused_ln(sp, ldr, ldc):
            bits |= REDUCE_LN
        elif sp.ln_frag:
            return E_UNSUPPORTED, form | bits, ks, grid_x  # (refused by the reduce, after the partials were written)
    return OK, form | bits, ks, grid_x


def expected(sp, n_cu):
    return plan(sp, n_cu)[:3]


def form_name(form):
    low = form & 0xFFFF
    if low // 1000 != 6:
        return R.form_name(form)
    kind, rest = (low - 6000) // 100, low % 100
    out = ("plain" if kind == 0 else f"dma-{rest // 10}-{'pre' if rest % 10 else 'rolled'}" if kind == 1 else f"nb-{rest // 10}-{rest % 10}" if kind == 2
           else f"rows32-{rest}" if kind == 3 else f"w8-{rest // 10}-{'pre' if rest % 10 else 'rolled'}")
    return (out + ("+split" if form & SPLIT_K else "") + ("+ln" if form & REDUCE_LN else "") + ("+stream" if form & STREAM else "")
            + ("+w8x" if form & R.W8_EXPANDED else ""))


def family_of(form):
    """The instance (the coverage key): the name without the bits."""
    low = form & 0xFFFF
    return form_name(low) if low // 1000 == 6 else R.family_of(form)


REQUIRED = (["plain"] + [f"dma-{mb}-{p}" for mb in (1, 2) for p in ("pre", "rolled")] + ["nb-1-2", "nb-1-4", "nb-2-2", "nb-2-4", "nb-2-8"]
            + ["rows32-5", "rows32-8", "rows32-10"] + [f"w8-{mb}-{p}" for mb in (1, 2) for p in ("pre", "rolled")]
            + ["skinny_reduce", "reduce_ln-2", "reduce_ln-4", "reduce_ln-0"])


def reduce_name(form, ks):
    """Which reduce kernel a split launch ends in (coverage key), or None."""
    if not form & SPLIT_K:
        return None
    return f"reduce_ln-{ks if ks in (2, 4) else 0}" if form & REDUCE_LN else "skinny_reduce"


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------

def n_adds(sp, form, ks):
    """fp32 additions that reach one output (module docstring)."""
    waves = 8 if (form & 0xFFFF) // 100 == 63 else 4
    return sp.K + waves + max(ks, 1) + 3


def tol(c, y, S, form, ks):
    sp = c.spec
    t = R.half_ulp(y, 24 if sp.out_f32 else 8) + R.ACC_C * n_adds(sp, form, ks) * 2.0 ** -24 * S * (1.13 if sp.epi == 1 else 1.0)
    if sp.epi == 1:
        t = t + R.gelu_forms()["deg12"]  # skinny_epilogue and the plain epilogue of gemm_rows32_kernel: gelu_erf
    return t


# ---- the launches of tests/test_hip_gemm_skinny.py ----------------------------------------------------------------------------------------------

def both(name, M, N, K, **kw):
    out = [SSpec(name + "-b", M, N, K, family="bounded", **kw)]
    if kw.get("epi", 0) != 1:
        out.append(SSpec(name + "-x", M, N, K, family="exact", **kw))
    return out


def plain_specs():
    S = []
    S += both("plain-1x40x72", 1, 40, 72, epi=2)
    S += both("plain-3x40x72", 3, 40, 72, resid=True)
    S += both("plain-16x1001x264", 16, 1001, 264, epi=1)                      # ragged N; K % 32 != 0: the kin tail
    S += both("plain-3x1001x264-f32", 3, 1001, 264, out_f32=True, resid=True, scale_cols=16, scale=0.125)
    S += both("plain-16x40x2056-split", 16, 40, 2056, scratch=scr(40), resid=True)   # ks = 2 + skinny_reduce_kernel
    S += both("plain-3x40x2056-nosplit", 3, 40, 2056)
    S += both("plain-16x200x512-nodma", 16, 200, 512, flags=SKINNY_NO_DMA, wscale=True)
    return S


def dma_specs():
    S = []
    # (none of these K has a rows32 shape: no switch is needed to keep 17..32 rows here — NO_ROWS32 is also bit 2 of the nb field)
    for m in (1, 3, 16, 17, 25, 32):
        S += both(f"dma-{m}x200x512", m, 200, 512, epi=(m % 3), resid=(m % 2 == 1))   # one tile: three idle waves
        S += both(f"dma-{m}x200x768", m, 200, 768, bias=(m != 3))
    S += both("dma-16x24x3072", 16, 24, 3072, epi=2)                                           # three tiles per wave
    S += both("dma-32x24x3072", 32, 24, 3072, resid=True)
    for m in (3, 16, 25):
        S += both(f"dma-{m}x200x2048-split", m, 200, 2048, scratch=scr(200), resid=True)
        S += both(f"dma-{m}x200x2048-fallback", m, 200, 2048, resid=True)
        S += both(f"dma-{m}x200x3328-rolled", m, 200, 3328)                                    # four tiles per wave without scratch
        S += both(f"dma-{m}x200x768-nopre", m, 200, 768, flags=NO_PRELOAD, epi=2)
    S += both("dma-16x200x2048-short-scratch", 16, 200, 2048, scratch=2 * 16 * 200 * 4 - 4)    # one word short of two planes: ks = 1
    return S


def nb_specs():
    S = []
    for v, ms in ((2, (3, 16, 17, 32)), (4, (1, 16, 25, 32)), (7, (16, 32))):
        for m in ms:
            S += both(f"nb{v}-{m}x200x768", m, 200, 768, flags=nb_flag(v), epi=(m % 3), resid=(m % 2 == 0))   # 13 blocks
            S += both(f"nb{v}-{m}x16x256", m, 16, 256, flags=nb_flag(v))                                        # total = 1
            S += both(f"nb{v}-{m}x200x2048-split", m, 200, 2048, flags=nb_flag(v), scratch=scr(200), resid=True)
    return S


def rows32_specs(n_cu):
    """The natural-grid cases of gemm_rows32_kernel (N follows the device's CU count)."""
    S = []
    for n in (200, 1000, 16 * n_cu - 16, 16 * n_cu + 16):
        S += both(f"r32-5-17x{n}x1280", 17, n, 1280, epi=(n % 3))
        S += both(f"r32-5-32x{n}x1280", 32, n, 1280, resid=True)
    # split: fewer blocks than CUs
    S += both("r32-5-split2-25x320x2560", 25, 320, 2560, scratch=scr(320), resid=True)
    S += both("r32-5-split4-32x320x5120", 32, 320, 5120, scratch=scr(320), resid=True)
    S += both("r32-nosplit-25x320x2560", 25, 320, 2560, resid=True)        # without scratch: the mirror says which kernel takes over
    n = 16 * n_cu
    S += both(f"r32-10-32x{n}x2560", 32, n, 2560, epi=2)
    S += both(f"r32-8-17x{n}x2048", 17, n, 2048)
    S += both(f"r32-8-17x{n - 1}x2048", 17, n - 1, 2048)                    # one row fewer: still n_cu blocks
    S += both(f"r32-8-refused-17x{n - 16}x2048", 17, n - 16, 2048)          # one BLOCK fewer: nb < n_cu with per_wave == 8 is not rows32
    return S


def ring_specs():
    """Grid override 8: nblk = 2 RB - 1, 2 RB, 2 RB + 1, 3 RB + 1 blocks per workgroup (RB = 4 for KS = 5, 3 for KS = 8 / 10), N % grid != 0."""
    S = []
    for K, RB in ((1280, 4), (2560, 3), (2048, 3)):
        for nblk in (2 * RB - 1, 2 * RB, 2 * RB + 1, 3 * RB + 1):
            n = 8 * 16 * nblk - 3          # five workgroups with nblk blocks whose last has 15 rows ... and three with one row fewer
            m = 17 if nblk % 2 else 32
            S += both(f"ring-{K}-{nblk}blk-{m}x{n}", m, n, K, grid=8, epi=(nblk % 3), stream=(nblk % 2 == 0), dense_w=(nblk % 2 == 0))
        n = 8 * 16 * (2 * RB) + 8 * 5 + 3  # a short last block (nv = 5 or 6) behind whole ones
        S += both(f"ring-{K}-short-25x{n}", 25, n, K, grid=8, stream=True, dense_w=True, resid=True)
        n = 8 * 16 * (2 * RB) + 3          # shares of different block counts: three workgroups with one more block of ONE row
        S += both(f"ring-{K}-uneven-32x{n}", 32, n, K, grid=8, stream=True, dense_w=True)
    return S


def natural_ring_spec(n_cu):
    return SSpec(f"ring-natural-32x{81 * n_cu}x2560", 32, 81 * n_cu, 2560, family="exact", stream=True, dense_w=True, epi=2)


def rows32_epilogue_specs():
    S = []
    n = 8 * 16 * 2 + 40
    for tag, kw in (("bias-relu", dict(epi=2)), ("gelu", dict(epi=1)), ("scale16", dict(scale_cols=16, scale=0.125)),
                    ("scale-third", dict(scale_cols=n // 3, scale=0.125)), ("f32", dict(out_f32=True)), ("nobias", dict(bias=False)),
                    ("resid", dict(resid=True, epi=2)), ("wscale", dict(wscale=True)), ("f32-resid", dict(out_f32=True, resid=True))):
        S += both(f"r32epi-{tag}", 25, n, 1280, grid=8, **kw)
    return S


def stream_specs():
    S = []
    S += both("stream-25x296x1280", 25, 296, 1280, grid=8, stream=True, dense_w=True)
    S += both("stream-off-ldw", 25, 296, 1280, grid=8, stream=True)                               # ldw != K: Wp ignored
    S += both("stream-off-flag", 25, 296, 1280, grid=8, stream=True, dense_w=True, flags=NO_STREAM)
    S += both("stream-split-32x320x2560", 32, 320, 2560, grid=64, stream=True, dense_w=True, scratch=scr(320), resid=True)
    return S


def frag_specs():
    S = []
    S += both("frag-a-25x296x1280", 25, 296, 1280, grid=8, a_frag=True)
    S += both("frag-ac-17x288x1280", 17, 288, 1280, grid=8, a_frag=True, c_frag=True, epi=2)
    S += both("frag-c-32x320x2560", 32, 320, 2560, grid=8, c_frag=True, stream=True, dense_w=True)
    S += both("frag-ln-25x320x2560", 25, 320, 2560, grid=64, a_frag=True, ln_frag=True, ln_out=1, scratch=scr(320), resid=True)
    return S


def w8_specs():
    S = []
    for m in (3, 16, 17, 32):
        S += both(f"w8-{m}x200x512", m, 200, 512, w8=True, epi=(m % 3 if m % 3 != 1 else 2))
        S += both(f"w8-{m}x200x2048-split", m, 200, 2048, w8=True, scratch=scr(200), resid=True)
        S += both(f"w8-{m}x200x768-nopre", m, 200, 768, w8=True, flags=NO_PRELOAD)
    S += both("w8-16x40x272-expanded", 16, 40, 272, w8=True)      # K % 256 != 0 (and K % 16 == 0, which w8_check asks for): expansion, then the plain kernel
    return S


def reduce_specs():
    """skinny_reduce_kernel: every epilogue, fp32, residual, ks = 2, 3, 4."""
    S = []
    for ks, K in ((2, 2048), (3, 3072), (4, 4096)):
        for tag, kw in (("relu", dict(epi=2)), ("gelu", dict(epi=1)), ("f32-resid", dict(out_f32=True, resid=True)),
                        ("scale", dict(scale_cols=16, scale=0.125, resid=True)), ("wscale", dict(wscale=True))):
            S += both(f"reduce-ks{ks}-{tag}", 3 if ks == 3 else 16, 72, K, scratch=scr(72), **kw)
    return S


def reduce_ln_specs():
    """reduce_ln_wg_kernel<2 / 4 / 0>; epi != 0 and the switch take the two-launch form.  (N = 4104 is past the fused reduce AND past what the
    separate LayerNorm launch takes, cols <= 4096: launch_gemm refuses it before anything runs, see the refusals of test_hip_gemm_skinny.py.)"""
    S = []
    for ks, K in ((2, 2048), (3, 3072), (4, 4096)):
        for n in (320, 4096):  # N / 8 = 40 threads (no multiple of 64) and 512 (the maximum); 256 blocks of N = 4096 split K in two at most
            if n == 4096 and ks != 2:
                continue
            S.append(SSpec(f"rln-ks{ks}-ln-{n}", 16, n, K, family="bounded", scratch=scr(n), ln_out=1, resid=True))
            S.append(SSpec(f"rln-ks{ks}-rms-{n}", 16 if n == 4096 else 25, n, K, family="bounded", scratch=scr(n), ln_out=2, bias=False))
        S.append(SSpec(f"rln-ks{ks}-ln-320-x", 3, 320, K, family="exact", scratch=scr(320), ln_out=1, resid=True, wscale=True))
    S.append(SSpec("rln-two-launch-relu", 16, 320, 2048, family="bounded", scratch=scr(320), ln_out=1, epi=2))
    S.append(SSpec("rln-unfused-flag", 16, 320, 2048, family="bounded", scratch=scr(320), ln_out=1, resid=True, flags=NO_REDUCE_LN))
    return S


def route_specs(n_cu):
    return (plain_specs() + dma_specs() + nb_specs() + rows32_specs(n_cu) + ring_specs() + [natural_ring_spec(n_cu)] + rows32_epilogue_specs()
            + stream_specs() + frag_specs() + w8_specs() + reduce_specs() + reduce_ln_specs())
