"""The int4 weight format of include/eilev_w4.h for the tests: a brute-force restatement of the stated word order, operands for the kernel
tests, the float64 reference of eilev_w4_linear with its per-element bound, and the mistakes that reference must catch.  CPU only.

The bound is the one tests/gemm_skinny_ref.py derives for the bf16 decode kernels, applied to (A, W'): both operands are exactly bf16 and the
int4 kernel multiplies them on the bf16 MFMA with fp32 accumulation, so the same argument holds —
    half a unit of the output format at |y|  +  ACC_C * n_adds * 2^-24 * S
with S = |A| |W'|^T (+ |bias| and |residual|: the magnitudes the epilogue's fp32 additions round at) and n_adds = K products accumulated
+ 4 wave partials + ks split planes + 3 epilogue operations, as gemm_skinny_ref.n_adds counts them for a four-wave kernel."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import gemm_ref as R
from eilev_amd import quant

GROUP = quant.INT4_GROUP

# (N, K) of the kernel tests and the rows they run with; the four OPT-2.7B shapes run with 1 and 32 rows
SMALL = [(16, 256), (40, 512), (272, 2560), (32, 10240)]
SMALL_M = [1, 3, 16, 17, 32]
OPT27 = [(7680, 2560), (2560, 2560), (10240, 2560), (2560, 10240)]
OPT27_M = [1, 32]
LINEAR_CASES = [(m, n, k) for n, k in SMALL for m in SMALL_M] + [(m, n, k) for n, k in OPT27 for m in OPT27_M]
EXPAND_CASES = [(16, 128), (40, 256), (272, 384)]  # (eilev_w4_expand takes whole groups)


def brute_pack(q: np.ndarray) -> np.ndarray:
    """int8 codes (N, K) -> bytes (N, K / 2), one weight at a time from the header's byte statement: byte 4 j + b holds weight
    8 j + 4 (b & 1) + (b >> 1) in its low nibble and weight 8 j + 4 (b & 1) + (b >> 1) + 2 in its high nibble, as u = q + 8."""
    n, k = q.shape
    out = np.zeros((n, k // 2), np.uint8)
    for row in range(n):
        for j in range(k // 8):
            for b in range(4):
                lo = 8 * j + 4 * (b & 1) + (b >> 1)
                out[row, 4 * j + b] = (int(q[row, lo]) + 8) | ((int(q[row, lo + 2]) + 8) << 4)
    return out


def brute_words(q: np.ndarray) -> np.ndarray:
    """... and from the word statement: weight 8 j + e in bits [4 p, 4 p + 4) of word j, p = (e & 1) * 4 + (e >> 1)."""
    n, k = q.shape
    out = np.zeros((n, k // 8), np.uint32)
    for row in range(n):
        for j in range(k // 8):
            w = 0
            for e in range(8):
                w |= (int(q[row, 8 * j + e]) + 8) << (4 * ((e & 1) * 4 + (e >> 1)))
            out[row, j] = w
    return out


def all_codes(n, k, seed=0):
    """Codes that cycle through all 16 values (-8 included) with a different phase per row, shuffled per row."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.arange(n * k).view(n, k) + torch.arange(n)[:, None] * 5) % 16 - 8
    perm = torch.argsort(torch.rand(n, k, generator=g), dim=1)
    return torch.gather(base, 1, perm).to(torch.int8)


def wide_scales(n, groups, seed=0, lo=-20, hi=6):
    """bf16 scales 2^lo .. 2^hi with non-power-of-two mantissas."""
    g = torch.Generator().manual_seed(seed + 1)
    e = torch.randint(lo, hi, (n, groups), generator=g).float()
    mant = 1.0 + torch.randint(1, 128, (n, groups), generator=g).float() / 128.0
    return (mant * torch.pow(2.0, e)).to(torch.bfloat16)


def pow2_scales(n, groups, seed=0):
    g = torch.Generator().manual_seed(seed + 2)
    return torch.pow(2.0, torch.randint(-3, 3, (n, groups), generator=g).float()).to(torch.bfloat16)


def twin64(q, s) -> np.ndarray:
    """W' in float64 (exactly bf16)."""
    return quant.twin_int4(q, s).to(torch.float64).numpy()


def linear_ref(A, W, bias=None, resid=None, scale=1.0, scale_cols=0, relu=False):
    """(y, S) in float64: eilev_w4_linear's value on the matrix W and the magnitude sum its fp32 operations round at."""
    A64, W64 = np.asarray(A, np.float64), np.asarray(W, np.float64)
    y, S = A64 @ W64.T, np.abs(A64) @ np.abs(W64).T
    if bias is not None:
        y, S = y + np.asarray(bias, np.float64)[None, :], S + np.abs(np.asarray(bias, np.float64))[None, :]
    if scale_cols:
        y[:, :scale_cols] *= scale
        S[:, :scale_cols] *= abs(scale)
    if relu:
        y = np.maximum(y, 0.0)
    if resid is not None:
        y, S = y + np.asarray(resid, np.float64), S + np.abs(np.asarray(resid, np.float64))
    return y, S


def tol(y, S, K, ks, out_f32):
    return R.half_ulp(y, 24 if out_f32 else 8) + R.ACC_C * (K + 4 + max(ks, 1) + 3) * 2.0 ** -24 * S


def ln_ref(rows_bf16, gamma, beta, eps):
    """(ref, tol) of ln_out over the bf16 rows the device wrote: gemm_ref.ln_out_ref (the LayerNorm form)."""
    n = np.asarray(rows_bf16).shape[1]
    c = SimpleNamespace(spec=SimpleNamespace(N=n, ln_out=1), gamma=np.asarray(gamma, np.float32), beta=np.asarray(beta, np.float32), ln_eps=eps)
    return R.ln_out_ref(c, rows_bf16)


# ---- the mistakes a kernel could make reading the format: each returns the matrix such a kernel would multiply by (float64) ----------------------
def _swapped_nibbles(q, s):
    p = quant.pack_int4(q)
    return twin64(quant.unpack_int4(((p << 4) | (p >> 4)).to(torch.uint8)), s)


def _neighbour_scale(q, s):
    idx = torch.arange(s.shape[1]) ^ 1
    return twin64(q, s[:, idx.clamp(max=s.shape[1] - 1)])


def _offset_7(q, s):
    return quant.twin_int4(q.to(torch.int16) + 1, s).to(torch.float64).numpy()


def _minus8_as_plus8(q, s):
    q16 = q.to(torch.int16)
    return quant.twin_int4(torch.where(q16 == -8, torch.full_like(q16, 8), q16), s).to(torch.float64).numpy()


def _no_rounding(q, s):
    n, k = q.shape
    return (q.to(torch.float64).view(n, k // GROUP, GROUP) * s.to(torch.float64)[:, :, None]).view(n, k).numpy()


MISTAKES = {"swapped nibble order": _swapped_nibbles, "the neighbouring group's scale": _neighbour_scale, "offset 7 instead of 8": _offset_7,
            "code -8 read as +8": _minus8_as_plus8, "no bf16 rounding of q * s": _no_rounding}


def dense_operands(m, n, k, seed):
    """bf16 activations, codes over all 16 values, scales around the size of real weights with full mantissas."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(m, k, generator=g).to(torch.bfloat16)
    q = all_codes(n, k, seed)
    s = wide_scales(n, k // GROUP, seed, lo=-8, hi=-4)
    return A, q, s


def exact_operands(m, n, k, seed):
    """Integer activations in [-4, 4] and power-of-two scales 2^-3 .. 2^2: every product is a multiple of 2^-3 of at most 2^10 units, every partial sum
    of K <= 10240 of them below 2^24 units: exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-4, 5, (m, k), generator=g).to(torch.bfloat16)
    return A, all_codes(n, k, seed), pow2_scales(n, k // GROUP, seed)
