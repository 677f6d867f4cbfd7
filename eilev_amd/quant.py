"""fp8 (OCP e4m3, torch.float8_e4m3fn) weight-only quantisation with one fp32 scale per output channel — the weight format of
``eilev_linear_w8`` (include/eilev.h; BASELINE configs[4] "fp8 MFMA weights").

    scale[n] = max_k |W[n, k]| / 448          (448 = largest finite e4m3 value; an all-zero row gets scale 1)
    Wq[n, k] = e4m3(W[n, k] / scale[n])       (round to nearest even — torch's cast)
    W ≈ Wq * scale[n]

The linear layer then computes ``(x @ Wq.T) * scale + bias``: the scale is factored out of the sum, so the kernel
multiplies bf16 activations with exactly-represented weights and scales the fp32 sum once per output.

int4 weight-only quantisation with one bf16 scale per group of 128 weights — the weight format of include/eilev_w4.h (libeilev_hip_w4.so,
``HipEngine(lm_weights="int4")``), restated in torch:

    amax[n, g] = max |W[n, 128 g : 128 g + 128]|  (fp32)
    s[n, g]    = bf16_rne(amax / 7)               (an all-zero group gets s = 1)
    q[n, k]    = clamp(round_half_even(W[n, k] / float(s)), -8, 7)      (|w| / s reaches 7.03: nothing clamps, code -8 is never emitted)
    W'[n, k]   = bf16_rne(float(q) * float(s))    (q * s is exact in fp32: ONE rounding) — the TWIN, the matrix the int4 kernels multiply by
    |W' - W| <= s / 2 + 2^-8 |q s| (+ the fp32 division's rounding)

Stored: u = q + 8 in 32-bit little-endian words [N, K / 8], word j = weights 8 j .. 8 j + 7, weight 8 j + e in bits [4 p, 4 p + 4) with
p = (e & 1) * 4 + (e >> 1) (``pack_int4`` / ``unpack_int4`` handle them as bytes [N, K / 2]); scales [N, K / 128] bf16.
"""
from __future__ import annotations

E4M3_MAX = 448.0
INT4_GROUP = 128
INT4_KTILE = 256  # K of every quantised matrix is a multiple of this


def quantize_e4m3_per_channel(weight):
    """weight: floating tensor (N, K) -> (uint8 tensor (N, K) holding the e4m3 bytes, float32 scales (N,))."""
    import torch

    w = weight.detach().to(torch.float32)
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (w / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def dequantize(q_bytes, scale):
    """float32 (N, K) = e4m3(q_bytes) * scale[:, None] (the matrix the quantised layer effectively multiplies by)."""
    import torch

    return q_bytes.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None]


def linear_w8(x, q_bytes, scale, bias=None, residual=None, epilogue: int = 0, out_dtype=None, lib=None):
    """``epilogue((x @ dq(Wq).T) * scale + bias) (+ residual)`` on the GPU through ``eilev_linear_w8``.  x: bf16 (M, K) CUDA."""
    import ctypes as C

    import torch

    from . import abi

    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise RuntimeError("linear_w8 runs on the GPU (HIP library) with bf16 activations")
    lib = lib or abi.load_hip()
    m, k = x.shape
    n = q_bytes.shape[0]
    out_f32 = out_dtype == torch.float32
    out = torch.empty((m, n), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    nb = lib.eilev_linear_w8_scratch_bytes(m, n, k)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    abi.check(lib.eilev_linear_w8(p(x.contiguous()), p(q_bytes), p(scale), p(bias), p(residual), p(out), m, n, k, epilogue, int(out_f32),
                                  p(ws), nb, C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "eilev_linear_w8")
    return out


def quantize_int4(weight):
    """weight: floating tensor (N, K), K a multiple of 128 -> (int8 codes q in [-8, 7] (N, K), bf16 scales (N, K / 128))."""
    import torch

    w = weight.detach().to(torch.float32)
    n, k = w.shape
    if k % INT4_GROUP:
        raise ValueError(f"int4 groups are {INT4_GROUP} consecutive weights: K = {k}")
    g = w.view(n, k // INT4_GROUP, INT4_GROUP)
    amax = g.abs().amax(dim=2)
    s = torch.where(amax > 0, amax / 7.0, torch.ones_like(amax)).to(torch.bfloat16)
    q = torch.round(g / s.to(torch.float32)[:, :, None]).clamp(-8, 7).to(torch.int8)
    return q.view(n, k).contiguous(), s.contiguous()


def twin_int4(q, scales):
    """bf16 (N, K): W' = bf16_rne(float(q) * float(s)), the matrix a quantised linear multiplies by."""
    import torch

    n, k = q.shape
    return (q.to(torch.float32).view(n, k // INT4_GROUP, INT4_GROUP) * scales.to(torch.float32)[:, :, None]).to(torch.bfloat16).view(n, k)


def _int4_shift(dev):
    """bit position of weight e = 0 .. 7 of a word: 4 * ((e & 1) * 4 + (e >> 1))"""
    import torch

    e = torch.arange(8, device=dev)
    return 4 * ((e & 1) * 4 + (e >> 1))


def pack_int4(q):
    """int8 codes (N, K) in [-8, 7], K a multiple of 8 -> uint8 (N, K / 2): the stored words of include/eilev_w4.h as little-endian bytes."""
    import torch

    n, k = q.shape
    u = (q.to(torch.int64) + 8).view(n, k // 8, 8)
    if bool(((u < 0) | (u > 15)).any()):
        raise ValueError("int4 codes are -8 .. 7")
    word = (u << _int4_shift(q.device)).sum(dim=2)  # (N, K / 8), 0 .. 2^32 - 1
    b = torch.stack([(word >> (8 * i)) & 0xFF for i in range(4)], dim=2)
    return b.to(torch.uint8).view(n, k // 2).contiguous()


def unpack_int4(packed):
    """uint8 (N, K / 2) -> int8 codes (N, K): the inverse of pack_int4."""
    import torch

    n, kb = packed.shape
    b = packed.to(torch.int64).view(n, kb // 4, 4)
    word = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16) | (b[:, :, 3] << 24)
    u = (word[:, :, None] >> _int4_shift(packed.device)) & 0xF
    return (u - 8).to(torch.int8).view(n, kb * 2).contiguous()


def int4_refusal(config):
    """Why ``lm_weights="int4"`` does not take the model of ``config`` (a Blip2Config), or None: OPT with hidden and ffn widths that are
    multiples of 256, hidden at most 4096."""
    t = config.text_config
    if getattr(t, "model_type", "opt") != "opt":
        return "the int4 kernels are built for the OPT language model, not flan-t5"
    d, f = int(t.hidden_size), int(t.ffn_dim)
    if d % INT4_KTILE or f % INT4_KTILE:
        return f"the int4 kernels stream K in tiles of {INT4_KTILE}: hidden_size {d} and ffn_dim {f} must be multiples of {INT4_KTILE}"
    if d > 4096:
        return f"the int4 decode step writes the LayerNorm rows in its split-K reduce, which takes hidden sizes up to 4096: hidden_size {d}"
    return None
