"""Reference, case builder, per-element bounds, kernel restatements and planted mistakes of the backward (training) kernel tests
(test_bwd_reference.py on the CPU, test_hip_bwd.py on the GPU).  A plain module: no fixtures, no GPU; the sibling of
attn_prefill_ref.py, whose generic helpers (bf16_bits, bits_to_f32, worst_ratio, the mask kinds, the hashed normal generator) it imports.

Reference: numpy float64 on the bf16-exact inputs, stated from the documented operation of include/eilev.h, per (batch b, head h):
  visible(i, j): j < skv, mask[b, j] != 0 where a mask is given, j <= i + (skv - sq) where causal
  s_ij   = scale q_i . k_j + rel[h, clamp(j - i - (skv - sq) + rel_off, 0, rel_n - 1)]
  P      = softmax of s over the visible keys of a row;  lse_i = log sum_visible exp(s_ij)
  M_ij   = (hash(seed, ((b heads + h) sq + i) skv + j) >= p 2^32) / (1 - p)                      (1 without dropout)
  delta_i = sum_d o_id dO_id with the GIVEN bf16 o (it is an input of the operation; the cases take o = bf16((P o M) V))
  dV = (P o M)^T dO,  dP = dO V^T,  dS = P o (M o dP - delta),  dQ = scale dS K,  dK = scale dS^T Q
A row with no visible key has lse = 1e30, dq = 0 and contributes nothing to dK / dV.

Bounds (derived from csrc/backward.hip, not measured).  U = 2^-8 is what ONE bf16 rounding can cost relative to the value rounded: the half
ulp is 2^-9 of the TOP of a binade and 2^-8 of its bottom (the caveat of the decode docstring); taking U = 2^-8 for every rounding holds
anywhere in a binade, so no input is narrowed for it.  F = 2^-24 is one fp32 rounding.
  attention, kernel by kernel:
   * relative error of a recomputed probability p = exp(s scale + bias - lse): eps_ij = e_s + e_lse + 2^-22 + 2 F (|s| + |lse| + 2 |s - lse|),
     written out in _attn_bh(): the score dot (<= hd + 2 roundings of partial sums bounded by scale sum_d |q k| + |bias|), the lse of pass 1
     (the P-weighted score error, 18 roundings per 64-key tile and stream of the online sum, __logf and the final add) and __expf.
   * dV: P o M is rounded to bf16 (U (PM)_ij each), accumulated in fp32 over sq rows, dV rounded to bf16:
       tol_dV_jd = (1 + U) sum_i [U + eps_ij + (sq + 2) F] (PM)_ij |dO_id| + U |dV_jd|
   * dS: x = M dP - delta is a cancellation: its fp32 error is relative to the MAGNITUDES, e_x = (hd + 2) F M sum_d |dO v| + e_delta +
     2 F (M |dP| + |delta|), e_delta = (hd / 8 + 8) F sum_d |o dO| (any order of the LDS adds); dS = p x is rounded to bf16:
       e_dS_ij = U |dS_ij| + (eps_ij + F) |dS_ij| + P_ij e_x
       tol_dQ_id = (1 + U) scale sum_j [e_dS_ij + (skv + 2) F |dS_ij|] |k_jd| + U |dQ_id|      (dK: the same over i with |q_id|)
   * lse: e_lse above; delta: e_delta.  Both fp32-sized; lse of a row without a visible key is 1e30 exactly.
   * fp32 share: the non-bf16 part of each bound is asserted (CPU test) <= 2^-9 of the element's sum of magnitudes
     (scale sum_j P (M sum_d |dO v| + sum_d |o dO|) |k|, resp. sum_i PM |dO|): scores reach ~65 in the tile profiles, (hd + 2) F 65 = 2^-10.9 at hd 128, once for
     the score and once more through the lse.
  No absolute floor beyond the smallest normal fp32 (worst_ratio's own 1e-30 guards the division only).
  row kernels: see ln_ref(), rms_ref(), colsum_ref(), act_ref(), gated_ref(), ce_ref(), dropout_add_ref(): one U per stored bf16 (two for
  the forwards of rmsnorm, which rounds x rstd before gamma, and of gated_gelu, which rounds gelu_new(a) before b), explicit fp32 terms relative to the sum of magnitudes for g - s1 - xhat s2 and for
  softmax - onehot at the target, and for dgamma / dbeta / colsum an order-free summation bound (rows + 66) F sum |terms| plus the statistics term
  (their global atomics have no fixed order).  act_fwd's erf-GELU is the degree-12 polynomial of common.h: its documented 2e-4 absolute error
  (tests/test_gelu_poly.py) is part of that kernel's bound.

Cases.  q = bf16(0.5 n + u_h) with u_h a +-1 pattern per head, k, v, dO ~ N(0, 1): scores ~ N(0, 1.25).  A score profile adds g_j u / (scale hd)
to key j, i.e. ~g_j (0.8 .. 1.2) to every row's score: "rise" / "fall" 26 per 64-key tile, "late" +30 on one key at 4/5 of skv, "hi" / "lo" +26 on
keys 32..63 / 0..31 of the second tile: each of pass 1's merges (tile to tile, lane half to lane half, key-block wave to wave) sees a running
maximum that moves by more than 20.  Memory no kernel may touch (stride gaps, the row behind each output, lse_delta beyond 2 B H sq, the gap of
a "gap" table) holds NaN bits; the row behind q / k / v / dO holds +-64, not zeros."""
from __future__ import annotations

from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from attn_decode_ref import TOL_REL, _normal_rows, _signs
from attn_prefill_ref import SENT16, _mask, bf16_bits, bits_to_f32, worst_ratio
from eilev_amd.synth import round_bf16

f32, f64 = np.float32, np.float64
U = 2.0 ** -8
F = 2.0 ** -24
FLT_MIN = 2.0 ** -126
FP32_SHARE = 2.0 ** -9
SENT32 = 0x7FA5A5A5  # poison of the fp32 outputs (a NaN)
SENTF = f32(1.5)     # behind the ACCUMULATED fp32 outputs (dgamma, dbeta, colsum): an atomic add onto a NaN would leave a NaN
STEP = 26.0


def ratio(got, ref, tol) -> float:
    """max |got - ref| / tol per element (inf for a non-finite output); the floor is the smallest normal fp32."""
    return worst_ratio(got, ref, np.maximum(tol, FLT_MIN) / TOL_REL)


def hash32(seed, idx):
    """include/eilev.h: the splitmix64 finaliser of (seed, element index); numpy uint64 wraps like the C code."""
    with np.errstate(over="ignore"):
        z = np.asarray(idx).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(seed + 1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def keep_mask(seed, idx, p):
    return hash32(seed, idx) >= np.uint32(min(int(f64(f32(p)) * 4294967296.0), 4294967295))


# ---- attention: a case -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    name: str
    batch: int = 2
    heads: int = 2
    hd: int = 64
    sq: int = 64
    skv: int = 64
    layout: str = "sep"       # "sep", "packed" (q|k|v and dq|dk|dv thirds, stride 3 W, sq == skv), "kv" (q alone, k|v halves at stride 2 W)
    causal: int = 0
    mask: tuple = ()          # () = null pointer; else one kind per batch entry, cycled: "ones", "left<L>", "right<R>", "holes", "dead"
    rel: str = ""             # "", "tight", "gap" (rel_stride > rel_n, NaN in the gap), "short" (both ends clamp)
    drop: float = 0.0
    profile: str = ""         # "", "rise", "fall", "late", "hi", "lo"
    scale1: bool = False      # scale = 1 with pre-scaled q (what T5 and OPT pass)
    seed: int = 0


def instance(sp: Spec):
    """launch_attn_bwd's selection restated: (DB, EXTRA)."""
    return (2 if sp.hd <= 64 else (3 if sp.hd <= 96 else 4)), bool(sp.rel or sp.drop > 0)


def entry_of(sp: Spec, k: int = 0) -> str:
    """The public entry a case goes through: a plain case takes the three in turn (null table, p = 0), a table without dropout two."""
    if sp.drop > 0:
        return "dropout"
    return ("rel", "dropout")[k % 2] if sp.rel else ("plain", "rel", "dropout")[k % 3]


def visible(c, b: int, mut: str = "") -> np.ndarray:
    sp = c.spec
    vis = np.ones((sp.sq, sp.skv), bool)
    if c.mask is not None:
        vis &= (c.mask[0 if mut == "mask0" else b] != 0)[None, :]
    if sp.causal:
        off = 0 if mut == "causal_nooff" else sp.skv - sp.sq
        lim = np.arange(sp.sq)[:, None] + off
        j = np.arange(sp.skv)[None, :]
        vis &= (j < lim) if mut == "causal_lt" else (j <= lim)
    if mut == "droplastkey":
        vis[:, sp.skv - 1] = False
    return vis


def rel_index(c, mut: str = ""):
    sp = c.spec
    idx = np.arange(sp.skv)[None, :] - np.arange(sp.sq)[:, None] - (0 if mut == "rel_nooff" else sp.skv - sp.sq) + c.rel_off
    lo = -8 if mut == "noclamp_lo" else 0
    hi = c.rel_n + 7 if mut == "noclamp_hi" else c.rel_n - 1
    return np.clip(idx, lo, hi)


def bias(c, h: int, mut: str = ""):
    """(sq, skv) float32 or None, read from the flat table as the kernel does."""
    if c.rel_flat is None:
        return None
    return c.rel_flat[c.rel_lead + h * c.rel_hs + rel_index(c, mut)]


def drop_factor(c, b, h, mut: str = ""):
    """(sq, skv) M / (1 - p) as float32 (the kernel's 1.0f / (1.0f - p)); None without dropout."""
    sp = c.spec
    if not sp.drop > 0:
        return None
    i, j = np.arange(sp.sq, dtype=np.uint64)[:, None], np.arange(sp.skv, dtype=np.uint64)[None, :]
    bh = np.uint64(b * sp.heads + h)
    idx = ((bh * np.uint64(sp.skv) + i) * np.uint64(sp.sq) + j) if mut == "dropidx" else ((bh * np.uint64(sp.sq) + i) * np.uint64(sp.skv) + j)
    return np.where(keep_mask(c.drop_seed, idx, sp.drop), f32(1.0) / (f32(1.0) - f32(sp.drop)), f32(0.0)).astype(f32)


def _drop64(c, b, h):
    """M / (1 - p) in float64 (p is the float32 the entry receives)."""
    df = drop_factor(c, b, h)
    return None if df is None else np.where(df > 0, 1.0 / (1.0 - float(f32(c.spec.drop))), 0.0)


def _profile_gain(sp: Spec):
    j = np.arange(sp.skv)
    tile, nt = j // 64, -(-sp.skv // 64)
    return {"rise": STEP * tile, "fall": STEP * (nt - 1 - tile), "late": np.where(j == (4 * sp.skv) // 5, 30.0, 0.0),
            "hi": np.where((j >= 96) & (j < 128), STEP, 0.0), "lo": np.where((j >= 64) & (j < 96), STEP, 0.0)}[sp.profile]


def build_case(sp: Spec) -> SimpleNamespace:
    """Logical tensors of one launch as bf16-exact float32: Q, dO, O (batch, heads, sq, hd); K, V (batch, heads, skv, hd)."""
    assert sp.layout in ("sep", "packed", "kv") and (sp.layout != "packed" or sp.sq == sp.skv) and sp.hd % 8 == 0
    B, H, hd = sp.batch, sp.heads, sp.hd
    c = SimpleNamespace(spec=sp, mask=_mask(sp), rel_flat=None, rel_hs=0, rel_off=0, rel_n=0, rel_lead=8, drop_seed=1000 + sp.seed)
    c.scale = f32(1.0) if sp.scale1 else f32(1.0 / np.sqrt(f32(hd)))
    c.u = _signs(977, np.arange(H), 0, hd)
    gen = lambda name, s: _normal_rows("bwd" + name, B, H, s * hd, sp.seed).reshape(B, H, s, hd)
    q = 0.5 * gen("q", sp.sq) + c.u[None, :, None, :]
    c.Q = round_bf16((q * (f32(1.0 / np.sqrt(f32(hd))) if sp.scale1 else f32(1))).astype(f32))
    k = gen("k", sp.skv)
    if sp.profile:
        qs = 1.0 / np.sqrt(hd) if sp.scale1 else 1.0  # (q . u = hd qs on average)
        k = k + (_profile_gain(sp) / (float(c.scale) * hd * qs))[None, None, :, None] * c.u[None, :, None, :]
    c.K = round_bf16(k.astype(f32))
    c.V = round_bf16(gen("v", sp.skv))
    c.dO = round_bf16(gen("do", sp.sq))
    if sp.rel:
        need = sp.sq + sp.skv - 1
        c.rel_off, c.rel_n = {"tight": (sp.skv - 1, need), "gap": (sp.skv + 2, need + 6), "short": (sp.skv - 1 - 3, need - 7)}[sp.rel]
        assert c.rel_n > 0
        c.rel_hs = c.rel_n + (8 if sp.rel == "gap" else 0)
        tab = np.full(c.rel_lead + H * c.rel_hs + 8, np.nan, f32)
        for h in range(H):
            tab[c.rel_lead + h * c.rel_hs:c.rel_lead + h * c.rel_hs + c.rel_n] = 0.7 * _normal_rows("bwdrel", 1, H, c.rel_n, sp.seed)[0, h]
        c.rel_flat = tab
    c.O = np.zeros_like(c.Q)
    for b in range(B):
        for h in range(H):
            c.O[b, h] = round_bf16(_forward(c, b, h).astype(f32))
    return c


def _softmax(c, b, h):
    """float64 (s, vis, P, lse, live) of one (batch, head)."""
    sp = c.spec
    s = float(c.scale) * (c.Q[b, h].astype(f64) @ c.K[b, h].astype(f64).T)
    bb = bias(c, h)
    if bb is not None:
        s = s + bb.astype(f64)
    vis = visible(c, b)
    m = np.where(vis, s, -np.inf).max(1)
    live = np.isfinite(m)
    m0 = np.where(live, m, 0.0)
    e = np.where(vis, np.exp(np.where(vis, s, 0.0) - m0[:, None]), 0.0)
    l = e.sum(1)
    P = e / np.where(live, l, 1.0)[:, None]
    lse = np.where(live, m0 + np.log(np.where(live, l, 1.0)), 1e30)
    return s, vis, P, lse, live


def _forward(c, b, h):
    _, _, P, _, _ = _softmax(c, b, h)
    M = _drop64(c, b, h)
    return (P if M is None else P * M) @ c.V[b, h].astype(f64)


def _attn_bh(c, b, h):
    """Reference and bounds of one (batch, head): dict of (value, tol, fp32 part of tol, magnitude sum) per tensor."""
    sp = c.spec
    hd, sc = sp.hd, float(c.scale)
    Q, K, V, dO, O = (x[b, h].astype(f64) for x in (c.Q, c.K, c.V, c.dO, c.O))
    s, vis, P, lse, live = _softmax(c, b, h)
    M = _drop64(c, b, h)
    M = np.ones_like(P) if M is None else M
    dP = dO @ V.T
    delta = (O * dO).sum(1)
    PM = P * M
    dS = P * (M * dP - delta[:, None])
    dV, dQ, dK = PM.T @ dO, sc * (dS @ K), sc * (dS.T @ Q)
    # --- bounds
    bb = bias(c, h)
    ab = 0.0 if bb is None else np.abs(bb.astype(f64))
    e_s = np.where(vis, (hd + 2) * F * (sc * (np.abs(Q) @ np.abs(K).T) + ab), 0.0)
    ntile = -(-sp.skv // 64)
    lsef = np.where(live, lse, 0.0)
    mx = np.where(live, np.where(vis, s, -np.inf).max(1), 0.0)
    e_lse = np.where(live, (P * e_s).sum(1) + 2.0 ** -21 + (18 * ntile + 8) * F + 2.0 ** -22 * (1 + np.abs(lsef - mx)) + 4 * F * (np.abs(mx) + np.abs(lsef)), 0.0)
    eps = np.where(vis, e_s + e_lse[:, None] + 2.0 ** -22 + 2 * F * (np.abs(s) + np.abs(lsef)[:, None] + 2 * np.abs(s - lsef[:, None])), 0.0)
    e_delta = (hd / 8 + 8) * F * (np.abs(O) * np.abs(dO)).sum(1)
    e_x = (hd + 2) * F * M * (np.abs(dO) @ np.abs(V).T) + e_delta[:, None] + 2 * F * (M * np.abs(dP) + np.abs(delta)[:, None])
    mag = P * (M * (np.abs(dO) @ np.abs(V).T) + (np.abs(O) * np.abs(dO)).sum(1)[:, None])  # of the products behind dS, not of dP and delta
    dS_fp = (eps + F) * np.abs(dS) + P * e_x
    out = {"lse": (lse, e_lse, e_lse, np.abs(lsef) + 1.0), "delta": (delta, e_delta, e_delta, (np.abs(O) * np.abs(dO)).sum(1))}

    def fin(ref, bf, fp, magsum):
        return ref, (1 + U) * (bf + fp) + U * np.abs(ref), (1 + U) * fp, magsum

    out["dq"] = fin(dQ, sc * U * (np.abs(dS) @ np.abs(K)), sc * ((dS_fp + (sp.skv + 2) * F * np.abs(dS)) @ np.abs(K)), sc * (mag @ np.abs(K)))
    out["dk"] = fin(dK, sc * U * (np.abs(dS).T @ np.abs(Q)), sc * ((dS_fp + (sp.sq + 2) * F * np.abs(dS)).T @ np.abs(Q)), sc * (mag.T @ np.abs(Q)))
    out["dv"] = fin(dV, U * (PM.T @ np.abs(dO)), ((eps + (sp.sq + 2) * F) * PM).T @ np.abs(dO), PM.T @ np.abs(dO))
    return out


TENSORS = ("dq", "dk", "dv", "lse", "delta")


def reference(c):
    """{tensor: (ref, tol, fp32 part, magnitudes)}: dq (batch, heads, sq, hd), dk / dv (batch, heads, skv, hd), lse / delta (batch, heads, sq)."""
    sp = c.spec
    parts = [[_attn_bh(c, b, h) for h in range(sp.heads)] for b in range(sp.batch)]
    return {t: tuple(np.stack([np.stack([parts[b][h][t][k] for h in range(sp.heads)]) for b in range(sp.batch)]) for k in range(4)) for t in TENSORS}


def dead_rows(c):
    """(batch, sq) bool: rows without a visible key."""
    return np.stack([~visible(c, b).any(1) for b in range(c.spec.batch)])


def fp32_share(ref) -> float:
    """max over the elements of the five tensors of (fp32 part of the bound) / (sum of magnitudes)."""
    worst = 0.0
    for t in ("dq", "dk", "dv"):
        _, _, fp, mag = ref[t]
        ok = mag > 0
        if ok.any():
            worst = max(worst, float((fp[ok] / mag[ok]).max()))
    return worst


# ---- attention: memory images -----------------------------------------------------------------------------------------------------------
def pack(c) -> SimpleNamespace:
    """The launch's memory: bufs name -> int16 / int32 / float32 arrays; q / k / v / dq / dk / dv = (buffer, element offset, ld); the outputs
    hold sentinels everywhere."""
    sp = c.spec
    B, H, hd, sq, skv = sp.batch, sp.heads, sp.hd, sp.sq, sp.skv
    W = H * hd
    P = SimpleNamespace(W=W, bufs={})

    def rows(x, s):  # (B, H, s, hd) -> (B s, W)
        return x.transpose(0, 2, 1, 3).reshape(B * s, W)

    def inbuf(name, s, ld, parts):
        img = np.full((B * s + 1, ld), np.nan, f32)
        for off, x, tag in parts:
            img[:B * s, off:off + W] = rows(x, s)
            img[B * s, off:off + W] = 64.0 * _signs(tag, 0, 0, W)  # the row behind: values, not zeros
        P.bufs[name] = bf16_bits(img).reshape(-1)

    def outbuf(name, s, ld):
        P.bufs[name] = np.full((B * s + 1) * ld, np.uint16(SENT16).view(np.int16), np.int16)

    if sp.layout == "sep":
        inbuf("q", sq, W + 8, [(0, c.Q, 1)]); inbuf("k", skv, W + 16, [(0, c.K, 2)]); inbuf("v", skv, W + 24, [(0, c.V, 3)])
        outbuf("dq", sq, W + 32); outbuf("dk", skv, W + 40); outbuf("dv", skv, W + 48)
        P.q, P.k, P.v = ("q", 0, W + 8), ("k", 0, W + 16), ("v", 0, W + 24)
        P.dq, P.dk, P.dv = ("dq", 0, W + 32), ("dk", 0, W + 40), ("dv", 0, W + 48)
    elif sp.layout == "packed":
        inbuf("qkv", sq, 3 * W, [(0, c.Q, 1), (W, c.K, 2), (2 * W, c.V, 3)])
        outbuf("dqkv", sq, 3 * W)
        P.q, P.k, P.v = ("qkv", 0, 3 * W), ("qkv", W, 3 * W), ("qkv", 2 * W, 3 * W)
        P.dq, P.dk, P.dv = ("dqkv", 0, 3 * W), ("dqkv", W, 3 * W), ("dqkv", 2 * W, 3 * W)
    else:
        inbuf("q", sq, W, [(0, c.Q, 1)]); inbuf("kv", skv, 2 * W, [(0, c.K, 2), (W, c.V, 3)])
        outbuf("dq", sq, W); outbuf("dkv", skv, 2 * W)
        P.q, P.k, P.v = ("q", 0, W), ("kv", 0, 2 * W), ("kv", W, 2 * W)
        P.dq, P.dk, P.dv = ("dq", 0, W), ("dkv", 0, 2 * W), ("dkv", W, 2 * W)
    P.bufs["o"] = bf16_bits(rows(c.O, sq)).reshape(-1)
    inbuf("do", sq, W, [(0, c.dO, 4)])
    P.bufs["ws"] = np.full(2 * B * H * sq + 16, np.uint32(SENT32).view(np.int32), np.int32)
    if c.mask is not None:  # (the 3 words behind the last row say "visible")
        P.bufs["mask"] = np.concatenate([c.mask.reshape(-1), np.ones(3, np.int32)]).astype(np.int32)
    if c.rel_flat is not None:
        P.bufs["rel"] = c.rel_flat
    return P


OUT_BUFS = ("dq", "dk", "dv", "dqkv", "dkv", "ws")


def _gather(img, off, ld, B, s, H, hd):
    """(B, H, s, hd) read through (base offset, ld) as the kernels address it; an address outside the buffer reads its last element."""
    r = (np.arange(B)[:, None, None, None] * s + np.arange(s)[None, None, :, None]) * ld
    idx = off + r + np.arange(H)[None, :, None, None] * hd + np.arange(hd)[None, None, None, :]
    return np.take(img, idx, mode="clip")


def unpack(c, P, bufs):
    """({tensor: float32 array}, intact): the five outputs read back from the images, and whether every sentinel is still there."""
    sp = c.spec
    B, H, hd, sq, skv = sp.batch, sp.heads, sp.hd, sp.sq, sp.skv
    got, touched = {}, {n: np.zeros(bufs[n].shape, bool) for n in OUT_BUFS if n in bufs}
    for t, s in (("dq", sq), ("dk", skv), ("dv", skv)):
        name, off, ld = getattr(P, t)
        r = (np.arange(B)[:, None, None, None] * s + np.arange(s)[None, None, :, None]) * ld
        idx = off + r + np.arange(H)[None, :, None, None] * hd + np.arange(hd)[None, None, None, :]
        got[t] = bits_to_f32(bufs[name][idx])
        touched[name][idx] = True
    n = B * H * sq
    ws = bufs["ws"].view(f32)
    got["lse"], got["delta"] = ws[:n].reshape(B, H, sq).copy(), ws[n:2 * n].reshape(B, H, sq).copy()
    touched["ws"][:2 * n] = True
    intact = all(bool((bufs[nm][~touched[nm]].view(np.uint16 if nm != "ws" else np.uint32) == (SENT16 if nm != "ws" else SENT32)).all()) for nm in touched)
    return got, intact


# ---- attention: the kernels restated in fp32 / bf16 ---------------------------------------------------------------------------------------
def _exp(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp(x.astype(f32)).astype(f32)


def _merge(m1, l1, m2, l2, rescale=True):
    m = np.maximum(m1, m2)
    return m, ((l1 * _exp(m1 - m) + l2 * _exp(m2 - m)) if rescale else (l1 + l2)).astype(f32)


def _pass1(sm, rescale=True):
    """attn_bwd_dq_kernel pass 1: four online-softmax streams per row (key-block wave kb = (j % 64) / 32, lane half hi = (j % 8) / 4), 16 keys
    per 64-key tile each, merged half to half, then wave to wave.  sm: (sq, skv) fp32 scores, -1e30 where not visible."""
    sq, skv = sm.shape
    nt = -(-skv // 64)
    pad = np.full((sq, nt * 64), f32(-1e30), f32)
    pad[:, :skv] = sm
    pad = pad.reshape(sq, nt, 64)
    col = np.arange(64)
    st = []
    for kb in range(2):
        for hi in range(2):
            sub = pad[:, :, (col // 32 == kb) & ((col % 8) // 4 == hi)]
            m_run, l_run = np.full(sq, f32(-1e30), f32), np.zeros(sq, f32)
            for t in range(nt):
                m_new = np.maximum(m_run, sub[:, t].max(1))
                add = np.where(sub[:, t] > f32(-1e29), _exp(sub[:, t] - m_new[:, None]), f32(0)).sum(1, dtype=f32)
                l_run = ((l_run * _exp(m_run - m_new) if rescale else l_run) + add).astype(f32)
                m_run = m_new
            st.append((m_run, l_run))
    m0, l0 = _merge(*st[0], *st[1], rescale)
    m1, l1 = _merge(*st[2], *st[3], rescale)
    m, l = _merge(m0, l0, m1, l1, rescale)
    with np.errstate(divide="ignore"):
        return np.where(l > 0, (m + np.log(np.where(l > 0, l, f32(1)).astype(f32))).astype(f32), f32(1e30)).astype(f32)


ATTN_MUTATIONS = ("causal_lt", "causal_nooff", "mask0", "droplastkey", "lastrow", "nodelta", "norescale", "head0", "dk_unscaled", "dq_twice",
                  "dk_blocks", "drop_on_delta", "dv_undropped", "dropidx", "noclamp_lo", "noclamp_hi", "rel_nooff", "swap_ldk_ldv", "swap_lddk_lddv")


def emulate(c, P=None, mut: str = ""):
    """Both kernels restated on the memory image of pack(): bf16 P / dS, fp32 products and sums, pass 1's merge order, bf16 outputs written
    through (offset, ld).  Returns the output images.  `mut` plants one mistake (ATTN_MUTATIONS)."""
    assert mut == "" or mut in ATTN_MUTATIONS, mut
    sp = c.spec
    B, H, hd, sq, skv = sp.batch, sp.heads, sp.hd, sp.sq, sp.skv
    P = pack(c) if P is None else P
    bufs = {n: a.copy() for n, a in P.bufs.items()}
    (qn, qo, ldq), (kn, ko, ldk), (vn, vo, ldv) = P.q, P.k, P.v
    if mut == "swap_ldk_ldv":
        ldk, ldv = ldv, ldk
    img = lambda n: bits_to_f32(bufs[n])
    Q, K, V = _gather(img(qn), qo, ldq, B, sq, H, hd), _gather(img(kn), ko, ldk, B, skv, H, hd), _gather(img(vn), vo, ldv, B, skv, H, hd)
    O, dO = _gather(img("o"), 0, P.W, B, sq, H, hd), _gather(img("do"), 0, P.W, B, sq, H, hd)
    sc = c.scale
    lse, delta = np.zeros((B, H, sq), f32), np.zeros((B, H, sq), f32)
    keep = {}
    for b in range(B):
        vis = visible(c, b, mut)
        for h in range(H):
            s = ((Q[b, h] @ K[b, h].T).astype(f32) * sc).astype(f32)
            bb = bias(c, h, mut)
            if bb is not None:
                s = (s + bb).astype(f32)
            lse[b, h] = _pass1(np.where(vis, s, f32(-1e30)).astype(f32), mut != "norescale")
            delta[b, h] = (O[b, h] * dO[b, h]).sum(1, dtype=f32)
            keep[b, h] = (s, vis)
    res = {t: np.zeros((B, H, n, hd), f32) for t, n in (("dq", sq), ("dk", skv), ("dv", skv))}
    for b in range(B):
        for h in range(H):
            s, vis = keep[b, h]
            df = drop_factor(c, b, h, mut)
            df = np.ones((sq, skv), f32) if df is None else df
            dp = (dO[b, h] @ V[b, h].T).astype(f32)

            def probs_ds(l, d):
                with np.errstate(invalid="ignore", over="ignore"):
                    p = np.where(vis, _exp((s - l[:, None]).astype(f32)), f32(0)).astype(f32)
                    x = dp * df if mut == "nodelta" else ((dp - d[:, None]) * df if mut == "drop_on_delta" else dp * df - d[:, None])
                    return p, round_bf16((p * x.astype(f32)).astype(f32))

            _, dS = probs_ds(lse[b, h], delta[b, h])
            res["dq"][b, h] = round_bf16(((dS @ K[b, h]).astype(f32) * sc * (sc if mut == "dq_twice" else f32(1))).astype(f32))
            hh = 0 if mut == "head0" else h
            p, dSt = probs_ds(lse[b, hh], delta[b, hh])
            Pt = round_bf16(p if mut == "dv_undropped" else (p * df).astype(f32))
            if mut == "lastrow":
                Pt[sq - 1], dSt[sq - 1] = 0, 0
            res["dv"][b, h] = round_bf16((Pt.T @ dO[b, h]).astype(f32))
            acc = (dSt.T @ Q[b, h]).astype(f32)
            fk = np.full(hd, sc, f32)
            if mut == "dk_unscaled":
                fk[:] = 1
            elif mut == "dk_blocks":
                fk[64:] = 1
            res["dk"][b, h] = round_bf16((acc * fk[None, :]).astype(f32))
    outs = {"dq": P.dq, "dk": P.dk, "dv": P.dv}
    if mut == "swap_lddk_lddv":
        outs["dk"], outs["dv"] = (P.dk[0], P.dk[1], P.dv[2]), (P.dv[0], P.dv[1], P.dk[2])
    for t, s_ in (("dq", sq), ("dk", skv), ("dv", skv)):
        name, off, ld = outs[t]
        r = (np.arange(B)[:, None, None, None] * s_ + np.arange(s_)[None, None, :, None]) * ld
        idx = off + r + np.arange(H)[None, :, None, None] * hd + np.arange(hd)[None, None, None, :]
        np.put(bufs[name], idx, bf16_bits(res[t]), mode="clip")
    n = B * H * sq
    bufs["ws"][:n] = lse.reshape(-1).view(np.int32)
    bufs["ws"][n:2 * n] = delta.reshape(-1).view(np.int32)
    return bufs


def check(c, P, bufs, ref=None):
    """{tensor: worst err / tol}, intact, dead-rows-exact of one launch's output images."""
    ref = reference(c) if ref is None else ref
    got, intact = unpack(c, P, bufs)
    ratios = {t: ratio(got[t], ref[t][0], ref[t][1]) for t in ("dq", "dk", "dv", "delta")}
    dead = dead_rows(c)[:, None, :].repeat(c.spec.heads, 1)
    ratios["lse"] = ratio(got["lse"][~dead], ref["lse"][0][~dead], ref["lse"][1][~dead]) if (~dead).any() else 0.0
    exact = bool((got["lse"][dead] == f32(1e30)).all() and (got["dq"][dead] == 0).all())
    if c.mask is not None:
        for b in range(c.spec.batch):
            if not c.mask[b].any():
                exact = exact and bool((got["dk"][b] == 0).all() and (got["dv"][b] == 0).all())
    return ratios, intact, exact, got


# ---- attention: the launches of the GPU test ----------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (31, 33), (64, 64), (65, 129), (130, 130), (33, 200), (97, 40))
HDS = {2: (8, 24, 64), 3: (72, 80, 88, 96), 4: (104, 128)}
MASKS = (("left5", "right7", "holes"), ("holes", "left3", "ones"), ("right9", "dead", "left2"))


def attn_specs():
    """Every launch of test_hip_bwd.py's attention part (and of the CPU test's restatement check)."""
    out = []
    for db, hds in HDS.items():
        k = 0

        def add(tag, **kw):
            nonlocal k
            kw.setdefault("hd", hds[k % len(hds)])
            kw.setdefault("batch", 2 + k % 2)
            kw.setdefault("heads", 3 - k % 2)
            out.append(Spec(f"db{db}-{tag}", seed=k, **kw))
            k += 1

        for n, (sq, skv) in enumerate(SHAPES):  # plain: the shapes x the layouts (packed where sq == skv), masks cycled
            lay = "packed" if sq == skv else ("sep", "kv")[(n // 2) % 2]
            causal = 1 if (sq, skv) == (97, 40) else n % 2
            add(f"plain-{sq}x{skv}-{lay}", sq=sq, skv=skv, layout=lay, causal=causal, mask=MASKS[n % 3] if skv > 9 and n % 3 != 1 else ())
            if sq == skv and sq > 1:
                add(f"plain-{sq}x{skv}-sep", sq=sq, skv=skv, layout="sep", causal=1 - causal, mask=MASKS[(n + 1) % 3])
        for hd in hds:  # every head size, ragged, packed and kv
            add(f"hd{hd}-packed", hd=hd, sq=70, skv=70, layout="packed", causal=1, mask=("left5", "ones", "left70"))
            add(f"hd{hd}-kv", hd=hd, sq=33, skv=75, layout="kv", mask=("holes", "right11"))
        add("leftpad-causal", sq=66, skv=66, layout="packed", causal=1, mask=("left9", "left64", "left1"), batch=3)
        add("dead-entry", sq=40, skv=70, layout="sep", mask=("holes", "dead", "right3"), batch=3)
        add("sq-gt-skv-causal", sq=97, skv=40, layout="kv", causal=1, mask=("left3", "ones"))
        # EXTRA: rel alone
        add("rel-tight", sq=65, skv=65, layout="packed", rel="tight", scale1=True)
        add("rel-gap", sq=40, skv=100, layout="sep", rel="gap", scale1=True)
        add("rel-short", sq=50, skv=90, layout="kv", rel="short", scale1=True)
        add("rel-mask-causal", sq=70, skv=130, layout="sep", rel="tight", causal=1, mask=("left5", "holes", "right4"), scale1=True, batch=3)
        add("rel-short-mask-causal", sq=66, skv=66, layout="packed", rel="short", causal=1, mask=("left2", "holes"))
        # EXTRA: dropout alone
        add("drop01", sq=65, skv=129, layout="sep", drop=0.1)
        add("drop05-mask", sq=64, skv=64, layout="packed", drop=0.5, mask=("holes", "right5", "left3"))
        add("drop01-causal", sq=130, skv=130, layout="packed", drop=0.1, causal=1)
        add("drop05-causal-prefix", sq=33, skv=200, layout="kv", drop=0.5, causal=1, mask=("left7", "ones"))
        # EXTRA: both
        add("rel-drop", sq=66, skv=66, layout="packed", rel="tight", drop=0.1, causal=1, mask=("left4", "holes"), scale1=True)
        add("rel-gap-drop", sq=31, skv=33, layout="sep", rel="gap", drop=0.5)
        add("rel-drop-kv", sq=1, skv=1, layout="kv", rel="tight", drop=0.1)
        for prof in ("rise", "fall", "late", "hi", "lo"):  # three key tiles
            add(f"profile-{prof}", hd=hds[-1], sq=70, skv=192, layout=("sep", "kv")[k % 2], profile=prof, batch=2, heads=2)
        add("profile-rise-causal-packed", hd=hds[-1], sq=192, skv=192, layout="packed", profile="rise", causal=1, batch=2, heads=2)
        add("profile-fall-rel", hd=hds[-1], sq=64, skv=192, layout="sep", profile="fall", rel="tight", batch=2, heads=2)
    names = [sp.name for sp in out]
    assert len(set(names)) == len(names)
    return out


def coverage(specs):
    """{(DB, EXTRA, layout): launches}."""
    cov = {}
    for sp in specs:
        key = instance(sp) + (sp.layout,)
        cov[key] = cov.get(key, 0) + 1
    return cov


def assert_coverage(specs):
    cov = coverage(specs)
    for db in (2, 3, 4):
        for extra in (False, True):
            for lay in ("sep", "packed", "kv"):
                assert cov.get((db, extra, lay), 0) >= 1, f"attn_bwd<{db},{extra}> never launched in layout {lay}"
    return cov


# the planted mistake -> the GPU case that detects it (test_bwd_reference.py asserts ratio > 1 or a broken sentinel / exact-zero check there)
DETECTED_BY = {
    "causal_lt": "db3-plain-130x130-sep", "causal_nooff": "db3-sq-gt-skv-causal", "mask0": "db3-dead-entry", "droplastkey": "db3-plain-65x129-kv",
    "lastrow": "db3-plain-65x129-kv", "nodelta": "db3-plain-64x64-packed", "norescale": "db3-profile-rise", "head0": "db3-plain-64x64-packed",
    "dk_unscaled": "db3-plain-64x64-packed", "dq_twice": "db3-plain-64x64-packed", "dk_blocks": "db3-plain-64x64-packed",
    "drop_on_delta": "db3-drop05-mask", "dv_undropped": "db3-drop05-mask", "dropidx": "db3-drop01", "noclamp_lo": "db3-rel-short",
    "noclamp_hi": "db3-rel-short", "rel_nooff": "db3-rel-gap", "swap_ldk_ldv": "db3-plain-31x33-sep", "swap_lddk_lddv": "db3-plain-31x33-sep",
}


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------
def _nsum(cols):
    """fp32 roundings of one wave_sum over a row: cols / 64 sequential adds per lane and the 6-step tree (+ slack for the division)."""
    return cols / 64 + 8


def _ln_stats(x, eps):
    cols = x.shape[1]
    mean = x.mean(1)
    v = x - mean[:, None]
    var = (v * v).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    e_mean = _nsum(cols) * F * np.abs(x).mean(1)
    e_rstd = 0.5 * (_nsum(cols) * F + 2 * e_mean * rstd + 4 * F) + 2.0 ** -22  # relative (rsqrtf: 2 ulp)
    xhat = v * rstd[:, None]
    e_xhat = (e_mean * rstd)[:, None] + (e_rstd[:, None] + 3 * F) * np.abs(xhat)
    return mean, rstd, xhat, e_mean, e_rstd, e_xhat


def ln_ref(x, gamma, dy, eps, prior_g=None, prior_b=None):
    """float64 LayerNorm backward with the (mean, rstd) statistics and the bounds: dict name -> (ref, tol)."""
    x, gamma, dy = (a.astype(f64) for a in (x, gamma, dy))
    rows, cols = x.shape
    mean, rstd, xhat, e_mean, e_rstd, e_xhat = _ln_stats(x, eps)
    g = dy * gamma[None, :]
    s1, s2 = g.mean(1), (g * xhat).mean(1)
    dx = rstd[:, None] * (g - s1[:, None] - xhat * s2[:, None])
    e_s1 = _nsum(cols) * F * np.abs(g).mean(1)
    e_s2 = _nsum(cols) * F * np.abs(g * xhat).mean(1) + (np.abs(g) * e_xhat).mean(1)
    mag = np.abs(g) + np.abs(s1)[:, None] + np.abs(xhat * s2[:, None])  # the cancellation g - s1 - xhat s2: relative to the magnitudes
    fp = rstd[:, None] * (4 * F * mag + e_s1[:, None] + np.abs(xhat) * e_s2[:, None] + np.abs(s2)[:, None] * e_xhat) + (e_rstd[:, None] + F) * np.abs(dx)
    pg = np.zeros(cols) if prior_g is None else prior_g.astype(f64)
    pb = np.zeros(cols) if prior_b is None else prior_b.astype(f64)
    tg = dy * xhat
    return {"dx": (dx, (1 + U) * fp + U * np.abs(dx)),
            "dgamma": (pg + tg.sum(0), (rows + 66) * F * (np.abs(pg) + np.abs(tg).sum(0)) + (np.abs(dy) * e_xhat).sum(0)),
            "dbeta": (pb + dy.sum(0), (rows + 66) * F * (np.abs(pb) + np.abs(dy).sum(0))),
            "mean": (mean, e_mean + F * np.abs(mean)), "rstd": (rstd, e_rstd * rstd)}


def ln_emulate(x, gamma, dy, eps, prior_g=None, prior_b=None, mut=""):
    """layernorm_bwd_kernel + col_reduce_kernel<true> in fp32: dx (bf16-exact), dgamma / dbeta images of ceil32(cols) + 32 floats (SENTF
    behind cols), mean, rstd.  mut: "onepass" (variance as E[x^2] - mean^2), "noguard" (col_reduce without c < cols)."""
    rows, cols = x.shape
    x, gamma, dy = x.astype(f32), gamma.astype(f32), dy.astype(f32)
    mean = (x.sum(1, dtype=f32) / f32(cols)).astype(f32)
    v = (x - mean[:, None]).astype(f32)
    if mut == "onepass":
        var = ((x * x).sum(1, dtype=f32) / f32(cols) - mean * mean).astype(f32)
    else:
        var = ((v * v).sum(1, dtype=f32) / f32(cols)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
    xhat = (v * rstd[:, None]).astype(f32)
    g = (dy * gamma[None, :]).astype(f32)
    s1 = (g.sum(1, dtype=f32) / f32(cols)).astype(f32)
    s2 = ((g * xhat).astype(f32).sum(1, dtype=f32) / f32(cols)).astype(f32)
    dx = round_bf16((rstd[:, None] * (g - s1[:, None] - xhat * s2[:, None]).astype(f32)).astype(f32))
    wide = -(-cols // 32) * 32
    n_w = wide if mut == "noguard" else cols
    xh2 = ((x - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32)
    dg, db = np.full(wide + 32, SENTF, f32), np.full(wide + 32, SENTF, f32)
    dg[:cols] = 0 if prior_g is None else prior_g
    db[:cols] = 0 if prior_b is None else prior_b
    tg, tb = np.zeros(n_w, f32), np.zeros(n_w, f32)
    tg[:cols], tb[:cols] = (dy * xh2).astype(f32).sum(0, dtype=f32), dy.sum(0, dtype=f32)
    if n_w > cols:  # column c >= cols of row r is element c - cols of row r + 1
        over = np.take(dy.reshape(-1), np.arange(rows)[:, None] * cols + np.arange(cols, n_w)[None, :], mode="clip")
        tg[cols:], tb[cols:] = over.sum(0, dtype=f32), over.sum(0, dtype=f32)
    dg[:n_w] = (dg[:n_w] + tg).astype(f32)
    db[:n_w] = (db[:n_w] + tb).astype(f32)
    return {"dx": dx, "dgamma": dg, "dbeta": db, "mean": mean, "rstd": rstd}


def rms_ref(x, gamma, dy, eps):
    """T5LayerNorm forward y and dx: name -> (ref, tol).  The forward rounds x rstd to bf16 before gamma (hf casts there): two roundings."""
    x, gamma, dy = (a.astype(f64) for a in (x, gamma, dy))
    cols = x.shape[1]
    rstd = 1.0 / np.sqrt((x * x).mean(1) + eps)
    e_rstd = 0.5 * (_nsum(cols) + 4) * F + 2.0 ** -22
    xhat = x * rstd[:, None]
    y = gamma[None, :] * xhat
    g = dy * gamma[None, :]
    s2 = (g * xhat).mean(1)
    dx = rstd[:, None] * (g - xhat * s2[:, None])
    e_xhat = (e_rstd + 2 * F) * np.abs(xhat)
    e_s2 = _nsum(cols) * F * np.abs(g * xhat).mean(1) + (np.abs(g) * e_xhat).mean(1)
    mag = np.abs(g) + np.abs(xhat * s2[:, None])
    fp = rstd[:, None] * (4 * F * mag + np.abs(xhat) * e_s2[:, None] + np.abs(s2)[:, None] * e_xhat) + (e_rstd + F) * np.abs(dx)
    return {"y": (y, (2 * U + U * U + 2 * (e_rstd + 2 * F)) * np.abs(y)), "dx": (dx, (1 + U) * fp + U * np.abs(dx))}


def rms_emulate(x, gamma, dy, eps):
    cols = x.shape[1]
    x, gamma, dy = x.astype(f32), gamma.astype(f32), dy.astype(f32)
    rstd = (f32(1) / np.sqrt(((x * x).sum(1, dtype=f32) / f32(cols) + f32(eps)).astype(f32))).astype(f32)
    xhat = (x * rstd[:, None]).astype(f32)
    y = round_bf16((gamma[None, :] * round_bf16(xhat)).astype(f32))
    g = (dy * gamma[None, :]).astype(f32)
    s2 = ((g * xhat).astype(f32).sum(1, dtype=f32) / f32(cols)).astype(f32)
    return {"y": y, "dx": round_bf16((rstd[:, None] * (g - xhat * s2[:, None]).astype(f32)).astype(f32))}


def colsum_ref(dy, prior):
    dy, prior = dy.astype(f64), prior.astype(f64)
    return prior + dy.sum(0), (dy.shape[0] + 258) * F * (np.abs(prior) + np.abs(dy).sum(0))


def _erf(x):
    from math import erf
    return np.vectorize(erf, otypes=[f64])(x)


GELU_POLY_ABS = 2e-4  # common.h gelu_erf: degree-12 polynomial, max abs error (tests/test_gelu_poly.py)


def act_ref(pre, dy, kind):
    """kind 1 erf-GELU, 2 ReLU: name -> (ref, tol)."""
    x, g = pre.astype(f64), dy.astype(f64)
    if kind == 1:
        cdf = 0.5 * (1.0 + _erf(x / np.sqrt(2.0)))
        pdf = np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
        y, d = x * cdf, cdf + x * pdf
        ty = U * np.abs(y) + GELU_POLY_ABS * (1 + U)
        # cdf = 0.5 (1 + erff) is a cancellation for x < 0: erff's 4 ulp of 1 and the add's rounding are ABSOLUTE, 2^-22 after the 0.5;
        # x pdf: __expf with a 2^-24-relative argument x^2 / 2 and the products
        td = 2.0 ** -22 + 2.0 ** -20 * (cdf + np.abs(x) * pdf * (1 + x * x))
    else:
        y, d = np.maximum(x, 0.0), (x > 0).astype(f64)
        ty, td = U * np.abs(y), 0.0
    dx = g * d
    return {"y": (y, ty), "dx": (dx, (1 + U) * np.abs(g) * td + U * np.abs(dx))}


def _gelu_new(x):
    k = 0.79788456080286535588
    u = k * (x + 0.044715 * x ** 3)
    t = np.tanh(u)
    return 0.5 * x * (1 + t), 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x), t


def gated_ref(ab, dy, f):
    """out = gelu_new(a) b, dab = [dy b gelu_new'(a) | dy gelu_new(a)]: name -> (ref, tol).  t = 1 - 2 / (1 + e^{2u}) is a cancellation for small u:
    its fp32 error is absolute (4 F from the two roundings of terms near 1, plus __expf's 2^-21 relative on 2 / (1 + e)), so the bound of act
    and act' carries it times |x| / 2, never relative to the result."""
    a, b, g = ab[:, :f].astype(f64), ab[:, f:].astype(f64), dy.astype(f64)
    act, dact, t = _gelu_new(a)
    e_t = 8 * F + 2.0 ** -20 * (1 - np.abs(t)) * (1 + np.abs(a) * (1 + a * a))
    e_act = 0.5 * np.abs(a) * e_t + 4 * F * np.abs(act)
    k = 0.79788456080286535588
    w = 0.5 * np.abs(a) * k * (1 + 3 * 0.044715 * a * a)
    e_dact = 0.5 * e_t + w * 2 * np.abs(t) * e_t + 8 * F * (0.5 * (1 + np.abs(t)) + w * (1 - t * t)) + w * 4 * F
    out = act * b
    da, db = g * b * dact, g * act
    return {"out": (out, (1 + U) ** 2 * np.abs(b) * e_act + (2 * U + U * U) * np.abs(out)),  # bf16(bf16(gelu_new(a)) b): two roundings (hf's bf16 graph)
            "dab": (np.concatenate([da, db], 1), np.concatenate([(1 + U) * np.abs(g * b) * (e_dact + 2 * F * np.abs(dact)) + U * np.abs(da),
                                                                 (1 + U) * np.abs(g) * e_act + U * np.abs(db)], 1))}


def gated_emulate(ab, dy, f):
    a, b, g = ab[:, :f].astype(f32), ab[:, f:].astype(f32), dy.astype(f32)
    k = f32(0.79788456080286535588)
    u = (k * (a + f32(0.044715) * a * a * a).astype(f32)).astype(f32)
    t = (f32(1) - f32(2) / (f32(1) + _exp((f32(2) * u).astype(f32)))).astype(f32)
    act = (f32(0.5) * a * (f32(1) + t)).astype(f32)
    dact = (f32(0.5) * (f32(1) + t) + f32(0.5) * a * (f32(1) - t * t) * k * (f32(1) + f32(3) * f32(0.044715) * a * a)).astype(f32)
    return {"out": round_bf16((round_bf16(act) * b).astype(f32)), "dab": round_bf16(np.concatenate([g * b * dact, g * act], 1).astype(f32))}


def ce_ref(logits, targets, grad_scale):
    """row_loss and dlogits (bf16): name -> (ref, tol).  Ignored (< 0) and out-of-range (>= vocab) targets give zeros and loss 0."""
    rows, vocab = logits.shape
    x = logits.astype(f64)
    gs = float(f32(grad_scale))
    live = (targets >= 0) & (targets < vocab)
    t = np.where(live, targets, 0)
    mx = x.max(1)
    e = np.exp(x - mx[:, None])
    ssum = e.sum(1)
    lse = mx + np.log(ssum)
    xt = x[np.arange(rows), t]
    loss = np.where(live, lse - xt, 0.0)
    e_sum = (vocab / 256 + 12) * F + 2.0 ** -21  # relative: the strided per-thread sums, the wave and block reductions, __expf
    p = e / ssum[:, None]
    d = p * gs
    onehot = np.zeros_like(d)
    onehot[np.arange(rows), t] = gs
    eps_p = e_sum + 2.0 ** -21 + 2 * F * np.abs(x - mx[:, None]) + 4 * F
    fp = eps_p * np.abs(d) + 2 * F * onehot * (1 + p)  # softmax - onehot at the target: relative to the magnitudes p gs + gs
    d = d - onehot
    tol_d = (1 + U) * fp + U * np.abs(d)
    tol_l = e_sum + 2.0 ** -22 * (1 + np.abs(np.log(ssum))) + 4 * F * (np.abs(mx) + np.abs(lse) + np.abs(xt))
    return {"loss": (loss, np.where(live, tol_l, 0.0)), "dlogits": (np.where(live[:, None], d, 0.0), np.where(live[:, None], tol_d, 0.0))}


def ce_emulate(logits, targets, grad_scale, mut=""):
    """ce_loss_kernel in fp32.  mut: "inv" (non-target entries scaled by 1 + 2^-5), "tplus1" (the target's - grad_scale one column late)."""
    rows, vocab = logits.shape
    x = logits.astype(f32)
    gs = f32(grad_scale)
    live = (targets >= 0) & (targets < vocab)
    t = np.where(live, targets, 0)
    mx = x.max(1)
    e = _exp((x - mx[:, None]).astype(f32))
    ssum = e.sum(1, dtype=f32)
    inv = (gs / ssum).astype(f32)
    d = (e * inv[:, None]).astype(f32)
    if mut == "inv":
        tgt = d[np.arange(rows), t].copy()
        d = (d * f32(1 + 2.0 ** -5)).astype(f32)
        d[np.arange(rows), t] = tgt
    tt = np.minimum(t + 1, vocab - 1) if mut == "tplus1" else t
    d[np.arange(rows), tt] -= gs
    loss = ((mx + np.log(ssum).astype(f32)).astype(f32) - x[np.arange(rows), t]).astype(f32)
    return {"loss": np.where(live, loss, f32(0)).astype(f32), "dlogits": round_bf16(np.where(live[:, None], d, f32(0)).astype(f32))}


def dropout_add_ref(x, resid, p, seed):
    """y = bf16(x M / (1 - p)) + resid: (ref, tol, keep).  The dropped value is rounded to bf16 before the residual add."""
    keep = keep_mask(seed, np.arange(x.size), p).reshape(x.shape)
    kept = np.where(keep, x.astype(f64) / (1.0 - float(f32(p))), 0.0)
    if resid is None:
        return kept, (U + 4 * F) * np.abs(kept), keep
    y = kept + resid.astype(f64)
    return y, (1 + U) * (U + 4 * F) * np.abs(kept) + U * np.abs(y), keep


def dropout_add_emulate(x, resid, p, seed):
    keep = keep_mask(seed, np.arange(x.size), p).reshape(x.shape)
    kept = np.where(keep, (x.astype(f32) * (f32(1) / (f32(1) - f32(p)))).astype(f32), f32(0)).astype(f32)
    return round_bf16(kept) if resid is None else round_bf16((round_bf16(kept) + resid.astype(f32)).astype(f32))


LN_COLS = (8, 1000, 1536, 1544, 2560, 2568, 4088, 4096)
LN_ROWS = (1, 5, 67)
CE_VOCABS = (7, 255, 256, 257, 1000, 50272)


def row_inputs(name, rows, cols, seed=0, offset=0.0, scale=1.0):
    return round_bf16((offset + scale * _normal_rows("bwdrow" + name, 1, 1, rows * cols, seed).reshape(rows, cols)).astype(f32))


def ln_inputs(rows, cols, seed=0):
    """x (the odd rows are 100 + noise: a variance taken in one pass loses them), gamma, dy, prior dgamma / dbeta."""
    x = row_inputs("x", rows, cols, seed, 0.3, 2.0)
    x[1::2] = row_inputs("x100", rows, cols, seed, 100.0, 1.0)[1::2]
    gamma = row_inputs("g", 1, cols, seed, 1.0, 0.2)[0]
    dy = row_inputs("dy", rows, cols, seed)
    pg = _normal_rows("bwdrowpg", 1, 1, cols, seed)[0, 0]
    pb = _normal_rows("bwdrowpb", 1, 1, cols, seed)[0, 0]
    return x, gamma, dy, pg, pb


def ce_inputs(vocab, seed=0):
    """8 rows: targets -100, 0, vocab - 1, vocab (out of range), ordinary ones; row 5 has one logit of +80, row 6 all logits -80."""
    rows = 8
    logits = (3.0 * _normal_rows("bwdrowlg", 1, 1, rows * vocab, seed).reshape(rows, vocab)).astype(f32)
    tgt = np.array([-100, 0, vocab - 1, vocab, vocab // 2, min(3, vocab - 1), vocab // 3, (2 * vocab) // 3], np.int64)
    logits[5, min(5, vocab - 1)] = 80.0
    logits[6, :] = -80.0
    return logits, tgt, f32(1.0 / 6.0)
