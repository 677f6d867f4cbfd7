"""The fp8 KV cache of include/eilev_kv8.h restated: the quantiser in torch, and the reference, case builder, tolerance and planted
mistakes of the attention kernel's tests (test_kv8_ref.py on the CPU, test_hip_kv8.py on the GPU).  A plain module: no fixtures, no GPU;
a sibling of attn_decode_ref.py, whose generic helpers it imports.

The format.  One scale 2^e per vector of hd elements, e the smallest integer with amax <= 448 * 2^e, e >= -126; stored as the byte
e + 127; amax == 0 or a non-finite amax: byte 127.  Element byte = e4m3_rne(x * 2^-e).  dequantize() = e4m3 * 2^e is exactly a bf16 value.

Reference: numpy float64 softmax attention over the DEQUANTISED planes (exact in float64: the quantisation loss is not part of the bound),
no scale factor; with fuse_new the newest slot kv_total - 1 is taken from the bf16 q|k|v row.  Visible: j < kv_total and (j >= seq_len, or
no mask, or mask[row][j] != 0).  A row with no visible key gives zeros.  A_i = sum_j p_j |v_ji| / sum_j p_j.

Tolerance (derived from attn_decode8_kernel's arithmetic, not measured): tol_i = TOL_REL * A_i with attn_decode_ref's TOL_REL = 2^-8 +
2^-11, because the kernel adds NO rounding to the bf16 decode kernels':
 * e4m3 -> fp32 is exact; the score is a fp32 dot of <= 128 products times 2^ek (a power of two: exact) — the fp32 term of the bf16 kernels;
 * P is rounded to bf16 for the product (2^-9 A_i), then multiplied by 2^ev (exact); the row sum comes from the unrounded P;
 * o accumulates in fp32, the ranges' partials are merged with fp32 weights exp(m_r - M) <= 1 (fp32 terms, with the dot, exp and the sums
   over <= 1025 keys under 2^-11 A_i together, as in attn_decode_ref.py);
 * the output is rounded to bf16 once: 2^-9 (1 + 2^-9) A_i.
Where the derivation holds (attn_prefill_ref.py, "where the derivation holds"): the output term needs A_i >= the top of the binade of
|out_i|, and a spike's probability need not be the range's maximum, so its own rounding reaches 2^-8 * 8 w.  The inputs are narrowed for
it as there, not the bound: every ordinary value has |v| in [4, 7.5] (on the e4m3 grid for either scale), every (row, head) with two or
more visible keys owns ONE spike key of softmax weight w in [W_LO, W_HI) = [0.45, 0.5) with v = +-8, element by element the sign that
opposes the weighted mean of the row's other visible values: |out_i| = 8 w - (1 - w) |rest_i| < 4 <= 5.9 <= A_i.  A (row, head) with one
visible key has weight 1 and out = its v exactly.

Planted keys.  Spike: k_j = Q(q t / |q|^2) — the quantised form, or bf16 for the newest slot of a fuse_new launch — with t scanned until
the weight of the key AS STORED lies in [W_LO, W_HI).  Trap: a masked prompt key scores >= 25 above the row's maximum and has v = +-64.
Unwritten slots (at or beyond kv_total, and the newest slot of a fuse_new launch) hold the byte 0x7F (e4m3 NaN) and the exponent 0xFF
(2^128 = inf in the kernel): any read of them that reaches a result shows up as a non-finite output."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from attn_decode_ref import TOL_FLOOR, TOL_REL, _normal_rows, _signs, bf16_bits, bits_to_f32, tolerance, worst_ratio  # noqa: F401 (re-exported)
from eilev_amd.synth import _splitmix64, round_bf16

E4M3_MAX = 448.0
E_MIN = -126
RANGE = 256                # keys per workgroup of attn_decode8_kernel (EILEV_KV8_RANGE)
NAN_BYTE, NAN_EXP = 0x7F, 0xFF
W_TARGET, W_LO, W_HI = 0.483, 0.45, 0.5
MASK_KINDS = ("left0", "left1", "left300", "holes", "dead")  # dead: every prompt key masked


# ---- the quantiser -------------------------------------------------------------------------------------------------------------------------
def exponents(amax: torch.Tensor) -> torch.Tensor:
    """e (int32) per amax: the smallest integer with amax <= 448 * 2^e = 0.875 * 2^(9 + e), clamped to e >= -126; 0 for amax == 0 or non-finite."""
    amax = amax.float()
    m, x = torch.frexp(amax)  # amax = m * 2^x, m in [0.5, 1)
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp(min=E_MIN)
    return torch.where((amax == 0) | ~torch.isfinite(amax), torch.zeros_like(e), e).to(torch.int32)


def quantize(x: torch.Tensor):
    """x (..., hd) -> (bytes (..., hd) uint8, exponent bytes (...) uint8)."""
    xf = x.float()
    e = exponents(xf.abs().amax(-1))
    scaled = xf * torch.ldexp(torch.ones_like(xf[..., 0]), -e)[..., None]  # = x.float() * 2.0 ** -e, exact
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), (e + 127).to(torch.uint8)


def dequantize(b: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    """e4m3 * 2^e as float32 (exactly a bf16 value)."""
    return b.view(torch.float8_e4m3fn).float() * torch.ldexp(torch.ones(exps.shape, device=exps.device), exps.to(torch.int32) - 127)[..., None]


def _q_np(x: np.ndarray):
    b, e = quantize(torch.from_numpy(np.ascontiguousarray(x, np.float32)))
    return b.numpy(), e.numpy()


def _dq_np(b: np.ndarray, e: np.ndarray) -> np.ndarray:
    return dequantize(torch.from_numpy(np.ascontiguousarray(b)), torch.from_numpy(np.ascontiguousarray(e))).numpy()


# ---- a case ----------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    name: str
    hd: int = 80
    batch: int = 3
    heads: int = 3
    n: int = 257              # kv_total
    gen: object = None        # None: state == nullptr, seq_len = n, fuse_new = 0; g >= 1: state[0] = g, seq_len = n - g, fuse_new = 1
    extra_cap: int = 5        # unwritten slots behind kv_total
    mask: str = "none"        # "none" (null pointer), "mixed" (rows cycle through MASK_KINDS from mask_first)
    mask_first: int = 0
    spikes: object = "mix"    # "mix", ("cover", k)
    ldq_extra: int = 0
    seed: int = 0

    @property
    def seq_len(self):
        return self.n if self.gen is None else self.n - self.gen

    @property
    def fuse_new(self):
        return 0 if self.gen is None else 1

    @property
    def cap(self):
        return self.n + self.extra_cap


def _mask(sp: Spec):
    if sp.mask == "none" or sp.seq_len == 0:
        return None
    m = np.ones((sp.batch, sp.seq_len), np.int32)
    j = np.arange(sp.seq_len, dtype=np.uint64)
    for r in range(sp.batch):
        kind = MASK_KINDS[(r + sp.mask_first) % len(MASK_KINDS)]
        if kind.startswith("left"):
            m[r, :min(int(kind[4:]), max(sp.seq_len - 1, 0))] = 0  # (left padding keeps one prompt key)
        elif kind == "holes":
            with np.errstate(over="ignore"):
                m[r, (_splitmix64(j + np.uint64(7919 * (r + 1) + sp.seed)) % np.uint64(10)) < np.uint64(3)] = 0
            m[r, :min(3, sp.seq_len - 1)] = 0
            m[r, sp.seq_len - 1] = 1
        else:
            m[r, :] = 0
    return m


def _visible(sp: Spec, mask, b):
    vis = np.ones(sp.n, bool)
    if mask is not None:
        vis[:sp.seq_len] = mask[b, :sp.seq_len] != 0
    return vis


def _spike_slot(sp: Spec, b, h, vis):
    idx = b * sp.heads + h
    visible = np.flatnonzero(vis)
    if len(visible) == 0:
        return -1
    with np.errstate(over="ignore"):
        r = int(_splitmix64(np.array([idx * 2654435761 + sp.seed * 97 + sp.n], np.uint64))[0] >> np.uint64(16))
    anyone = int(visible[r % len(visible)])
    if isinstance(sp.spikes, tuple):  # ("cover", k): launch k of a set in which every slot is some (row, head)'s spike
        j = sp.spikes[1] * sp.batch * sp.heads + idx
        return j if j < sp.n and vis[j] else anyone
    last_of_range = ((sp.n - 1) // RANGE) * RANGE - 1  # the last key of the last FULL range
    # the newest key, the last key of a full range, the first visible key (behind the padding), the key at seq_len, any visible one
    pick = [sp.n - 1, last_of_range if last_of_range >= 0 and vis[last_of_range] else anyone, int(visible[0]),
            sp.seq_len if sp.seq_len < sp.n else anyone, anyone][idx % 5]
    return pick


def build_case(sp: Spec) -> SimpleNamespace:
    """One launch: the q|k|v rows (bf16-exact float32), the byte and exponent planes with spikes and traps planted and the unwritten slots
    poisoned, their dequantised twin, the mask and the state word."""
    H, hd, B, n, cap = sp.heads, sp.hd, sp.batch, sp.n, sp.cap
    d = H * hd
    assert 1 <= n <= cap and 0 <= sp.seq_len and (sp.gen is None or sp.gen >= 1)
    c = SimpleNamespace(spec=sp, d=d, n=n, ldq=3 * d + sp.ldq_extra, mask=_mask(sp))
    rows = _normal_rows("kv8.qkv", B, H, 3 * hd, sp.seed).reshape(B, H, 3, hd)
    q = round_bf16(0.35 * rows[:, :, 0])
    grid = lambda name, shape_n: (4.0 + 0.5 * (np.abs(_normal_rows(name, B, H, shape_n, sp.seed)) * 1e4 % 8).astype(np.int64)).astype(np.float32)
    knew = round_bf16(rows[:, :, 1])
    vnew = grid("kv8.vnew", hd) * np.sign(rows[:, :, 2] + 1e-30).astype(np.float32)
    K = round_bf16(_normal_rows("kv8.k", B, H, cap * hd, sp.seed)).reshape(B, H, cap, hd)
    vs = _normal_rows("kv8.vs", B, H, cap * hd, sp.seed).reshape(B, H, cap, hd)
    V = grid("kv8.v", cap * hd).reshape(B, H, cap, hd) * np.where(vs >= 0, 1.0, -1.0).astype(np.float32)
    hh = np.arange(H)[:, None]
    q64 = q.astype(np.float64)
    qq = (q64 * q64).sum(-1)  # (B, H)
    new = n - 1 if sp.fuse_new else -1
    c.spike_pos = np.full((B, H), -1, np.int64)
    c.spike_w = np.full((B, H), np.nan)
    # traps on the masked prompt keys (before the spikes: a spike's score is about the log-sum-exp of the others, <= max + log n)
    Kd = _dq_np(*_q_np(K))
    for b in range(B):
        vis = _visible(sp, c.mask, b)
        if vis.all():
            continue
        s = np.einsum("hd,hnd->hn", q64[b], Kd[b, :, :n].astype(np.float64))
        if new >= 0:
            s[:, new] = (q64[b] * knew[b]).sum(-1)
        smax = np.where(vis[None, :], s, -np.inf).max(1) if vis.any() else np.zeros(H)
        jm = np.flatnonzero(~vis)
        K[b][:, jm] = round_bf16((q64[b] * ((smax + 30.0) / qq[b])[:, None]).astype(np.float32))[:, None, :]
        V[b][:, jm] = 64.0 * _signs(b, hh, jm[None, :], hd)
    k8, ek = _q_np(K)
    v8, ev = _q_np(V)
    Kd, Vd = _dq_np(k8, ek), _dq_np(v8, ev)
    delta = np.linspace(-0.6, 0.6, 481)
    for b in range(B):
        vis = _visible(sp, c.mask, b)
        for h in range(H):
            j = _spike_slot(sp, b, h, vis)
            if j < 0:
                continue
            c.spike_pos[b, h] = j
            Ke, Ve = Kd[b, h, :n].astype(np.float64), Vd[b, h, :n].astype(np.float64)
            if new >= 0:
                Ke[new], Ve[new] = knew[b, h], vnew[b, h]
            others = vis.copy()
            others[j] = False
            sign = _signs(b, h, j, hd)
            if not others.any():  # a single visible key: weight 1
                c.spike_w[b, h] = 1.0
                cand_k = round_bf16((q[b, h] / np.float32(qq[b, h])).astype(np.float32))
            else:
                so = Ke[others] @ q64[b, h]
                lse = float(so.max() + np.log(np.exp(so - so.max()).sum()))
                rest = np.exp(so - so.max()) @ Ve[others]
                sign = np.where(rest > 0, -1.0, np.where(rest < 0, 1.0, sign)).astype(np.float32)
                t = lse + np.log(W_TARGET / (1.0 - W_TARGET)) + delta
                cand = round_bf16((q64[b, h][None, :] * (t / qq[b, h])[:, None]).astype(np.float32))
                stored = cand if j == new else _dq_np(*_q_np(cand))
                w = 1.0 / (1.0 + np.exp(lse - stored.astype(np.float64) @ q64[b, h]))
                best = int(np.argmin(np.abs(w - W_TARGET)))
                assert W_LO <= w[best] < W_HI, (sp.name, b, h, j, w[best])
                c.spike_w[b, h] = w[best]
                cand_k = cand[best]
            if j == new:
                knew[b, h], vnew[b, h] = cand_k, 8.0 * sign
            else:
                K[b, h, j], V[b, h, j] = cand_k, 8.0 * sign
                k8[b, h, j], ek[b, h, j] = _q_np(K[b, h, j])
                v8[b, h, j], ev[b, h, j] = _q_np(V[b, h, j])
    Kd, Vd = _dq_np(k8, ek), _dq_np(v8, ev)
    # what the launch must not read: slots at / beyond kv_total, and the newest slot of a fuse_new launch (the kernel writes it)
    dead = np.zeros(cap, bool)
    dead[n:] = True
    if new >= 0:
        dead[new] = True
    k8[:, :, dead], v8[:, :, dead], ek[:, :, dead], ev[:, :, dead] = NAN_BYTE, NAN_BYTE, NAN_EXP, NAN_EXP
    Kd[:, :, dead], Vd[:, :, dead] = np.nan, np.nan
    c.qkv = np.zeros((B, c.ldq), np.float32)
    c.qkv[:, :d] = q.reshape(B, d)
    if sp.fuse_new:
        c.qkv[:, d:2 * d], c.qkv[:, 2 * d:3 * d] = knew.reshape(B, d), vnew.reshape(B, d)
    c.k8, c.v8, c.ek, c.ev, c.kd, c.vd = k8, v8, ek, ev, Kd, Vd
    return c


def effective(c, b: int):
    """What row b attends to: K, V (heads, kv_total, hd) float64 and visible (kv_total,)."""
    sp, n, hd = c.spec, c.n, c.spec.hd
    K, V = c.kd[b, :, :n].astype(np.float64), c.vd[b, :, :n].astype(np.float64)
    if sp.fuse_new:
        K[:, n - 1] = c.qkv[b, c.d:2 * c.d].reshape(sp.heads, hd)
        V[:, n - 1] = c.qkv[b, 2 * c.d:3 * c.d].reshape(sp.heads, hd)
    return K, V, _visible(sp, c.mask, b)


def _q(c, b):
    return c.qkv[b, :c.d].reshape(c.spec.heads, c.spec.hd).astype(np.float64)


def _attend(s, V, vis):
    """softmax over the visible keys of scores s (heads, n) times V: (out, A), zeros without a visible key."""
    H, hd = V.shape[0], V.shape[2]
    if not vis.any():
        return np.zeros((H, hd)), np.zeros((H, hd))
    s = s[:, vis]
    p = np.exp(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return np.einsum("hn,hnd->hd", p, V[:, vis]), np.einsum("hn,hnd->hd", p, np.abs(V[:, vis]))


def reference(c):
    """(out, A): (batch, heads * hd) float64."""
    sp = c.spec
    out, A = np.zeros((sp.batch, sp.heads, sp.hd)), np.zeros((sp.batch, sp.heads, sp.hd))
    for b in range(sp.batch):
        K, V, vis = effective(c, b)
        out[b], A[b] = _attend(np.einsum("hd,hnd->hn", _q(c, b), K), V, vis)
    return out.reshape(sp.batch, c.d), A.reshape(sp.batch, c.d)


# ---- planted mistakes: the attention with ONE index or scale mistake of the kind the kernel could make, in float64 -------------------------------
MUTATIONS = ("k_exp_neighbour", "v_exp_from_k", "no_scale", "exp_plus_one", "new_from_cache", "seq_len_key_masked", "masked_visible",
             "range_last_dropped", "next_head", "merge_no_rescale")


def applies(mut: str, sp: Spec) -> bool:
    if mut == "new_from_cache":
        return bool(sp.fuse_new)
    if mut == "seq_len_key_masked":
        return sp.seq_len < sp.n
    if mut == "masked_visible":
        return sp.mask != "none" and sp.seq_len > 1
    if mut in ("range_last_dropped", "merge_no_rescale"):
        return sp.n > RANGE
    if mut == "k_exp_neighbour":
        return sp.n > 1
    return True


def mutated(c, mut: str):
    """(batch, heads * hd) float64: the reference's arithmetic with the mistake `mut`."""
    sp, n, hd, H = c.spec, c.n, c.spec.hd, c.spec.heads
    out = np.zeros((sp.batch, H, hd))
    f8 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    pow2 = lambda e: np.ldexp(1.0, e.astype(np.int64) - 127)
    new = n - 1 if sp.fuse_new else -1
    for b in range(sp.batch):
        with np.errstate(invalid="ignore", over="ignore"):
            k8, v8, ek, ev = c.k8[b, :, :n], c.v8[b, :, :n], c.ek[b, :, :n], c.ev[b, :, :n]
            if mut == "next_head":
                k8, v8, ek, ev = (np.roll(a, -1, axis=0) for a in (k8, v8, ek, ev))
            if mut == "k_exp_neighbour":
                ek = np.concatenate([ek[:, 1:], ek[:, :1]], 1)
            if mut == "v_exp_from_k":
                ev = ek
            sk, sv = pow2(ek), pow2(ev)
            if mut == "no_scale":
                sk, sv = np.ones_like(sk), np.ones_like(sv)
            if mut == "exp_plus_one":
                sk, sv = 2 * sk, 2 * sv
            K, V = f8(k8) * sk[..., None], f8(v8) * sv[..., None]
        if new >= 0:
            row = lambda o: c.qkv[b, o * c.d:(o + 1) * c.d].reshape(H, hd).astype(np.float64)
            K[:, new], V[:, new] = row(1), row(2)
            if mut == "new_from_cache":  # what a LATER step reads in that slot: the quantised form of the row
                K[:, new], V[:, new] = _dq_np(*_q_np(row(1))), _dq_np(*_q_np(row(2)))
        vis = _visible(sp, c.mask, b)
        if mut == "seq_len_key_masked":
            vis[sp.seq_len] = False
        if mut == "masked_visible" and not vis[:sp.seq_len].all():
            vis[np.flatnonzero(~vis[:sp.seq_len])[-1]] = True
        if mut == "range_last_dropped":
            vis[RANGE - 1::RANGE] = False
        s = np.einsum("hd,hnd->hn", _q(c, b), np.nan_to_num(K))
        if mut == "merge_no_rescale":  # every range's (sum, o) relative to its OWN maximum, added up as they are
            l, o = np.zeros(H), np.zeros((H, hd))
            for k0 in range(0, n, RANGE):
                v = vis[k0:k0 + RANGE]
                if not v.any():
                    continue
                sr = s[:, k0:k0 + RANGE][:, v]
                p = np.exp(sr - sr.max(1, keepdims=True))
                l += p.sum(1)
                o += np.einsum("hn,hnd->hd", p, V[:, k0:k0 + RANGE][:, v])
            out[b] = o / np.where(l > 0, l, 1.0)[:, None]
        else:
            out[b] = _attend(s, np.nan_to_num(V), vis)[0]
    return out.reshape(sp.batch, c.d)


# ---- the launches of the GPU test -----------------------------------------------------------------------------------------------------------
SWEEP = (1, 2, 255, 256, 257, 511, 512, 513, 1025)


def _cases():
    out = []
    for hd in (80, 128):
        for n in SWEEP:
            batch = 1 if n in (2, 256, 513) else 3
            for by in ("seq", "state"):
                gen = None if by == "seq" else max(1, n - n // 2)
                masked = n >= 255 and (by == "state" or n % 2 == 1)
                out.append(Spec(name=f"sweep-hd{hd}-n{n}-{by}", hd=hd, batch=batch, n=n, gen=gen, extra_cap=0 if n % RANGE == 0 else 5,
                                mask="mixed" if masked else "none", mask_first=n % 5, ldq_extra=8 if n % 2 else 0, seed=n))
        # every mask kind in one launch of 32 rows: a prompt of 527 keys + 3 generated, and a prompt alone
        out.append(Spec(name=f"mask-hd{hd}-state", hd=hd, batch=32, n=530, gen=3, mask="mixed", seed=1))
        out.append(Spec(name=f"mask-hd{hd}-seq", hd=hd, batch=32, n=530, gen=None, mask="mixed", mask_first=2, seed=2))
        # every slot of a 288-key cache (a full range and a part of the next) is the spike of some (row, head)
        for k in range(3):
            out.append(Spec(name=f"cover-hd{hd}-{k}", hd=hd, batch=32, n=288, gen=1, extra_cap=0, spikes=("cover", k), seed=3 + k))
    return out


CASES = _cases()


def by_name(name: str) -> Spec:
    return next(sp for sp in CASES if sp.name == name)


def pack(c):
    """The launch's buffers as numpy arrays in device layout: qkv as bf16 bits (int16), the planes as uint8, the mask, state = (gen, 0)."""
    sp = c.spec
    return SimpleNamespace(qkv=bf16_bits(c.qkv), k8=c.k8.copy(), v8=c.v8.copy(), ek=c.ek.copy(), ev=c.ev.copy(),
                           mask=None if c.mask is None else c.mask.copy(), state=None if sp.gen is None else np.array([sp.gen, 0], np.int32))


def new_slot_expected(c):
    """(k bytes, k exponent, v bytes, v exponent) of the newest slot after a fuse_new launch: quantize() of the step's rows, (batch, heads, ...)."""
    sp = c.spec
    row = lambda o: c.qkv[:, o * c.d:(o + 1) * c.d].reshape(sp.batch, sp.heads, sp.hd)
    return (*_q_np(row(1)), *_q_np(row(2)))


__all__ = [n for n in dir() if not n.startswith("__")]
