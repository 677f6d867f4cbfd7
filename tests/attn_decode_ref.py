"""Reference, case builder and tolerance of the decode-attention kernel tests (test_attn_decode_reference.py on the CPU,
test_hip_attn_decode.py on the GPU).  A plain module: no fixtures, no GPU.

Reference: numpy float64 on the bf16-exact inputs, softmax(q . k_j + bias_j over the visible j) . v, no scale factor (the kernels apply
none).  Visible: j < kv_total and (j >= seq_len, or no mask, or mask[row][j] != 0).  A row with no visible key gives zeros.

Tolerance (derived, not measured).  The kernels round P to bf16 for the product, take the row sum from the unrounded P and round the
output to bf16.  With A_i = sum_j p_j |v_ji| / sum_j p_j the error of output element i is at most 2^-9 A_i (P) + 2^-9 (1 + 2^-9) A_i
(output); the fp32 terms (score dots of <= 128 products, __expf, sums over <= 2304 keys: each ~2^-13 relative for these inputs) stay
under 2^-11 together.  tol_i = (2^-8 + 2^-11) A_i, no absolute floor beyond 1e-30.

Where the derivation holds.  "2^-9" is bf16's half ulp relative to the TOP of a binade; at the bottom of one it is 2^-8 of the value.  The
output term is therefore within 2^-9 A_i exactly when A_i is at least the top of the binade that holds |out_i|, and fails for a row
whose values all share a sign with |out_i| = A_i just above a power of two: with two keys, a spike of +8 and a value of +0.09, the fp32
restatement itself gives 4.0625 for 4.0408, 1.22 tol.  That is an error of the derivation, not of a kernel, and the bound is NOT widened
for it.  The inputs keep inside the derivation instead: element by element the spike's value takes the sign that OPPOSES the weighted
mean of the row's other visible values (|v| < 3.47 from the generator), so |out_i| = 4 - |rest_i| / 2 lies in [2, 4) (half ulp 2^-7)
while A_i >= 4; a key without visible company keeps the hashed sign (out = +-8 exactly).  test_attn_decode_reference.py holds the fp32
restatement of the kernels to tol on every launch of the GPU tests.

Planted keys.  Spike: k_j = bf16(q c / |q|^2) with c = log sum_{other visible} exp(s), so the key takes softmax weight 0.5, v_j = +-8:
dropping, doubling or mis-pairing that one key moves the row by many tol.  Trap: a position that must not be seen (a masked prompt key, a
slot at or beyond kv_total) gets a score 30 above the row's maximum and v = +-64 — or, in the NaN variant, the bf16 NaN bits 0x7FC0."""
from __future__ import annotations

from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from eilev_amd.synth import _splitmix64, fnv1a64, round_bf16

TOL_REL = 2.0 ** -8 + 2.0 ** -11
TOL_FLOOR = 1e-30
NAN_BITS = 0x7FC0
EMPTY_MAX = np.float32(-1e30)  # (max, sum) = (-1e30, 0) of a key range with nothing in it


# ---- deterministic inputs: one stream per (tensor, row, head) -----------------------------------------------------------------------
_base_cache: dict = {}


def _normal_rows(name: str, rows: int, heads: int, n: int, seed: int) -> np.ndarray:
    """(rows, heads, n) float32 ~ N(0, 1): synth.det_normal's generator with its own seed per (row, head)."""
    bases = np.array([[(fnv1a64(f"{name}.{b}.{h}") ^ (seed * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF for h in range(heads)]
                      for b in range(rows)], dtype=np.uint64)
    out = np.empty((rows, heads, n), np.float32)
    idx = np.arange(n, dtype=np.uint64)
    for b in range(rows):  # (row by row: the uint64 temporaries of a whole cache plane are several GB)
        with np.errstate(over="ignore"):
            z = _splitmix64(bases[b][:, None] + idx[None, :])
        s = np.zeros(z.shape, np.int64)
        for k in range(4):
            s += ((z >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.int64)
        out[b] = ((s - 2 * 65535) / np.sqrt(4.0 * (65536.0 ** 2 - 1.0) / 12.0)).astype(np.float32)
    return out


def base_plane(name: str, rows: int, heads: int, slots: int, hd: int, seed: int = 0) -> np.ndarray:
    """A bf16-exact (rows, heads, slots, hd) plane.  A (row, head)'s stream runs over (slot, hd), so a smaller capacity is a prefix of a
    larger one: the planes are generated once at a rounded-up capacity and sliced."""
    big = 1056 if slots <= 1056 else (2304 if slots <= 2304 else slots)
    key = (name, rows, heads, hd, seed)
    got = _base_cache.get(key)
    if got is None or got.shape[2] < big:
        got = round_bf16(_normal_rows(name, rows, heads, big * hd, seed)).reshape(rows, heads, big, hd)
        _base_cache[key] = got
    return got[:, :, :slots].copy()


def _signs(b: int, h, j, hd: int) -> np.ndarray:
    """+-1 per element, hashed from (row, head, key slot, element); h and j broadcast."""
    h, j = np.asarray(h, np.uint64), np.asarray(j, np.uint64)
    with np.errstate(over="ignore"):
        base = ((np.uint64(b) * np.uint64(4096) + h) * np.uint64(65536) + j) * np.uint64(256)
        z = _splitmix64(base[..., None] + np.arange(hd, dtype=np.uint64))
    return np.where((z >> np.uint64(17)) & np.uint64(1), 1.0, -1.0).astype(np.float32)


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """The bf16 bit patterns (as int16) of a bf16-exact float32 array; NaN -> 0x7FC0."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16)


def bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def frag32_index(row, col):
    """common.h frag32_index restated: element (row, col) of the row-block layout of <= 32 activation rows."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    return (col >> 5) * 1024 + row * 32 + (col & 31)


# ---- a case --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    name: str
    form: str                 # the kernel the launch must reach (the table of test_hip_attn_decode.py)
    launcher: int = 0         # 0 launch_attn_decode, 1 launch_attn_decode1, 2 launch_attn_decode_part
    part32: int = 1           # eilev_debug_attn_part32
    beam_part: int = 1        # eilev_debug_beam_part
    batch: int = 8
    heads: int = 32
    hd: int = 80
    seq_len: int = 16
    cap: int = 64
    n_gen: object = 1         # state[0]; None: state == nullptr (kv_total = seq_len)
    fuse_new: int = 1
    ldq_extra: int = -1       # -1: ldq = 0 (the default 3 * heads * hd); else the row stride is the packed width + this
    mask: str = "none"        # "none" (null pointer), "ones", "mixed" (rows cycle through MASK_KINDS), "pad300+dead" (cross-attention)
    mask_first: int = 0       # "mixed": the kind of row 0
    spikes: str = "newest"    # "none", "newest", "second", "mix", "beam", ("cover", k)
    stale: str = "trap"       # slots at / beyond kv_total: "rand", "trap", "nan"
    bias: str = ""            # "", "rel" (rel_off >= 0), "row" (rel_off < 0)
    beams: int = 0            # > 0: the beam form, batch = samples * beams
    cap_g: int = 0
    out_null: bool = False    # out == nullptr: the partials stay in `part`
    out_frag: int = 0
    part_short: int = 0       # 128 / 256: part_bytes one byte short of that range size
    seed: int = 0


MASK_KINDS = ("left0", "left1", "left127", "left128", "left129", "left300", "holes", "dead")  # dead: every prompt key masked


def kv_total_of(sp: Spec) -> int:
    g = 0 if sp.n_gen is None else sp.n_gen
    return sp.seq_len + min(sp.cap_g, g) if sp.beams else min(sp.cap, sp.seq_len + g)


def _mask(sp: Spec, srows: int):
    if sp.mask == "none":
        return None
    m = np.ones((srows, sp.seq_len), np.int32)
    j = np.arange(sp.seq_len, dtype=np.uint64)
    for r in range(srows):
        kind = {"ones": "left0", "mixed": MASK_KINDS[(r + sp.mask_first) % len(MASK_KINDS)], "pad300+dead": "dead" if r == srows - 1 else ("holes" if r & 1 else "left300")}[sp.mask]
        if kind.startswith("left"):
            m[r, :min(int(kind[4:]), max(sp.seq_len - 1, 0))] = 0  # (left padding keeps one prompt key)
        elif kind == "holes":
            with np.errstate(over="ignore"):
                m[r, (_splitmix64(j + np.uint64(7919 * (r + 1) + sp.seed)) % np.uint64(10)) < np.uint64(3)] = 0
            m[r, :3] = 0
        else:
            m[r, :] = 0
    return m


def build_case(sp: Spec) -> SimpleNamespace:
    """Inputs of one launch as bf16-exact float32 arrays (NaN where the NaN variant plants it), spikes and traps planted."""
    beam = sp.beams > 0
    srows = sp.batch // sp.beams if beam else sp.batch
    d = sp.heads * sp.hd
    width = 3 * d if sp.fuse_new else d
    ldq = width + sp.ldq_extra if sp.ldq_extra >= 0 else 3 * d
    c = SimpleNamespace(spec=sp, beam=beam, srows=srows, d=d, ldq=ldq, n=kv_total_of(sp), anc=None, kg=None, vg=None, rel_tab=None, rel_hs=0, rel_off=0)
    assert 1 <= c.n <= (sp.seq_len + sp.cap_g if beam else sp.cap) and (sp.fuse_new or sp.n_gen is None)
    row = base_plane("qkv", sp.batch, sp.heads, 1, 3 * sp.hd, sp.seed)[:, :, 0].reshape(sp.batch, sp.heads, 3, sp.hd)
    c.qkv = np.zeros((sp.batch, ldq), np.float32)
    c.qkv[:, :d] = round_bf16(0.35 * row[:, :, 0]).reshape(sp.batch, d)
    if sp.fuse_new:
        c.qkv[:, d:2 * d] = row[:, :, 1].reshape(sp.batch, d)
        c.qkv[:, 2 * d:3 * d] = row[:, :, 2].reshape(sp.batch, d)
    c.kc = base_plane("k", srows, sp.heads, sp.cap, sp.hd, sp.seed)
    c.vc = base_plane("v", srows, sp.heads, sp.cap, sp.hd, sp.seed)
    c.mask = _mask(sp, srows)
    if beam:
        c.kg = base_plane("kg", sp.batch, sp.heads, sp.cap_g, sp.hd, sp.seed)
        c.vg = base_plane("vg", sp.batch, sp.heads, sp.cap_g, sp.hd, sp.seed)
        # a valid ancestry: generated key g of row b lives in a row of the same sample; the newest one (this step's) in the row itself
        g = np.arange(sp.cap_g, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(sp.batch, dtype=np.uint64)[None, :]
        with np.errstate(over="ignore"):
            pick = (_splitmix64(g + np.uint64(1000003 * (sp.seed + 1))) % np.uint64(sp.beams)).astype(np.int64)
        c.anc = ((np.arange(sp.batch) // sp.beams) * sp.beams)[None, :] + pick
        c.anc[c.n - sp.seq_len - 1, :] = np.arange(sp.batch)
        c.anc = c.anc.astype(np.int32)
    if sp.bias:
        c.rel_off = (c.n - 1 + 5) if sp.bias == "rel" else -1
        c.rel_hs = (c.rel_off + 1 + 3) if sp.bias == "rel" else c.n + 3
        c.rel_tab = (2.0 * _normal_rows("rel", 1, sp.heads, c.rel_hs, sp.seed)[0]).astype(np.float32)
    c.spike_pos = np.full((sp.batch, sp.heads), -1, np.int64)
    _plant_spikes(c)
    _plant_traps(c)
    return c


def _store(c, b, h, j):
    """(array of K, array of V, index) where key j of (row b, head h) is held."""
    sp = c.spec
    if sp.fuse_new and j == c.n - 1:
        return c.qkv, c.qkv, (b, slice(c.d + h * sp.hd, c.d + (h + 1) * sp.hd)), (b, slice(2 * c.d + h * sp.hd, 2 * c.d + (h + 1) * sp.hd))
    if c.beam and j >= sp.seq_len:
        i = (int(c.anc[j - sp.seq_len, b]), h, j - sp.seq_len)
        return c.kg, c.vg, i, i
    i = (b // sp.beams if c.beam else b, h, j)
    return c.kc, c.vc, i, i


def effective(c, b: int):
    """What row b attends to: K, V (heads, kv_total, hd) float32, visible (kv_total,) bool, bias (heads, kv_total) float64 or None."""
    sp, n = c.spec, c.n
    srow = b // sp.beams if c.beam else b
    npr = min(sp.seq_len, n) if c.beam else n
    K, V = c.kc[srow, :, :npr], c.vc[srow, :, :npr]
    if c.beam and n > npr:
        g = np.arange(n - npr)
        K = np.concatenate([K, c.kg[c.anc[g, b], :, g].transpose(1, 0, 2)], 1)
        V = np.concatenate([V, c.vg[c.anc[g, b], :, g].transpose(1, 0, 2)], 1)
    else:
        K, V = K.copy(), V.copy()
    if sp.fuse_new:
        K[:, n - 1] = c.qkv[b, c.d:2 * c.d].reshape(sp.heads, sp.hd)
        V[:, n - 1] = c.qkv[b, 2 * c.d:3 * c.d].reshape(sp.heads, sp.hd)
    j = np.arange(n)
    vis = j >= sp.seq_len
    if c.mask is None:
        vis = np.ones(n, bool)
    else:
        vis[:min(sp.seq_len, n)] = c.mask[srow, :min(sp.seq_len, n)] != 0
    bias = None
    if c.rel_tab is not None:
        bias = c.rel_tab[:, (j - (n - 1) + c.rel_off) if c.rel_off >= 0 else j].astype(np.float64)
    return K, V, vis, bias


def _q(c, b):
    return c.qkv[b, :c.d].reshape(c.spec.heads, c.spec.hd)


def scores64(c, b, K=None, bias=None):
    if K is None:
        K, _, _, bias = effective(c, b)
    s = np.einsum("hd,hnd->hn", _q(c, b).astype(np.float64), K.astype(np.float64))
    return s if bias is None else s + bias


def _spike_slot(c, b, h, vis):
    sp, n = c.spec, c.n
    mode = sp.spikes
    idx = b * sp.heads + h
    with np.errstate(over="ignore"):
        r = int(_splitmix64(np.array([idx * 2654435761 + sp.seed * 97 + n], np.uint64))[0] >> np.uint64(16))
    visible = np.flatnonzero(vis)
    if mode == "none" or len(visible) == 0:
        return -1
    if isinstance(mode, tuple):  # ("cover", k): launch k of a set in which every slot is some (row, head)'s spike
        j = mode[1] * sp.batch * sp.heads + idx
        return j if j < n else int(visible[r % len(visible)])
    if mode == "newest":
        return n - 1
    if mode == "second":
        return n - 2 if n >= 2 and vis[n - 2] else -1
    if mode == "mix":  # the first visible key (behind the padding), the last prompt key, the newest, any visible one
        return [int(visible[0]), int(visible[visible < max(sp.seq_len, 1)][-1]) if (visible < sp.seq_len).any() else n - 1, n - 1, int(visible[r % len(visible)])][idx % 4]
    if mode == "beam":  # a prompt key, a generated key held by another row where there is one, the newest key
        kind = idx % 3
        prompt = visible[visible < sp.seq_len]
        if kind == 2:
            return n - 1
        if kind == 1 and n - 1 > sp.seq_len:
            g = np.arange(n - 1 - sp.seq_len)
            other = g[c.anc[g, b] != b]
            pool = other if len(other) else g
            return sp.seq_len + int(pool[r % len(pool)])
        return int(prompt[r % len(prompt)]) if len(prompt) else n - 1
    raise ValueError(mode)


def _plant_spikes(c):
    sp = c.spec
    for b in range(sp.batch):
        K, V, vis, bias = effective(c, b)
        s = scores64(c, b, K, bias)
        q = _q(c, b).astype(np.float64)
        for h in range(sp.heads):
            j = _spike_slot(c, b, h, vis)
            if j < 0:
                continue
            others = vis.copy()
            others[j] = False
            so = s[h, others]
            cval = float(so.max() + np.log(np.exp(so - so.max()).sum())) if so.size else 0.0
            sign = _signs(b, h, j, sp.hd)
            if so.size:  # (see the module docstring: the spike opposes the rest of the row, element by element)
                rest = np.exp(so - so.max()) @ V[h, others].astype(np.float64)
                sign = np.where(rest > 0, -1.0, np.where(rest < 0, 1.0, sign)).astype(np.float32)
            if bias is not None:
                cval -= bias[h, j]
            ka, va, ik, iv = _store(c, b, h, j)
            ka[ik] = round_bf16((q[h] * cval / (q[h] @ q[h])).astype(np.float32))
            va[iv] = 8.0 * sign
            c.spike_pos[b, h] = j


def _plant_traps(c):
    sp, n = c.spec, c.n
    if sp.stale == "rand" and c.mask is None:
        return
    for b in range(sp.batch):
        K, _, vis, bias = effective(c, b)
        s = scores64(c, b, K, bias)
        smax = np.where(vis[None, :], s, -np.inf).max(1) if vis.any() else np.zeros(sp.heads)
        q = _q(c, b).astype(np.float64)
        ktrap = round_bf16((q * ((smax + 30.0) / (q * q).sum(1))[:, None]).astype(np.float32))  # (heads, hd)
        hh = np.arange(sp.heads)[:, None]
        srow = b // sp.beams if c.beam else b
        if c.mask is not None and (not c.beam or b % sp.beams == 0):
            jm = np.flatnonzero(c.mask[srow] == 0)
            jm = jm[jm < sp.cap]
            if len(jm):
                c.kc[srow][:, jm] = ktrap[:, None, :]
                c.vc[srow][:, jm] = 64.0 * _signs(b, hh, jm[None, :], sp.hd)
        if sp.stale == "rand":
            continue
        # slots at / beyond kv_total: of the cache (plain form) or of this row's generation cache (beam form; its prompt cache ends at seq_len)
        ka, va, first, last = (c.kg, c.vg, n - sp.seq_len, sp.cap_g) if c.beam else (c.kc, c.vc, n, sp.cap)
        js = np.arange(first, last)
        if len(js) == 0:
            continue
        if sp.stale == "nan":
            ka[b][:, js] = np.nan
            va[b][:, js] = np.nan
        else:
            ka[b][:, js] = ktrap[:, None, :]
            va[b][:, js] = 64.0 * _signs(b, hh, js[None, :] + 4096, sp.hd)


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------
def reference(c):
    """(out, A): (batch, heads * hd) float64 rows and the A_i of the tolerance."""
    sp = c.spec
    out = np.zeros((sp.batch, sp.heads, sp.hd))
    A = np.zeros_like(out)
    for b in range(sp.batch):
        K, V, vis, bias = effective(c, b)
        if not vis.any():
            continue
        s = scores64(c, b, K, bias)[:, vis]
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        V64 = V[:, vis].astype(np.float64)
        out[b] = np.einsum("hn,hnd->hd", p, V64)
        A[b] = np.einsum("hn,hnd->hd", p, np.abs(V64))
    return out.reshape(sp.batch, c.d), A.reshape(sp.batch, c.d)


def tolerance(A):
    return np.maximum(TOL_REL * A, TOL_FLOOR)


def worst_ratio(got, ref, A) -> float:
    """max_i |got_i - ref_i| / tol_i (inf for a non-finite output)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / tolerance(A)).max())


def partials_ref(c, keys: int):
    """float64 flash-decoding partials (max, sum, o[hd]) per (row, head, range of `keys` keys): (batch, heads, nsplit, hd + 2)."""
    sp = c.spec
    total = sp.seq_len + sp.cap_g if c.beam else sp.cap
    ns = -(-total // keys)
    part = np.zeros((sp.batch, sp.heads, ns, sp.hd + 2))
    part[..., 0] = -1e30
    for b in range(sp.batch):
        K, V, vis, bias = effective(c, b)
        s = np.where(vis[None, :], scores64(c, b, K, bias), -np.inf)
        for r in range(-(-c.n // keys)):
            sl = slice(r * keys, min(c.n, (r + 1) * keys))
            if not vis[sl].any():
                continue
            m = s[:, sl].max(1)
            p = np.exp(s[:, sl] - m[:, None])
            part[b, :, r, 0], part[b, :, r, 1] = m, p.sum(1)
            part[b, :, r, 2:] = np.einsum("hn,hnd->hd", p, V[:, sl].astype(np.float64))
    return part


def merge_ref(part):
    """float64 merge of partials (batch, heads, nsplit, hd + 2) -> (batch, heads * hd).  A range with sum == 0 carries nothing (its o may
    be unwritten memory); a row whose every range is empty gives zeros."""
    with np.errstate(invalid="ignore"):  # (unwritten o of empty ranges may hold NaN bit patterns)
        part = np.asarray(part, np.float64)
    mx, l = part[..., 0], part[..., 1]
    live = l > 0
    m = np.where(live, mx, -np.inf).max(-1, keepdims=True)
    w = np.where(live, np.exp(np.where(live, mx, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
    lsum = (w * np.where(live, l, 0.0)).sum(-1)
    o = (w[..., None] * np.where(live[..., None], part[..., 2:], 0.0)).sum(-2)
    out = np.where(lsum[..., None] > 0, o / np.where(lsum > 0, lsum, 1.0)[..., None], 0.0)
    return out.reshape(out.shape[0], -1)


# ---- fp32 restatement of the kernels' range loop ---------------------------------------------------------------------------------------
def emulate_ranges(c, keys: int, mutate: str = ""):
    """What attn_decode_loop_kernel computes, in numpy float32: ranges of `keys` keys, P rounded to bf16 for the product, the row sum from
    the unrounded P, the online rescale, the output rounded to bf16.  mutate: "drop" / "double" the spike key of every (row, head), or
    "shift" (P of slot j paired with V of slot j + 1) — the index mistakes the GPU tests must be able to see."""
    sp = c.spec
    f = np.float32
    out = np.zeros((sp.batch, sp.heads, sp.hd), f)
    hh = np.arange(sp.heads)
    for b in range(sp.batch):
        K, V, vis, bias = effective(c, b)
        s = np.einsum("hd,hnd->hn", _q(c, b), K).astype(f)
        if bias is not None:
            s = s + bias.astype(f)
        s = np.where(vis[None, :], s, f(-1e30))
        if mutate == "shift":
            V = np.roll(V, -1, axis=1)
        m_run, l_run, acc = np.full(sp.heads, -1e30, f), np.zeros(sp.heads, f), np.zeros((sp.heads, sp.hd), f)
        for k0 in range(0, c.n, keys):
            k1 = min(c.n, k0 + keys)
            sl = s[:, k0:k1]
            m_new = np.maximum(m_run, sl.max(1))
            p = np.where(sl > -1e29, np.exp(sl - m_new[:, None]), f(0)).astype(f)
            if mutate in ("drop", "double"):
                j = c.spike_pos[b]
                sel = (j >= k0) & (j < k1)
                p[hh[sel], j[sel] - k0] *= f(0.0 if mutate == "drop" else 2.0)
            scale = np.exp(m_run - m_new).astype(f)
            l_run = l_run * scale + p.sum(1, dtype=f)
            acc = acc * scale[:, None] + np.einsum("hn,hnd->hd", round_bf16(p), V[:, k0:k1]).astype(f)
            m_run = m_new
        out[b] = round_bf16(np.where(l_run[:, None] > 0, acc / np.where(l_run > 0, l_run, f(1))[:, None], f(0)).astype(f))
    return out.reshape(sp.batch, c.d)


# ---- the launches of the GPU tests -------------------------------------------------------------------------------------------------------
SWEEP = (1, 2, "G-1", "G", "G+1", 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
SWEEP_BIG = (1025, 2047, 2048, 2049)

# form -> (how it is selected, key-group stride G = threads / NCH, largest kv_total, footprint in `part`: key range size or 0 = untouched)
FORMS = {
    "one80": dict(sel=dict(launcher=1, hd=80, batch=8), G=102, top=1024, rng=0),
    "one64": dict(sel=dict(launcher=1, hd=64, batch=8), G=128, top=1024, rng=0),
    "part128": dict(sel=dict(launcher=2, hd=80, batch=8), G=25, top=1024, rng=128),
    "part128_l0": dict(sel=dict(launcher=0, hd=80, batch=8), G=25, top=2048, rng=128),
    "part256": dict(sel=dict(launcher=0, hd=80, batch=8, part32=2), G=25, top=2048, rng=256),
    "loop80": dict(sel=dict(launcher=0, hd=80, batch=8, part32=3), G=25, top=2048, rng=0),
    "loop80_auto": dict(sel=dict(launcher=0, hd=80, batch="2cu"), G=25, top=2048, rng=0),
    "loop64": dict(sel=dict(launcher=0, hd=64, batch="2cu"), G=32, top=2304, rng=0),
    "beam": dict(sel=dict(launcher=0, hd=80), G=25, top=2048, rng=128),
    "split": dict(sel=dict(launcher=0, hd=80, batch=8, part32=0), G=25, top=2304, rng=256),
}


def rows_for_2cu(num_cu: int, heads: int = 32) -> int:
    return -(-2 * num_cu // heads)


def _sel(form: str, num_cu: int, **over) -> dict:
    kw = dict(FORMS[form]["sel"])
    if kw.get("batch") == "2cu":
        kw["batch"] = rows_for_2cu(num_cu)
    kw.update(over)
    return kw


def cover_specs(num_cu: int = 256):
    """Every key slot of a full cache is the spike of some (row, head): ceil(cap / (rows * heads)) launches per form."""
    out = []
    for form, cap in (("one80", 1024), ("one64", 1024), ("part128", 1024), ("part128_l0", 2048), ("part256", 2048), ("loop80", 2048),
                      ("loop80_auto", 2048), ("loop64", 2304), ("split", 2304)):
        kw = _sel(form, num_cu)
        if kw["batch"] > 32:
            continue
        for k in range(-(-cap // (kw["batch"] * 32))):
            out.append(Spec(name=f"cover-{form}-{k}", form=form.split("_")[0], seq_len=cap - 1, cap=cap, n_gen=1, spikes=("cover", k), stale="rand", **kw))
    return out


def sweep_specs(num_cu: int = 256):
    """kv_total at the group stride, the range boundaries and the capacity; each value reached once by seq_len (state[0] = 1) and once by
    state[0] (seq_len fixed at 1); the spike on the newest key and, in a second pass, on kv_total - 2."""
    out = []
    for form in ("one80", "one64", "part128", "part256", "loop80", "loop64", "split"):
        F = FORMS[form]
        vals = [v if isinstance(v, int) else F["G"] + {"G-1": -1, "G": 0, "G+1": 1}[v] for v in SWEEP] + [v for v in SWEEP_BIG if v <= F["top"]]
        vals = sorted(set(vals))  # (G = 128 of the hd-64 one-pass kernel: its stride values are the range boundaries)
        small = dict(batch=2) if form != "loop64" else {}
        kw = _sel(form, num_cu, **small)
        if kw["batch"] > 32:
            continue
        for n in vals:
            for by in ("seq", "state"):
                if by == "state" and n == 1:
                    continue  # (kv_total = 1 = seq_len 0 + state[0] 1 either way)
                seq, gen = (n - 1, 1) if by == "seq" else (1, n - 1)
                # the capacity is the value itself at the range boundaries and at the top, a few trapped slots more elsewhere
                cap = n if (n % 128 == 0 or n in (1, F["top"], 2049, F["G"])) else n + 5
                if form not in ("loop64", "split"):
                    cap = min(cap, F["top"])  # (the largest capacity the form takes)
                for spike in ("newest", "second"):
                    if spike == "second" and n < 2:
                        continue
                    out.append(Spec(name=f"sweep-{form}-{n}-{by}-{spike}", form=form, seq_len=seq, cap=cap, n_gen=gen, spikes=spike,
                                    mask="ones" if by == "seq" and n % 2 and seq else "none", stale="trap", **kw))
    return out


def mask_specs(num_cu: int = 256):
    """Left padding of 0, 1, 127, 128, 129 and 300 keys, holes, and a row with every prompt key masked: one row each (MASK_KINDS), a trap on
    every masked key, traps or NaN bits in every slot at / beyond kv_total."""
    out = []
    for form in ("one80", "one64", "part128", "part256", "loop80", "loop80_auto", "loop64", "split"):
        kw = _sel(form, num_cu)
        if kw["batch"] > 32:
            continue
        for stale in ("trap", "nan"):
            out.append(Spec(name=f"mask-{form}-{stale}", form=form.split("_")[0], seq_len=530, cap=1024, n_gen=3, spikes="mix", mask="mixed", stale=stale, **kw))
    return out


def beam_specs():
    out = []
    for beams, samples in ((3, 1), (3, 2), (5, 1)):
        for gen in (1, 2, 17, 40):
            for stale in ("trap", "nan"):
                for beam_part, form in ((1, "beam"), (0, "split")):
                    if form == "split" and (stale == "nan") != (gen == 17):
                        continue  # (the split kernel's beam form: one stale variant per step count)
                    out.append(Spec(name=f"beam-{form}-{beams}x{samples}-g{gen}-{stale}", form=form, beam_part=beam_part, batch=beams * samples, beams=beams,
                                    seq_len=420, cap=420, cap_g=40, n_gen=gen, spikes="beam", mask="mixed", mask_first=5, stale=stale))
    return out


def t5_specs(num_cu: int = 256):
    """flan-t5 (head size 64): the four variants of the hd-64 loop kernel and the same launches at a batch size that leaves them to the split kernel."""
    out = []
    for form, batch in (("loop64", rows_for_2cu(num_cu)), ("split", 4)):
        if batch > 32:
            continue
        kw = dict(form=form, batch=batch, hd=64)
        # cross-attention over 960 encoder keys: no state, nothing to store, a padding mask; the last row has no visible key at all
        out.append(Spec(name=f"t5-cross-{form}", seq_len=960, cap=960, n_gen=None, fuse_new=0, ldq_extra=64, mask="pad300+dead", spikes="mix", stale="rand", **kw))
        out.append(Spec(name=f"t5-cross-nomask-{form}", seq_len=960, cap=1024, n_gen=None, fuse_new=0, ldq_extra=0, mask="none", spikes="mix", stale="nan", **kw))
        # self-attention with the position bias in both addressings; the spike's score includes its bias
        for bias in ("rel", "row"):
            for gen, stale in ((1, "trap"), (130, "nan"), (300, "trap")):
                out.append(Spec(name=f"t5-self-{bias}-g{gen}-{form}", seq_len=0, cap=300, n_gen=gen, fuse_new=1, ldq_extra=128, mask="none", bias=bias,
                                spikes="second" if gen == 130 else "mix", stale=stale, **kw))
        out.append(Spec(name=f"t5-self-nostate-{form}", seq_len=77, cap=80, n_gen=None, fuse_new=0, ldq_extra=32, mask="ones", bias="row", spikes="mix", stale="trap", **kw))
        out.append(Spec(name=f"t5-self-masked-rel-{form}", seq_len=200, cap=256, n_gen=9, fuse_new=1, mask="mixed", bias="rel", spikes="mix", stale="nan", **kw))
    return out


def other_specs(num_cu: int = 256):
    """What the other forms refuse and the split kernel takes; the row-block output of the loop kernel; partials left to the caller."""
    out = []
    for hd in (8, 40, 64, 96, 128):
        out.append(Spec(name=f"split-hd{hd}", form="split", batch=3, heads=5, hd=hd, seq_len=290, cap=520, n_gen=7, mask="mixed", spikes="mix", stale="nan"))
    out.append(Spec(name="split-cap2304", form="split", batch=2, seq_len=2100, cap=2304, n_gen=50, mask="mixed", spikes="mix", stale="trap"))
    out.append(Spec(name="split-outnull", form="split", batch=4, seq_len=530, cap=1024, n_gen=3, mask="mixed", spikes="mix", stale="nan", out_null=True, part32=0))
    out.append(Spec(name="part128-l0-small", form="part128", batch=1, seq_len=530, cap=700, n_gen=3, mask="ones", spikes="mix", stale="nan"))
    out.append(Spec(name="split-part-short128", form="split", batch=2, seq_len=530, cap=1024, n_gen=3, mask="mixed", spikes="mix", stale="trap", part_short=128))
    rows = rows_for_2cu(num_cu)
    if rows <= 32:
        for frag in (0, 1):
            out.append(Spec(name=f"loop80-auto-frag{frag}", form="loop80", batch=rows, seq_len=975, cap=1024, n_gen=6, mask="mixed", spikes="mix", stale="nan", out_frag=frag))
    return out


def all_specs(num_cu: int = 256):
    return cover_specs(num_cu) + sweep_specs(num_cu) + mask_specs(num_cu) + beam_specs() + t5_specs(num_cu) + other_specs(num_cu)


def emu_keys(sp: Spec) -> int:
    """The range size of the form's arithmetic (the one-pass kernels see every key in one range)."""
    return {"one80": 1024, "one64": 1024, "part128": 128, "beam": 128}.get(sp.form, 256)


__all__ = [n for n in dir() if not n.startswith("__")]
_ = replace  # (Spec variants in the tests)
