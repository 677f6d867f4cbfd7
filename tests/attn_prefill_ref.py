"""Reference, case builder, tolerance, kernel restatements and mutations of the prefill-attention kernel tests
(test_attn_prefill_reference.py on the CPU, test_hip_attn_prefill.py on the GPU).  A plain module: no fixtures, no GPU; the sibling of
attn_decode_ref.py, whose generic helpers it imports.

Reference: numpy float64 on the bf16-exact inputs, per (batch, head, query row i):
softmax_j(scale * q_i . k_j + rel[h, clamp(j - i - (skv - sq) + rel_off, 0, rel_n - 1)]) over the visible j, times v (the clamp is v1's; v2 is
only routed to when the table covers the launch).  Visible: j < skv, mask[b, j] != 0 where a mask is given, j <= i + (skv - sq) where
causal.  A row with no visible key gives exact zeros (both kernels: inv = l_run > 0 ? 1 / l_run : 0).  A_i = sum p |v| / sum p.

Tolerance (derived from the kernels' code, not measured): tol_i = (2^-8 + 2^-11) A_i, no absolute floor.
 * v1 (attn_prefill_kernel) and v2 (attn_prefill_v2_kernel) round P to bf16 for the second MFMA (2^-9 A_i), take the row sum from the
   unrounded P and round O / l to bf16 (2^-9 (1 + 2^-9) A_i, see "where the derivation holds").  v2's lazy rescale lets P reach 2^6 before
   the running maximum is raised: bf16 rounding is relative, the term is unchanged.
 * attn_frame_kernel is a single pass (all scores of a row in registers, p = exp2(s * scale * log2 e - max)): the same two roundings, no
   rescale at all.  attn_frame3_kernel's patch rows are that arithmetic; its CLS row is merged from eight partial softmaxes (own maximum
   m_w, P rounded to bf16 relative to m_w, partial sums and O in fp32, weights exp2(m_w - M) <= 1 in fp32): the P term is
   sum_w f_w 2^-9 sum_{j in w} p_j |v_j| = 2^-9 A_i again, the merge adds fp32 terms only.  The same bound holds for both.
 * fp32 terms, bounded explicitly per case by fp32_term() (the CPU test asserts <= 2^-11 on every launch): the score dot (<= hd roundings of
   partial sums bounded by sum_d |q_d k_d|: with the scale folded into the exponent the raw scores reach |40 / scale|, ~450 at hd 128, so this
   is the largest term: hd 2^-24 scale sum|q k|, ~2^-12.5 in the exponent of a spike key at hd 128), the fma into the exponent
   (2^-23 |x|, |x| <= 64 log2 units), exp2 (2^-22), the row sum and the O accumulation (2 N 2^-24, N <= 704).  Measured on the generated
   cases the sum stays under 2^-11 A_i everywhere (largest: see test_attn_prefill_reference.py), so the term is not widened.

Where the derivation holds (decode docstring, same failure): "2^-9" is bf16's half ulp relative to the TOP of a binade; at the bottom of
one it is 2^-8 of the value.  That bites twice here, and the inputs are narrowed for it, not the bound.
 * Output: the term needs A_i >= the top of the binade that holds |out_i|.  The spike takes weight w in [0.45, 0.5) (target 0.483; bf16 k) and,
   element by element, the sign that OPPOSES the weighted mean of the row's other visible values (settled row by row):
   |out_i| = 8 w - (1 - w) |rest_i| < 4 <= A_i, half ulp <= 2^-7.  A row with a single visible key gives +-8 exactly.
 * P: the spike carries w of the row in ONE probability.  Where that p is exp2(0) = 1 (the key is the running maximum: v1, the frame
   kernels) it is exact, but v2's running maximum lags by up to 2^6 and the tile profiles put other keys on top: p is then anywhere in
   its binade and its rounding alone reaches 2^-8 8 w = 2^-8 3.86.  With small other values (A_i ~ 4.4) that and the output's 2^-7 are
   1.3 tol; the fp32 restatement of v2 showed it on 4 of ~960 launches.  So every ordinary value has |v| in [4, ~8]:
   A_i = 8 w + (1 - w) mean|v| >= 5.9 and 2^-8 8 w + 2^-7 = 2^-8 5.86 < tol_i, with the rest of tol_i for the other keys' roundings,
   which are many and independent (a row with few keys has its maximum, an exact p, among them).
Every row with a visible key owns a spike in every launch: a row without one would see only other rows' +-8 (asserted on the CPU).

Planted keys.  q_i = bf16(0.35 n_i + u_h): u_h is a fixed +-0.35 pattern per head, so that ONE key direction (t u_h) scores high against every
row: the traps.  Row i's spike is k_j = c_i n'_i / (scale n'_i . q_i), n'_i = q_i minus its component along u_h: score exactly c_i for its own
row and a random ~N(0, c_i^2 / hd) for the others (keys are shared by the rows of a (batch, head)); c_i = log sum_{other visible} exp(s) +
logit(0.483) - bias, settled in PASSES passes over the whole plane (every row's spike is every other row's ordinary key).  v_j = +-8.  A
row with one visible key has weight 1 (asserted as such); where a launch has more rows than visible keys (non-causal, sq > visible keys:
the key-count sweeps of the 8-wave forms) row r >= nv repeats q of row r - nv and shares its spike; with a position bias, where a shared key
cannot balance two rows, the launches keep sq <= visible keys.
Trap: every key no row may see (mask == 0, the guard row behind skv in the row layouts = slot skv, the cache slots [skv, cap)) is
t u_h with t such that its score is AT LEAST 30 above the launch's maximum for every row, v = +-64.  Memory no kernel may touch (the row
behind the guard, q of the guard rows, pad columns) holds bf16 NaN bits; the output is poisoned with a sentinel row behind each batch
entry and 8 sentinel columns behind the last head."""
from __future__ import annotations

from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from attn_decode_ref import NAN_BITS, TOL_REL, _normal_rows, _signs, bf16_bits, bits_to_f32, tolerance, worst_ratio
from eilev_amd.synth import _splitmix64, round_bf16

LOG2E = np.float32(1.44269504088896340736)
W_TARGET = 0.483
W_LO, W_HI = 0.45, 0.5        # where the tolerance derivation holds; the issue's interval [0.25, 0.75] contains it
PASSES = 4
SENT16 = 0x7FA5               # poison of the output (a NaN as bf16)
V1_64, V1_96, V1_128, FRAME, FRAME3 = 64, 96, 128, 2000, 2003


def V2(nwq, db=3, rel=0):
    return 1000 + 100 * nwq + 10 * db + rel


def family(form: int) -> str:
    return "v1" if form < 1000 else ("v2" if form < 2000 else ("frame" if form == FRAME else "frame3"))


def form_name(form: int) -> str:
    if form < 1000:
        return f"v1<{form}>"
    if form < 2000:
        return f"v2<{(form - 1000) // 100},{(form // 10) % 10}{',rel' if form % 10 else ''}>"
    return "frame<88,17>" if form == FRAME else "frame3<88,17>"


@dataclass(frozen=True)
class Spec:
    name: str
    form: int                 # the kernel instance the launch must reach (the code eilev_debug_attention reports)
    batch: int = 2
    heads: int = 2
    hd: int = 80
    sq: int = 64
    skv: int = 64
    layout: str = "sep"       # "fused" q|k|v rows (ld 3D, sq == skv), "kv" q rows + k|v rows (ld 2D), "sep" three buffers, "cache" K/V planes
    cap: int = 0              # "cache": slots per (batch, head) plane, > skv
    scale1: bool = False      # scale = 1.0 with pre-scaled q (what OPT and T5 pass) instead of 1 / sqrt(hd)
    causal: int = 0
    mask: tuple = ()          # () = null pointer; else one kind per batch entry, cycled: "ones", "left<L>", "right<R>", "holes", "dead"
    rel: str = ""             # "", "tight" (rel_off = skv - 1, rel_n = sq + skv - 1 = rel_hs), "gap" (rel_hs > rel_n, traps in the gap),
    #                           "n4096" / "n4097" (rel_n), "short" (the table does not cover the launch: v1 clamps)
    spikes: str = "hash"      # "hash"; "last": every third row on its last visible key where it is free
    profile: str = ""         # "", "rise", "fall", "late", "lazy" (scores by key tile: the online softmax)
    force: int = 0            # the argument of eilev_debug_attn_v1 (bit 0: v1; flag << 1)
    seed: int = 0


# ---- a case -----------------------------------------------------------------------------------------------------------------------------
def _mask(sp: Spec):
    if not sp.mask:
        return None
    m = np.ones((sp.batch, sp.skv), np.int32)
    j = np.arange(sp.skv, dtype=np.uint64)
    for b in range(sp.batch):
        kind = sp.mask[b % len(sp.mask)]
        if kind.startswith("left"):
            m[b, :int(kind[4:])] = 0
        elif kind.startswith("right"):
            m[b, sp.skv - int(kind[5:]):] = 0
        elif kind == "holes":
            with np.errstate(over="ignore"):
                m[b, (_splitmix64(j + np.uint64(7919 * (b + 1) + sp.seed)) % np.uint64(10)) < np.uint64(3)] = 0
            m[b, :3] = 0
        elif kind == "dead":
            m[b, :] = 0
        else:
            assert kind == "ones", kind
    return m


def scale_of(sp: Spec) -> np.float32:
    return np.float32(1.0) if sp.scale1 else np.float32(1.0 / np.sqrt(np.float32(sp.hd)))


def visible(c, b: int) -> np.ndarray:
    """(sq, skv) bool."""
    sp = c.spec
    vis = np.ones((sp.sq, sp.skv), bool)
    if c.mask is not None:
        vis &= (c.mask[b] != 0)[None, :]
    if sp.causal:
        vis &= np.arange(sp.skv)[None, :] <= np.arange(sp.sq)[:, None] + (sp.skv - sp.sq)
    return vis


def rel_index(c, shift: int = 0) -> np.ndarray:
    sp = c.spec
    idx = np.arange(sp.skv)[None, :] - np.arange(sp.sq)[:, None] - (sp.skv - sp.sq) + c.rel_off + shift
    return np.clip(idx, 0, c.rel_n - 1)


def bias(c, h: int, shift: int = 0):
    """(sq, skv) float64 or None."""
    return None if c.rel_tab is None else c.rel_tab[h, c.rel_lead + rel_index(c, shift)].astype(np.float64)


def scores64(c, b, h, Q=None, K=None, scale=None, B="own"):
    Q = c.Q[b, h] if Q is None else Q
    K = c.K[b, h, :c.spec.skv] if K is None else K
    s = float(c.scale if scale is None else scale) * (Q.astype(np.float64) @ K.astype(np.float64).T)
    B = bias(c, h) if isinstance(B, str) else B
    return s if B is None else s + B


def _hash(*xs) -> int:
    with np.errstate(over="ignore"):
        z = np.uint64(0x9E3779B97F4A7C15)
        for x in xs:
            z = _splitmix64(np.array([z ^ np.uint64(x)], np.uint64))[0]
    return int(z >> np.uint64(16))


def _assign_spikes(c, b, h, vis):
    """Key slot of every row's spike (-1: a row without a visible key).  Distinct keys wherever the visible sets allow it."""
    sp = c.spec
    pos = np.full(sp.sq, -1, np.int64)
    r0 = _hash(b, h, sp.seed, sp.skv)
    if not sp.causal:
        v = np.flatnonzero(vis[0])
        if len(v):
            pos[:] = v[(r0 + np.arange(sp.sq) % len(v)) % len(v)]  # a rotation: with sq >= visible keys EVERY visible key is some row's spike
            assert not sp.rel or sp.sq <= len(v), "a shared spike needs the same bias: with a position bias keep sq <= visible keys"
        return pos
    taken = np.zeros(sp.skv, bool)
    for i in range(sp.sq):  # the visible sets are nested: greedy in row order always finds a free key
        cand = np.flatnonzero(vis[i] & ~taken)
        if not len(cand):
            continue
        pos[i] = cand[-1] if (sp.spikes == "last" and i % 3 == 0) else cand[(r0 + 7 * i) % len(cand)]
        taken[pos[i]] = True
    return pos


def _profile(c):
    """Scores by 64-key tile for every row: k_j += g_j u / (scale u.u) adds ~g_j (q_i.u / u.u in [0.5, 1.5]) to row i's score of key j."""
    sp = c.spec
    if sp.profile in ("", "lazy"):
        return
    nt = -(-sp.skv // 64)
    tile = np.arange(sp.skv) // 64
    step = 2.5 if sp.hd <= 96 else 2.0  # (the raw scores grow with 1 / scale: fp32_term() stays under 2^-11)
    g = {"rise": step * tile, "fall": step * (nt - 1 - tile), "late": np.where(np.arange(sp.skv) == (4 * sp.skv) // 5, 16.0, 0.0)}[sp.profile]
    for h in range(sp.heads):
        uu = float(c.u[h] @ c.u[h])
        c.K[:, h, :sp.skv] = round_bf16((c.K[:, h, :sp.skv] + (g / (float(c.scale) * uu))[None, :, None] * c.u[h][None, None, :]).astype(np.float32))


LAZY_RISE = (5.5, 5.9, 6.1, 6.5, 3.0, 9.0, 5.95, 6.05, 12.0)  # base-2 exponent units between tile 0 and tile 1, per (batch, head)


def _profile_lazy(c, b, h):
    """sq == 1 (the wave's other 31 rows are q = 0: score 0, they never outgrow their maximum after the first tile): key 64 + 5 is set so
    that the row's maximum rises by LAZY_RISE over its tile-0 maximum.  Keys 65.. of that tile stay ordinary (below)."""
    sp = c.spec
    rise = LAZY_RISE[(b * sp.heads + h) % len(LAZY_RISE)]
    q = c.Q[b, h, 0].astype(np.float64)
    s = scores64(c, b, h)[0]
    m0 = s[:64].max()
    want = m0 + rise / float(LOG2E) - (0.0 if c.rel_tab is None else bias(c, h)[0, 69])
    c.K[b, h, 69] = round_bf16((q * (want / (float(c.scale) * (q @ q)))).astype(np.float32))
    c.lazy_rise[b, h] = (scores64(c, b, h)[0, 69] - m0) * float(LOG2E)


def build_case(sp: Spec) -> SimpleNamespace:
    """Logical inputs of one launch as bf16-exact float32 arrays: Q (batch, heads, sq, hd); K, V (batch, heads, nk, hd) with nk = skv + 1
    (row layouts: slot skv is the guard row) or cap (cache planes); spikes and traps planted.  pack() lays them out in memory."""
    assert sp.layout in ("fused", "kv", "sep", "cache") and (sp.layout != "fused" or sp.sq == sp.skv) and (sp.layout != "cache" or sp.cap > sp.skv)
    nk = sp.cap if sp.layout == "cache" else sp.skv + 1
    c = SimpleNamespace(spec=sp, nk=nk, scale=scale_of(sp), mask=_mask(sp), rel_tab=None, rel_hs=0, rel_off=0, rel_n=0, rel_lead=0)
    c.u = 0.35 * _signs(977, np.arange(sp.heads), 0, sp.hd)  # (heads, hd)
    n = _normal_rows("q", sp.batch, sp.heads, sp.sq * sp.hd, sp.seed).reshape(sp.batch, sp.heads, sp.sq, sp.hd)
    q = 0.35 * n + c.u[None, :, None, :]
    c.Q = round_bf16((q * (np.float32(1.0 / np.sqrt(np.float32(sp.hd))) if sp.scale1 else np.float32(1))).astype(np.float32))
    c.K = round_bf16(_normal_rows("k", sp.batch, sp.heads, nk * sp.hd, sp.seed)).reshape(sp.batch, sp.heads, nk, sp.hd)
    v = _normal_rows("v", sp.batch, sp.heads, nk * sp.hd, sp.seed).reshape(sp.batch, sp.heads, nk, sp.hd)
    c.V = round_bf16((np.where(v < 0, -1.0, 1.0) * (4.0 + np.abs(v))).astype(np.float32))  # |v| >= 4: see the module docstring
    if sp.rel:
        need = sp.sq + sp.skv - 1
        c.rel_off, c.rel_n = sp.skv - 1, need
        if sp.rel == "gap":
            c.rel_off, c.rel_n = sp.skv + 2, need + 6
        elif sp.rel in ("n4096", "n4097"):
            c.rel_n = int(sp.rel[1:])
            c.rel_off = c.rel_n - sp.sq - 1
        elif sp.rel == "short":
            c.rel_off, c.rel_n = sp.skv - 1 - 3, need - 7
        else:
            assert sp.rel == "tight"
        c.rel_lead = 8
        c.rel_hs = c.rel_n + (8 if sp.rel == "gap" else 0)
        tab = np.full(c.rel_lead + sp.heads * c.rel_hs + 8, 60.0, np.float32)  # +60 wherever the table is not: a read there is a trap
        for h in range(sp.heads):
            tab[c.rel_lead + h * c.rel_hs:c.rel_lead + h * c.rel_hs + c.rel_n] = _normal_rows("rel", 1, sp.heads, c.rel_n, sp.seed)[0, h]
        c.rel_flat = tab
        c.rel_tab = np.stack([tab[h * c.rel_hs:h * c.rel_hs + c.rel_lead + c.rel_n] for h in range(sp.heads)])  # [h, rel_lead + index]
    _profile(c)
    c.spike_pos = np.full((sp.batch, sp.heads, sp.sq), -1, np.int64)
    c.lazy_rise = np.zeros((sp.batch, sp.heads))
    for b in range(sp.batch):
        vis = visible(c, b)
        for h in range(sp.heads):
            if sp.profile == "lazy":
                assert sp.sq == 1 and sp.skv >= 192 and not sp.causal
                _profile_lazy(c, b, h)
            _plant_spikes(c, b, h, vis)
    _plant_traps(c)
    return c


def _plant_spikes(c, b, h, vis):
    sp = c.spec
    pos = _assign_spikes(c, b, h, vis)
    if sp.profile == "lazy":
        pos[0] = 128 + _hash(b, h) % (sp.skv - 128)  # behind the rising tile
    c.spike_pos[b, h] = pos
    rows = np.flatnonzero(pos >= 0)
    if not len(rows):
        return
    nv = int(vis[0].sum())
    if not sp.causal and sp.sq > nv:  # more rows than keys: row r >= nv repeats q of row r - nv (and shares its spike)
        for r in range(nv, sp.sq):
            c.Q[b, h, r] = c.Q[b, h, r - nv]
    Q = c.Q[b, h].astype(np.float64)
    u = c.u[h].astype(np.float64)
    nperp = Q - np.outer(Q @ u / (u @ u), u)
    direction = nperp / (float(c.scale) * np.einsum("id,id->i", nperp, Q))[:, None]  # score 1 for the own row, 0 from u
    owner = np.full(sp.skv, -1, np.int64)
    owner[pos[rows][::-1]] = rows[::-1]  # (shared spikes: the first row that holds the key sets it)
    own = owner[owner >= 0]
    keys = np.flatnonzero(owner >= 0)
    B = bias(c, h)
    logit = float(np.log(W_TARGET / (1.0 - W_TARGET)))
    for _ in range(PASSES):
        s = scores64(c, b, h, B=B)
        s = np.where(vis, s, -np.inf)
        s[rows, pos[rows]] = -np.inf
        m = s.max(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lse = np.where(np.isfinite(m), m + np.log(np.exp(s - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(1)), 0.0)
        cval = np.where(np.isfinite(m), lse + logit, 0.0)
        if B is not None:
            cval[rows] -= B[rows, pos[rows]]
        c.K[b, h, keys] = round_bf16((direction[own] * cval[own][:, None]).astype(np.float32))
    # values: +-8, element by element against the weighted mean of the row's other visible values (two rounds: the spikes are each other's rest)
    c.V[b, h, keys] = 8.0 * _signs(b, h, keys, sp.hd)
    s = np.where(vis, scores64(c, b, h, B=B), -np.inf)
    s[rows, pos[rows]] = -np.inf
    with np.errstate(invalid="ignore"):
        p = np.where(np.isfinite(s), np.exp(s - np.where(np.isfinite(s.max(1)), s.max(1), 0.0)[:, None]), 0.0)
    V64 = c.V[b, h, :sp.skv].astype(np.float64)
    for _ in range(3):  # (row by row, each choice seen by the next: simultaneous updates can flip two coupled rows for ever)
        for i, j in zip(own, keys):
            rest = p[i] @ V64
            V64[j] = np.where(rest > 0, -8.0, np.where(rest < 0, 8.0, V64[j]))
    c.V[b, h, keys] = V64[keys].astype(np.float32)


def _plant_traps(c):
    sp = c.spec
    smax, relmax = -np.inf, 0.0 if c.rel_tab is None else float(np.abs(c.rel_tab[:, c.rel_lead:]).max())
    for b in range(sp.batch):
        vis = visible(c, b)
        if vis.any():
            smax = max(smax, max(float(np.where(vis, scores64(c, b, h), -np.inf).max()) for h in range(sp.heads)))
    smax = 0.0 if not np.isfinite(smax) else smax
    c.smax = smax
    for h in range(sp.heads):
        u = c.u[h].astype(np.float64)
        qu = c.Q[:, h].astype(np.float64) @ u
        assert qu.min() > 0.2 * qu.mean(), "q . u must stay positive for the traps to beat every row"
        t = (smax + 30.0 + relmax) / (float(c.scale) * qu.min())
        ktrap = round_bf16((1.01 * t * u).astype(np.float32))
        for b in range(sp.batch):
            js = np.arange(sp.skv, c.nk)
            if c.mask is not None:
                js = np.concatenate([np.flatnonzero(c.mask[b] == 0), js])
            c.K[b, h, js] = ktrap[None, :]
            c.V[b, h, js] = 64.0 * _signs(b + 64, h, js, sp.hd)


# ---- float64 reference --------------------------------------------------------------------------------------------------------------------
def _softmax_v(s, vis, V):
    """rows of softmax over the visible keys times V, zeros for a row without one; also A."""
    s = np.where(vis, s, -np.inf)
    m = s.max(1)
    live = np.isfinite(m)
    p = np.where(vis, np.exp(np.where(vis, s, 0.0) - np.where(live, m, 0.0)[:, None]), 0.0)
    l = p.sum(1)
    p = p / np.where(live, l, 1.0)[:, None]
    V = V.astype(np.float64)
    return p @ V, p @ np.abs(V), p


def reference(c):
    """(out, A): (batch, heads, sq, hd) float64."""
    sp = c.spec
    out = np.zeros((sp.batch, sp.heads, sp.sq, sp.hd))
    A = np.zeros_like(out)
    for b in range(sp.batch):
        vis = visible(c, b)
        for h in range(sp.heads):
            out[b, h], A[b, h], _ = _softmax_v(scores64(c, b, h), vis, c.V[b, h, :sp.skv])
    return out, A


def spike_weights(c):
    """(weights of the rows with >= 2 visible keys, weights of the rows with exactly one)."""
    sp = c.spec
    many, single = [], []
    for b in range(sp.batch):
        vis = visible(c, b)
        cnt = vis.sum(1)
        for h in range(sp.heads):
            p = _softmax_v(scores64(c, b, h), vis, c.V[b, h, :sp.skv])[2]
            pos = c.spike_pos[b, h]
            assert ((pos >= 0) == (cnt > 0)).all(), "every row with a visible key owns a spike"
            w = p[np.arange(sp.sq), np.maximum(pos, 0)]
            many.append(w[cnt >= 2])
            single.append(w[cnt == 1])
    return np.concatenate(many), np.concatenate(single)


def fp32_term(c, A) -> float:
    """The module docstring's explicit bound of the fp32 terms, as max over the elements of (bound / A_i)."""
    sp = c.spec
    worst = 0.0
    for b in range(sp.batch):
        vis = visible(c, b)
        for h in range(sp.heads):
            s = scores64(c, b, h)
            out, _, p = _softmax_v(s, vis, c.V[b, h, :sp.skv])
            qk = np.abs(c.Q[b, h].astype(np.float64)) @ np.abs(c.K[b, h, :sp.skv].astype(np.float64)).T
            eps = np.where(vis, sp.hd * 2.0 ** -24 * float(c.scale) * qk + 2.0 ** -23 * np.abs(s) + 2.0 ** -22, 0.0)  # relative error of p_ij
            absv = np.abs(c.V[b, h, :sp.skv].astype(np.float64))
            bound = (p * eps) @ absv + ((p * eps).sum(1))[:, None] * np.abs(out) + 2.0 * sp.skv * 2.0 ** -24 * A[b, h]
            live = A[b, h] > 0
            if live.any():
                worst = max(worst, float((bound[live] / A[b, h][live]).max()))
    return worst


# ---- fp32 / bf16 restatements of the kernels -------------------------------------------------------------------------------------------------
f32 = np.float32


def _fma(a, b, cc):
    return (a.astype(np.float64) * np.float64(b) + cc).astype(f32)


def _exp2(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(x.astype(np.float64)).astype(f32)


def _raw(c, b, h):
    sp = c.spec
    return (c.Q[b, h] @ c.K[b, h, :sp.skv].T).astype(f32)


def emulate(c):
    """The launch's kernel family restated in numpy float32 with bf16 P: (batch, heads, sq, hd) float32."""
    sp = c.spec
    fam = family(sp.form)
    out = np.zeros((sp.batch, sp.heads, sp.sq, sp.hd), f32)
    c.emu_rescales = {}
    for b in range(sp.batch):
        vis = visible(c, b)
        for h in range(sp.heads):
            fn = {"v1": _emu_v1, "v2": _emu_v2, "frame": _emu_frame, "frame3": _emu_frame3}[fam]
            out[b, h] = fn(c, b, h, vis)
    return out


def _emu_v1(c, b, h, vis):
    """attn_prefill_kernel: 64-key tiles, s = fl(raw * scale log2e) (+ fma of the bias), online maximum raised on every tile, p = exp2(s - m)."""
    sp = c.spec
    sl2 = f32(c.scale * LOG2E)
    s = (_raw(c, b, h) * sl2).astype(f32)
    if c.rel_tab is not None:
        s = _fma(c.rel_tab[h, c.rel_lead + rel_index(c)], LOG2E, s)
    m_run, l_run, acc = np.full(sp.sq, -1e30, f32), np.zeros(sp.sq, f32), np.zeros((sp.sq, sp.hd), f32)
    V = c.V[b, h]
    for k0 in range(0, sp.skv, 64):
        k1 = min(sp.skv, k0 + 64)
        ok = vis[:, k0:k1]
        m_new = np.maximum(m_run, np.where(ok, s[:, k0:k1], f32(-1e30)).max(1))
        alpha = _exp2(m_run - m_new)
        p = np.where(ok, _exp2(s[:, k0:k1] - m_new[:, None]), f32(0))
        l_run = (l_run * alpha + p.sum(1, dtype=f32)).astype(f32)
        acc = (acc * alpha[:, None] + (round_bf16(p) @ V[k0:k1]).astype(f32)).astype(f32)
        m_run = m_new
    inv = np.where(l_run > 0, f32(1) / np.where(l_run > 0, l_run, f32(1)), f32(0)).astype(f32)
    return round_bf16((acc * inv[:, None]).astype(f32))


def _emu_v2(c, b, h, vis):
    """attn_prefill_v2_kernel: raw scores (+ bias / scale), masked to -1e30, steps of 64 keys (32 at 9 waves and at hd 128 with 8 waves), the
    maximum raised only when some row of the WAVE (32 rows, rows past sq are q = 0) outgrows it by 2^6, p = exp2(fma(raw, scale log2e, -m))."""
    sp = c.spec
    nwq, db = (sp.form - 1000) // 100, (sp.form // 10) % 10
    step = 32 if (nwq > 8 or (db == 4 and nwq == 8)) else 64
    sl2 = f32(c.scale * LOG2E)
    rows = -(-sp.sq // 32) * 32
    off = sp.skv - sp.sq
    raw = np.zeros((rows, sp.skv), f32)
    raw[:sp.sq] = _raw(c, b, h)
    ok = np.ones((rows, sp.skv), bool)
    ok[:sp.sq] = vis
    if c.mask is not None:
        ok[sp.sq:] = (c.mask[b] != 0)[None, :]
    if sp.causal:
        ok[sp.sq:] &= np.arange(sp.skv)[None, :] <= np.arange(sp.sq, rows)[:, None] + off
    if c.rel_tab is not None:  # (the route guarantees cover for the real rows; the ghost rows index up to 31 slots into the zero slack)
        idx = np.arange(sp.skv)[None, :] - np.arange(rows)[:, None] - off + c.rel_off
        tab = np.concatenate([np.zeros(64, f32), c.rel_tab[h, c.rel_lead:c.rel_lead + c.rel_n], np.zeros(64, f32)])
        raw = _fma(tab[idx + 64], f32(1) / c.scale, raw)
    st = np.where(ok, raw, f32(-1e30))
    m_run, l_run, acc = np.full(rows, -1e30, f32), np.zeros(rows, f32), np.zeros((rows, sp.hd), f32)
    V = c.V[b, h]
    flags = []
    for k0 in range(0, sp.skv, step):
        k1 = min(sp.skv, k0 + step)
        # a wave skips the steps at and beyond its last row's causal limit (nothing visible there: the arithmetic below would add zeros)
        mxs = np.maximum((st[:, k0:k1].max(1) * sl2).astype(f32), f32(-1e30))
        trig = (~(mxs <= m_run + f32(6.0))).reshape(-1, 32).any(1).repeat(32)
        m_new = np.where(trig, np.maximum(m_run, mxs), m_run)
        alpha = _exp2(m_run - m_new)
        l_run = (l_run * alpha).astype(f32)
        acc = (acc * alpha[:, None]).astype(f32)
        m_run = m_new
        nm = -np.maximum(m_run, f32(-1e20))
        p = _exp2(_fma(st[:, k0:k1], sl2, nm.astype(np.float64)[:, None]))
        l_run = (l_run + p.sum(1, dtype=f32)).astype(f32)
        acc = (acc + (round_bf16(p) @ V[k0:k1]).astype(f32)).astype(f32)
        flags.append(trig[::32].copy())
    c.emu_rescales[(b, h)] = np.array(flags)  # [step, wave]
    inv = np.where(l_run > 0, f32(1) / np.where(l_run > 0, l_run, f32(1)), f32(0)).astype(f32)
    return round_bf16((acc * inv[:, None]).astype(f32))[:sp.sq]


def _single_pass(raw, sl2, V):
    """(sum, O) of one exact softmax pass relative to the rows' own maximum; also the maximum in exponent units."""
    mx = raw.max(1)
    nm = (-mx * sl2).astype(f32)
    p = _exp2(_fma(raw, sl2, nm.astype(np.float64)[:, None]))
    return p.sum(1, dtype=f32), (round_bf16(p) @ V).astype(f32), (mx * sl2).astype(f32)


def _emu_frame(c, b, h, vis):
    """attn_frame_kernel: every score of a row in registers, one pass, O * rcp(l)."""
    sp = c.spec
    l, o, _ = _single_pass(_raw(c, b, h), f32(c.scale * LOG2E), c.V[b, h, :sp.skv])
    return round_bf16((o * (f32(1) / l)[:, None]).astype(f32))


def _emu_frame3(c, b, h, vis):
    """attn_frame3_kernel: the patch rows as attn_frame_kernel; row 256 from eight partial softmaxes over keys 32 w .. 32 w + 31 (wave 0 also
    key 256), each relative to its own maximum, merged in fp32 in wave order."""
    sp = c.spec
    out = _emu_frame(c, b, h, vis)
    raw, sl2, V = _raw(c, b, h)[256:257], f32(c.scale * LOG2E), c.V[b, h, :sp.skv]
    parts = []
    for w in range(8):
        keys = np.r_[32 * w:32 * w + 32, 256] if w == 0 else np.r_[32 * w:32 * w + 32]
        parts.append(_single_pass(raw[:, keys], sl2, V[keys]))
    M = max(float(p[2][0]) for p in parts)
    L, o = f32(0), np.zeros(sp.hd, f32)
    for l_w, o_w, m_w in parts:
        fw = _exp2(np.array([m_w[0] - f32(M)], f32))[0]
        L = f32(np.float64(l_w[0]) * np.float64(fw) + np.float64(L))
        o = (o_w[0].astype(np.float64) * np.float64(fw) + o).astype(f32)
    out[256] = round_bf16((o / L).astype(f32))
    return out


# ---- mutations: the mistakes the tests must catch, in float64 ------------------------------------------------------------------------------
MUTATIONS = ("drop", "double", "swap_v", "shift", "causal+1", "causal-1", "mask_tile", "past_skv", "next_head_k", "next_row_q", "norescale",
             "rel+1", "rel-1", "rel_head", "scale_dropped")


def applies(mut: str, c) -> bool:
    sp = c.spec
    if mut in ("causal+1", "causal-1"):
        # the causal-diagonal cases: behind a left padding some row sees a handful of keys, so that one key more or less is a large part of it
        return bool(sp.causal) and sp.sq >= 2 and any(1 <= int(n) <= 8 for b in range(sp.batch) for n in visible(c, b).sum(1)[:-1])
    if mut == "mask_tile":
        return c.mask is not None and bool((c.mask == 0).any()) and bool((c.mask != 0).any())
    if mut == "past_skv":
        return not sp.causal
    if mut == "next_head_k":
        return sp.heads >= 2
    if mut == "next_row_q":
        # ("late": one key and the spike that balances it carry every row, and the spikes' values all oppose that one key's: the rows' outputs
        # are nearly the same vector, whichever q is used)
        return sp.sq >= 2 and _most_visible(c) >= 2 and sp.profile != "late"
    if mut == "norescale":
        return sp.profile in ("rise", "late") and family(sp.form) in ("v1", "v2")
    if mut in ("rel+1", "rel-1", "rel_head"):
        return c.rel_tab is not None and (mut != "rel_head" or sp.heads >= 2)
    if mut == "scale_dropped":
        return not sp.scale1
    if mut == "swap_v":
        return _most_visible(c) >= 2
    if mut == "double":
        return _most_visible(c) >= 2
    return True


def _most_visible(c) -> int:
    return max(int(visible(c, b).sum(1).max()) for b in range(c.spec.batch))


def mutated(c, mut: str):
    """The output (batch, heads, sq, hd) float64 of a kernel that makes the named mistake and is exact otherwise."""
    sp = c.spec
    out = np.zeros((sp.batch, sp.heads, sp.sq, sp.hd))
    ii = np.arange(sp.sq)
    for b in range(sp.batch):
        vis0 = visible(c, b)
        for h in range(sp.heads):
            vis, V, pos = vis0, c.V[b, h, :sp.skv], c.spike_pos[b, h]
            has = pos >= 0
            s = None
            if mut == "drop":
                vis = vis.copy()
                vis[ii[has], pos[has]] = False
            elif mut == "double":
                s = scores64(c, b, h)
                s[ii[has], pos[has]] += np.log(2.0)
            elif mut == "swap_v":  # row by row: the spike's V and the V of the row's first other visible key change places
                s = scores64(c, b, h)
                o, _, p = _softmax_v(s, vis, V)
                V64 = V.astype(np.float64)
                for i in ii[has]:
                    other = np.flatnonzero(vis[i] & (np.arange(sp.skv) != pos[i]))
                    if len(other):
                        j, k = pos[i], other[0]
                        o[i] += (p[i, j] - p[i, k]) * (V64[k] - V64[j])
                out[b, h] = o
                continue
            elif mut == "shift":  # P of key j meets V of key j + 1 (the guard row / stale slot for the last)
                V = c.V[b, h, 1:sp.skv + 1]
            elif mut in ("causal+1", "causal-1"):
                d = 1 if mut == "causal+1" else -1
                vis = np.arange(sp.skv)[None, :] <= ii[:, None] + (sp.skv - sp.sq) + d
                if c.mask is not None:
                    vis = vis & (c.mask[b] != 0)[None, :]
            elif mut == "mask_tile":  # the key mask is ignored in the first 64-key tile that holds a masked key
                j0 = int(np.flatnonzero(c.mask[b] == 0)[0]) // 64 * 64 if (c.mask[b] == 0).any() else -64
                m = c.mask[b] != 0
                m[max(j0, 0):j0 + 64] = True
                vis = np.ones((sp.sq, sp.skv), bool) & m[None, :]
                if sp.causal:
                    vis &= np.arange(sp.skv)[None, :] <= ii[:, None] + (sp.skv - sp.sq)
            elif mut == "past_skv":  # skv + 1 keys: the guard row / the first stale slot is read as a key
                s = scores64(c, b, h, K=c.K[b, h, :sp.skv + 1], B=None)
                if c.rel_tab is not None:
                    Bm = bias(c, h)
                    s += np.concatenate([Bm, Bm[:, -1:]], 1)
                vis = np.concatenate([vis, np.ones((sp.sq, 1), bool)], 1)
                V = c.V[b, h, :sp.skv + 1]
            elif mut == "next_head_k":
                s = scores64(c, b, h, K=c.K[b, (h + 1) % sp.heads, :sp.skv])
            elif mut == "next_row_q":
                s = scores64(c, b, h, Q=np.roll(c.Q[b, h], -1, axis=0))
            elif mut in ("rel+1", "rel-1"):
                s = scores64(c, b, h, B=bias(c, h, 1 if mut == "rel+1" else -1))
            elif mut == "rel_head":
                s = scores64(c, b, h, B=bias(c, (h + 1) % sp.heads))
            elif mut == "scale_dropped":
                s = scores64(c, b, h, scale=1.0)
            elif mut == "norescale":
                out[b, h] = _norescale(scores64(c, b, h), vis, V)
                continue
            out[b, h] = _softmax_v(scores64(c, b, h) if s is None else s, vis, V)[0]
    return out


def _norescale(s, vis, V):
    """Online softmax over 64-key tiles in float64 where O (not the row sum) misses its rescale on the LAST tile on which the row's
    maximum moves (the first tile with a visible key aside: there is nothing to rescale yet)."""
    sq, skv = s.shape
    s = np.where(vis, s, -np.inf)
    tmax = np.maximum.accumulate(np.stack([s[:, k0:k0 + 64].max(1) for k0 in range(0, skv, 64)], 1), 1)  # running maximum after each tile
    moved = np.isfinite(tmax[:, :-1]) & (tmax[:, 1:] > tmax[:, :-1])
    last = np.where(moved.any(1), moved.shape[1] - np.argmax(moved[:, ::-1], 1), -1)  # tile index of the last move
    m_run, l_run, acc = np.full(sq, -np.inf), np.zeros(sq), np.zeros((sq, V.shape[1]))
    V = V.astype(np.float64)
    for t, k0 in enumerate(range(0, skv, 64)):
        sl = s[:, k0:k0 + 64]
        m_new = np.maximum(m_run, sl.max(1))
        safe = np.where(np.isfinite(m_new), m_new, 0.0)
        alpha = np.where(np.isfinite(m_run), np.exp(np.where(np.isfinite(m_run), m_run, 0.0) - safe), 1.0)
        p = np.where(np.isfinite(sl), np.exp(np.where(np.isfinite(sl), sl, 0.0) - safe[:, None]), 0.0)
        skip = last == t
        l_run = l_run * alpha + p.sum(1)
        acc = acc * np.where(skip, 1.0, alpha)[:, None] + p @ V[k0:k0 + 64]
        m_run = m_new
    return np.where(l_run[:, None] > 0, acc / np.where(l_run > 0, l_run, 1.0)[:, None], 0.0)


# ---- memory layout ------------------------------------------------------------------------------------------------------------------------
def pack(c) -> SimpleNamespace:
    """The launch's buffers as bf16 bit patterns (int16) and its arguments in elements.  Row layouts: per batch entry the rows, ONE guard row
    (slot skv of K / V: traps; NaN bits in its q part) and one row of NaN bits; pad columns behind the last head hold NaN bits.  The output
    is (batch, sq + 1, D + 8) of SENT16."""
    sp = c.spec
    D, hd, n = sp.heads * sp.hd, sp.hd, sp.skv
    nan = np.int16(np.uint16(NAN_BITS).view(np.int16))

    def rows_of(x, upto):  # (batch, heads, r, hd) -> (batch, r, D) bits
        return bf16_bits(x[:, :, :upto]).transpose(0, 2, 1, 3).reshape(sp.batch, upto, D)

    P = SimpleNamespace(hs=hd)
    if sp.layout == "fused":
        buf = np.full((sp.batch, n + 2, 3 * D), nan, np.int16)
        buf[:, :n, :D] = rows_of(c.Q, n)
        buf[:, :n + 1, D:2 * D] = rows_of(c.K, n + 1)
        buf[:, :n + 1, 2 * D:] = rows_of(c.V, n + 1)
        P.bufs = {"qkv": buf}
        P.q, P.k, P.v = ("qkv", 0), ("qkv", D), ("qkv", 2 * D)
        P.ldq = P.ldk = P.ldv = 3 * D
        P.q_bs = P.k_bs = P.v_bs = (n + 2) * 3 * D
        P.q_hs = P.k_hs = P.v_hs = hd
        P.o_ld, P.o_rows = D + 8, sp.sq + 1
        return P
    qb = np.full((sp.batch, sp.sq + 1, D + 8), nan, np.int16)
    qb[:, :sp.sq, :D] = rows_of(c.Q, sp.sq)
    P.bufs = {"q": qb}
    P.q, P.ldq, P.q_bs, P.q_hs = ("q", 0), D + 8, (sp.sq + 1) * (D + 8), hd
    if sp.layout == "kv":
        kv = np.full((sp.batch, n + 2, 2 * D), nan, np.int16)
        kv[:, :n + 1, :D] = rows_of(c.K, n + 1)
        kv[:, :n + 1, D:] = rows_of(c.V, n + 1)
        P.bufs["kv"] = kv
        P.k, P.v = ("kv", 0), ("kv", D)
        P.ldk = P.ldv = 2 * D
        P.k_bs = P.v_bs = (n + 2) * 2 * D
        P.k_hs = P.v_hs = hd
    elif sp.layout == "sep":
        kb = np.full((sp.batch, n + 2, D + 8), nan, np.int16)
        vb = np.full((sp.batch, n + 2, D + 16), nan, np.int16)
        kb[:, :n + 1, :D] = rows_of(c.K, n + 1)
        vb[:, :n + 1, :D] = rows_of(c.V, n + 1)
        P.bufs.update(k=kb, v=vb)
        P.k, P.v = ("k", 0), ("v", 0)
        P.ldk, P.ldv = D + 8, D + 16
        P.k_bs, P.v_bs = (n + 2) * (D + 8), (n + 2) * (D + 16)
        P.k_hs = P.v_hs = hd
    else:  # cache planes [batch][heads][cap][hd]: nothing between them
        P.bufs.update(k=bf16_bits(c.K), v=bf16_bits(c.V))
        P.k, P.v = ("k", 0), ("v", 0)
        P.ldk = P.ldv = hd
        P.k_hs = P.v_hs = sp.cap * hd
        P.k_bs = P.v_bs = sp.heads * sp.cap * hd
    P.o_ld, P.o_rows = D + 8, sp.sq + 1
    return P


def unpack_out(c, obits: np.ndarray):
    """(values (batch, heads, sq, hd) float32, True iff every sentinel element is intact)."""
    sp = c.spec
    D = sp.heads * sp.hd
    o = obits.reshape(sp.batch, sp.sq + 1, D + 8)
    inside = np.zeros(o.shape, bool)
    inside[:, :sp.sq, :D] = True
    intact = bool((o[~inside].view(np.uint16) == SENT16).all())
    vals = bits_to_f32(np.ascontiguousarray(o[:, :sp.sq, :D])).reshape(sp.batch, sp.sq, sp.heads, sp.hd).transpose(0, 2, 1, 3)
    return vals, intact


def dead_rows(c) -> np.ndarray:
    """(batch, sq) bool: rows without a visible key."""
    return np.stack([~visible(c, b).any(1) for b in range(c.spec.batch)])


# ---- the launches of the GPU tests ------------------------------------------------------------------------------------------------------------
KEY_SWEEP = (32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)
LEFT_PAD = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)

# form -> the (hd, sq for the sweeps, force, smallest skv) pairs it is swept at: hd 80 where the form takes it and one other
SWEEP_AT = {
    V1_64: ((64, 100, 1, 32), (48, 100, 0, 32)),
    V1_96: ((80, 100, 1, 32), (96, 100, 0, 32)),
    V1_128: ((128, 100, 1, 32), (104, 100, 0, 32)),
    V2(2): ((80, 33, 0, 32), (72, 64, 0, 32)),
    V2(4): ((80, 100, 0, 32), (88, 128, 0, 32)),
    V2(8): ((80, 200, 0, 32), (72, 600, 0, 32)),
    V2(9): ((80, 270, 0, 32), (88, 288, 0, 32)),
    V2(4, 2): ((64, 128, 0, 64),),
    V2(8, 2): ((64, 170, 0, 64),),
    V2(4, 2, 1): ((64, 128, 0, 64),),
    V2(8, 2, 1): ((64, 170, 0, 64),),
    V2(4, 4): ((128, 70, 0, 64),),
    V2(8, 4): ((128, 140, 0, 64),),
}


def _rel_of(form):
    return "tight" if form in (V2(4, 2, 1), V2(8, 2, 1)) else ""


def sweep_specs(form: int):
    """The key-count sweep (guards trapped, every other one in the cache-plane layout with stale slots) of one v1 / v2 form."""
    out = []
    for hd, sq, force, lo in SWEEP_AT[form]:
        # (with a position bias a spike cannot be shared by two rows: the sweep is cut to skv >= sq, a key for every row)
        for n, skv in enumerate(v for v in KEY_SWEEP if v >= (sq if _rel_of(form) else lo)):
            lay = ("sep", "cache", "kv")[n % 3]
            out.append(Spec(f"keys-{form_name(form)}-hd{hd}-{skv}", form, batch=1, heads=2, hd=hd, sq=sq, skv=skv, layout=lay, cap=skv + 3 if lay == "cache" else 0,
                            rel=_rel_of(form), force=force, scale1=bool(n & 1), seed=n))
    return out


def pad_specs(form: int):
    """Left padding L on both sides of every 32- and 64-key boundary: causal with off = 0 (sq = skv > L where the form's row counts reach
    that far), causal with off > 0 (row L - off sees exactly one key, the rows before it none) and not causal.  Batch entry 1 carries the
    padding, entry 0 none."""
    out = []
    hd, sq, force, _ = SWEEP_AT[form][0]
    rel = _rel_of(form)
    for n, L in enumerate(LEFT_PAD):
        for kind in ("causal0", "causal+", "plain"):
            if kind == "causal0":
                q = k = max(sq, L + 40)
                if _first_form(hd, q, k, force, rel) != form:
                    q = k = sq
                    if L >= sq - 1:
                        continue  # (the form's row counts end before this padding does)
            elif kind == "causal+":
                q, k = sq, max(sq + 5, L + 8)
            else:
                q, k = sq, (L + sq + 5 if rel else max(sq + 37, L + 40))
            assert _first_form(hd, q, k, force, rel) == form
            out.append(Spec(f"pad-{form_name(form)}-L{L}-{kind}", form, batch=2, heads=2, hd=hd, sq=q, skv=k, layout="fused" if q == k and n & 1 else "sep",
                            causal=int(kind != "plain"), mask=("ones", f"left{L}"), rel=rel, force=force, spikes="last", scale1=not (n & 1), seed=n))
    return out


def mask_specs(form: int):
    """Holes, right padding, a different mask per batch entry, a batch entry with every key masked, a first tile fully masked; query counts
    that leave the last 32- and 64-row block partly empty.  (Causal: left padding only, and not causal with a position bias: twice as
    many keys as rows, so that every row finds a free key for its spike.)"""
    hd, sq, force, lo = SWEEP_AT[form][-1]
    out = []
    for d, lay, causal in ((0, "sep", 0), (1, "kv", 1)):
        skv = sq + d + 20 if causal else max(2 * lo, 200, 2 * sq if _rel_of(form) else 0)
        mask = ("left64", "ones", "dead") if causal else ("holes", "right70", "dead")
        if _first_form(hd, sq + d, skv, force, _rel_of(form)) == form:
            out.append(Spec(f"mask-{form_name(form)}-{sq + d}", form, batch=3, heads=2, hd=hd, sq=sq + d, skv=skv, layout=lay, causal=causal,
                            mask=mask, rel=_rel_of(form), force=force, seed=d))
    return out


def cache_specs(form: int):
    """Cache planes with 1, 5 and 33 query rows, as extend and the prompt-lookup verify step launch them (causal, left padding, stale slots)."""
    hd, _, force, lo = SWEEP_AT[form][0]
    out = []
    for sq in (1, 5, 33):
        skv = 150 + sq
        if _first_form(hd, sq, skv, force, _rel_of(form)) == form:
            out.append(Spec(f"cache-{form_name(form)}-q{sq}", form, batch=2, heads=3, hd=hd, sq=sq, skv=skv, layout="cache", cap=skv + 9, causal=1,
                            mask=("left7", "ones"), rel=_rel_of(form), force=force, scale1=True, spikes="last", seed=sq))
    return out


def online_specs(form: int):
    """Scores that rise tile by tile (every tile rescales), fall, one late dominant key; ten key tiles through the two-stage ring."""
    hd, sq, force, _ = SWEEP_AT[form][0]
    return [Spec(f"online-{form_name(form)}-{prof}", form, batch=1, heads=2, hd=hd, sq=sq, skv=640 + n, layout="sep", profile=prof, rel=_rel_of(form), force=force,
                 mask=("left70",) if prof == "rise" else (), scale1=prof == "fall", seed=n) for n, prof in enumerate(("rise", "fall", "late"))]


def lazy_specs():
    """v2: one query row whose maximum rises by LAZY_RISE base-2 units from key tile 0 to key tile 1: both sides of the threshold 6."""
    return [Spec(f"lazy-{form_name(form)}-hd{hd}", form, batch=3, heads=3, hd=hd, sq=1, skv=200, layout="cache", cap=208, profile="lazy", scale1=hd == 80)
            for form, hd in ((V2(2), 80), (V2(2), 88))]


def _first_form(hd, sq, skv, force, rel):
    """The route restated for the case builders only (test_attn_prefill_reference.form_of is the checked restatement)."""
    if force & 1:
        return 64 if hd <= 64 else (96 if hd <= 96 else 128)
    qt = -(-sq // 32)
    if hd == 64 and sq >= 128 and skv >= 64:
        return V2(8 if qt >= 5 else 4, 2, int(bool(rel)))
    if hd == 128 and sq >= 64 and skv >= 64 and not rel:
        return V2(8 if qt >= 5 else 4, 4)
    if hd in (72, 80, 88) and skv >= 32 and not rel:
        return V2(9 if qt == 9 else (8 if qt >= 5 else (4 if qt >= 3 else 2)))
    return 64 if hd <= 64 else (96 if hd <= 96 else 128)


def route_specs():
    """Both sides of every route boundary of launch_attention (the table of test_hip_attn_prefill.py)."""
    S = []

    def add(name, form, **kw):
        S.append(Spec(f"route-{name}", form, **{**dict(batch=1, heads=2, layout="sep"), **kw}))

    # v1<64>: hd 64 below 128 rows or below 64 keys (Q-Former self 32 x 32, cross 32 x several tiles in k|v rows); hd 32 / 48; a table that does not cover the launch
    add("qformer-self", V1_64, hd=64, sq=32, skv=32, layout="fused", batch=2, heads=3, mask=("ones", "right5"))
    add("qformer-cross", V1_64, hd=64, sq=32, skv=3 * 64 + 65, layout="kv", batch=2, heads=3)
    add("hd64-sq127", V1_64, hd=64, sq=127, skv=127, layout="fused")
    add("hd64-sq128", V2(4, 2), hd=64, sq=128, skv=128, layout="fused")
    add("hd64-skv63", V1_64, hd=64, sq=128, skv=63)
    add("hd64-skv64", V2(4, 2), hd=64, sq=128, skv=64)
    add("hd64-sq160", V2(8, 2), hd=64, sq=160, skv=160, causal=1)
    add("hd64-sq161", V2(8, 2), hd=64, sq=161, skv=161, layout="fused", causal=1)
    add("hd32", V1_64, hd=32, sq=130, skv=70)
    add("hd48", V1_64, hd=48, sq=130, skv=70, causal=1)
    add("rel-tight-127", V1_64, hd=64, sq=127, skv=127, rel="tight")
    add("rel-tight-128", V2(4, 2, 1), hd=64, sq=128, skv=128, rel="tight")
    add("rel-tight-160", V2(8, 2, 1), hd=64, sq=160, skv=160, rel="tight", scale1=True)
    add("rel-tight-161", V2(8, 2, 1), hd=64, sq=161, skv=161, rel="tight", scale1=True)
    add("rel-masked", V2(8, 2, 1), hd=64, sq=161, skv=200, rel="tight", scale1=True, mask=("left33",))
    add("rel-gap", V2(8, 2, 1), hd=64, sq=170, skv=190, rel="gap", scale1=True, causal=1)
    add("rel-gap4", V2(4, 2, 1), hd=64, sq=128, skv=130, rel="gap", scale1=True)
    add("rel-short", V1_64, hd=64, sq=130, skv=140, rel="short", scale1=True)
    add("rel-n4096", V2(8, 2, 1), hd=64, sq=130, skv=140, rel="n4096", scale1=True)
    add("rel-n4097", V1_64, hd=64, sq=130, skv=140, rel="n4097", scale1=True)
    # v1<96>: hd 72 / 80 / 88 below 32 keys; hd 96
    for hd in (72, 80, 88):
        add(f"hd{hd}-17x17", V1_96, hd=hd, sq=17, skv=17, layout="fused", causal=1, batch=2)
        add(f"hd{hd}-skv31", V1_96, hd=hd, sq=40, skv=31)
        add(f"hd{hd}-skv32", V2(2), hd=hd, sq=40, skv=32)
    add("hd96", V1_96, hd=96, sq=70, skv=130, causal=1)
    # v1<128>: hd 128 below 64 rows or keys; hd 104 / 120
    add("hd128-sq63", V1_128, hd=128, sq=63, skv=63, layout="fused")
    add("hd128-sq64", V2(4, 4), hd=128, sq=64, skv=64, layout="fused")
    add("hd128-skv63", V1_128, hd=128, sq=70, skv=63)
    add("hd128-skv64", V2(4, 4), hd=128, sq=70, skv=64)
    add("hd128-sq128", V2(4, 4), hd=128, sq=128, skv=128, layout="fused", causal=1)
    add("hd128-sq129", V2(8, 4), hd=128, sq=129, skv=129, layout="fused", causal=1)
    add("hd104", V1_128, hd=104, sq=70, skv=70, layout="fused")
    add("hd120", V1_128, hd=120, sq=70, skv=130, causal=1)
    # forced v1: multi-tile causal + mask + rel
    for hd, form in ((64, V1_64), (80, V1_96), (128, V1_128)):
        add(f"forced-hd{hd}", form, hd=hd, sq=150, skv=200, causal=1, mask=("left33",), rel="tight", force=1, batch=2, spikes="last")
    # v2<2> / <4> / <8> / <9> by ceil(sq / 32): 1-2 | 3-4 | 5-8 and 10-16 | 9 | > 16
    for sq, form in ((64, V2(2)), (65, V2(4)), (128, V2(4)), (129, V2(8)), (256, V2(8)), (257, V2(9)), (288, V2(9)), (289, V2(8)), (512, V2(8)), (513, V2(8))):
        for hd in (80, 72) if sq in (64, 257, 513) else (80,):
            add(f"hd{hd}-sq{sq}", form, hd=hd, sq=sq, skv=sq, layout="fused", causal=int(sq % 2 == 0), mask=("left3",) if sq % 2 else ())
    # hd 88, 257..272 rows: what the frame route refuses
    add("hd88-257-mask", V2(9), hd=88, sq=257, skv=257, layout="fused", mask=("holes",))
    add("hd88-264-causal", V2(9), hd=88, sq=264, skv=264, layout="fused", causal=1)
    add("hd88-272-ldk", V2(9), hd=88, sq=272, skv=272, layout="sep")
    add("hd88-257-sqskv", V2(9), hd=88, sq=257, skv=258, layout="sep")
    for n in (257, 258, 264, 272):
        add(f"frame-{n}", FRAME, hd=88, sq=n, skv=n, layout="fused", batch=2, heads=3)
    add("frame3-257", FRAME3, hd=88, sq=257, skv=257, layout="fused", batch=1, heads=3, force=16 << 1)
    return S


def frame_specs(num_cu: int = 256):
    """(frame, head) pair counts below, at and above the CU count with a ragged last round; frame3 at 1 and 3 frames and above the CU count."""
    kw = dict(hd=88, sq=257, skv=257, layout="fused")
    out = [Spec(f"frame-pairs{p}", FRAME, batch=p // 2, heads=2, seed=p, **kw) for p in (num_cu - 2, num_cu, num_cu + 38)]
    out += [Spec(f"frame3-frames{f}", FRAME3, batch=f, heads=2, force=16 << 1, seed=f, **kw) for f in (1, 3)]
    out.append(Spec(f"frame3-pairs{num_cu + 37}", FRAME3, batch=num_cu + 37, heads=1, force=16 << 1, seed=5, **kw))
    return out


V12_FORMS = tuple(SWEEP_AT)


def form_specs(form: int):
    return sweep_specs(form) + pad_specs(form) + mask_specs(form) + cache_specs(form) + online_specs(form)


def all_specs(num_cu: int = 256, frames: bool = True):
    out = route_specs() + lazy_specs()
    for form in V12_FORMS:
        out += form_specs(form)
    return out + (frame_specs(num_cu) if frames else [])


PRODUCT_CASES = ("route-qformer-cross", "route-hd96", "route-hd120", "route-hd80-sq64", "route-hd80-sq128", "route-hd80-sq256", "route-hd80-sq257",
                 "route-hd64-sq128", "route-hd64-sq160", "route-rel-tight-128", "route-rel-tight-161", "route-hd128-sq64", "route-hd128-sq129", "route-frame-257")

__all__ = [n for n in dir() if not n.startswith("__")]
_ = (replace, TOL_REL, tolerance, worst_ratio)
