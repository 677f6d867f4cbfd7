"""Cases, float64 reference, fp32 restatement and mutations of the shared-prefix attention kernel (eilev_prefix_attention,
eilev_amd/csrc/prefix.hip; test_prefix_ref.py holds the list to the restatement on the CPU, test_hip_prefix.py runs it on the GPU).  A plain
module: no fixtures, no GPU; built from the pieces of attn_prefill_ref.py / attn_decode_ref.py.

A launch: R rows of n new positions (stacked index s = r n + t) after one prefix of P keys in planes [heads][cap][hd].  Query s sees the
prefix keys [0, P) and the new keys s' of its own row with s' <= s.  Per head the launch is ONE attention problem of S = R n queries over
T = P + S keys with that visibility; the reference is numpy float64 softmax(scale q . k) v on the bf16-exact inputs, A_i = sum p |v| / sum p.

Tolerance: attn_decode_ref.tolerance, (2^-8 + 2^-11) A_i with no floor — the kernel's arithmetic is attn_prefill_kernel's (P rounded to bf16,
the row sum from the unrounded P, O / l rounded once), so the derivation in attn_prefill_ref.py applies with its preconditions, which
test_prefix_ref.py asserts: every query with >= 2 visible keys owns a spike of weight in [W_LO, W_HI] whose value +-8 opposes the rest,
ordinary |v| in [4, 8], fp32_term <= 2^-11.

Planted keys (attn_prefill_ref.py's construction on the general visibility).  q_s = bf16(0.35 n_s + u_h).  Even s take a free prefix key as
their spike (s = 0 always does), the others their own new key s; k = c_s n'_s / (scale n'_s . q_s), c_s settled in PASSES passes.  Prefix
slots [P, cap) are traps t u_h (score >= 30 above the launch's maximum for every query, v = +-64) except the last one of a cap >= P + 2,
which holds NaN bits, as do the guard rows behind the last q|k|v row.
Row marks: the last three head dims carry q = a onehot(r % 3) and k_new = a (1 - onehot(r' % 3)) (zero in the prefix, in u_h and in the
spike directions): exactly 0 for a key of the query's own row, a^2 scale >= maximum + 30 for a key of the row before or after — a new key
that leaks across rows is as loud as a trap."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from attn_decode_ref import NAN_BITS, _normal_rows, _signs, bf16_bits, tolerance, worst_ratio  # noqa: F401  (re-exported for the tests)
from attn_prefill_ref import LOG2E, PASSES, SENT16, W_HI, W_LO, W_TARGET, _exp2, _hash, _softmax_v  # noqa: F401
from eilev_amd.synth import round_bf16

f32 = np.float32
TILE = 64  # stacked queries per workgroup, keys per tile


@dataclass(frozen=True)
class Spec:
    name: str
    hd: int
    heads: int
    P: int
    cap: int
    n: int
    R: int
    scale1: bool = True  # scale = 1.0 with pre-scaled q (the OPT path); else 1 / sqrt(hd)
    seed: int = 0


CASES = (
    Spec("one", 80, 2, 1, 1, 1, 1),
    Spec("p1-n2", 128, 3, 1, 4, 2, 3),
    Spec("p1-n5", 80, 2, 1, 3, 5, 3, scale1=False),
    Spec("p31-n5-r45", 80, 3, 31, 31, 5, 45),      # a tile spans 13 rows; 225 stacked queries: boundaries inside rows, a ragged last tile
    Spec("p32-n5-r45", 128, 2, 32, 40, 5, 45),
    Spec("p33-n33-r3", 80, 2, 33, 36, 33, 3),      # the tile boundary falls inside row 1
    Spec("p33-n33-r3-s", 128, 2, 33, 33, 33, 3, scale1=False),
    Spec("p127-n70-r3", 128, 2, 127, 127, 70, 3),  # a row spans two tiles
    Spec("p128-n200-r2", 80, 2, 128, 130, 200, 2),  # a row spans four tiles: a window of up to 263 new keys
    Spec("p129-n200-r2", 128, 2, 129, 129, 200, 2),
    Spec("p129-n70-r1", 80, 2, 129, 140, 70, 1, scale1=False),
    Spec("p300-n2-r32", 80, 2, 300, 320, 2, 32),   # exactly one tile of 32 rows
    Spec("p300-n1-r45", 128, 3, 300, 300, 1, 45),
)


def by_name(name):
    return next(sp for sp in CASES if sp.name == name)


def visible(sp: Spec) -> np.ndarray:
    """(S, P + S) bool."""
    S = sp.R * sp.n
    s = np.arange(S)
    new = (s[None, :] // sp.n == s[:, None] // sp.n) & (s[None, :] <= s[:, None])
    return np.concatenate([np.ones((S, sp.P), bool), new], axis=1)


def _scores(c, h, Kall=None):
    Kall = c.Kall(h) if Kall is None else Kall
    return float(c.scale) * (c.Q[h].astype(np.float64) @ Kall.astype(np.float64).T)


def build_case(sp: Spec) -> SimpleNamespace:
    """Logical inputs as bf16-exact float32: Q, Kn, Vn (heads, S, hd); Kp, Vp (heads, cap, hd) (a NaN slot where the docstring says)."""
    S, P, hd = sp.R * sp.n, sp.P, sp.hd
    c = SimpleNamespace(spec=sp, S=S, T=P + S, scale=f32(1.0) if sp.scale1 else f32(1.0 / np.sqrt(f32(hd))), vis=visible(sp))
    marks = np.arange(hd - 3, hd)
    c.u = 0.35 * _signs(977, np.arange(sp.heads), 0, hd)
    c.u[:, marks] = 0.0
    nq = _normal_rows("pq", 1, sp.heads, S * hd, sp.seed)[0].reshape(sp.heads, S, hd)
    q = (0.35 * nq + c.u[:, None, :]) * (f32(1.0 / np.sqrt(f32(hd))) if sp.scale1 else f32(1))
    k = _normal_rows("pk", 1, sp.heads, (sp.cap + S) * hd, sp.seed)[0].reshape(sp.heads, sp.cap + S, hd)
    v = _normal_rows("pv", 1, sp.heads, (sp.cap + S) * hd, sp.seed)[0].reshape(sp.heads, sp.cap + S, hd)
    v = np.where(v < 0, -1.0, 1.0) * (4.0 + np.minimum(np.abs(v), 4.0))  # ordinary |v| in [4, 8]
    # the row marks
    c.mark = f32(8.0 if sp.scale1 else 32.0)
    row = np.arange(S) // sp.n
    onehot = (row[:, None] % 3 == np.arange(3)[None, :]).astype(f32)
    q[:, :, marks] = c.mark * onehot[None]
    k[:, :sp.cap, marks] = 0.0
    k[:, sp.cap:, marks] = c.mark * (1.0 - onehot)[None]
    c.Q, K, V = round_bf16(q.astype(f32)), round_bf16(k.astype(f32)), round_bf16(v.astype(f32))
    c.Kp, c.Kn, c.Vp, c.Vn = K[:, :sp.cap], K[:, sp.cap:], V[:, :sp.cap], V[:, sp.cap:]
    c.Kall = lambda h: np.concatenate([c.Kp[h, :P], c.Kn[h]])
    c.Vall = lambda h: np.concatenate([c.Vp[h, :P], c.Vn[h]])
    c.spike_pos = np.zeros((sp.heads, S), np.int64)
    for h in range(sp.heads):
        _plant_spikes(c, h, marks)
    _plant_traps(c)
    return c


def _assign_spikes(sp: Spec, h: int) -> np.ndarray:
    S = sp.R * sp.n
    order = sorted(range(sp.P), key=lambda j: _hash(j, h, sp.seed, sp.P))  # the prefix keys in a hashed order
    pos = sp.P + np.arange(S)
    for i, s in enumerate(range(0, S, 2)):
        if i < len(order):
            pos[s] = order[i]
    return pos


def _set_key(c, h, j, val):
    (c.Kp if j < c.spec.P else c.Kn)[h, j if j < c.spec.P else j - c.spec.P] = val


def _set_val(c, h, j, val):
    (c.Vp if j < c.spec.P else c.Vn)[h, j if j < c.spec.P else j - c.spec.P] = val


def _plant_spikes(c, h, marks):
    sp, vis = c.spec, c.vis
    pos = _assign_spikes(sp, h)
    c.spike_pos[h] = pos
    rows = np.arange(c.S)
    Q = c.Q[h].astype(np.float64)
    u = c.u[h].astype(np.float64)
    nperp = Q - np.outer(Q @ u / (u @ u), u)
    nperp[:, marks] = 0.0
    direction = nperp / (float(c.scale) * np.einsum("id,id->i", nperp, Q))[:, None]  # score 1 for the own query
    keep_marks = np.zeros((c.S, sp.hd))
    new = pos >= sp.P
    keep_marks[new] = c.Kn[h][pos[new] - sp.P] * (np.arange(sp.hd) >= sp.hd - 3)  # a new key keeps its row mark (0 against its own row)
    logit = float(np.log(W_TARGET / (1.0 - W_TARGET)))
    for _ in range(PASSES):
        s = np.where(vis, _scores(c, h), -np.inf)
        s[rows, pos] = -np.inf
        m = s.max(1)
        live = np.isfinite(m)  # (a query whose only visible key is its spike: weight 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lse = np.where(live, m + np.log(np.exp(s - np.where(live, m, 0.0)[:, None]).sum(1)), 0.0)
        cval = np.where(live, lse + logit, 0.0)
        for i in rows:
            _set_key(c, h, pos[i], round_bf16((direction[i] * cval[i] + keep_marks[i]).astype(f32)))
    for i in rows:
        _set_val(c, h, pos[i], 8.0 * _signs(0, h, pos[i], sp.hd))
    s = np.where(vis, _scores(c, h), -np.inf)
    s[rows, pos] = -np.inf
    with np.errstate(invalid="ignore"):
        mx = s.max(1)
        p = np.where(np.isfinite(s), np.exp(s - np.where(np.isfinite(mx), mx, 0.0)[:, None]), 0.0)
    V64 = c.Vall(h).astype(np.float64)
    for _ in range(3):  # (query by query, each choice seen by the next)
        for i in rows:
            rest = p[i] @ V64
            V64[pos[i]] = np.where(rest > 0, -8.0, np.where(rest < 0, 8.0, V64[pos[i]]))
    for i in rows:
        _set_val(c, h, pos[i], V64[pos[i]].astype(f32))


def _plant_traps(c):
    sp = c.spec
    smax = max(float(np.where(c.vis, _scores(c, h), -np.inf).max()) for h in range(sp.heads))
    c.smax = smax
    assert float(c.scale) * float(c.mark) ** 2 >= smax + 30.0, "a leaked new key must be as loud as a trap"
    for h in range(sp.heads):
        u = c.u[h].astype(np.float64)
        qu = c.Q[h].astype(np.float64) @ u
        assert qu.min() > 0.2 * qu.mean(), "q . u must stay positive for the traps to beat every query"
        t = (smax + 30.0) / (float(c.scale) * qu.min())
        js = np.arange(sp.P, sp.cap)
        c.Kp[h, js] = round_bf16((1.01 * t * u).astype(f32))[None, :]
        c.Vp[h, js] = 64.0 * _signs(64, h, js, sp.hd)
    c.nan_slot = sp.cap - 1 if sp.cap >= sp.P + 2 else -1


# ---- float64 reference ------------------------------------------------------------------------------------------------------------------
def reference(c):
    """(out, A): (S, heads, hd) float64 — the layout of the kernel's output."""
    sp = c.spec
    out, A = np.zeros((c.S, sp.heads, sp.hd)), np.zeros((c.S, sp.heads, sp.hd))
    for h in range(sp.heads):
        out[:, h], A[:, h], _ = _softmax_v(_scores(c, h), c.vis, c.Vall(h))
    return out, A


def spike_weights(c):
    """(weights of the queries with >= 2 visible keys, weights of those with exactly one)."""
    cnt = c.vis.sum(1)
    many, single = [], []
    for h in range(c.spec.heads):
        p = _softmax_v(_scores(c, h), c.vis, c.Vall(h))[2]
        w = p[np.arange(c.S), c.spike_pos[h]]
        many.append(w[cnt >= 2])
        single.append(w[cnt == 1])
    return np.concatenate(many), np.concatenate(single)


def ordinary_abs_v(c):
    """|v| of every visible key that is no query's spike."""
    out = []
    for h in range(c.spec.heads):
        keep = np.ones(c.T, bool)
        keep[c.spike_pos[h]] = False
        out.append(np.abs(c.Vall(h)[keep]).ravel())
    return np.concatenate(out)


def fp32_term(c, A) -> float:
    """attn_prefill_ref.fp32_term on this visibility: the explicit bound of the fp32 terms as max over the elements of (bound / A_i)."""
    sp = c.spec
    worst = 0.0
    for h in range(sp.heads):
        s = _scores(c, h)
        out, _, p = _softmax_v(s, c.vis, c.Vall(h))
        qk = np.abs(c.Q[h].astype(np.float64)) @ np.abs(c.Kall(h).astype(np.float64)).T
        eps = np.where(c.vis, sp.hd * 2.0 ** -24 * float(c.scale) * qk + 2.0 ** -23 * np.abs(s) + 2.0 ** -22, 0.0)
        absv = np.abs(c.Vall(h).astype(np.float64))
        nkeys = sp.P + min(sp.n, c.S)
        bound = (p * eps) @ absv + ((p * eps).sum(1))[:, None] * np.abs(out) + 2.0 * nkeys * 2.0 ** -24 * A[:, h]
        worst = max(worst, float((bound / A[:, h]).max()))
    return worst


# ---- the kernel restated in fp32 ----------------------------------------------------------------------------------------------------------
def emulate(c):
    """prefix_attn_kernel in numpy float32 with bf16 P: per tile of 64 stacked queries the prefix tiles [0, P) in steps of 64, then the
    window of new keys [first row of the tile * n, last query of the tile] in steps of 64 from its start; s = fl(raw * scale log2 e), the
    maximum raised on every tile, p = exp2(s - m).  (S, heads, hd) float32."""
    sp = c.spec
    sl2 = f32(c.scale * LOG2E)
    out = np.zeros((c.S, sp.heads, sp.hd), f32)
    for h in range(sp.heads):
        Kall, Vall = c.Kall(h), c.Vall(h)
        for s0 in range(0, c.S, TILE):
            s1 = min(s0 + TILE, c.S)
            nq = s1 - s0
            s = ((c.Q[h, s0:s1] @ Kall.T).astype(f32) * sl2).astype(f32)
            vis = c.vis[s0:s1]
            m_run, l_run, acc = np.full(nq, -1e30, f32), np.zeros(nq, f32), np.zeros((nq, sp.hd), f32)
            w0 = (s0 // sp.n) * sp.n
            tiles = [(k0, min(k0 + TILE, sp.P)) for k0 in range(0, sp.P, TILE)] + [(sp.P + k0, sp.P + min(k0 + TILE, s1)) for k0 in range(w0, s1, TILE)]
            for k0, k1 in tiles:
                ok = vis[:, k0:k1]
                m_new = np.maximum(m_run, np.where(ok, s[:, k0:k1], f32(-1e30)).max(1))
                alpha = _exp2(m_run - m_new)
                p = np.where(ok, _exp2(s[:, k0:k1] - m_new[:, None]), f32(0))
                l_run = (l_run * alpha + p.sum(1, dtype=f32)).astype(f32)
                acc = (acc * alpha[:, None] + (round_bf16(p) @ Vall[k0:k1]).astype(f32)).astype(f32)
                m_run = m_new
            inv = np.where(l_run > 0, f32(1) / np.where(l_run > 0, l_run, f32(1)), f32(0)).astype(f32)
            out[s0:s1, h] = round_bf16((acc * inv[:, None]).astype(f32))
    return out


# ---- mutations: the mistakes the tests must catch, in float64 ------------------------------------------------------------------------------
MUTATIONS = ("prefix_drop", "prefix_double", "prefix_wrong_v", "slot_P", "causal+1", "causal-1", "prev_row", "next_row", "next_head", "norescale")


def applies(mut: str, sp: Spec) -> bool:
    if mut == "prefix_wrong_v":
        return sp.cap >= 2  # (there is another slot whose value can be taken)
    if mut == "slot_P":
        return sp.cap > sp.P
    if mut == "causal+1":
        # one ordinary key more must be a large part of what some query sees: the handful-of-keys cases (attn_prefill_ref.applies has the same rule)
        return sp.n >= 2 and sp.P + 1 <= 8
    if mut in ("prev_row", "next_row"):
        return sp.R >= 2
    if mut == "next_head":
        return sp.heads >= 2
    if mut == "norescale":
        # some query's maximum must rise in the second phase: a query whose spike is its own new key, over a prefix of many ordinary keys (the
        # spike then sits log(number of keys) above them)
        return sp.R * sp.n >= 2 and sp.P >= 31
    return True


def mutated(c, mut: str):
    """The float64 result of a kernel with the mistake `mut`: (S, heads, hd)."""
    sp = c.spec
    S, P = c.S, sp.P
    out = np.zeros((S, sp.heads, sp.hd))
    s_idx = np.arange(S)
    same_row = s_idx[None, :] // sp.n == s_idx[:, None] // sp.n
    for h in range(sp.heads):
        hk = (h + 1) % sp.heads if mut == "next_head" else h
        K = np.concatenate([c.Kp[hk, :P], c.Kn[hk]]).astype(np.float64)
        V = c.Vall(h).astype(np.float64)
        vis = c.vis.copy()
        jm = int(c.spike_pos[h][0])  # the prefix key that is query 0's spike
        assert jm < P
        if mut == "prefix_drop":
            vis[:, jm] = False
        elif mut == "prefix_double":
            K, V, vis = np.vstack([K, K[jm:jm + 1]]), np.vstack([V, V[jm:jm + 1]]), np.hstack([vis, np.ones((S, 1), bool)])
        elif mut == "prefix_wrong_v":
            V[jm] = c.Vp[h, jm + 1 if jm + 1 < sp.cap and jm + 1 != c.nan_slot else jm - 1]
        elif mut == "slot_P":
            K, V, vis = np.vstack([K, c.Kp[hk, P:P + 1]]), np.vstack([V, c.Vp[h, P:P + 1]]), np.hstack([vis, np.ones((S, 1), bool)])
        elif mut == "causal+1":
            vis[:, P:] = same_row & (s_idx[None, :] <= s_idx[:, None] + 1)
        elif mut == "causal-1":
            vis[:, P:] = same_row & (s_idx[None, :] < s_idx[:, None])
        elif mut == "prev_row":
            vis[:, P:] |= s_idx[None, :] // sp.n == s_idx[:, None] // sp.n - 1
        elif mut == "next_row":
            vis[:, P:] |= s_idx[None, :] // sp.n == s_idx[:, None] // sp.n + 1
        sc = float(c.scale) * (c.Q[h].astype(np.float64) @ K.T)
        if mut != "norescale":
            out[:, h] = _softmax_v(sc, vis, V)[0]
            continue
        # the running (sum, O) of the prefix phase kept relative to ITS maximum while the new keys are taken relative to the raised one
        m1 = np.where(vis[:, :P], sc[:, :P], -np.inf).max(1)
        m2 = np.maximum(m1, np.where(vis[:, P:], sc[:, P:], -np.inf).max(1))
        p1 = np.where(vis[:, :P], np.exp(sc[:, :P] - m1[:, None]), 0.0)
        p2 = np.where(vis[:, P:], np.exp(sc[:, P:] - m2[:, None]), 0.0)
        out[:, h] = (p1 @ V[:P] + p2 @ V[P:]) / (p1.sum(1) + p2.sum(1))[:, None]
    return out


# ---- memory images ---------------------------------------------------------------------------------------------------------------------
def pack(c):
    """int16 bf16 bit patterns: qkv (S + 1, 3 heads hd) — one q|k|v buffer, its guard row NaN bits; kp, vp (heads, cap, hd); out (S + 1,
    heads hd) filled with the sentinel."""
    sp = c.spec
    D = sp.heads * sp.hd
    qkv = np.full((c.S + 1, 3 * D), NAN_BITS, np.uint16).view(np.int16)
    for i, a in enumerate((c.Q, c.Kn, c.Vn)):
        qkv[:c.S, i * D:(i + 1) * D] = bf16_bits(a.transpose(1, 0, 2).reshape(c.S, D))
    kp, vp = bf16_bits(c.Kp).copy(), bf16_bits(c.Vp).copy()
    if c.nan_slot >= 0:
        kp[:, c.nan_slot] = np.uint16(NAN_BITS).view(np.int16)
        vp[:, c.nan_slot] = np.uint16(NAN_BITS).view(np.int16)
    out = np.full((c.S + 1, D), SENT16, np.uint16).view(np.int16)
    return SimpleNamespace(qkv=qkv, kp=kp, vp=vp, out=out, D=D)
