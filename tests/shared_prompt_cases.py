"""Cases and fp32 restatement of the shared-prompt decode attention (include/eilev_prefix.h eilev_prefix_decode_attention) for
test_shared_prompt_ref.py (CPU) and test_hip_shared_prompt.py (GPU).  A plain module: no fixtures, no GPU.

The reference, the case builder and the derived tolerance are attn_decode_ref's, unchanged: a case is one of its ``Spec``s in the beam form
(beams > 0).  What this module adds on top of ``build_case``:
  * stale PROMPT slots.  The beam-form builder traps the generation cache only (its prompt planes end at seq_len); here the planes hold
    ``cap`` > seq_len slots and those at or beyond seq_len carry +-64 ("trap") or the bf16 NaN bits ("nan").  ``effective`` never reads them.
  * n_gen > cap_g.  The kernel then writes nothing and reads the newest key (slot cap_g - 1) from the row's own cache slot, while the
    builder keeps that key in the q|k|v row: the slot is given the row's k / v, so both hold the same key.
  * spikes with one owner per storage slot (``_plant_shared``): the builder's slots, planted so that rows which share a prompt key or an
    ancestor's generated key do not undo each other's spike.
  * ancestor entries outside [0, rows): ``anc_raw`` is the table with entries that the kernel's clamp maps back to ``anc``.

The restatement (``emulate``) is the kernel's partition in numpy float32: per SAMPLE the prompt ranges of PROMPT_KEYS keys in 64-key tiles
(online rescale between the tiles of a range), per ROW the GEN_KEYS ranges of the generated keys from seq_len on through the ancestor
table, one merge of all records; P rounded to bf16 for the product, the row sum from the unrounded P, one rounding of O / l."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import attn_decode_ref as R
from attn_decode_ref import Spec
from eilev_amd import abi
from eilev_amd.synth import round_bf16

PROMPT_KEYS = abi.PREFIX_DECODE_PROMPT_KEYS  # R: the prompt range of one workgroup
GEN_KEYS = abi.PREFIX_DECODE_GEN_KEYS
TILE = 64
FOREIGN = -20.0  # the score of a spike in shared storage for the rows that do not own it

SAMPLES_BEAMS = ((1, 1), (1, 5), (2, 3), (1, 17), (1, 32), (4, 8), (3, 7))
SEQ_LENS = tuple(sorted({1, TILE - 1, TILE, TILE + 1, PROMPT_KEYS - 1, PROMPT_KEYS, PROMPT_KEYS + 1, 2 * PROMPT_KEYS - 1, 2 * PROMPT_KEYS,
                         2 * PROMPT_KEYS + 1, 300}))
CAPG_NGEN = ((1, 1), (4, 1), (4, 2), (4, 4), (4, 7), (130, 1), (130, 2), (130, 130), (130, 133), (1, 4))
# "mixed" rows cycle through attn_decode_ref.MASK_KINDS from mask_first: the last sample of each is "dead" (every prompt key masked)
MIXED_FIRST = {1: (7, 2, 5), 2: (6,), 3: (5,), 4: (4,)}


def _spec(name, samples, beams, heads, hd, seq_len, cap_g, n_gen, mask, stale, spikes="beam", k=0, pad=5, seed=0):
    first = MIXED_FIRST[samples][k % len(MIXED_FIRST[samples])] if mask == "mixed" else 0
    return Spec(name=name, form="shared", batch=samples * beams, beams=beams, heads=heads, hd=hd, seq_len=seq_len, cap=seq_len + pad, cap_g=cap_g, n_gen=n_gen,
                mask=mask, mask_first=first, spikes=spikes, stale=stale, seed=seed)


def sweep_specs():
    """Every seq_len of SEQ_LENS twice; the other dimensions cycle with strides that are pairwise coprime to each other's lengths."""
    out = []
    for i, seq in enumerate(SEQ_LENS):
        for k in range(2):
            idx = 2 * i + k
            samples, beams = SAMPLES_BEAMS[idx % 7]
            cap_g, n_gen = CAPG_NGEN[(idx * 3) % 10]
            hd = (80, 128)[(idx // 2 + idx) % 2]
            out.append(_spec(f"sweep-L{seq}-{k}", samples, beams, (2, 3)[(idx // 3) % 2], hd, seq, cap_g, n_gen, ("none", "ones", "mixed")[idx % 3],
                             ("trap", "nan")[(idx // 2) % 2], k=idx, pad=(5, 70)[idx % 2]))
    return out


def extra_specs():
    out = []
    for hd in (80, 128):  # the full generation cache and the count beyond it, at both head sizes, two generated ranges
        out.append(_spec(f"gen-full-{hd}", 2, 3, 2, hd, 65, 130, 130, "mixed", "nan"))
        out.append(_spec(f"gen-over-{hd}", 1, 5, 3, hd, 129, 130, 133, "ones", "trap"))
        out.append(_spec(f"gen-over-small-{hd}", 3, 7, 2, hd, 300, 4, 7, "mixed", "nan"))
        out.append(_spec(f"dead-only-{hd}", 1, 17, 2, hd, 257, 4, 2, "mixed", "trap", k=0))  # one sample, every prompt key masked
    # cover: every key slot of [0, 384) (prompt range and tile boundaries) is the spike of some (row, head) of 32 rows x 3 heads
    for k in range(4):
        out.append(_spec(f"cover-prompt-{k}", 1, 32, 3, (80, 128)[k % 2], 383, 4, 1, "none", "trap", spikes=("cover", k)))
    # ... and every slot of 65 prompt + 130 generated keys (the generated-range boundary at key 65 + 128) of 4 samples x 8 beams
    for k in range(3):
        out.append(_spec(f"cover-gen-{k}", 4, 8, 3, (128, 80)[k % 2], 65, 130, 130, "ones", "nan", spikes=("cover", k)))
    out.append(_spec("bad-ancestors", 2, 3, 3, 80, 129, 130, 40, "mixed", "trap"))
    return out


def all_specs():
    return sweep_specs() + extra_specs()


def nsplit_of(sp: Spec) -> int:
    return -(-sp.seq_len // PROMPT_KEYS) + -(-sp.cap_g // GEN_KEYS)


def part_bytes_of(sp: Spec) -> int:
    return abi.prefix_decode_part_bytes(sp.batch, sp.heads, sp.hd, sp.seq_len, sp.cap_g)


def _plant_shared(c):
    """The builder's spike slots (attn_decode_ref._spike_slot: "beam", ("cover", k)), planted for rows that SHARE storage.  The builder plants
    row after row; a prompt key belongs to every row of its sample and a generated key to every row that descends from its writer, so a
    later row's spike moves an earlier row's scores and values, and the earlier spike no longer opposes the rest of its row — the
    precondition of the derived tolerance (attn_decode_ref's docstring).  Here a storage slot has ONE owner: a (row, head) whose slot is
    taken falls back to the newest key, which lives in its own q|k|v row, and a key in shared storage scores FOREIGN (-20: no weight) for the
    other rows of its sample, so a spike is a spike to its owner alone; two passes, the second over the final keys."""
    sp = c.spec
    taken = set()
    for b in range(sp.batch):
        vis = R.effective(c, b)[2]
        for h in range(sp.heads):
            j = R._spike_slot(c, b, h, vis)
            j = c.n - 1 if j < 0 else j
            ka, _, ik, _ = R._store(c, b, h, j)
            where = (id(ka), b, h, j) if ka is c.qkv else (id(ka),) + tuple(int(x) for x in ik)
            if where in taken:
                j = c.n - 1
            else:
                taken.add(where)
            c.spike_pos[b, h] = j
    for _ in range(2):
        for b in range(sp.batch):
            K, V, vis, _ = R.effective(c, b)
            s = R.scores64(c, b, K, None)
            q = R._q(c, b).astype(np.float64)
            for h in range(sp.heads):
                j = int(c.spike_pos[b, h])
                others = vis.copy()
                others[j] = False
                so = s[h, others]
                cval = float(so.max() + np.log(np.exp(so - so.max()).sum())) if so.size else 0.0
                sign = R._signs(b, h, j, sp.hd)
                if so.size:
                    rest = np.exp(so - so.max()) @ V[h, others].astype(np.float64)
                    sign = np.where(rest > 0, -1.0, np.where(rest < 0, 1.0, sign)).astype(np.float32)
                ka, va, ik, iv = R._store(c, b, h, j)
                if ka is c.qkv:
                    k = q[h] * cval / (q[h] @ q[h])
                else:  # score cval for the owner, FOREIGN for the rows that share the slot: the least-norm key that does both (beams <= 32 < hd)
                    g0 = b - b % sp.beams
                    Q = np.stack([R._q(c, r)[h] for r in range(g0, g0 + sp.beams)]).astype(np.float64)
                    t = np.full(sp.beams, FOREIGN)
                    t[b - g0] = cval
                    k = np.linalg.lstsq(Q, t, rcond=None)[0]
                ka[ik] = round_bf16(k.astype(np.float32))
                va[iv] = 8.0 * sign


def build(sp: Spec):
    """attn_decode_ref.build_case plus the additions of the module docstring; c.writes = the step stores its K / V."""
    c = R.build_case(replace(sp, spikes="none"))  # (the traps of the masked and stale slots; the spikes follow, shared-aware)
    c.spec = sp
    _plant_shared(c)
    d = c.d
    if sp.cap > sp.seq_len:
        js = np.arange(sp.seq_len, sp.cap)
        for s in range(c.srows):
            if sp.stale == "nan":
                c.kc[s][:, js] = np.nan
                c.vc[s][:, js] = np.nan
            else:
                hh = np.arange(sp.heads)[:, None]
                c.kc[s][:, js] = 64.0 * R._signs(s, hh, js[None, :] + 8192, sp.hd)
                c.vc[s][:, js] = 64.0 * R._signs(s, hh, js[None, :] + 12288, sp.hd)
    c.writes = 1 <= sp.n_gen <= sp.cap_g
    if not c.writes:  # the newest key is read from the row's own slot cap_g - 1
        for b in range(sp.batch):
            c.kg[b][:, sp.cap_g - 1] = c.qkv[b, d:2 * d].reshape(sp.heads, sp.hd)
            c.vg[b][:, sp.cap_g - 1] = c.qkv[b, 2 * d:3 * d].reshape(sp.heads, sp.hd)
    c.anc_raw = c.anc.copy()
    if sp.name == "bad-ancestors":
        c.anc_raw[c.anc == 0] = -5
        c.anc_raw[c.anc == sp.batch - 1] = sp.batch + 7
        c.anc_raw[c.n - sp.seq_len - 1, :] = c.anc[c.n - sp.seq_len - 1, :]
        live = c.anc_raw[:c.n - sp.seq_len]
        assert ((live < 0) | (live >= sp.batch)).any()
        c.anc_raw[c.n - sp.seq_len:] = 2 ** 31 - 1  # (rows of steps not reached: never read)
    return c


MUTATIONS = ("other_sample_plane", "other_sample_mask", "neighbour_query", "drop_boundary", "double_boundary", "ignore_ancestors", "stale_newest",
             "gen_from_0")


def _record(s, V, f=np.float32):
    """One range in tiles of 64 keys: s (heads, n) float32 scores with -1e30 where invisible, V (heads, n, hd) -> (max, sum, o)."""
    H = s.shape[0]
    m_run, l_run, acc = np.full(H, -1e30, f), np.zeros(H, f), np.zeros((H, V.shape[2]), f)
    for k0 in range(0, s.shape[1], TILE):
        sl, vl = s[:, k0:k0 + TILE], V[:, k0:k0 + TILE]
        okv = sl > -1e29
        m_new = np.maximum(m_run, np.where(okv, sl, f(-1e30)).max(1))
        p = np.where(okv, np.exp(sl - m_new[:, None]), f(0)).astype(f)
        scale = np.exp(m_run - m_new).astype(f)
        l_run = l_run * scale + p.sum(1, dtype=f)
        acc = acc * scale[:, None] + np.einsum("hn,hnd->hd", round_bf16(p), np.where(okv[..., None], vl, f(0))).astype(f)
        m_run = m_new
    return np.where(l_run > 0, m_run, f(-1e30)), l_run, acc


def emulate(c, mutate: str = ""):
    """The kernel's partition in float32 (module docstring) -> (batch, heads * hd) bf16-exact rows.  mutate: one of MUTATIONS."""
    sp, f = c.spec, np.float32
    assert mutate in ("",) + MUTATIONS
    n, L = c.n, sp.seq_len
    out = np.zeros((sp.batch, sp.heads, sp.hd), f)
    for b in range(sp.batch):
        smp = b // sp.beams
        q = R._q(c, (b + 1) % sp.batch if mutate == "neighbour_query" else b)
        ps = (smp + 1) % c.srows if mutate == "other_sample_plane" else smp
        ms = (smp + 1) % c.srows if mutate == "other_sample_mask" else smp
        recs = []
        # ---- the prompt ranges of the sample
        for r0 in range(0, L, PROMPT_KEYS):
            lo, hi = r0, min(L, r0 + PROMPT_KEYS)
            if mutate == "double_boundary" and hi < L:
                hi += 1  # the first key of the next range is counted here too
            if mutate == "drop_boundary" and r0 > 0:
                lo += 1  # the first key of the range is lost
            K, V = c.kc[ps][:, lo:hi], c.vc[ps][:, lo:hi]
            vis = np.ones(hi - lo, bool) if c.mask is None else c.mask[ms, lo:hi] != 0
            with np.errstate(invalid="ignore"):
                s = np.einsum("hd,hnd->hn", q, np.where(vis[None, :, None], K, f(0))).astype(f)
            recs.append(_record(np.where(vis[None, :], s, f(-1e30)), V))
        # ---- the generated ranges of the row
        start = 0 if mutate == "gen_from_0" else L
        Kall, Vall, visall, _ = R.effective(c, b)
        for g0 in range(0, sp.cap_g, GEN_KEYS):
            lo, hi = start + g0, min(n, start + g0 + GEN_KEYS)
            if hi <= lo:
                recs.append((np.full(sp.heads, -1e30, f), np.zeros(sp.heads, f), np.zeros((sp.heads, sp.hd), f)))
                continue
            K, V, vis = Kall[:, lo:hi].copy(), Vall[:, lo:hi].copy(), visall[lo:hi]
            for j in range(max(lo, L), hi):
                g = j - L
                if mutate == "ignore_ancestors" and j != n - 1:
                    K[:, j - lo], V[:, j - lo] = c.kg[b][:, g], c.vg[b][:, g]
                if mutate == "stale_newest" and j == n - 1:
                    K[:, j - lo], V[:, j - lo] = c.kg_before[b][:, g], c.vg_before[b][:, g]
            with np.errstate(invalid="ignore"):
                s = np.einsum("hd,hnd->hn", q, np.where(vis[None, :, None], K, f(0))).astype(f)
            recs.append(_record(np.where(vis[None, :], s, f(-1e30)), V))
        # ---- one merge (attn_decode_merge_kernel)
        mx = np.max([m for m, _, _ in recs], axis=0)
        l, o = np.zeros(sp.heads, f), np.zeros((sp.heads, sp.hd), f)
        for m, ls, acc in recs:
            with np.errstate(invalid="ignore", over="ignore"):
                w = np.where(ls > 0, np.exp(m - mx), f(0)).astype(f)
                o = o + w[:, None] * np.where(np.isfinite(acc), acc, f(0))
            l = l + w * ls
        out[b] = round_bf16(np.where(l[:, None] > 0, o / np.where(l > 0, l, f(1))[:, None], f(0)).astype(f))
    return out.reshape(sp.batch, c.d)


def build_for_emulation(sp: Spec):
    """build() plus what the cache slot of the newest key held BEFORE the step (kg_before / vg_before): the "stale_newest" mistake reads it."""
    c = build(sp)
    c.kg_before, c.vg_before = c.kg, c.vg
    if not c.writes:  # (the slot was given the step's key: a stale read is what the base plane held there)
        c.kg_before = R.base_plane("kg", sp.batch, sp.heads, sp.cap_g, sp.hd, sp.seed)
        c.vg_before = R.base_plane("vg", sp.batch, sp.heads, sp.cap_g, sp.hd, sp.seed)
    return c


__all__ = [n for n in dir() if not n.startswith("__")]
_ = replace  # (Spec variants in the tests)
