"""The launches of the shared-sample cross-attention test (eilev_t5beam_cross_attention; test_t5beam_ref.py holds the list to the fp32
restatement on the CPU, test_hip_t5_beam.py runs it on the GPU).  A plain module: no fixtures, no GPU.

A case is attn_decode_ref.Spec in the beam form with nothing generated: `beams` rows per sample over that sample's seq_len = enc_len keys
(cap_g = 1 and state == nullptr keep the generation cache out of it), head size 64, q rows only (fuse_new = 0).  spikes=("cover", k) gives
every (row, head) its own key slot k * rows * heads + row * heads + head: the rows of a sample share K, so with the "mix" placement the
spikes of different rows would overwrite each other."""
from __future__ import annotations

from attn_decode_ref import Spec

HEADS = 8


def _spec(name, beams, samples, enc_len, cap=None, heads=HEADS, k=0, **kw):
    return Spec(name=name, form="cross", beams=beams, batch=beams * samples, hd=64, heads=heads, seq_len=enc_len, cap=enc_len if cap is None else cap,
                cap_g=1, n_gen=None, fuse_new=0, spikes=("cover", k), stale="rand", **kw)


def cover_specs():
    """(a) 5 x 2 rows over 960 keys, launches k = 0 .. 11: every slot is some (row, head)'s spike (12 * 10 * 8 = 960)."""
    return [_spec(f"cover-{k}", 5, 2, 960, k=k) for k in range(12)]


def tiny_specs():
    """(b) fewer keys than key groups, than rows, than one wave; a few stale slots behind them."""
    return [_spec(f"tiny-{n}-{b}x{s}-h{h}", b, s, n, cap=n + 3, heads=h)
            for n, b, s, h in ((1, 1, 1, 1), (2, 2, 1, 1), (3, 3, 1, 1), (8, 2, 2, 2), (16, 2, 2, 4), (63, 2, 2, 8), (64, 2, 2, 8), (65, 2, 2, 8))]


def sweep_specs():
    """(c) enc_len around the 128-key range boundaries."""
    return [_spec(f"sweep-{n}", 2, 2, n, cap=n if n % 128 == 0 else n + 5, mask="ones" if n % 2 else "none")
            for n in (127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025, 2048)]


def beams_specs():
    """(d) every row-group shape: fewer than 8 rows, exactly 8, 8 + 1, two and four full groups; a left-padded sample, one with holes and one
    with no visible key at all; the spikes behind the 300 padded keys; q rows with a stride beyond their width."""
    out = []
    for b, s in ((1, 3), (2, 3), (3, 3), (5, 3), (8, 3), (9, 3), (16, 2), (32, 1)):
        k = -(-300 // (b * s * HEADS))
        out.append(_spec(f"beams-{b}x{s}", b, s, 960, k=k, ldq_extra=64, mask="none" if (b, s) == (32, 1) else "pad300+dead"))
    return out


def mixed_specs():
    """(e) one sample per mask kind (attn_decode_ref.MASK_KINDS).  The second case has 40 rows: more than one call takes, the GPU test
    launches it in sample groups of 32 // beams, as the engine does."""
    return [_spec("mixed-3x8", 3, 8, 530, mask="mixed"), _spec("mixed-5x8", 5, 8, 530, cap=640, k=1, mask="mixed", mask_first=5)]


GROUPS = dict(cover=cover_specs, tiny=tiny_specs, sweep=sweep_specs, beams=beams_specs, mixed=mixed_specs)


def all_specs():
    return [sp for make in GROUPS.values() for sp in make()]
