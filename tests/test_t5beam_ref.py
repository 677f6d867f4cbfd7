"""CPU side of the flan-t5 beam-search library (include/eilev_t5beam.h, libeilev_hip_t5beam.so): its surface (header = abi = dynamic
symbols), the refusals that return before any HIP call, and the case list of the shared-sample cross-attention test held to the fp32
restatement of the kernels (tests/attn_decode_ref.py) — the GPU side is tests/test_hip_t5_beam.py."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import attn_decode_ref as R
import t5beam_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code: str):
    """Run `code` in a child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)])


def test_library_exports_exactly_the_header():
    """The entry points of include/eilev_t5beam.h = abi.T5BEAM_EXPORTS = the library's dynamic symbols (the core library's code it carries
    stays local); the header's version = abi.T5BEAM_ABI_VERSION = what the library reports."""
    from eilev_amd import abi

    hdr = open(os.path.join(ROOT, "include", "eilev_t5beam.h")).read()
    code_part = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(eilev_t5beam_\w+)\s*\(", code_part))) == sorted(abi.T5BEAM_EXPORTS)
    assert int(re.search(r"#define EILEV_T5BEAM_ABI_VERSION (\d+)", hdr).group(1)) == abi.T5BEAM_ABI_VERSION
    assert abi.t5beam_supported(abi.T5Dims(d_kv=64)) and not abi.t5beam_supported(abi.T5Dims(d_kv=8)) and not abi.t5beam_supported(None)
    if not os.path.exists(abi.T5BEAM_LIB_PATH):
        pytest.skip("libeilev_hip_t5beam.so has not been built")
    _child("import ctypes\nfrom eilev_amd import abi\nh = ctypes.CDLL(abi.T5BEAM_LIB_PATH)\n"
           "assert all(hasattr(h, s) for s in abi.T5BEAM_EXPORTS)\nassert h.eilev_t5beam_abi_version() == abi.T5BEAM_ABI_VERSION\n"
           "assert not hasattr(h, 'eilev_t5_decode') and not hasattr(h, 'eilev_abi_version')\n")
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.T5BEAM_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.T5BEAM_EXPORTS), syms


_REFUSALS = r"""
import ctypes as C
from eilev_amd import abi
tb = abi.load_t5beam()
BAD, UNSUP = -1, -2
d = abi.T5Dims(d_model=64, d_kv=64, heads=2, d_ff=128, enc_layers=1, dec_layers=1, vocab=128, rel_buckets=32, rel_max_dist=128, eps=1e-6)
w = abi.T5Weights()
buf = C.create_string_buffer(4096)  # a non-null address that a refused call never follows
p = C.cast(buf, C.c_void_p).value
p = (p + 63) & ~63
def step(**kw):
    a = dict(d=C.byref(d), w=C.byref(w), tokens=p, state=p, enc_mask=p, rows=10, beams=5, start=p, gen=p, gen_cap=8, anc=p, ckv=p, enc_len=16,
             logits=p, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return tb.eilev_t5beam_decode_step(a["d"], a["w"], a["tokens"], a["state"], a["enc_mask"], a["rows"], a["beams"], a["start"], a["gen"], a["gen_cap"],
                                       a["anc"], a["ckv"], a["enc_len"], a["logits"], a["ws"], a["ws_bytes"], a["stream"])
for name in ("d", "w", "tokens", "state", "enc_mask", "start", "gen", "anc", "ckv", "logits", "ws"):
    assert step(**{name: None}) == BAD, name
assert step(rows=10, beams=3) == BAD and step(rows=33, beams=3) == BAD and step(rows=40, beams=5) == BAD and step(rows=0) == BAD
assert step(beams=0) == BAD and step(gen_cap=0) == BAD and step(enc_len=0) == BAD
d8 = abi.T5Dims(d_model=64, d_kv=8, heads=8, d_ff=128, enc_layers=1, dec_layers=1, vocab=128, rel_buckets=32, rel_max_dist=128, eps=1e-6)
assert step(d=C.byref(d8)) == UNSUP
assert step(ws_bytes=16) == -3
assert tb.eilev_t5beam_workspace_bytes(C.byref(d), 10, 5, 16, 8) > 0 and tb.eilev_t5beam_workspace_bytes(C.byref(d), 10, 3, 16, 8) == 0
def cross(**kw):
    a = dict(q=p, ldq=512, kc=p, vc=p, mask=p, rows=10, beams=5, heads=8, hd=64, enc_len=16, cap=16, out=p, part=p, part_bytes=1 << 40, stream=None)
    a.update(kw)
    return tb.eilev_t5beam_cross_attention(a["q"], a["ldq"], a["kc"], a["vc"], a["mask"], a["rows"], a["beams"], a["heads"], a["hd"], a["enc_len"],
                                           a["cap"], a["out"], a["part"], a["part_bytes"], a["stream"])
for name in ("q", "kc", "vc", "out", "part"):
    assert cross(**{name: None}) == BAD, name
assert cross(rows=10, beams=3) == BAD and cross(rows=33, beams=3) == BAD and cross(rows=40, beams=5) == BAD and cross(rows=0) == BAD
assert cross(cap=15) == BAD and cross(enc_len=0) == BAD and cross(ldq=511) == BAD and cross(kc=p + 2) == BAD
for hd in (8, 32, 80, 128):
    assert cross(hd=hd, ldq=8 * hd) == UNSUP, hd
assert cross(part_bytes=4 * 10 * 8 * 66 - 1) == -3
"""


def test_refusals_return_before_any_hip_call():
    """Null pointers, rows % beams != 0, rows > 32, a head size other than 64, a workspace too small: refused on a machine without a GPU,
    with pointers that no kernel could follow."""
    from eilev_amd import abi

    if not os.path.exists(abi.T5BEAM_LIB_PATH):
        pytest.skip("libeilev_hip_t5beam.so has not been built")
    _child(_REFUSALS)


# ---- the case list of the cross-attention GPU test ----------------------------------------------------------------------------------------
def _own_visible_spike(c):
    """(rows, heads) bool: the spike slot of (row, head) is visible to the row and no other row of its (sample, head) has its spike there."""
    sp = c.spec
    ok = np.zeros((sp.batch, sp.heads), bool)
    for b in range(sp.batch):
        _, _, vis, _ = R.effective(c, b)
        s0 = (b // sp.beams) * sp.beams
        for h in range(sp.heads):
            j = c.spike_pos[b, h]
            mates = [c.spike_pos[o, h] for o in range(s0, s0 + sp.beams) if o != b]
            ok[b, h] = j >= 0 and vis[j] and j not in mates
    return ok


_FIGURES = dict(restate=0.0, drop=np.inf, double=np.inf, shift=np.inf)


@pytest.mark.parametrize("group", list(cases.GROUPS))
def test_case_list_against_the_fp32_restatement(group):
    """Every case: the kernels' arithmetic restated in fp32 over ranges of 128 keys (the kernel's) and of 256 stays within 1.0 tol of the
    float64 reference, so the GPU test's bound is reachable; and where there are at least 8 keys a dropped, a doubled and a mis-paired
    spike key each move every (row, head) that owns a visible spike slot by more than 10 tol, so the GPU test can see them."""
    for sp in cases.GROUPS[group]():
        c = R.build_case(sp)
        ref, A = R.reference(c)
        for keys in (128, 256):
            ratio = R.worst_ratio(R.emulate_ranges(c, keys), ref, A)
            _FIGURES["restate"] = max(_FIGURES["restate"], ratio)
            assert ratio <= 1.0, (sp.name, keys, ratio)
        if sp.seq_len < 8:
            continue
        own = _own_visible_spike(c)
        assert own.any(), sp.name
        tol = R.tolerance(A).reshape(sp.batch, sp.heads, sp.hd)
        for mut in ("drop", "double", "shift"):
            err = (np.abs(R.emulate_ranges(c, 128, mut).astype(np.float64) - ref).reshape(sp.batch, sp.heads, sp.hd) / tol).max(-1)
            worst = float(err[own].min())
            _FIGURES[mut] = min(_FIGURES[mut], worst)
            assert worst > 10.0, (sp.name, mut, worst)
    print(f"[t5beam cases] {group}: restatement <= {_FIGURES['restate']:.3f} tol; mutations >= "
          f"{_FIGURES['drop']:.1f} / {_FIGURES['double']:.1f} / {_FIGURES['shift']:.1f} tol (drop / double / shift), so far")


def test_case_list_covers_what_it_says():
    """(a): over its 12 launches every one of the 960 slots is the spike of some (row, head); (d): the spikes lie behind the padding and one
    sample has no visible key; (e): the second case has more rows than one call takes."""
    seen = np.zeros(960, bool)
    for sp in cases.cover_specs():
        seen[R.build_case(sp).spike_pos.ravel()] = True
    assert seen.all()
    for sp in cases.beams_specs():
        c = R.build_case(sp)
        if sp.mask != "none":
            assert not c.mask[-1].any() and (c.spike_pos[: sp.beams] >= 300).all(), sp.name
            assert (c.spike_pos[-sp.beams:] == -1).all(), sp.name
    assert [sp.batch for sp in cases.mixed_specs()] == [24, 40]
    assert len(cases.all_specs()) == 12 + 8 + 12 + 8 + 2
