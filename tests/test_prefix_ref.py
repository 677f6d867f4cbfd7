"""CPU side of the shared-prefix library (include/eilev_prefix.h, libeilev_hip_prefix.so): its surface (header = abi = dynamic symbols), the
refusals that return before any HIP call, and the case list of the attention kernel's GPU test (tests/prefix_cases.py) held to the float64
reference: the preconditions of the derived tolerance, the kernel's fp32 restatement within 1.0 tol, every mutation beyond it — the GPU side
is tests/test_hip_prefix.py."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import prefix_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code: str):
    """Run `code` in a child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)])


def test_library_exports_exactly_the_header():
    """The entry points of include/eilev_prefix.h = abi.PREFIX_EXPORTS = the library's dynamic symbols (the core library's code it carries
    stays local); the header's version and limits = abi's = what the library reports."""
    from eilev_amd import abi

    hdr = open(os.path.join(ROOT, "include", "eilev_prefix.h")).read()
    code_part = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(eilev_prefix_\w+)\s*\(", code_part))) == sorted(abi.PREFIX_EXPORTS)
    for name in ("ABI_VERSION", "MAX_ROWS", "MAX_NEW", "MAX_STACKED"):
        assert int(re.search(r"#define EILEV_PREFIX_%s (\d+)" % name, hdr).group(1)) == getattr(abi, "PREFIX_" + name)
    assert abi.prefix_supported(abi.Dims(t_hidden=160, t_heads=2)) and abi.prefix_supported(abi.Dims(t_hidden=256, t_heads=2))
    assert not abi.prefix_supported(abi.Dims(t_hidden=128, t_heads=2)) and not abi.prefix_supported(None)
    assert os.path.exists(abi.PREFIX_LIB_PATH), "libeilev_hip_prefix.so has not been built"
    _child("import ctypes\nfrom eilev_amd import abi\nh = ctypes.CDLL(abi.PREFIX_LIB_PATH)\n"
           "assert all(hasattr(h, s) for s in abi.PREFIX_EXPORTS)\nassert h.eilev_prefix_abi_version() == abi.PREFIX_ABI_VERSION\n"
           "assert not hasattr(h, 'eilev_opt_prefill') and not hasattr(h, 'eilev_abi_version')\n")
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.PREFIX_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.PREFIX_EXPORTS), syms


_REFUSALS = r"""
import ctypes as C
from eilev_amd import abi
px = abi.load_prefix()
BAD, UNSUP, WS = -1, -2, -3
buf = C.create_string_buffer(4096)  # a non-null address that a refused call never follows
p = (C.cast(buf, C.c_void_p).value + 63) & ~63
def attn(**kw):
    a = dict(q=p, ldq=480, k=p, ldk=480, v=p, ldv=480, kp=p, vp=p, P=16, cap=16, rows=3, n=4, heads=2, hd=80, scale=1.0, out=p, stream=None)
    a.update(kw)
    return px.eilev_prefix_attention(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["kp"], a["vp"], a["P"], a["cap"], a["rows"], a["n"],
                                     a["heads"], a["hd"], a["scale"], a["out"], a["stream"])
for name in ("q", "k", "v", "kp", "vp", "out"):
    assert attn(**{name: None}) == BAD, name
    assert attn(**{name: p + 2}) == BAD, name
assert attn(rows=0) == BAD and attn(n=0) == BAD and attn(rows=abi.PREFIX_MAX_ROWS + 1) == BAD and attn(n=abi.PREFIX_MAX_NEW + 1) == BAD
assert attn(rows=abi.PREFIX_MAX_ROWS, n=abi.PREFIX_MAX_STACKED // abi.PREFIX_MAX_ROWS + 1) == BAD
assert attn(P=0) == BAD and attn(cap=15) == BAD and attn(heads=0) == BAD and attn(scale=0.0) == BAD
assert attn(ldq=159) == BAD and attn(ldk=484) == BAD and attn(ldv=152) == BAD
for hd in (8, 64, 72, 88, 96):
    assert attn(hd=hd, ldq=6 * hd, ldk=6 * hd, ldv=6 * hd) == UNSUP, hd
d = abi.Dims(t_hidden=160, t_heads=2, t_ffn=320, t_layers=1, vocab=128, max_pos=64, t_eps=1e-5)
w = abi.OptWeights()
def extend(**kw):
    a = dict(d=C.byref(d), w=C.byref(w), x=p, rows=3, n=4, kvp=p, P=16, kvr=p, cap=8, last=p, alll=p, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return px.eilev_prefix_extend(a["d"], a["w"], a["x"], a["rows"], a["n"], a["kvp"], a["P"], a["kvr"], a["cap"], a["last"], a["alll"], a["ws"],
                                  a["ws_bytes"], a["stream"])
for name in ("d", "w", "x", "kvp", "ws"):
    assert extend(**{name: None}) == BAD, name
assert extend(last=None, alll=None) == BAD
assert extend(rows=0) == BAD and extend(n=0) == BAD and extend(P=0) == BAD and extend(P=61) == BAD and extend(cap=3) == BAD
assert extend(rows=abi.PREFIX_MAX_ROWS + 1) == BAD
d64 = abi.Dims(t_hidden=128, t_heads=2, t_ffn=320, t_layers=1, vocab=128, max_pos=64, t_eps=1e-5)
assert extend(d=C.byref(d64)) == UNSUP
assert extend(ws_bytes=16) == WS
nb = px.eilev_prefix_workspace_bytes
assert nb(C.byref(d), 3, 4) > 0 and nb(C.byref(d), 0, 4) == 0 and nb(None, 3, 4) == 0
# the workspace follows rows * new_len alone
assert nb(C.byref(d), 6, 4) == nb(C.byref(d), 3, 8) and nb(C.byref(d), 6, 4) > nb(C.byref(d), 3, 4)
"""


def test_refusals_return_before_any_hip_call():
    """Null and misaligned pointers, shapes beyond the limits of the header, a head size other than 80 / 128, a workspace too small: refused
    on a machine without a GPU, with pointers that no kernel could follow."""
    _child(_REFUSALS)


# ---- the case list of the attention GPU test ----------------------------------------------------------------------------------------------
_BUILT = {}


def _case(sp):
    if sp.name not in _BUILT:
        c = cases.build_case(sp)
        _BUILT[sp.name] = (c, *cases.reference(c))
    return _BUILT[sp.name]


@pytest.mark.parametrize("sp", cases.CASES, ids=lambda sp: sp.name)
def test_preconditions_of_the_tolerance(sp):
    """Where the (2^-8 + 2^-11) A_i bound was derived (attn_prefill_ref.py): every query with two or more visible keys owns a spike of weight
    in [W_LO, W_HI] (one with a single key: weight 1), ordinary |v| in [4, 8], the explicit fp32 terms <= 2^-11 A_i."""
    c, ref, A = _case(sp)
    many, single = cases.spike_weights(c)
    assert len(many) == 0 or (many.min() >= cases.W_LO and many.max() <= cases.W_HI), (sp.name, many.min(), many.max())
    assert len(single) == 0 or np.allclose(single, 1.0)
    absv = cases.ordinary_abs_v(c)
    assert absv.min() >= 4.0 and absv.max() <= 8.0
    term = cases.fp32_term(c, A)
    print(f"[prefix cases] {sp.name}: spike weights {many.min() if len(many) else 1:.3f} .. {many.max() if len(many) else 1:.3f}, fp32 term 2^{np.log2(term):.2f}")
    assert term <= 2.0 ** -11, (sp.name, term)
    assert (A > 0).all() and np.isfinite(ref).all()


@pytest.mark.parametrize("sp", cases.CASES, ids=lambda sp: sp.name)
def test_restatement_and_mutations(sp):
    """The kernel's arithmetic restated in fp32 stays within 1.0 tol of the float64 reference, so the GPU test's bound is reachable; every
    mutation that applies to the case moves some element by more than 1.0 tol, so the GPU test can see it."""
    c, ref, A = _case(sp)
    ratio = cases.worst_ratio(cases.emulate(c), ref, A)
    figures = [f"restatement {ratio:.3f}"]
    assert ratio <= 1.0, (sp.name, ratio)
    for mut in cases.MUTATIONS:
        if not cases.applies(mut, sp):
            continue
        worst = cases.worst_ratio(cases.mutated(c, mut), ref, A)
        figures.append(f"{mut} {worst:.1f}")
        assert worst > 1.0, (sp.name, mut, worst)
    print(f"[prefix cases] {sp.name}: " + ", ".join(figures) + " tol")


def test_case_list_covers_what_it_says():
    """Head sizes, prefix lengths around the 32 / 128 boundaries, a capacity beyond P with traps and NaN bits, and every tile situation."""
    L = cases.CASES
    assert {sp.hd for sp in L} == {80, 128} and {sp.heads for sp in L} == {2, 3}
    assert {sp.P for sp in L} == {1, 31, 32, 33, 127, 128, 129, 300}
    assert {sp.n for sp in L} == {1, 2, 5, 33, 70, 200} and {sp.R for sp in L} == {1, 2, 3, 32, 45}
    assert any(sp.cap >= sp.P + 2 for sp in L) and any(sp.cap == sp.P for sp in L) and any(not sp.scale1 for sp in L)
    T = cases.TILE
    assert any(sp.n == 5 and sp.R == 45 for sp in L)                                # a tile spans >= 3 rows
    assert any(T % sp.n and sp.n < T and sp.R * sp.n > T for sp in L)              # a tile boundary inside a row
    assert any(sp.n == 200 and sp.R == 2 for sp in L)                               # a row spans >= 2 tiles
    assert any((sp.R * sp.n) % T for sp in L) and any((sp.R * sp.n) % T == 0 for sp in L)
    for mut in cases.MUTATIONS:
        assert sum(cases.applies(mut, sp) for sp in L) >= 2, mut
    c = cases.build_case(cases.by_name("p128-n200-r2"))
    pk = cases.pack(c)
    assert pk.qkv.shape == (401, 3 * 2 * 80) and c.nan_slot == 129
    assert (pk.kp[:, 129].view(np.uint16) == cases.NAN_BITS).all() and (pk.qkv[400].view(np.uint16) == cases.NAN_BITS).all()
