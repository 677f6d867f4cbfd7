"""CPU side of the shared-prompt decode step (include/eilev_prefix.h eilev_prefix_decode_*): the case list of the attention's GPU test
(tests/shared_prompt_cases.py) held to attn_decode_ref's float64 reference — the preconditions of its derived tolerance, the fp32
restatement of the kernel's partition within 1.0 tol, every planted mistake beyond it — the refusals of the three C entries that return
before any HIP call, and generate(shared_prompt_reads=True)'s refusals, by name, before any encode.  The GPU side is
tests/test_hip_shared_prompt.py."""
from __future__ import annotations

import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_decode_ref as R
import shared_prompt_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = cases.all_specs()
_BUILT = {}


def _case(sp):
    if sp.name not in _BUILT:
        c = cases.build_for_emulation(sp)
        _BUILT[sp.name] = (c, *R.reference(c))
    return _BUILT[sp.name]


def test_the_case_list_reaches_every_dimension_it_names():
    names = [sp.name for sp in SPECS]
    assert len(set(names)) == len(names)
    assert {(sp.batch // sp.beams, sp.beams) for sp in SPECS} == set(cases.SAMPLES_BEAMS)
    assert {sp.seq_len for sp in SPECS} >= set(cases.SEQ_LENS) and all(sp.cap > sp.seq_len for sp in SPECS)
    assert {(sp.cap_g, sp.n_gen) for sp in SPECS} >= set(cases.CAPG_NGEN)
    assert {sp.hd for sp in SPECS} == {80, 128} and {sp.heads for sp in SPECS} == {2, 3}
    assert {sp.mask for sp in SPECS} == {"none", "ones", "mixed"} and {sp.stale for sp in SPECS} == {"trap", "nan"}
    assert "beam" in {sp.spikes for sp in SPECS} and any(isinstance(sp.spikes, tuple) for sp in SPECS)
    for hd in (80, 128):  # both head sizes meet the full generation cache, the count beyond it and two generated ranges
        assert {(130, 130), (130, 133)} <= {(sp.cap_g, sp.n_gen) for sp in SPECS if sp.hd == hd}
    # a sample whose every prompt key is masked, next to samples that see theirs
    dead = [sp for sp in SPECS if sp.mask == "mixed" and (_case(sp)[0].mask == 0).all(1).any()]
    assert any(sp.batch // sp.beams > 1 for sp in dead) and any(sp.batch // sp.beams == 1 for sp in dead)
    # the cover cases: every slot of the prompt ranges, and of the prompt + generated keys, is some (row, head)'s spike
    for prefix, top in (("cover-prompt-", 384), ("cover-gen-", 195)):
        got = set()
        for sp in SPECS:
            if sp.name.startswith(prefix):
                got |= set(_case(sp)[0].spike_pos.ravel().tolist())
        assert got >= set(range(top)), prefix
    c = _case(next(sp for sp in SPECS if sp.name == "bad-ancestors"))[0]
    live = c.anc_raw[:c.n - c.spec.seq_len]
    assert (live < 0).any() and (live >= c.spec.batch).any() and np.array_equal(np.clip(live, 0, c.spec.batch - 1), c.anc[:c.n - c.spec.seq_len])


@pytest.mark.parametrize("sp", SPECS, ids=lambda sp: sp.name)
def test_preconditions_of_the_tolerance(sp):
    """Where attn_decode_ref's (2^-8 + 2^-11) A_i was derived: visible scores below 50 in magnitude over at most 2304 keys of at most 128
    elements (the fp32 terms), a spike of weight 0.5 with values +-8 that opposes the rest of its row, A_i >= |out_i|, finite inputs wherever
    a row looks; the stale prompt slots and the masked keys hold what must not be seen."""
    c, ref, A = _case(sp)
    assert sp.beams > 0 and sp.batch <= 32 and sp.hd <= 128 and c.n <= 2304 and sp.fuse_new == 1
    for b in range(sp.batch):
        K, V, vis, _ = R.effective(c, b)
        assert np.isfinite(K[:, vis]).all() and np.isfinite(V[:, vis]).all()
        s = R.scores64(c, b, K, None)
        assert vis.any() and np.abs(s[:, vis]).max() < 50.0
        p = np.exp(s[:, vis] - s[:, vis].max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        where = np.flatnonzero(vis).tolist()
        for h in range(sp.heads):
            j = int(c.spike_pos[b, h])
            assert j >= 0 and vis[j] and np.abs(V[h, j]).max() == 8.0
            if vis.sum() > 1:
                assert abs(p[h, where.index(j)] - 0.5) < 0.02, (sp.name, b, h, p[h, where.index(j)])
                # element by element the spike opposes the weighted mean of the row's other visible values: |out_i| < 4 <= A_i
                others = [i for i, k in enumerate(where) if k != j]
                rest = p[h, others] @ V[h][vis][others].astype(np.float64)
                assert (np.sign(V[h, j]) == -np.sign(rest))[np.abs(rest) > 1e-6].all(), (sp.name, b, h)
    assert (A >= np.abs(ref) - 1e-12).all() and np.isfinite(ref).all()
    stale_k, stale_v = c.kc[:, :, sp.seq_len:], c.vc[:, :, sp.seq_len:]
    assert stale_k.size and (np.isnan(stale_k).all() if sp.stale == "nan" else (np.abs(stale_k) == 64.0).all()) and stale_k.shape == stale_v.shape


@pytest.mark.parametrize("sp", SPECS, ids=lambda sp: sp.name)
def test_restatement_is_within_tol(sp):
    c, ref, A = _case(sp)
    r = R.worst_ratio(cases.emulate(c), ref, A)
    print(f"[shared prompt cases] {sp.name}: fp32 restatement worst err/tol {r:.3f}")
    assert r <= 1.0, (sp.name, r)


@pytest.mark.parametrize("mutate", cases.MUTATIONS)
def test_a_planted_mistake_exceeds_tol_on_some_case(mutate):
    """Another sample's prompt plane or mask row, a neighbouring row's query, a key dropped or doubled at a range boundary, the ancestor table
    ignored, the newest key read from its stale cache slot, a generated range started at 0 instead of seq_len."""
    worst = (0.0, "")
    for sp in SPECS:
        if sp.name.startswith("sweep-") and sp.seq_len < 300:
            continue  # (the extra cases and the longest sweep cases: enough for every mistake, and quick)
        c, ref, A = _case(sp)
        worst = max(worst, (R.worst_ratio(cases.emulate(c, mutate), ref, A), sp.name))
    print(f"[shared prompt cases] {mutate}: worst err/tol {worst[0]:.1f} at {worst[1]}")
    assert worst[0] > 1.0, (mutate, worst)


def _child(code: str):
    """Run `code` in a child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)])


_REFUSALS = r"""
import ctypes as C
from eilev_amd import abi
px = abi.load_prefix()
BAD, UNSUP, WS = -1, -2, -3
buf = C.create_string_buffer(4096)  # a non-null address that a refused call never follows
p = (C.cast(buf, C.c_void_p).value + 63) & ~63
def attn(**kw):
    a = dict(qkv=p, ldq=480, kp=p, vp=p, L=16, cap=20, mask=p, state=p, kg=p, vg=p, cap_g=4, anc=p, rows=6, beams=3, heads=2, hd=80, out=p, part=p,
             part_bytes=None, stream=None)
    a.update(kw)
    if a["part_bytes"] is None:
        a["part_bytes"] = abi.prefix_decode_part_bytes(a["rows"], a["heads"], a["hd"], a["L"], a["cap_g"])
    return px.eilev_prefix_decode_attention(a["qkv"], a["ldq"], a["kp"], a["vp"], a["L"], a["cap"], a["mask"], a["state"], a["kg"], a["vg"], a["cap_g"],
                                            a["anc"], a["rows"], a["beams"], a["heads"], a["hd"], a["out"], a["part"], a["part_bytes"], a["stream"])
for name in ("qkv", "kp", "vp", "state", "kg", "vg", "anc", "out", "part"):
    assert attn(**{name: None}) == BAD, name
for name in ("qkv", "kp", "vp", "kg", "vg", "out", "part"):
    assert attn(**{name: p + 2}) == BAD, name
assert attn(rows=7) == BAD and attn(rows=0) == BAD and attn(beams=0) == BAD            # rows % beams
assert attn(rows=33, beams=3) == BAD and attn(rows=33, beams=33) == BAD and attn(rows=64, beams=32) == BAD  # rows > 32
assert attn(L=0) == BAD and attn(cap=15) == BAD and attn(cap_g=0) == BAD and attn(heads=0) == BAD
assert attn(ldq=479) == BAD and attn(ldq=484) == BAD
for hd in (8, 64, 72, 96):
    assert attn(hd=hd, ldq=6 * hd) == UNSUP, hd
full = abi.prefix_decode_part_bytes(6, 2, 80, 16, 4)
assert full == 4 * 6 * 2 * 2 * 82
assert attn(part_bytes=full - 1) == WS
assert attn(hd=128, ldq=768, part_bytes=abi.prefix_decode_part_bytes(6, 2, 128, 16, 4) - 1) == WS

d = abi.Dims(t_hidden=160, t_heads=2, t_ffn=320, t_layers=1, vocab=128, max_pos=64, t_eps=1e-5)
d64 = abi.Dims(t_hidden=128, t_heads=2, t_ffn=320, t_layers=1, vocab=128, max_pos=64, t_eps=1e-5)
w = abi.OptWeights()
nb = px.eilev_prefix_decode_workspace_bytes
core = abi.load_hip().eilev_opt_workspace_bytes(C.byref(d), 6, 1)
assert nb(C.byref(d), 6, 16, 4) >= core + full and nb(C.byref(d), 6, 16, 4) < core + full + 512
assert nb(C.byref(d), 6, 300, 4) > nb(C.byref(d), 6, 16, 4)   # the records follow the prompt length ...
assert nb(C.byref(d), 6, 16, 300) > nb(C.byref(d), 6, 16, 4)  # ... and the generation capacity
assert nb(None, 6, 16, 4) == 0 and nb(C.byref(d), 0, 16, 4) == 0 and nb(C.byref(d), 33, 16, 4) == 0 and nb(C.byref(d), 6, 0, 4) == 0
assert nb(C.byref(d), 6, 16, 0) == 0 and nb(C.byref(d64), 6, 16, 4) == 0
def step(**kw):
    a = dict(d=C.byref(d), w=C.byref(w), tok=p, state=p, mask=p, nv=p, rows=6, beams=3, L=16, kvp=p, kvg=p, cap_g=4, anc=p, logits=p, ws=p, ws_bytes=1 << 40,
             stream=None)
    a.update(kw)
    return px.eilev_prefix_decode_step(a["d"], a["w"], a["tok"], a["state"], a["mask"], a["nv"], a["rows"], a["beams"], a["L"], a["kvp"], a["kvg"],
                                       a["cap_g"], a["anc"], a["logits"], a["ws"], a["ws_bytes"], a["stream"])
for name in ("d", "w", "tok", "state", "mask", "nv", "kvp", "kvg", "anc", "logits", "ws"):
    assert step(**{name: None}) == BAD, name
for name in ("kvp", "kvg", "ws"):
    assert step(**{name: p + 2}) == BAD, name
assert step(rows=7) == BAD and step(rows=0) == BAD and step(beams=0) == BAD and step(rows=33, beams=3) == BAD and step(L=0) == BAD and step(cap_g=0) == BAD
assert step(d=C.byref(d64)) == UNSUP
assert step(ws_bytes=nb(C.byref(d), 6, 16, 4) - 1) == WS
"""


def test_c_refusals_return_before_any_hip_call():
    """eilev_prefix_decode_attention, _decode_workspace_bytes and _decode_step: nulls, rows % beams, rows > 32, misaligned planes, head size
    64 -> EILEV_E_UNSUPPORTED, part_bytes / workspace one byte short — refused on a machine without a GPU, with pointers no kernel could follow."""
    _child(_REFUSALS)


def test_the_core_step_is_internal_and_the_core_abi_keeps_its_exports():
    from eilev_amd import abi

    assert abi.PREFIX_ABI_VERSION == 2 and {"eilev_prefix_decode_attention", "eilev_prefix_decode_step", "eilev_prefix_decode_workspace_bytes"} <= set(abi.PREFIX_EXPORTS)
    _child("import ctypes\nfrom eilev_amd import abi\nh = ctypes.CDLL(abi.HIP_LIB_PATH)\n"
           "assert hasattr(h, 'eilev_opt_decode_step_beam') and not hasattr(h, 'opt_decode_step_beam') and not hasattr(h, 'eilev_prefix_decode_step')\n"
           "assert len(abi.EXPORTS) == 68, len(abi.EXPORTS)\n")


# ---- generate(shared_prompt_reads=True): refused by name before any encode -----------------------------------------------------------------
def _model(name):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    return VideoBlipForConditionalGeneration(blip2_config(name))


def _context(P=10):
    from eilev_amd.model.v2 import VideoContext

    return VideoContext(SimpleNamespace(P=P), torch.ones(1, P, dtype=torch.long), key=None)


def test_generate_refuses_by_name_before_any_encode():
    from eilev_amd.configs import CONFIGS

    one = torch.ones(1, 4, dtype=torch.long)
    mid = _model("mid")  # head size 80
    mid._encode = None   # (an encode would fail loudly: every refusal below comes before it)
    for kw in (dict(), dict(do_sample=True), dict(repetition_penalty=1.3), dict(num_beams=1, eos_token_id=[2, 5])):
        with pytest.raises(NotImplementedError, match="no rows share a prompt") as e:
            mid.generate(one, max_new_tokens=4, shared_prompt_reads=True, **kw)
        assert "shared_prompt_reads" in str(e.value)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens") as e:
        mid.generate(one, max_new_tokens=4, shared_prompt_reads=True, prompt_lookup_num_tokens=3)
    assert "shared_prompt_reads" in str(e.value)
    tiny = _model("tiny")  # head size 8
    tiny._encode = None
    for kw in (dict(num_beams=3), dict(context=_context())):
        with pytest.raises(NotImplementedError, match="head size 8") as e:
            tiny.generate(one, max_new_tokens=4, shared_prompt_reads=True, **kw)
        assert "shared_prompt_reads" in str(e.value)
    t5 = _model(next(n for n, c in CONFIGS.items() if c["text_config"].get("model_type") == "t5"))
    t5._encode = None
    with pytest.raises(NotImplementedError, match="flan-t5") as e:
        t5.generate(one, max_new_tokens=4, shared_prompt_reads=True, num_beams=3)
    assert "shared_prompt_reads" in str(e.value)
    # what generate(context=...) and kv_cache_dtype="fp8" refuse, they still refuse with the keyword
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        mid.generate(one, max_new_tokens=4, shared_prompt_reads=True, context=_context(), num_beams=3)
    with pytest.raises(NotImplementedError, match="fp8"):
        mid.generate(one, max_new_tokens=4, shared_prompt_reads=True, num_beams=3, kv_cache_dtype="fp8")
    # without the keyword, or with it off, the parse is what it was
    a = mid._parse_generate(one, dict(max_new_tokens=4, num_beams=3))
    b = mid._parse_generate(one, dict(max_new_tokens=4, num_beams=3, shared_prompt_reads=False))
    assert not a.shared_reads and not b.shared_reads and mid._parse_generate(one, dict(max_new_tokens=4, num_beams=3, shared_prompt_reads=True)).shared_reads
    assert {k: v for k, v in vars(a).items() if k != "sampler"} == {k: v for k, v in vars(b).items() if k != "sampler"}


def test_engine_switch_is_off_by_default_and_adds_no_argument():
    import inspect

    from eilev_amd import beam, sampling
    from eilev_amd.engine import HipEngine

    src = inspect.getsource(HipEngine.__init__)
    assert "self.shared_prompt_reads = False" in src
    assert "shared" not in inspect.signature(HipEngine.greedy_decode_context).parameters and len(inspect.signature(HipEngine.greedy_decode_context).parameters) == 9
    for fn in (HipEngine._beam_device_loop, beam.beam_search, sampling.sample_loop):
        assert not any("shared" in p for p in inspect.signature(fn).parameters)
    # an engine made without __init__ (tools/route_table.py) reads the switch as off
    eng = object.__new__(HipEngine)
    assert getattr(eng, "shared_prompt_reads", False) is False and HipEngine._reads_record(False) == {} and HipEngine._reads_record(True) == dict(reads="shared")
