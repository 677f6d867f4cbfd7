"""CPU side of the fp8 KV-cache library (include/eilev_kv8.h, libeilev_hip_kv8.so): its surface (header = abi = dynamic symbols), the
refusals that return before any HIP call, the quantiser's torch restatement (tests/kv8_ref.py) against brute force, the planted mistakes the
attention reference must catch, and generate(kv_cache_dtype=...)'s argument checks — the GPU side is tests/test_hip_kv8.py."""
from __future__ import annotations

import functools
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kv8_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code: str):
    """Run `code` in a child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)])


# ---- 1. the surface ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    from eilev_amd import abi

    hdr = open(os.path.join(ROOT, "include", "eilev_kv8.h")).read()
    code_part = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(eilev_kv8_\w+)\s*\(", code_part))) == sorted(abi.KV8_EXPORTS)
    for name in ("ABI_VERSION", "RANGE", "MAX_ROWS"):
        assert int(re.search(r"#define EILEV_KV8_%s (\d+)" % name, hdr).group(1)) == getattr(abi, "KV8_" + name)
    assert abi.KV8_RANGE == ref.RANGE
    assert abi.kv8_supported(abi.Dims(t_hidden=160, t_heads=2)) and abi.kv8_supported(abi.Dims(t_hidden=256, t_heads=2))
    assert not abi.kv8_supported(abi.Dims(t_hidden=128, t_heads=2)) and not abi.kv8_supported(None)
    assert os.path.exists(abi.KV8_LIB_PATH), "libeilev_hip_kv8.so has not been built"
    _child("import ctypes\nfrom eilev_amd import abi\nh = ctypes.CDLL(abi.KV8_LIB_PATH)\n"
           "assert all(hasattr(h, s) for s in abi.KV8_EXPORTS)\nassert h.eilev_kv8_abi_version() == abi.KV8_ABI_VERSION\n"
           "assert not hasattr(h, 'eilev_opt_decode_step') and not hasattr(h, 'eilev_abi_version')\n")
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.KV8_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.KV8_EXPORTS), syms
    # the core library's header and export list are untouched: no kv8 name appears in them
    assert "kv8" not in open(os.path.join(ROOT, "include", "eilev.h")).read() and not any("kv8" in s for s in abi.EXPORTS)


_REFUSALS = r"""
import ctypes as C
from eilev_amd import abi
kv = abi.load_kv8()
BAD, UNSUP, WS = -1, -2, -3
buf = C.create_string_buffer(4096)  # a non-null address that a refused call never follows
p = (C.cast(buf, C.c_void_p).value + 63) & ~63
def attn(**kw):
    a = dict(qkv=p, ldq=480, k8=p, v8=p, ek=p, ev=p, mask=p, state=p, batch=3, seq=16, cap=20, heads=2, hd=80, fuse=1, part=p, pb=1 << 30, out=p, stream=None)
    a.update(kw)
    return kv.eilev_kv8_attention(a["qkv"], a["ldq"], a["k8"], a["v8"], a["ek"], a["ev"], a["mask"], a["state"], a["batch"], a["seq"], a["cap"], a["heads"],
                                  a["hd"], a["fuse"], a["part"], a["pb"], a["out"], a["stream"])
for name in ("qkv", "k8", "v8", "ek", "ev", "part", "out"):
    assert attn(**{name: None}) == BAD, name
for name in ("qkv", "k8", "v8", "out"):
    assert attn(**{name: p + 2}) == BAD, name
assert attn(batch=0) == BAD and attn(heads=0) == BAD and attn(cap=15) == BAD and attn(seq=-1) == BAD and attn(cap=0, seq=0) == BAD
assert attn(ldq=479) == BAD and attn(ldq=484) == BAD and attn(ldq=160, fuse=1) == BAD
for hd in (8, 64, 72, 96):
    assert attn(hd=hd, ldq=6 * hd) == UNSUP, hd
assert attn(pb=4 * 3 * 2 * 1 * 82 - 1) == WS and attn(cap=257, pb=4 * 3 * 2 * 2 * 82 - 1) == WS
d = abi.Dims(t_hidden=160, t_heads=2, t_ffn=320, t_layers=2, vocab=128, max_pos=64, t_eps=1e-5)
d64 = abi.Dims(t_hidden=128, t_heads=2, t_ffn=320, t_layers=2, vocab=128, max_pos=64, t_eps=1e-5)
nb = kv.eilev_kv8_cache_bytes
# bytes, then the exponents from the next 256-byte boundary: 2 layers x (k | v) x 3 rows x 2 heads x 37 slots
planes = 2 * 2 * 3 * 2 * 37
assert nb(C.byref(d), 3, 37) == -(-(-(-planes * 80 // 256) * 256 + planes) // 256) * 256
assert nb(C.byref(d64), 3, 37) == 0 and nb(None, 3, 37) == 0 and nb(C.byref(d), 0, 37) == 0 and nb(C.byref(d), 3, 0) == 0
def quant(**kw):
    a = dict(d=C.byref(d), src=p, batch=3, src_cap=37, slots=29, dst=p, dst_cap=40, stream=None)
    a.update(kw)
    return kv.eilev_kv8_quantize(a["d"], a["src"], a["batch"], a["src_cap"], a["slots"], a["dst"], a["dst_cap"], a["stream"])
for name in ("d", "src", "dst"):
    assert quant(**{name: None}) == BAD, name
assert quant(src=p + 2) == BAD and quant(dst=p + 8) == BAD
assert quant(slots=0) == BAD and quant(slots=38) == BAD and quant(dst_cap=28) == BAD and quant(batch=0) == BAD
assert quant(d=C.byref(d64)) == UNSUP
w = abi.OptWeights()
def step(**kw):
    a = dict(d=C.byref(d), w=C.byref(w), tok=p, state=p, mask=p, nv=p, batch=3, seq=16, kv=p, cap=20, logits=p, fin=p, eos=-1, pad=1, out=p, max_new=4, ws=p,
             ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return kv.eilev_kv8_decode_step(a["d"], a["w"], a["tok"], a["state"], a["mask"], a["nv"], a["batch"], a["seq"], a["kv"], a["cap"], a["logits"], a["fin"],
                                    a["eos"], a["pad"], a["out"], a["max_new"], a["ws"], a["ws_bytes"], a["stream"])
for name in ("d", "w", "tok", "state", "mask", "nv", "kv", "logits", "fin", "out", "ws"):
    assert step(**{name: None}) == BAD, name
assert step(batch=0) == BAD and step(batch=abi.KV8_MAX_ROWS + 1) == BAD and step(max_new=6) == BAD and step(seq=0) == BAD
assert step(d=C.byref(d64)) == UNSUP
assert step(ws_bytes=16) == WS
ws = kv.eilev_kv8_workspace_bytes
assert ws(C.byref(d), 3) > 0 and ws(C.byref(d), 0) == 0 and ws(C.byref(d), 33) == 0 and ws(C.byref(d64), 3) == 0 and ws(None, 3) == 0
"""


def test_refusals_return_before_any_hip_call():
    """Null and misaligned pointers, shapes beyond the limits, a head size other than 80 / 128, partials or a workspace too small: refused
    on a machine without a GPU, with pointers that no kernel could follow; eilev_kv8_cache_bytes states the layout."""
    _child(_REFUSALS)


# ---- 2. the quantiser's restatement against brute force ------------------------------------------------------------------------------------------
def _bf16_patterns():
    """Finite non-negative bf16 values: every exponent with the mantissas around the 448 = 1.75 * 2^8 threshold (0x60) and the ends."""
    exps = np.arange(0, 255, dtype=np.uint32)
    mant = np.array([0, 1, 0x3F, 0x5F, 0x60, 0x61, 0x7E, 0x7F], np.uint32)
    bits = ((exps[:, None] << 7) | mant[None, :]).reshape(-1)
    return torch.from_numpy((bits << 16).view(np.float32).copy())


def test_exponent_is_minimal_for_every_amax():
    amax = _bf16_patterns()
    amax = amax[amax > 0]
    e = ref.exponents(amax).to(torch.float64)
    a = amax.to(torch.float64)
    assert bool((a <= ref.E4M3_MAX * torch.pow(2.0, e)).all())
    smaller_fits = a <= ref.E4M3_MAX * torch.pow(2.0, e - 1)
    assert bool((~smaller_fits | (e == ref.E_MIN)).all()), "a smaller exponent would do"
    assert int(e.min()) == ref.E_MIN and bool((e[a < ref.E4M3_MAX * 2.0 ** ref.E_MIN] == ref.E_MIN).all())  # the clamp, subnormal amax included
    assert int(ref.exponents(torch.tensor([448.0]))[0]) == 0 and int(ref.exponents(torch.tensor([450.0]))[0]) == 1
    assert ref.exponents(torch.tensor([0.0, float("inf"), float("nan")])).tolist() == [0, 0, 0]


def test_quantize_is_one_rounding_and_its_twin_is_bf16():
    g = torch.Generator().manual_seed(11)
    amax = _bf16_patterns()
    amax = amax[(amax > 0) & (amax < 3e38)]
    for hd in (80, 128):
        # one vector per amax pattern: the amax itself (either sign), values spread over many binades below it, zeros
        x = torch.rand((len(amax), hd), generator=g) * 2 - 1
        x = x * torch.pow(2.0, -torch.randint(0, 14, x.shape, generator=g).float()) * amax[:, None]
        x[:, 3] = amax * torch.where(torch.rand(len(amax), generator=g) < 0.5, -1.0, 1.0)
        x[:, 5] = 0.0
        x = x.to(torch.bfloat16)
        b, eb = ref.quantize(x)
        assert b.dtype == torch.uint8 and eb.dtype == torch.uint8 and b.shape == x.shape and eb.shape == x.shape[:-1]
        e = eb.to(torch.int32) - 127
        assert torch.equal(e, ref.exponents(x.float().abs().amax(-1)))
        scaled = x.double() * torch.pow(2.0, -e.double())[:, None]
        assert float(scaled.abs().max()) <= ref.E4M3_MAX
        # the statement of the header, row by row with a python scalar
        for r in range(0, len(amax), 97):
            assert torch.equal(b[r], (x[r].float() * 2.0 ** -int(e[r])).to(torch.float8_e4m3fn).view(torch.uint8)), r
        # one rounding: the byte is the e4m3 value nearest to the exactly scaled element
        back = b.view(torch.float8_e4m3fn).double()
        assert torch.equal(b, scaled.float().to(torch.float8_e4m3fn).view(torch.uint8)) and bool(((back - scaled).abs() <= scaled.abs() * 2.0 ** -4 + 2.0 ** -10).all())
        dq = ref.dequantize(b, eb)
        assert bool(torch.isfinite(dq).all()) and torch.equal(dq.to(torch.bfloat16).float(), dq), "the twin is not bf16-exact"
        assert bool((b[:, 5] == 0).all()) and bool((dq[:, 5] == 0).all())
        low = e == ref.E_MIN
        assert bool(low.any()) and bool(((b[low] & 0x78) == 0).any()), "no e4m3 subnormal under the clamp"
    zb, ze = ref.quantize(torch.zeros(2, 80, dtype=torch.bfloat16))
    assert bool((zb == 0).all()) and ze.tolist() == [127, 127] and bool((ref.dequantize(zb, ze) == 0).all())
    bad = torch.ones(3, 80)
    bad[0, 7], bad[1, 9] = float("inf"), float("nan")
    assert ref.quantize(bad)[1].tolist() == [127, 127, 127 - 8]
    sub = torch.full((1, 80), 2.0 ** -7) * 2.0 ** -126  # the smallest bf16 subnormal: the clamp, bytes = the e4m3 subnormal 4 * 2^-9
    sb, se = ref.quantize(sub.to(torch.bfloat16))
    assert se.tolist() == [1] and bool((sb == 4).all()) and torch.equal(ref.dequantize(sb, se), sub)


# ---- 3. the attention reference catches planted mistakes -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    c = ref.build_case(ref.by_name(name))
    return (c, *ref.reference(c))


@functools.lru_cache(maxsize=None)
def _mistakes(name):
    """mistake -> the worst error it causes on the case, in units of tol (the mistakes that apply to it)."""
    c, out, A = _case(name)
    return {mut: ref.worst_ratio(ref.mutated(c, mut), out, A) for mut in ref.MUTATIONS if ref.applies(mut, c.spec)}


@pytest.mark.parametrize("sp", ref.CASES, ids=lambda sp: sp.name)
def test_cases_meet_the_preconditions_and_show_every_mistake(sp):
    """Where TOL_REL * A_i was derived (kv8_ref.py): every (row, head) with two or more visible keys owns a spike of weight in [W_LO, W_HI),
    ordinary |v| in [4, 7.5]; unwritten slots are poisoned; the twin is the planes' exact value, bf16-exact, and quantising it again loses nothing.  Every mistake that
    applies to the case is evaluated (test_every_planted_mistake_is_seen_beyond_the_bound holds them to the bound)."""
    c, out, A = _case(sp.name)
    w = c.spike_w[c.spike_pos >= 0]
    many = w[w < 1.0]
    assert len(many) == 0 or (many.min() >= ref.W_LO and many.max() < ref.W_HI)
    assert np.isfinite(out).all() and (A[np.abs(out).reshape(A.shape) > 0] >= 4.0).all()
    n, new = sp.n, (sp.n - 1 if sp.fuse_new else -1)
    live = np.ones(sp.cap, bool)
    live[n:] = False
    if new >= 0:
        live[new] = False
    assert (c.k8[:, :, ~live] == ref.NAN_BYTE).all() and (c.ev[:, :, ~live] == ref.NAN_EXP).all() and np.isnan(c.kd[:, :, ~live]).all()
    for plane8, planee, twin in ((c.k8, c.ek, c.kd), (c.v8, c.ev, c.vd)):
        t = torch.from_numpy(twin[:, :, live])
        assert torch.equal(ref.dequantize(torch.from_numpy(plane8[:, :, live]), torch.from_numpy(planee[:, :, live])), t)
        assert torch.equal(ref.dequantize(*ref.quantize(t)), t) and torch.equal(t.to(torch.bfloat16).float(), t)  # quantising the twin again loses nothing
    assert ref.worst_ratio(out, out, A) == 0.0
    print(f"[kv8 cases] {sp.name}: " + ", ".join(f"{m} {r:.3g}" for m, r in _mistakes(sp.name).items()) + " tol")


def test_every_planted_mistake_is_seen_beyond_the_bound():
    """Each of the ten mistakes moves some element of at least one case by more than 1.0 tol — most by orders of magnitude."""
    assert len(ref.MUTATIONS) == 10
    for mut in ref.MUTATIONS:
        got = [_mistakes(sp.name)[mut] for sp in ref.CASES if ref.applies(mut, sp)]
        print(f"[kv8 mistakes] {mut}: beyond the bound in {sum(r > 1.0 for r in got)} of {len(got)} cases, worst {max(got):.3g} tol")
        assert max(got) > 1.0, mut


def test_case_list_covers_what_it_says():
    L = ref.CASES
    assert {sp.hd for sp in L} == {80, 128} and {sp.heads for sp in L} == {3} and {sp.batch for sp in L} == {1, 3, 32}
    for hd in (80, 128):
        for by in (None, "state"):
            assert {sp.n for sp in L if sp.hd == hd and (sp.gen is None) == (by is None)} >= set(ref.SWEEP)
    kinds = set()
    for sp in L:
        if sp.mask == "mixed" and sp.seq_len:
            kinds |= {ref.MASK_KINDS[(r + sp.mask_first) % 5] for r in range(sp.batch)}
    assert kinds == set(ref.MASK_KINDS)
    # the cover set: every slot of a 288-key cache is the spike of some (row, head)
    for hd in (80, 128):
        seen = set()
        for k in range(3):
            seen |= set(_case(f"cover-hd{hd}-{k}")[0].spike_pos.reshape(-1).tolist())
        assert seen >= set(range(288))


# ---- 4. generate(kv_cache_dtype=...) ------------------------------------------------------------------------------------------------------------
def _model(name="tiny"):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    return VideoBlipForConditionalGeneration(blip2_config(name))


def _supported_head_size(m):
    """The checks under test read the head size from the config: give the tiny model one the fp8 cache takes."""
    t = m.config.text_config
    t.hidden_size, t.num_attention_heads = 160, 2
    return m


def test_generate_refuses_what_the_fp8_cache_does_not_serve():
    from transformers import LogitsProcessorList, MaxLengthCriteria, MinLengthLogitsProcessor, StoppingCriteriaList

    from eilev_amd.model.v2 import VideoContext

    m = _supported_head_size(_model())
    one = torch.ones(1, 4, dtype=torch.long)
    ctx = VideoContext(SimpleNamespace(P=10), torch.ones(1, 10, dtype=torch.long), key=None)
    refused = [
        ("num_beams > 1", dict(num_beams=3)),
        ("context=", dict(context=ctx)),
        ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=3)),
        ("logits_processor", dict(logits_processor=LogitsProcessorList([MinLengthLogitsProcessor(2, 1)]))),
        ("stopping criteria", dict(stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(8)]))),
        ("max_time", dict(max_time=1.0)),
        ("more than 8 EOS ids", dict(eos_token_id=list(range(2, 11)))),
    ]
    for name, kw in refused:
        with pytest.raises(NotImplementedError, match=re.escape(name)) as e:
            m.generate(one, max_new_tokens=4, kv_cache_dtype="fp8", **kw)
        assert "kv_cache_dtype" in str(e.value), name
    # the route switches of an engine that exists
    for attr, kw in (("device_sampling", dict(do_sample=True)), ("device_rules", dict(repetition_penalty=1.5, no_repeat_ngram_size=3))):
        m._hip = (None, SimpleNamespace(device_sampling=attr != "device_sampling", device_rules=attr != "device_rules"))
        with pytest.raises(NotImplementedError, match=attr) as e:
            m.generate(one, max_new_tokens=4, kv_cache_dtype="fp8", **kw)
        assert "kv_cache_dtype" in str(e.value)
        m._hip = None
    # an unsupported head size (the tiny model's own), and the flan-t5 language model
    with pytest.raises(NotImplementedError, match="head size") as e:
        _model().generate(one, max_new_tokens=4, kv_cache_dtype="fp8")
    assert "kv_cache_dtype" in str(e.value)
    from eilev_amd.configs import CONFIGS

    t5 = next(n for n, c in CONFIGS.items() if c["text_config"].get("model_type") == "t5")
    with pytest.raises(NotImplementedError, match="flan-t5") as e:
        _model(t5).generate(one, max_new_tokens=2, kv_cache_dtype="fp8")
    assert "kv_cache_dtype" in str(e.value)
    for bad in ("fp16", "int8", 8, "FP8"):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            m.generate(one, max_new_tokens=4, kv_cache_dtype=bad)


def test_the_default_values_reach_the_engine():
    """None, "bf16" and a supported "fp8" call pass every check and reach the engine, which needs a GPU (no CPU fallback)."""
    one = torch.ones(1, 4, dtype=torch.long)  # (a CPU model: the engine refuses it with or without a GPU in the machine)
    for m, kw in ((_model(), dict()), (_model(), dict(kv_cache_dtype=None)), (_model(), dict(kv_cache_dtype="bf16")),
                  (_supported_head_size(_model()), dict(kv_cache_dtype="fp8")),
                  (_supported_head_size(_model()), dict(kv_cache_dtype="fp8", do_sample=True)),
                  (_supported_head_size(_model()), dict(kv_cache_dtype="fp8", repetition_penalty=1.5, no_repeat_ngram_size=3))):
        with pytest.raises(RuntimeError):
            m.generate(one, max_new_tokens=4, **kw)


def test_the_engine_routes_carry_the_argument():
    import inspect

    from eilev_amd.engine import HipEngine

    for fn in (HipEngine._select_decode_device, HipEngine.greedy_decode, HipEngine.sample_decode_device, HipEngine.rules_decode_device):
        assert inspect.signature(fn).parameters["kv_dtype"].default == "bf16", fn.__name__
