"""CPU side of the int4 weight-only library (include/eilev_w4.h, libeilev_hip_w4.so; HipEngine(lm_weights="int4")): its surface (header = abi =
dynamic symbols), the refusals that return before any HIP call, the quantiser and the packing of eilev_amd/quant.py against the stated bound
and against brute force, the planted mistakes the float64 reference of tests/w4_ref.py must catch, the Python mirror of eilev_w4_plan, and the
refusals of the engine and the model class — the GPU side is tests/test_hip_w4.py."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import w4_ref as ref
from eilev_amd import quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code: str):
    """Run `code` in a child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    subprocess.check_call([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)])


# ---- 1. the surface ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    from eilev_amd import abi

    hdr = open(os.path.join(ROOT, "include", "eilev_w4.h")).read()
    code_part = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(eilev_w4_\w+)\s*\(", code_part))) == sorted(abi.W4_EXPORTS)
    for name in ("ABI_VERSION", "GROUP", "KTILE", "MAX_ROWS", "WAVE_TILES"):
        assert int(re.search(r"#define EILEV_W4_%s (\d+)" % name, hdr).group(1)) == getattr(abi, "W4_" + name)
    assert abi.W4_GROUP == quant.INT4_GROUP and abi.W4_KTILE == quant.INT4_KTILE
    assert abi.w4_supported(abi.Dims(t_hidden=256, t_heads=2, t_ffn=512)) and abi.w4_supported(abi.Dims(t_hidden=2560, t_heads=32, t_ffn=10240))
    assert not abi.w4_supported(abi.Dims(t_hidden=160, t_heads=2, t_ffn=320)) and not abi.w4_supported(abi.Dims(t_hidden=256, t_heads=2, t_ffn=384))
    assert not abi.w4_supported(None)
    assert abi.w4_supported(abi.Dims(t_hidden=4096, t_heads=32, t_ffn=16384)) and not abi.w4_supported(abi.Dims(t_hidden=5120, t_heads=40, t_ffn=20480))
    assert os.path.exists(abi.W4_LIB_PATH), "libeilev_hip_w4.so has not been built"
    _child("import ctypes\nfrom eilev_amd import abi\nh = ctypes.CDLL(abi.W4_LIB_PATH)\n"
           "assert all(hasattr(h, s) for s in abi.W4_EXPORTS)\nassert h.eilev_w4_abi_version() == abi.W4_ABI_VERSION\n"
           "assert not hasattr(h, 'eilev_opt_decode_step') and not hasattr(h, 'eilev_abi_version')\n")
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.W4_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.W4_EXPORTS), syms
    # the core library's header and export list are untouched: no w4 name appears in them
    assert "w4" not in open(os.path.join(ROOT, "include", "eilev.h")).read().lower() and not any("w4" in s for s in abi.EXPORTS)


def test_ctypes_structs_match_the_header():
    """Field names and order of the three structs, read off the header."""
    from eilev_amd import abi

    hdr = open(os.path.join(ROOT, "include", "eilev_w4.h")).read()
    for cname, cls in (("EilevW4Matrix", abi.W4Matrix), ("EilevW4Layer", abi.W4Layer), ("EilevW4Linear", abi.W4Linear)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
        assert names == [f[0] for f in cls._fields_], cname


_REFUSALS = r"""
import ctypes as C
from eilev_amd import abi
w4 = abi.load_w4()
BAD, UNSUP, WS = -1, -2, -3
buf = C.create_string_buffer(4096)  # a non-null address that a refused call never follows
p = (C.cast(buf, C.c_void_p).value + 63) & ~63
form = (C.c_int32 * 5)()
assert w4.eilev_w4_plan(1, 7680, 2560, form) == 0 and list(form) == [1, 1, 480, 1, 3]
assert w4.eilev_w4_plan(0, 16, 256, form) == BAD and w4.eilev_w4_plan(33, 16, 256, form) == BAD and w4.eilev_w4_plan(1, 0, 256, form) == BAD
assert w4.eilev_w4_plan(1, 16, 256, None) == BAD and w4.eilev_w4_plan(1, 16, 0, form) == BAD
assert w4.eilev_w4_plan(1, 16, 128, form) == UNSUP and w4.eilev_w4_plan(1, 16, 384, form) == UNSUP and w4.eilev_w4_plan(1, 16, (1 << 20) + 256, form) == UNSUP
sb = w4.eilev_w4_linear_scratch_bytes
assert sb(1, 7680, 2560) == 0 and sb(32, 2560, 10240) == 4 * 32 * 2560 * 4 and sb(3, 2560, 2560) == 2 * 16 * 2560 * 4 and sb(1, 16, 128) == 0
def expand(**kw):
    a = dict(w4=p, s=p, n=16, k=256, out=p, stream=None)
    a.update(kw)
    return w4.eilev_w4_expand(a["w4"], a["s"], a["n"], a["k"], a["out"], a["stream"])
for name in ("w4", "s", "out"):
    assert expand(**{name: None}) == BAD and expand(**{name: p + 4}) == BAD, name
assert expand(n=0) == BAD and expand(k=0) == BAD and expand(k=64) == UNSUP and expand(k=200) == UNSUP
def linear(stream=None, **kw):
    l = abi.W4Linear(a=p, lda=2560, w=abi.W4Matrix(p, p), c=p, ldc=2560, m=3, n=2560, k=2560, scale=1.0, scratch=p, scratch_bytes=1 << 30)
    for k, v in kw.items():
        setattr(l, k, v)
    return w4.eilev_w4_linear(C.byref(l), stream)
assert w4.eilev_w4_linear(None, None) == BAD
for name in ("a", "c"):
    assert linear(**{name: None}) == BAD, name
assert linear(w=abi.W4Matrix(None, p)) == BAD and linear(w=abi.W4Matrix(p, None)) == BAD and linear(w=abi.W4Matrix(p + 4, p)) == BAD
assert linear(a=p + 2) == BAD and linear(lda=2552) == BAD and linear(lda=2564) == BAD and linear(ldc=2559) == BAD and linear(resid=p, ldr=8) == BAD
assert linear(m=0) == BAD and linear(m=33) == BAD and linear(scale_cols=-1) == BAD and linear(scale_cols=2561) == BAD
assert linear(k=2688, lda=2688) == UNSUP
assert linear(ln_out=p) == BAD and linear(ln_out=p, ln_gamma=p, ln_beta=p, out_f32=1) == UNSUP
assert linear(ln_out=p, ln_gamma=p, ln_beta=p, n=4104, ldc=4104) == UNSUP
assert linear(scratch=None) == WS and linear(scratch_bytes=2 * 16 * 2560 * 4 - 1) == WS
d = abi.Dims(t_hidden=256, t_heads=2, t_ffn=512, t_layers=2, vocab=128, max_pos=64, t_eps=1e-5)
d160 = abi.Dims(t_hidden=160, t_heads=2, t_ffn=320, t_layers=2, vocab=128, max_pos=64, t_eps=1e-5)
ws = w4.eilev_w4_workspace_bytes
assert ws(C.byref(d), 3) > 0 and ws(C.byref(d), 0) == 0 and ws(C.byref(d), 33) == 0 and ws(C.byref(d160), 3) == 0 and ws(None, 3) == 0
w, table = abi.OptWeights(), (abi.W4Layer * 2)()
def step(**kw):
    a = dict(d=C.byref(d), w=C.byref(w), t=table, tok=p, state=p, mask=p, nv=p, batch=3, seq=16, kv=p, cap=20, logits=p, fin=p, eos=-1, pad=1, out=p,
             max_new=4, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return w4.eilev_w4_decode_step(a["d"], a["w"], a["t"], a["tok"], a["state"], a["mask"], a["nv"], a["batch"], a["seq"], a["kv"], a["cap"], a["logits"],
                                   a["fin"], a["eos"], a["pad"], a["out"], a["max_new"], a["ws"], a["ws_bytes"], a["stream"])
for name in ("d", "w", "t", "tok", "state", "mask", "nv", "kv", "logits", "fin", "out", "ws"):
    assert step(**{name: None}) == BAD, name
assert step(batch=0) == BAD and step(batch=abi.W4_MAX_ROWS + 1) == BAD and step(max_new=6) == BAD and step(seq=0) == BAD
assert step(d=C.byref(d160)) == UNSUP
d5120 = abi.Dims(t_hidden=5120, t_heads=40, t_ffn=20480, t_layers=2, vocab=128, max_pos=64, t_eps=1e-5)
assert step(d=C.byref(d5120)) == UNSUP and ws(C.byref(d5120), 3) == 0
assert step(ws_bytes=16) == WS
"""


def test_refusals_return_before_any_hip_call():
    """Null and misaligned pointers, shapes beyond the limits, widths that are no multiple of 256, a scratch or a workspace too small: refused on
    a machine without a GPU, with pointers that no kernel could follow; eilev_w4_plan and the scratch size state the form."""
    _child(_REFUSALS)


# ---- 2. the quantiser and the packing ------------------------------------------------------------------------------------------------------------
def _weights(seed, n=24, k=512):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * torch.pow(2.0, torch.randint(-12, 3, (n, 1), generator=g).float())
    w[1, 128:256] = 0.0            # an all-zero group
    w[2, :128] = w[2, :128].abs()  # a group of one sign
    w[3, 5] = 40.0                 # one outlier sets its group's scale
    return w.to(torch.bfloat16).float()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quantiser_meets_the_stated_bound_and_the_twin_is_bf16(seed):
    w = _weights(seed)
    q, s = quant.quantize_int4(w)
    n, k = w.shape
    assert q.dtype == torch.int8 and s.dtype == torch.bfloat16 and s.shape == (n, k // 128)
    assert int(q.min()) >= -7 and int(q.max()) <= 7, "with s = amax / 7 rounded to bf16, |w| / s stays below 7.5: nothing clamps, -8 is never emitted"
    assert float(s[1, 1]) == 1.0 and bool((q[1, 128:256] == 0).all())
    s32 = s.float()
    g = w.view(n, k // 128, 128)
    amax = g.abs().amax(dim=2)
    want_s = torch.where(amax > 0, amax / 7.0, torch.ones_like(amax)).to(torch.bfloat16)
    assert torch.equal(s, want_s)
    assert float((g.abs() / s32[:, :, None]).max()) <= 7.04
    # brute force of the rounding: round half to even of the fp32 quotient
    quo = (g / s32[:, :, None]).numpy().astype(np.float32)
    assert np.array_equal(np.clip(np.rint(quo), -8, 7).astype(np.int8).reshape(n, k), q.numpy())
    twin = quant.twin_int4(q, s)
    assert twin.dtype == torch.bfloat16 and torch.equal(twin.float().to(torch.bfloat16), twin)
    prod = q.double().view(n, k // 128, 128) * s.double()[:, :, None]
    assert torch.equal(prod.float().double(), prod), "q * s is exact in fp32"
    assert torch.equal(prod.float().to(torch.bfloat16).view(n, k), twin), "the twin is ONE rounding of the exact product"
    # |W' - W| <= s / 2 + 2^-8 |q s| + the fp32 division's rounding (2^-24 |w / s| s)
    err = (twin.double().view(n, k // 128, 128) - g.double()).abs()
    bound = s.double()[:, :, None] / 2 + 2.0 ** -8 * prod.abs() + 2.0 ** -24 * g.double().abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((err / bound).max()) > 0.5, "the bound is not slack by more than a factor of two on these weights"


def test_pack_and_unpack_are_inverse_for_every_code_at_every_position():
    # every code 0 .. 15 at each of the 8 positions of a word, the other positions holding a different code
    rows = []
    for pos in range(8):
        for code in range(16):
            r = np.full(16, (code + 5) % 16 - 8, np.int8)
            r[pos] = code - 8
            r[8 + (pos + 3) % 8] = code - 8
            rows.append(r)
    q = torch.from_numpy(np.stack(rows))
    p = quant.pack_int4(q)
    assert p.dtype == torch.uint8 and p.shape == (128, 8)
    assert torch.equal(quant.unpack_int4(p), q)
    assert np.array_equal(p.numpy(), ref.brute_pack(q.numpy()))
    assert np.array_equal(p.numpy().view("<u4"), ref.brute_words(q.numpy()))
    # and the other way round: every byte value at every byte of a word
    b = torch.arange(256, dtype=torch.uint8).repeat(4, 1).T.contiguous()  # (256, 4): one word per row, all four bytes equal
    b = torch.cat([b, torch.roll(b, 1, 0)], dim=1)
    assert torch.equal(quant.pack_int4(quant.unpack_int4(b)), b)
    with pytest.raises(ValueError):
        quant.pack_int4(torch.full((1, 8), 8, dtype=torch.int8))
    q2 = ref.all_codes(40, 512, seed=3)
    assert sorted(set(q2.flatten().tolist())) == list(range(-8, 8))
    assert np.array_equal(quant.pack_int4(q2).numpy(), ref.brute_pack(q2.numpy()))
    # the pair extraction the kernels use: (word >> 4 i) & 0x000f000f = (u[2 i], u[2 i + 1])
    words = quant.pack_int4(q2).numpy().view("<u4").astype(np.uint64)
    u = (q2.numpy().astype(np.int64) + 8).reshape(40, 64, 8)
    for i in range(4):
        pair = (words >> np.uint64(4 * i)) & np.uint64(0x000F000F)
        assert np.array_equal(pair & np.uint64(0xFFFF), u[:, :, 2 * i]) and np.array_equal(pair >> np.uint64(16), u[:, :, 2 * i + 1])


# ---- 3. planted mistakes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f32", [True, False])
def test_every_planted_mistake_is_seen_beyond_the_bound(out_f32):
    """The float64 reference A . W'^T with the GPU tests' bound: a kernel that made one of these mistakes would leave it."""
    m, n, k = 17, 40, 512
    A, q, s = ref.dense_operands(m, n, k, seed=7)
    assert int((q == -8).sum()) > 0
    y, S = ref.linear_ref(A.float().numpy(), ref.twin64(q, s))
    t = ref.tol(y, S, k, 1, out_f32)
    assert float((t / (np.abs(y) + 1e-30)).min()) < 1.0
    for name, wrong in ref.MISTAKES.items():
        y_bad, _ = ref.linear_ref(A.float().numpy(), wrong(q, s))
        if not out_f32:  # a bf16 output: the mistaken kernel's value is rounded too
            y_bad = torch.from_numpy(y_bad).float().to(torch.bfloat16).double().numpy()
        worst = float(ref.R.ratio(np.abs(y_bad - y), t).max())
        if name == "no bf16 rounding of q * s" and not out_f32:
            # (the output's own bf16 rounding is as large as this mistake: only the fp32 output shows it — the GPU tests have both)
            continue
        assert worst > 1.0, (name, worst)
    # the honest kernel: fp32 accumulation in another order stays inside
    y32 = (A.float() @ torch.from_numpy(ref.twin64(q, s)).float().T).double().numpy()
    if not out_f32:
        y32 = torch.from_numpy(y32).float().to(torch.bfloat16).double().numpy()
    assert float(ref.R.ratio(np.abs(y32 - y), t).max()) <= 1.0


# ---- 4. the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan_mirror_agrees_with_the_library_and_the_cases_reach_every_form():
    from eilev_amd import abi

    shapes = sorted(set(ref.LINEAR_CASES) | {(m, n, k) for m in (1, 16, 17, 32) for n, k in ((4096, 4096), (16384, 4096), (4096, 16384), (12288, 4096))} |
                    {(0, 16, 256), (33, 16, 256), (1, 16, 128), (4, 0, 256)})
    code = "import ctypes as C\nfrom eilev_amd import abi\nw4 = abi.load_w4()\nform = (C.c_int32 * 5)()\nfor m, n, k in %r:\n" \
           "    rc = w4.eilev_w4_plan(m, n, k, form)\n    want = abi.w4_plan(m, n, k)\n" \
           "    assert (rc == 0) == (want is not None), (m, n, k, rc)\n    assert rc != 0 or tuple(form) == want, (m, n, k, tuple(form), want)\n" % (shapes,)
    _child(code)
    forms = {(abi.w4_plan(*c)[0], abi.w4_plan(*c)[1] > 1) for c in ref.LINEAR_CASES}
    assert forms == {(1, False), (1, True), (2, False), (2, True)}, "both MB instances, each unsplit and split"
    assert all(abi.w4_plan(*c)[4] <= abi.W4_WAVE_TILES for c in shapes if abi.w4_plan(*c))
    assert {abi.w4_plan(*c)[4] for c in ref.LINEAR_CASES} == {1, 2, 3}, "every tile count of a wave"
    # every tile of a shape belongs to exactly one (split, wave)
    for m, n, k in ref.LINEAR_CASES:
        _, ks, _, _, _ = abi.w4_plan(m, n, k)
        ktiles, seen = k // 256, []
        per_wg = -(-ktiles // ks)
        for y in range(ks):
            beg, end = y * per_wg, min(ktiles, y * per_wg + per_wg)
            per_w = (max(end - beg, 0) + 3) // 4
            for w in range(4):
                b, e = beg + w * per_w, min(end, beg + w * per_w + per_w)
                assert e - b <= abi.W4_WAVE_TILES
                seen += list(range(b, e))
        assert seen == list(range(ktiles)), (m, n, k)


# ---- 5. the refusals of the engine and the model class ------------------------------------------------------------------------------------------------
def _model(name):
    from eilev_amd.configs import blip2_config
    from eilev_amd.model.v2 import VideoBlipForConditionalGeneration

    m = VideoBlipForConditionalGeneration(blip2_config(name))
    m.hip_lm_weights = "int4"
    return m


def test_int4_names_its_reason_for_what_it_does_not_serve():
    from eilev_amd.configs import CONFIGS, blip2_config
    from eilev_amd.engine import HipEngine

    one = torch.ones(1, 4, dtype=torch.long)
    t5 = next(n for n, c in CONFIGS.items() if c["text_config"].get("model_type") == "t5")
    for name, why in ((t5, "flan-t5"), ("mid", "multiples of 256"), ("tiny", "multiples of 256")):
        with pytest.raises(NotImplementedError, match=why) as e:
            HipEngine(blip2_config(name), {}, lm_weights="int4")
        assert "int4" in str(e.value)
        with pytest.raises(NotImplementedError, match=why) as e:
            _model(name).generate(one, max_new_tokens=2)
        assert "int4" in str(e.value)
    with pytest.raises(NotImplementedError, match="OPT") as e:
        HipEngine(blip2_config("mid_k128"), {}, parts=("vit", "qf"), lm_weights="int4")
    wide = blip2_config("mid_k128")  # OPT-13B's width: the step's LayerNorm rows are built up to 4096
    wide.text_config.hidden_size, wide.text_config.ffn_dim, wide.text_config.num_attention_heads = 5120, 20480, 40
    with pytest.raises(NotImplementedError, match="4096") as e:
        HipEngine(wide, {}, lm_weights="int4")
    assert "int4" in str(e.value)
    with pytest.raises(ValueError, match="int4"):
        HipEngine(blip2_config("mid_k128"), {}, lm_weights="int3")
    m = _model("mid_k128")
    with pytest.raises(NotImplementedError, match="kv_cache_dtype") as e:
        m.generate(one, max_new_tokens=2, kv_cache_dtype="fp8")
    assert "int4" in str(e.value)
    with pytest.raises(NotImplementedError, match="int4") as e:
        m(one, labels=one)
    assert "labels" in str(e.value)
    m.train()
    with pytest.raises(NotImplementedError, match="int4") as e:
        m(one)
    assert "training" in str(e.value)
    # a model it serves passes every check and reaches the engine, which needs a GPU (a CPU model: refused with or without one in the machine)
    m.eval()
    for kw in (dict(), dict(do_sample=True), dict(num_beams=3), dict(repetition_penalty=1.5, no_repeat_ngram_size=3)):
        with pytest.raises(RuntimeError):
            m.generate(one, max_new_tokens=2, **kw)
