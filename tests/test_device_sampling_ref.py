"""The float64 restatement of the device sampling step (eilev_amd/sampling.py: sample_select_reference, keep_bounds, draw_ok) against
what it restates: `warp_logits` (the host loop's warpers), transformers' RepetitionPenaltyLogitsProcessor, and the distribution itself."""
import pytest
import torch

from eilev_amd.sampling import (SampleSpec, draw_ok, keep_bounds, processed_scores, row_history, sample_select_reference, warp_logits)

SETTINGS = [(1.0, 50, 1.0), (0.7, 0, 0.9), (1.5, 3, 1.0), (1.0, 0, 1.0), (0.7, 50, 0.9)]  # (temperature, top_k, top_p)
TOL = 1e-5  # warp_logits sums fp32 probabilities one after another over the whole vocabulary


def _call(logits, spec, uniforms=None, state=(0, 1), out=None, finished=None, max_new=4, **kw):
    R = logits.shape[0]
    uniforms = torch.rand((max_new, R), generator=torch.Generator().manual_seed(1)) if uniforms is None else uniforms
    out = torch.zeros((R, uniforms.shape[0]), dtype=torch.int64) if out is None else out
    finished = torch.zeros(R, dtype=torch.uint8) if finished is None else finished
    return sample_select_reference(logits, uniforms, list(state), finished, torch.zeros(R, dtype=torch.int64), out, spec, **kw)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
@pytest.mark.parametrize("vocab", [1000, 50272])
def test_kept_set_equals_warp_logits(vocab, setting):
    T, k, p = setting
    logits = torch.randn((32, vocab), generator=torch.Generator().manual_seed(vocab)) * 3
    spec = SampleSpec(T, k, p)
    ref = _call(logits, spec)
    kept = torch.isfinite(ref["scores"])
    host = torch.isfinite(warp_logits(logits, T, k, p))
    must, may = keep_bounds(logits, None, spec, TOL)
    for s in (kept, host):
        assert not bool((must & ~s).any()) and not bool((s & ~may).any())
    assert int((may & ~must).sum(dim=1).max()) <= 2
    assert bool(((kept == host) | (may & ~must)).all())
    assert torch.equal(ref["scores"][kept].float(), warp_logits(logits, T, k, p)[kept])
    u = torch.rand((4, 32), generator=torch.Generator().manual_seed(1))[0]
    assert bool(draw_ok(kept, ref["scores"], u, ref["drawn"], 1e-12).all())
    assert not bool(draw_ok(kept, ref["scores"], (u + 0.5) % 1.0, ref["drawn"], 1e-12).all())


def test_repetition_penalty_equals_transformers():
    from transformers import RepetitionPenaltyLogitsProcessor

    logits = torch.randn((4, 1000), generator=torch.Generator().manual_seed(2)) * 3
    out = torch.randint(0, 1000, (4, 6), generator=torch.Generator().manual_seed(3))
    out[:, 3] = out[:, 0]  # duplicates
    out[:, 4] = logits.argmax(dim=1)  # both signs
    out[:, 5] = logits.argmin(dim=1)
    for prefix in (-1, 7):
        hist = row_history(out, 6, prefix)
        assert all(len(h) == 6 + (prefix >= 0) for h in hist)
        ids = torch.tensor(hist)
        want = RepetitionPenaltyLogitsProcessor(penalty=1.5)(ids, logits.clone())
        assert torch.equal(processed_scores(logits, hist, SampleSpec(repetition_penalty=1.5)), want)
        ref = _call(logits, SampleSpec(1.0, 0, 1.0, repetition_penalty=1.5, prefix_id=prefix), state=(6, 1), out=out.clone(), max_new=8,
                    uniforms=torch.rand((8, 4), generator=torch.Generator().manual_seed(4)))
        assert torch.equal(ref["scores"].float(), want)
    # only the first `step` ids count
    assert torch.equal(processed_scores(logits, row_history(out, 0, -1), SampleSpec(repetition_penalty=1.5)), logits)


def test_grid_uniforms_give_the_distribution():
    n, vocab = 4096, 1000
    row = torch.randn((1, vocab), generator=torch.Generator().manual_seed(5)) * 3
    spec = SampleSpec(0.7, 50, 0.9)
    u = ((torch.arange(n, dtype=torch.float64) + 0.5) / n).view(1, n)
    ref = _call(row.expand(n, vocab), spec, uniforms=u, max_new=1)
    w = ref["scores"][0]
    prob = torch.where(torch.isfinite(w), torch.exp(w - w.max()), torch.zeros_like(w))
    prob = prob / prob.sum()
    counts = torch.bincount(ref["drawn"], minlength=vocab).double()
    assert float((counts - n * prob).abs().max()) <= 1.0
    assert bool(draw_ok(torch.isfinite(ref["scores"]), ref["scores"], u[0], ref["drawn"], 1e-12).all())


def test_top_k_1_is_the_arg_max_and_the_bookkeeping():
    logits = torch.randn((5, 1000), generator=torch.Generator().manual_seed(6)) * 3
    eos = int(logits[1].argmax())
    fin = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8)
    out = torch.full((5, 4), -7, dtype=torch.int64)
    ref = _call(logits, SampleSpec(1.0, 1, 1.0, eos=(999, eos), pad_id=3), state=(2, 1), out=out, finished=fin)
    assert torch.equal(ref["drawn"], logits.argmax(dim=1))
    want = logits.argmax(dim=1)
    want[2] = 3  # a finished row emits the pad id
    assert torch.equal(ref["tokens"], want) and torch.equal(ref["out_tokens"][:, 2], want) and bool((ref["out_tokens"][:, [0, 1, 3]] == -7).all())
    assert ref["finished"].tolist() == [0, 1, 1, 0, 0] and ref["state"] == [3, 1]
    after = _call(logits, SampleSpec(1.0, 1, 1.0, eos=(999, eos), pad_id=3), state=(3, 1), out=out, finished=fin, step_offset=-1, finalize=0)
    assert torch.equal(after["out_tokens"], ref["out_tokens"]) and after["state"] == [3, 1]
    # min_new: the EOS ids cannot be drawn below it
    banned = _call(logits, SampleSpec(1.0, 1, 1.0, eos=(999, eos), pad_id=3, min_new=3), state=(2, 1), out=out, finished=fin)
    assert int(banned["drawn"][1]) != eos and not bool(torch.isfinite(banned["scores"][:, [999, eos]]).any())
    assert banned["finished"].tolist() == [0, 0, 1, 0, 0]
    allfin = _call(logits[:2], SampleSpec(1.0, 1, 1.0, eos=(int(logits[0].argmax()), eos)), out=out[:2].clone())
    assert allfin["state"] == [1, 0]


def test_library_exports_exactly_the_header():
    """libeilev_hip_sample.so: the entry points of include/eilev_sample.h = abi.SAMPLE_EXPORTS = the library's dynamic symbols; checked in a
    child process (mapping a HIP library into this one would pick the HIP runtime for the whole test process)."""
    import ctypes
    import os
    import re
    import shutil
    import subprocess
    import sys

    from eilev_amd import abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "eilev_sample.h")).read()
    assert sorted(set(re.findall(r"\b(eilev_sample_\w+)\s*\(", header))) == sorted(abi.SAMPLE_EXPORTS)
    assert int(re.search(r"#define EILEV_SAMPLE_ABI_VERSION (\d+)", header).group(1)) == abi.SAMPLE_ABI_VERSION
    assert int(re.search(r"#define EILEV_SAMPLE_MAX_EOS (\d+)", header).group(1)) == abi.SAMPLE_MAX_EOS
    assert ctypes.sizeof(abi.SampleParams) == 4 * 4 + 3 * 8 + 8 * abi.SAMPLE_MAX_EOS + 2 * 8 + 2 * 4
    assert os.path.exists(abi.SAMPLE_LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    code = ("import ctypes, sys; sys.path.insert(0, %r); from eilev_amd import abi; h = ctypes.CDLL(abi.SAMPLE_LIB_PATH); "
            "assert all(hasattr(h, s) for s in abi.SAMPLE_EXPORTS); assert h.eilev_sample_abi_version() == abi.SAMPLE_ABI_VERSION; "
            "h.eilev_sample_scratch_bytes.restype = ctypes.c_size_t; assert h.eilev_sample_scratch_bytes(ctypes.c_int64(32), ctypes.c_int64(50272)) == 0") % root
    subprocess.check_call([sys.executable, "-c", code])
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", abi.SAMPLE_LIB_PATH], text=True)
        syms = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-2] in ("T", "t"))
        assert syms == sorted(abi.SAMPLE_EXPORTS), syms
    p = abi.sample_params(0.7, 0, 0.9, 1.5, 2, 64, [2, 5], 1, 0, -1, 0)
    assert (round(p.temperature, 6), p.top_k, round(p.top_p, 6), p.repetition_penalty, p.min_new, p.max_new, p.n_eos, list(p.eos)[:2], p.pad_id,
            p.prefix_id, p.step_offset, p.finalize) == (0.7, 0, 0.9, 1.5, 2, 64, 2, [2, 5], 1, 0, -1, 0)
    with pytest.raises(NotImplementedError):
        abi.sample_params(eos_ids=list(range(9)))
    assert abi.sample_supported(50272) and abi.sample_supported(32128) and not abi.sample_supported(1002) and not abi.sample_supported(65540)
