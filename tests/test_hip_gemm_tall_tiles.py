"""The tall tiles of the persistent GEMM's 16 x 16 instances (csrc/gemm_pp4.h TALL, csrc/gemm_common.h tile_coords_tall): where N % 256 == 128
the half column is covered by tiles of 384 rows x 128 columns, dealt with the group of four row tiles they start in.  Every case is one launch through the probe
entry eilev_debug_gemm, judged like tests/test_hip_gemm_wide.py judges its launches, on the cases, the float64 reference and the bound of
tests/gemm_ref.py: the form that ran is the one gemm_ref.expected names (and is a half-column instance: pp4-lean16ht / pp4-stats-lean16ht);
the exact family (integer operands: every fp32 partial sum is exact in any order) matches the reference bit for bit, outputs and (sum, sum of
squares) pairs alike; the bounded family stays within gemm_ref.tol / stat_ref; every word of C outside the M x N output (ldc > N, the guard
rows) and every statistics slot at or past N or row past M still holds its NaN sentinel.  No output is left out of a comparison.

Shapes: M = 43 776 + r is the smallest row count that reaches the persistent kernel at N = 1408 on 256 CUs (171 x 6 = 1026 tiles of 256 x 256);
K < 256 keeps N = 384 (one whole column + the half column) on it too.  r in {0, 1, 127, 255, 256, 257, 383} puts the last tall tile at 1 ..
383 valid rows with M % 256 and M % 384 in different combinations (43 776 = 114 x 384 = 171 x 256: r rows are the last tall tile's and the last
row tile's alike up to 255, from 256 on a further row tile follows the last full one); K = 64 / 128 / 192 is one K-step, two, and an
odd count.  Each r runs at both N with the K and the epilogue (bias / bias + residual in place as the ViT calls it / bias + residual +
statistics with stat_ld = M / ReLU) rotating, so that every r meets two kinds of epilogue, every N every K and every (N, epilogue) pair is
run; the bounded family runs each epilogue once; two cases run the real widths (fc2: K = 6144 with residual + statistics, proj-like:
K = 1408).  ldc = N + 8 and ldr = N + 16 throughout (gemm_ref pads), one case is dense."""
import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import Spec
from test_hip_gemm_wide import Launch, _check_stats, _same_bits

pytestmark = pytest.mark.gpu

M0 = 43776
TAILS = (0, 1, 127, 255, 256, 257, 383)
KS = (64, 128, 192)
EPILOGUES = ("bias", "inplace", "stats", "relu")


def _spec(name, M, N, K, epilogue, family="exact", pad=True):
    kw = dict(family=family, pad=pad)
    if epilogue == "inplace":
        kw.update(resid=True)
    elif epilogue == "stats":
        kw.update(resid=True, stats=True)
    elif epilogue == "relu":
        kw.update(epi=2)
    return Spec(name, M, N, K, **kw)


def _cases():
    out = []
    for ni, N in enumerate((384, 1408)):
        for i, r in enumerate(TAILS):
            e = EPILOGUES[(i + 2 * ni) % 4]
            out.append((f"n{N}-r{r}-k{KS[(i + ni) % 3]}-{e}", M0 + r, N, KS[(i + ni) % 3], e, "exact", True))
    # every epilogue on dense random operands, a tail in the last tall tile each; the statistics also at N = 1408
    for i, (e, r) in enumerate(zip(EPILOGUES, (383, 1, 257, 127))):
        out.append((f"bounded-n384-r{r}-{e}", M0 + r, 384, KS[i % 3], e, "bounded", True))
    out.append(("bounded-n1408-r383-stats", M0 + 383, 1408, 128, "stats", "bounded", True))
    out.append(("dense-n1408-r129-inplace", M0 + 129, 1408, 64, "inplace", "exact", False))
    # the real widths
    out.append(("fc2-k6144-stats", M0, 1408, 6144, "stats", "exact", True))
    out.append(("proj-k1408-bias", M0, 1408, 1408, "bias", "exact", True))
    return out


CASES = _cases()


def test_the_case_list_covers_what_it_claims():
    exact = [c for c in CASES if c[5] == "exact" and c[3] in KS]
    for N in (384, 1408):
        assert {c[1] - M0 for c in exact if c[2] == N} >= set(TAILS)
        assert {c[4] for c in exact if c[2] == N} == set(EPILOGUES)
        assert {c[3] for c in exact if c[2] == N} == set(KS)
    for r in TAILS:
        assert len({c[4] for c in exact if c[1] == M0 + r}) == 2
    assert {c[4] for c in CASES if c[5] == "bounded"} == set(EPILOGUES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tall_tiles(probes, case):
    name, M, N, K, epilogue, family, pad = case
    sp = _spec(name, M, N, K, epilogue, family, pad)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = R.build_case(sp)
    if epilogue == "stats":
        c.stat_ld = M  # slot after slot, as the ViT blocks lay the statistics out (gemm_ref's default leaves 8 sentinel rows between slots)
    y, S, _ = R.reference(c)
    want_rc, want_form = R.expected(sp, n_cu)
    assert want_rc == R.OK
    fam = R.family_of(want_form)
    assert fam == ("pp4-stats-lean16ht" if epilogue == "stats" else "pp4-lean16ht"), f"{name}: {fam} is not the instance with the tall tiles"
    L = Launch(c)
    if epilogue == "inplace":  # C == resid: the output rows start out as the residual, everything around them stays poisoned
        L.out.view(-1, c.ldc)[:M, :N] = L.keep["resid"][:M, :N]
        L.args.resid, L.args.ldr = L.args.C, c.ldc
    rc = L.launch(probes)
    assert rc == R.OK, (name, rc)
    assert L.form.value == want_form, f"{name}: launched {R.form_name(L.form.value)}, the dispatch mirror says {R.form_name(want_form)}"
    got, intact = L.output()
    assert intact, f"{name}: a write outside the rows and columns of the output"
    if family == "exact":
        same = _same_bits(got, y.astype(np.float32))
        if not same.all():
            i, j = np.argwhere(~same)[0]
            pytest.fail(f"{name}: {int((~same).sum())} of {same.size} elements differ on the exact family, first at [{i}, {j}]: got {got[i, j]}, ref {y[i, j]}")
    else:
        rt = R.ratio(np.abs(got.astype(np.float64) - y), R.tol(c, y, S, want_form))
        worst = float(rt.max())
        print(f"{name}: {R.form_name(want_form)} err/tol {worst:.3f}")
        if not worst <= 1.0:
            i, j = np.unravel_index(np.argmax(rt), rt.shape)
            pytest.fail(f"{name}: err/tol {worst:.3g} at [{i}, {j}] (got {got[i, j]}, ref {y[i, j]}); {int((rt > 1).sum())} of {rt.size} elements beyond tol")
    if epilogue == "stats":
        _check_stats(L, c, y, S, fam)
