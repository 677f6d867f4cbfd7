"""CPU checks of tests/bwd_ref.py, the reference of the backward-kernel GPU tests (test_hip_bwd.py):
 * the float64 references are torch.autograd's float64 gradients of the documented operations (so the GPU test's reference is independent of the
   fp32 oracle and of the kernels);
 * the fp32 / bf16 restatement of every kernel stays within the derived per-element bound on EVERY launch the GPU test makes: the bound is met
   by correct arithmetic, and the explicit fp32 terms stay below the share the derivation gives them;
 * each planted mistake, applied to the restatement, is detected (err / tol > 1, a broken sentinel or a broken exact-zero rule) by the GPU case
   bwd_ref.DETECTED_BY names for it."""
import numpy as np
import pytest
import torch

import bwd_ref as R

SPECS = R.attn_specs()
BY_NAME = {sp.name: sp for sp in SPECS}
f64 = np.float64


def _autograd_attention(c):
    sp = c.spec
    t = lambda x: torch.tensor(x.astype(f64), requires_grad=True)
    Q, K, V = t(c.Q), t(c.K), t(c.V)
    s = float(c.scale) * (Q @ K.transpose(-1, -2))
    if c.rel_flat is not None:
        s = s + torch.tensor(np.stack([R.bias(c, h) for h in range(sp.heads)]).astype(f64))[None]
    vis = torch.tensor(np.stack([R.visible(c, b) for b in range(sp.batch)]))[:, None]
    p = torch.nan_to_num(torch.softmax(s.masked_fill(~vis, float("-inf")), -1), nan=0.0)
    if sp.drop > 0:
        idx = np.arange(sp.batch * sp.heads * sp.sq * sp.skv).reshape(sp.batch, sp.heads, sp.sq, sp.skv)
        p = p * torch.tensor(R.keep_mask(c.drop_seed, idx, sp.drop).astype(f64) / (1.0 - float(np.float32(sp.drop))))
    o = p @ V
    o.backward(torch.tensor(c.dO.astype(f64)))
    lse = torch.logsumexp(s.masked_fill(~vis, float("-inf")), -1)
    return o.detach().numpy(), Q.grad.numpy(), K.grad.numpy(), V.grad.numpy(), lse.detach().numpy()


AUTOGRAD_CASES = ("db2-plain-64x64-packed", "db2-plain-65x129-kv", "db2-plain-97x40-kv", "db2-leftpad-causal", "db3-dead-entry", "db2-hd8-packed",
                  "db3-rel-tight", "db3-rel-gap", "db3-rel-short", "db4-rel-mask-causal", "db3-drop01", "db3-drop05-mask", "db2-drop05-causal-prefix",
                  "db4-rel-drop", "db3-profile-rise", "db3-profile-late")


@pytest.mark.parametrize("name", AUTOGRAD_CASES)
def test_attention_reference_is_float64_autograd(name):
    c = R.build_case(BY_NAME[name])
    o, dq, dk, dv, lse = _autograd_attention(c)
    c.O = o  # autograd differentiates at its own exact output; the cases carry the bf16 one
    ref = R.reference(c)
    for t, want in (("dq", dq), ("dk", dk), ("dv", dv)):
        np.testing.assert_allclose(ref[t][0], want, rtol=1e-9, atol=1e-11 * max(1.0, np.abs(want).max()))
    dead = R.dead_rows(c)[:, None, :].repeat(c.spec.heads, 1)
    np.testing.assert_allclose(ref["lse"][0][~dead], lse[~dead], rtol=1e-12, atol=1e-12)
    assert (ref["lse"][0][dead] == 1e30).all() and (ref["dq"][0][dead] == 0).all()
    np.testing.assert_allclose(ref["delta"][0], (o * c.dO.astype(f64)).sum(-1), rtol=1e-12, atol=1e-13)


def test_row_references_are_float64_autograd():
    rows, cols = 13, 40
    x, gamma, dy, pg, pb = R.ln_inputs(rows, cols, seed=1)
    ref = R.ln_ref(x, gamma, dy, 1e-5, pg, pb)
    tx, tg, tb = (torch.tensor(a.astype(f64), requires_grad=True) for a in (x, gamma, np.zeros(cols)))
    torch.nn.functional.layer_norm(tx, (cols,), tg, tb, 1e-5).backward(torch.tensor(dy.astype(f64)))
    np.testing.assert_allclose(ref["dx"][0], tx.grad.numpy(), rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(ref["dgamma"][0] - pg, tg.grad.numpy(), rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(ref["dbeta"][0] - pb, tb.grad.numpy(), rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(R.colsum_ref(dy, pb)[0] - pb, dy.astype(f64).sum(0), rtol=1e-12, atol=1e-12)
    ref = R.rms_ref(x, gamma, dy, 1e-6)
    tx = torch.tensor(x.astype(f64), requires_grad=True)
    ty = torch.tensor(gamma.astype(f64)) * (tx * torch.rsqrt(tx.pow(2).mean(-1, keepdim=True) + 1e-6))  # T5LayerNorm
    ty.backward(torch.tensor(dy.astype(f64)))
    np.testing.assert_allclose(ref["y"][0], ty.detach().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["dx"][0], tx.grad.numpy(), rtol=1e-8, atol=1e-9)
    pre, g = x.reshape(-1), dy.reshape(-1)
    for kind, fn in ((1, torch.nn.functional.gelu), (2, torch.relu)):
        ref = R.act_ref(pre, g, kind)
        tp = torch.tensor(pre.astype(f64), requires_grad=True)
        ty = fn(tp)
        ty.backward(torch.tensor(g.astype(f64)))
        np.testing.assert_allclose(ref["y"][0], ty.detach().numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(ref["dx"][0], tp.grad.numpy(), rtol=1e-10, atol=1e-12)
    f = 24
    ab = R.row_inputs("ab", rows, 2 * f, seed=2, scale=1.5)
    gy = R.row_inputs("gy", rows, f, seed=2)
    ref = R.gated_ref(ab, gy, f)
    tab = torch.tensor(ab.astype(f64), requires_grad=True)
    a, b = tab[:, :f], tab[:, f:]
    tout = 0.5 * a * (1.0 + torch.tanh(0.79788456080286535588 * (a + 0.044715 * a.pow(3)))) * b  # NewGELUActivation * the linear branch
    tout.backward(torch.tensor(gy.astype(f64)))
    np.testing.assert_allclose(ref["out"][0], tout.detach().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["dab"][0], tab.grad.numpy(), rtol=1e-10, atol=1e-12)
    logits, tgt, gs = R.ce_inputs(211, seed=3)
    ref = R.ce_ref(logits, tgt, gs)
    live = (tgt >= 0) & (tgt < 211)
    tl = torch.tensor(logits.astype(f64), requires_grad=True)
    loss = torch.nn.functional.cross_entropy(tl[live], torch.tensor(tgt[live]), reduction="none")
    (loss.sum() * float(gs)).backward()
    np.testing.assert_allclose(ref["loss"][0][live], loss.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["dlogits"][0], tl.grad.numpy(), rtol=1e-10, atol=1e-300)
    assert (ref["loss"][0][~live] == 0).all() and (ref["dlogits"][0][~live] == 0).all() and (~live).sum() == 2


def test_instance_selection_and_coverage():
    assert [R.instance(R.Spec("x", hd=hd))[0] for hd in (8, 64, 72, 96, 104, 128)] == [2, 2, 3, 3, 4, 4]
    assert R.instance(R.Spec("x", rel="tight"))[1] and R.instance(R.Spec("x", drop=0.1))[1] and not R.instance(R.Spec("x"))[1]
    cov = R.assert_coverage(SPECS)
    assert len(cov) == 18
    hds = {sp.hd for sp in SPECS}
    assert hds >= {8, 24, 64, 72, 80, 88, 96, 104, 128}
    for db in (2, 3, 4):
        mine = [sp for sp in SPECS if R.instance(sp)[0] == db]
        assert {(sp.sq, sp.skv) for sp in mine} >= set(R.SHAPES)
        assert {sp.rel for sp in mine} >= {"tight", "gap", "short"} and {sp.drop for sp in mine} >= {0.1, 0.5}
        assert {sp.profile for sp in mine} >= {"rise", "fall", "late", "hi", "lo"}
        assert any("dead" in sp.mask for sp in mine) and any(sp.causal and sp.sq > sp.skv for sp in mine)
        assert {R.entry_of(sp, k) for k, sp in enumerate(SPECS) if R.instance(sp) == (db, False)} == {"plain", "rel", "dropout"}


def test_profiles_move_the_running_maximum_by_more_than_20():
    """Tile to tile (rise, fall), lane half to lane half and wave to wave (late: one key; hi / lo: one 32-key block)."""
    for db in (2, 3, 4):
        for prof in ("rise", "fall", "late", "hi", "lo"):
            c = R.build_case(BY_NAME[f"db{db}-profile-{prof}"])
            s = R._softmax(c, 0, 0)[0]
            tiles = [s[:, t * 64:(t + 1) * 64].max(1) for t in range(3)]
            if prof in ("rise", "fall"):
                assert (np.abs(tiles[1] - tiles[0]) > 20).all() and (np.abs(tiles[2] - tiles[1]) > 20).all()
            elif prof == "late":
                j = (4 * c.spec.skv) // 5
                assert (s[:, j] - np.delete(s, j, 1).max(1) > 20).all()
            else:
                blk = slice(96, 128) if prof == "hi" else slice(64, 96)
                other = slice(64, 96) if prof == "hi" else slice(96, 128)
                assert (s[:, blk].max(1) - s[:, other].max(1) > 20).all() and (s[:, blk].max(1) - tiles[0] > 20).all()


@pytest.mark.parametrize("db", [2, 3, 4])
def test_restatement_within_the_bound_on_every_gpu_launch(db):
    worst, share = {}, 0.0
    for sp in SPECS:
        if R.instance(sp)[0] != db:
            continue
        c = R.build_case(sp)
        ref = R.reference(c)
        P = R.pack(c)
        ratios, intact, exact, _ = R.check(c, P, R.emulate(c, P), ref)
        assert intact and exact, sp.name
        for t, v in ratios.items():
            assert v <= 1.0, (sp.name, t, v)
            worst[t] = max(worst.get(t, 0.0), v)
        share = max(share, R.fp32_share(ref))
        assert share <= R.FP32_SHARE, (sp.name, share)
    print(f"DB {db}: restatement worst err/tol {worst}, fp32 share 2^{np.log2(share):.1f}")
    assert max(worst[t] for t in ("dq", "dk", "dv")) > 0.5, "the bound is several times what correct arithmetic needs"


@pytest.mark.parametrize("mut", R.ATTN_MUTATIONS)
def test_planted_attention_mistake_is_detected(mut):
    name = R.DETECTED_BY[mut]
    c = R.build_case(BY_NAME[name])
    ref = R.reference(c)
    P = R.pack(c)
    ratios, intact, exact, _ = R.check(c, P, R.emulate(c, P, mut), ref)
    print(f"{mut} on {name}: " + " ".join(f"{t} {v:.3g}" for t, v in ratios.items()) + f" intact {intact} exact {exact}")
    assert max(ratios.values()) > 1.0 or not intact or not exact, (mut, name, ratios)


def test_restatement_of_the_row_kernels_within_the_bound_and_their_planted_mistakes():
    for cols in R.LN_COLS + (40,):
        for rows in ((4100,) if cols == 40 else R.LN_ROWS):
            x, gamma, dy, pg, pb = R.ln_inputs(rows, cols, seed=cols + rows)
            ref = R.ln_ref(x, gamma, dy, 1e-5, pg, pb)
            em = R.ln_emulate(x, gamma, dy, 1e-5, pg, pb)
            for k in ("dx", "mean", "rstd"):
                assert R.ratio(em[k], *ref[k]) <= 1.0, (rows, cols, k)
            for k in ("dgamma", "dbeta"):
                assert R.ratio(em[k][:cols], *ref[k]) <= 1.0 and (em[k][cols:] == R.SENTF).all(), (rows, cols, k)
            x, gamma, dy, _, _ = R.ln_inputs(rows, cols, seed=7 * cols + rows)
            ref, em = R.rms_ref(x, gamma, dy, 1e-6), R.rms_emulate(x, gamma, dy, 1e-6)
            assert R.ratio(em["y"], *ref["y"]) <= 1.0 and R.ratio(em["dx"], *ref["dx"]) <= 1.0, (rows, cols)
    # LayerNorm variance in one pass on x = 100 + noise: caught by the rstd statistic of layernorm_bwd 67 x 1000
    x, gamma, dy, pg, pb = R.ln_inputs(67, 1000, seed=1067)
    ref, em = R.ln_ref(x, gamma, dy, 1e-5, pg, pb), R.ln_emulate(x, gamma, dy, 1e-5, pg, pb, "onepass")
    assert R.ratio(em["rstd"], *ref["rstd"]) > 1.0
    # col_reduce without its c < cols guard: the sentinels behind dgamma / dbeta of layernorm_bwd 5 x 1000 (1000 % 32 = 8)
    x, gamma, dy, pg, pb = R.ln_inputs(5, 1000, seed=1005)
    em = R.ln_emulate(x, gamma, dy, 1e-5, pg, pb, "noguard")
    assert not (em["dgamma"][1000:] == R.SENTF).all() and not (em["dbeta"][1000:] == R.SENTF).all()
    for vocab in R.CE_VOCABS:
        logits, tgt, gs = R.ce_inputs(vocab, seed=vocab)
        ref = R.ce_ref(logits, tgt, gs)
        em = R.ce_emulate(logits, tgt, gs)
        assert R.ratio(em["loss"], *ref["loss"]) <= 1.0 and R.ratio(em["dlogits"], *ref["dlogits"]) <= 1.0, vocab
        for mut in ("inv", "tplus1"):  # every vocab of test_hip_bwd.py::test_ce_loss detects both (the old bound, 8e-3 max|ref|, saw neither "inv")
            assert R.ratio(R.ce_emulate(logits, tgt, gs, mut)["dlogits"], *ref["dlogits"]) > 1.0, (vocab, mut)
    ab = R.row_inputs("ab", 37, 2 * 168, seed=1, scale=1.5)
    dy = R.row_inputs("gy2", 37, 168, seed=1)
    ref, em = R.gated_ref(ab, dy, 168), R.gated_emulate(ab, dy, 168)
    assert R.ratio(em["out"], *ref["out"]) <= 1.0 and R.ratio(em["dab"], *ref["dab"]) <= 1.0
    x, r = R.row_inputs("dx", 1, 6184, seed=5)[0], R.row_inputs("dr", 1, 6184, seed=6)[0]
    for p in (0.1, 0.5):
        for resid in (r, None):
            ref, tol, keep = R.dropout_add_ref(x, resid, p, 777)
            assert R.ratio(R.dropout_add_emulate(x, resid, p, 777), ref, tol) <= 1.0
            assert abs(keep.mean() - (1 - p)) < 0.03
