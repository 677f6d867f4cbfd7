"""Every backward (training) kernel of csrc/backward.hip launched on its own through the public entries and compared, element by element, with
the float64 references of tests/bwd_ref.py under the bounds derived there from the kernels' own roundings (no max-norm tolerance, no floor
beyond the smallest normal fp32).

Attention: the twelve instances attn_bwd_{dq,dkv}_kernel<DB in 2 3 4, EXTRA> are selected by head_dim (<= 64, <= 96, else) and by whether a
position table or dropout is given; bwd_ref.instance() restates that and the last test asserts that each instance was launched in each of the
three layouts ("sep": six distinct leading dimensions; "packed": q|k|v and dq|dk|dv thirds of one buffer at stride 3 W, as train.py's
self-attention passes them; "kv": k|v halves at stride 2 W, as its cross-attention does).  Per launch: err / tol <= 1 on dq, dk, dv, lse and
delta; lse == 1e30 and dq == 0 exactly on rows without a visible key, dk == dv == 0 exactly in a batch entry without one; every sentinel
(stride gaps, the row behind each output, lse_delta beyond 2 B H sq) intact; a second identical launch gives identical bits on all five
outputs; a packed launch gives the bits of the "sep" launch of the same tensors.
Row kernels: layernorm_bwd + col_reduce<true>, colsum, rmsnorm(_bwd), ce_loss, act_fwd / act_bwd, gated_gelu(_bwd), dropout_add: one launch per
shape against float64, the shapes on both sides of every MAXC boundary, of the 32-column block and of the slice caps.

Finding of the repeat launch: before the fixed-order sum of delta's chunks in attn_bwd_dq_kernel, db3-plain-31x33-sep (the first DB = 3 case
with a second launch) differed between two identical launches; DB = 2 and DB = 4 never did.

Which planted mistake each case catches is shown on the CPU by test_bwd_reference.py.  Measured worst err / tol per kernel instance and the
wall time: profiles/parity_r06.json, section bwd (record_parity)."""
import time

import numpy as np
import pytest
import torch

import bwd_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
SPECS = R.attn_specs()
_WORST: dict = {}
_SECONDS: dict = {}
_LAUNCHED: dict = {}
_REPEAT_DIFFERS: list = []


def _hip():
    from eilev_amd import abi

    return abi.load_hip()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _note(kernel, value, t0=None):
    _WORST[kernel] = max(_WORST.get(kernel, 0.0), float(value))
    if t0 is not None:
        _SECONDS[kernel] = _SECONDS.get(kernel, 0.0) + time.time() - t0


def _record():
    from hip_utils import record_parity

    record_parity("bwd", tol="per element, derived in tests/bwd_ref.py: 2^-8 per bf16 rounding on the sum of absolute products + explicit fp32 terms",
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()}, **{f"seconds_{k}": v for k, v in _SECONDS.items()},
                  seconds_total=sum(_SECONDS.values()), attention_repeat_launch_differs=len(_REPEAT_DIFFERS))


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def _launch_attn(hip, c, P, entry):
    """One launch on fresh device copies of the images; returns the output images."""
    sp = c.spec
    dev = {n: torch.from_numpy(a).cuda() for n, a in P.bufs.items()}
    at = lambda t: dev[t[0]].data_ptr() + 2 * t[1]
    mask = dev["mask"].data_ptr() if "mask" in dev else None
    common = (at(P.q), at(P.k), at(P.v), dev["o"].data_ptr(), dev["do"].data_ptr(), at(P.dq), at(P.dk), at(P.dv), dev["ws"].data_ptr(),
              sp.batch, sp.heads, sp.sq, sp.skv, sp.hd, P.q[2], P.k[2], P.v[2], P.dq[2], P.dk[2], P.dv[2], float(c.scale), sp.causal, mask)
    rel = (dev["rel"].data_ptr() + 4 * c.rel_lead, c.rel_hs, c.rel_off, c.rel_n) if "rel" in dev else (None, 0, 0, 0)
    if entry == "plain":
        rc = hip.eilev_attention_bwd(*common, _stream())
    elif entry == "rel":
        rc = hip.eilev_attention_rel_bwd(*common, *rel, _stream())
    else:
        rc = hip.eilev_attention_dropout_bwd(*common, *rel, float(sp.drop), c.drop_seed, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (sp.name, entry, rc)
    return {n: dev[n].cpu().numpy() for n in R.OUT_BUFS if n in dev}


def _worst_element(got, ref, tol):
    err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e300, posinf=1e300, neginf=1e300) - ref) / np.maximum(tol, R.FLT_MIN)
    at = np.unravel_index(np.argmax(err), err.shape)
    return at, got[at], ref[at], tol[at]


@pytest.mark.parametrize("k", range(len(SPECS)), ids=[sp.name for sp in SPECS])
def test_attention_bwd(k):
    sp = SPECS[k]
    hip = _hip()
    t0 = time.time()
    c = R.build_case(sp)
    ref = R.reference(c)
    P = R.pack(c)
    entry = R.entry_of(sp, k)
    db, extra = R.instance(sp)
    kernel = f"attn_bwd<{db},{'extra' if extra else 'plain'}>"
    bufs = _launch_attn(hip, c, P, entry)
    ratios, intact, exact, got = R.check(c, P, bufs, ref)
    print(f"{sp.name}: {kernel} via {entry}: " + " ".join(f"{t} {v:.3f}" for t, v in ratios.items()) + f" intact {intact} exact {exact}")
    again = _launch_attn(hip, c, P, entry)
    same = all(np.array_equal(bufs[n], again[n]) for n in bufs)
    if not same:
        _REPEAT_DIFFERS.append(sp.name)
    sep_same = True
    if sp.layout == "packed":  # the layout must not change the arithmetic
        sp2 = R.replace(sp, layout="sep")
        c2 = R.build_case(sp2)
        P2 = R.pack(c2)
        got2, intact2 = R.unpack(c2, P2, _launch_attn(hip, c2, P2, entry))
        sep_same = intact2 and all(np.array_equal(got[t].view(np.uint32), got2[t].view(np.uint32)) for t in R.TENSORS)
        _LAUNCHED[(db, extra, "sep")] = _LAUNCHED.get((db, extra, "sep"), 0) + 1
    _LAUNCHED[(db, extra, sp.layout)] = _LAUNCHED.get((db, extra, sp.layout), 0) + 1
    _note(kernel, max(ratios.values()), t0)
    _record()
    for t, v in ratios.items():
        if not v <= 1.0:
            g, r, tol = got[t], ref[t][0], ref[t][1]
            at, gv, rv, tv = _worst_element(g, r, tol)
            pytest.fail(f"{sp.name} ({kernel} via {entry}): {t} err/tol {v:.4g} at (b, h, row, d) = {tuple(int(x) for x in at)}: got {gv}, ref {rv}, tol {tv}")
    assert exact, f"{sp.name}: a row without a visible key must give lse 1e30 and exact zeros in dq (and dk / dv of a dead batch entry)"
    assert intact, f"{sp.name}: a sentinel outside the outputs was overwritten"
    assert sep_same, f"{sp.name}: the packed launch and the sep launch of the same tensors differ in bits"
    assert same, f"{sp.name}: two identical launches differ in bits"


def test_every_attention_instance_in_every_layout():
    """The count at the end of the module: the table reaches each of the twelve kernels (six (DB, EXTRA) pairs x dq / dkv, one launch runs both)
    in each layout, and what ran of it did launch them."""
    cov = R.assert_coverage(SPECS)
    ran = sum(v for (db, e, lay), v in _LAUNCHED.items())
    if ran >= len(SPECS):  # the whole module ran
        for key in cov:
            assert _LAUNCHED.get(key, 0) >= cov[key], (key, _LAUNCHED.get(key, 0), cov[key])
    assert not _REPEAT_DIFFERS, _REPEAT_DIFFERS


def test_attention_refusals_write_nothing():
    hip = _hip()
    sp = R.Spec("refuse", hd=80, sq=17, skv=17)
    c = R.build_case(sp)
    P = R.pack(c)
    for change in ({"hd": 12}, {"hd": 136}, {"ldk": P.k[2] + 4}, {"sq": 0}):
        dev = {n: torch.from_numpy(a).cuda() for n, a in P.bufs.items()}
        rc = hip.eilev_attention_bwd(dev["q"].data_ptr(), dev["k"].data_ptr(), dev["v"].data_ptr(), dev["o"].data_ptr(), dev["do"].data_ptr(),
                                     dev["dq"].data_ptr(), dev["dk"].data_ptr(), dev["dv"].data_ptr(), dev["ws"].data_ptr(), sp.batch, sp.heads,
                                     change.get("sq", sp.sq), sp.skv, change.get("hd", sp.hd), P.q[2], change.get("ldk", P.k[2]), P.v[2], P.dq[2], P.dk[2],
                                     P.dv[2], float(c.scale), 0, None, _stream())
        torch.cuda.synchronize()
        assert rc == (-1 if "sq" in change else -2), (change, rc)
        for n in ("dq", "dk", "dv", "ws"):
            assert np.array_equal(dev[n].cpu().numpy(), P.bufs[n]), (change, n)


# ---- row kernels -----------------------------------------------------------------------------------------------------------------------------
def _bf(a, tail=64):
    """bf16 device buffer of a bf16-exact array with `tail` sentinel elements behind."""
    bits = np.concatenate([R.bf16_bits(a).reshape(-1), np.full(tail, np.uint16(R.SENT16).view(np.int16), np.int16)])
    return torch.from_numpy(bits).cuda()


def _out16(n, tail=64):
    return torch.full((n + tail,), int(np.uint16(R.SENT16).view(np.int16)), dtype=torch.int16, device="cuda")


def _f32buf(values, tail=32):
    a = np.full(len(values) + tail, R.SENTF, f32)  # (finite: an atomic add onto a NaN would leave a NaN)
    a[:len(values)] = values
    return torch.from_numpy(a).cuda()


def _read16(t, shape):
    bits = t.cpu().numpy()
    n = int(np.prod(shape))
    return R.bits_to_f32(bits[:n]).reshape(shape), bool((bits[n:].view(np.uint16) == R.SENT16).all())


def _read32(t, n):
    a = t.cpu().numpy()
    return a[:n].copy(), bool((a[n:] == R.SENTF).all())


def _hold(kernel, what, got, ref_tol, intact=True, t0=None):
    ref, tol = ref_tol
    tol = np.broadcast_to(tol, ref.shape)
    v = R.ratio(got, ref, tol)
    _note(kernel, v, t0)
    _record()
    print(f"{what}: {kernel} err/tol {v:.3f}")
    if not v <= 1.0:
        at, gv, rv, tv = _worst_element(got, ref, tol)
        pytest.fail(f"{what}: err/tol {v:.4g} at {tuple(int(x) for x in at)}: got {gv}, ref {rv}, tol {tv}")
    assert intact, f"{what}: a sentinel behind the output was overwritten"


def _ln_launch(hip, x, gamma, dy, pg, pb, eps, train=True):
    rows, cols = x.shape
    dx = _out16(rows * cols)
    dg, db, st = _f32buf(pg), _f32buf(pb), _f32buf(np.zeros(2 * rows, f32))
    xd, gd, dyd = _bf(x), _bf(gamma), _bf(dy)
    if train:
        rc = hip.eilev_layernorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), st.data_ptr(), rows, cols, eps, _stream())
    else:
        rc = hip.eilev_layernorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), None, None, None, rows, cols, eps, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return dx, dg, db, st


@pytest.mark.parametrize("cols", R.LN_COLS + (40,))
def test_layernorm_bwd_and_col_reduce(cols):
    hip = _hip()
    for rows in ((4100,) if cols == 40 else R.LN_ROWS):  # (4100, 40): rows / 64 = 64, the slice cap
        t0 = time.time()
        x, gamma, dy, pg, pb = R.ln_inputs(rows, cols, seed=cols + rows)
        ref = R.ln_ref(x, gamma, dy, 1e-5, pg, pb)
        dx, dg, db, st = _ln_launch(hip, x, gamma, dy, pg, pb, 1e-5)
        what = f"layernorm_bwd {rows}x{cols}"
        gdx, ok = _read16(dx, (rows, cols))
        _hold("layernorm_bwd", what + " dx", gdx, ref["dx"], ok, t0)
        for name, t in (("dgamma", dg), ("dbeta", db)):
            g, ok = _read32(t, cols)
            _hold("col_reduce<ln>", f"{what} {name}", g, ref[name], ok)
        g, ok = _read32(st, 2 * rows)
        _hold("layernorm_bwd", what + " mean", g[0::2], ref["mean"], ok)
        _hold("layernorm_bwd", what + " rstd", g[1::2], ref["rstd"])
        dx2 = _ln_launch(hip, x, gamma, dy, pg, pb, 1e-5, train=False)[0]
        assert torch.equal(dx, dx2), f"{what}: the frozen form gives other dx bits"


def test_layernorm_bwd_refusals_write_nothing():
    hip = _hip()
    rows = 5
    for cols, trio, want in ((1004, 7, -2), (4104, 7, -2), (1000, 1, -1), (1000, 2, -1), (1000, 3, -1), (1000, 5, -1), (1000, 6, -1)):
        x, gamma, dy, pg, pb = R.ln_inputs(rows, cols, seed=3)
        dx, dg, db, st = _out16(rows * cols), _f32buf(pg), _f32buf(pb), _f32buf(np.zeros(2 * rows, f32))
        keep = [t.clone() for t in (dx, dg, db, st)]
        xd, gd, dyd = _bf(x), _bf(gamma), _bf(dy)
        rc = hip.eilev_layernorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), dg.data_ptr() if trio & 1 else None,
                                     db.data_ptr() if trio & 2 else None, st.data_ptr() if trio & 4 else None, rows, cols, 1e-5, _stream())
        torch.cuda.synchronize()
        assert rc == want, (cols, trio, rc)
        for a, b in zip((dx, dg, db, st), keep):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), (cols, trio)


@pytest.mark.parametrize("rows,cols", [(67, 1), (67, 33), (67, 1000), (16390, 40)])
def test_colsum(rows, cols):
    hip = _hip()
    t0 = time.time()
    dy = R.row_inputs("cs", rows, cols, seed=cols)
    prior = R.row_inputs("csp", 1, cols, seed=cols)[0]
    out, dyd = _f32buf(prior), _bf(dy)
    rc = hip.eilev_colsum(dyd.data_ptr(), out.data_ptr(), rows, cols, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    g, ok = _read32(out, cols)
    _hold("col_reduce<colsum>", f"colsum {rows}x{cols}", g, R.colsum_ref(dy, prior), ok, t0)


@pytest.mark.parametrize("cols", R.LN_COLS)
def test_rmsnorm_and_bwd(cols):
    hip = _hip()
    for rows in R.LN_ROWS:
        t0 = time.time()
        x, gamma, dy, _, _ = R.ln_inputs(rows, cols, seed=7 * cols + rows)
        ref = R.rms_ref(x, gamma, dy, 1e-6)
        y, dx = _out16(rows * cols), _out16(rows * cols)
        xd, gd, dyd = _bf(x), _bf(gamma), _bf(dy)
        assert hip.eilev_rmsnorm(xd.data_ptr(), gd.data_ptr(), y.data_ptr(), rows, cols, 1e-6, _stream()) == 0
        assert hip.eilev_rmsnorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), rows, cols, 1e-6, _stream()) == 0
        torch.cuda.synchronize()
        g, ok = _read16(y, (rows, cols))
        _hold("rmsnorm", f"rmsnorm {rows}x{cols} y", g, ref["y"], ok, t0)
        g, ok = _read16(dx, (rows, cols))
        _hold("rmsnorm_bwd", f"rmsnorm_bwd {rows}x{cols} dx", g, ref["dx"], ok)


@pytest.mark.parametrize("vocab", R.CE_VOCABS)
def test_ce_loss(vocab):
    hip = _hip()
    t0 = time.time()
    logits, tgt, gs = R.ce_inputs(vocab, seed=vocab)
    rows = len(tgt)
    ref = R.ce_ref(logits, tgt, gs)
    lg, tg = torch.from_numpy(logits).cuda(), torch.from_numpy(tgt).cuda()
    loss, dl = _f32buf(np.zeros(rows, f32)), _out16(rows * vocab)
    assert hip.eilev_ce_loss(lg.data_ptr(), tg.data_ptr(), float(gs), loss.data_ptr(), dl.data_ptr(), rows, vocab, _stream()) == 0
    torch.cuda.synchronize()
    g, ok = _read32(loss, rows)
    _hold("ce_loss", f"ce_loss vocab {vocab} row_loss", g, ref["loss"], ok, t0)
    gd, ok = _read16(dl, (rows, vocab))
    _hold("ce_loss", f"ce_loss vocab {vocab} dlogits", gd, ref["dlogits"], ok)
    dead = (tgt < 0) | (tgt >= vocab)
    assert (g[dead] == 0).all() and (gd[dead] == 0).all(), "ignored and out-of-range targets give zeros and loss 0"
    loss2, poisoned = _f32buf(np.zeros(rows, f32)), _out16(rows * vocab)  # dlogits == NULL: loss only; the poisoned buffer is passed nowhere
    assert hip.eilev_ce_loss(lg.data_ptr(), tg.data_ptr(), float(gs), loss2.data_ptr(), None, rows, vocab, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), "row_loss differs when dlogits is null"
    assert (poisoned.cpu().numpy().view(np.uint16) == R.SENT16).all()


N_ELT = 8 * (3 * 256 + 5)  # the last 256-thread block has 5 live threads


@pytest.mark.parametrize("kind", [1, 2])
def test_act_fwd_and_bwd(kind):
    hip = _hip()
    t0 = time.time()
    pre = R.row_inputs("pre", 1, N_ELT, seed=kind, scale=2.0)[0]
    pre[:16] = np.linspace(-7, 7, 16).astype(f32)
    pre = R.round_bf16(pre)
    dy = R.row_inputs("gy", 1, N_ELT, seed=kind)[0]
    ref = R.act_ref(pre, dy, kind)
    y, dx, pd, dyd = _out16(N_ELT), _out16(N_ELT), _bf(pre), _bf(dy)
    assert hip.eilev_act_fwd(pd.data_ptr(), y.data_ptr(), N_ELT, kind, _stream()) == 0
    assert hip.eilev_act_bwd(pd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), N_ELT, kind, _stream()) == 0
    torch.cuda.synchronize()
    g, ok = _read16(y, (N_ELT,))
    _hold("act_fwd", f"act_fwd kind {kind}", g, ref["y"], ok, t0)
    g, ok = _read16(dx, (N_ELT,))
    _hold("act_bwd", f"act_bwd kind {kind}", g, ref["dx"], ok)


def test_gated_gelu_and_bwd():
    hip = _hip()
    t0 = time.time()
    rows, f = 37, 168  # rows * f / 8 = 777 chunks: the last block is partly filled
    ab = R.row_inputs("ab", rows, 2 * f, seed=1, scale=1.5)
    dy = R.row_inputs("gy2", rows, f, seed=1)
    ref = R.gated_ref(ab, dy, f)
    out, dab, abd, dyd = _out16(rows * f), _out16(rows * 2 * f), _bf(ab), _bf(dy)
    assert hip.eilev_gated_gelu(abd.data_ptr(), out.data_ptr(), rows, f, _stream()) == 0
    assert hip.eilev_gated_gelu_bwd(abd.data_ptr(), dyd.data_ptr(), dab.data_ptr(), rows, f, _stream()) == 0
    torch.cuda.synchronize()
    g, ok = _read16(out, (rows, f))
    _hold("gated_gelu", "gated_gelu", g, ref["out"], ok, t0)
    g, ok = _read16(dab, (rows, 2 * f))
    _hold("gated_gelu_bwd", "gated_gelu_bwd", g, ref["dab"], ok)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_add(p):
    hip = _hip()
    t0 = time.time()
    seed = 777
    x = R.row_inputs("dx", 1, N_ELT, seed=5)[0]
    r = R.row_inputs("dr", 1, N_ELT, seed=6)[0]
    xd, rd = _bf(x), _bf(r)
    for resid in (r, None):
        y = _out16(N_ELT)
        assert hip.eilev_dropout_add(xd.data_ptr(), rd.data_ptr() if resid is not None else None, y.data_ptr(), N_ELT, p, seed, _stream()) == 0
        torch.cuda.synchronize()
        ref, tol, keep = R.dropout_add_ref(x, resid, p, seed)
        g, ok = _read16(y, (N_ELT,))
        _hold("dropout_add", f"dropout_add p {p} resid {resid is not None}", g, (ref, tol), ok, t0)
        if resid is None:
            assert np.array_equal(g == 0, ~keep | (x == 0)), "not the documented mask"
