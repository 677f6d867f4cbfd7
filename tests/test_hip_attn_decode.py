"""Every decode-attention kernel of csrc/attn_decode.hip, launched on its own through the probe entry eilev_debug_attn_decode and compared
with the float64 reference of tests/attn_decode_ref.py.

Why this is tighter than test_hip_kernels.py (1e-2 max|ref| for attention): that bound serves whole attention layers with random inputs,
where a dropped, doubled or mis-addressed key moves a row by ~1/N of a value and disappears in it.  Here the bound is derived from the
kernels' own arithmetic — tol_i = (2^-8 + 2^-11) A_i, A_i = sum_j p_j |v_ji| / sum_j p_j (bf16 P, bf16 output, fp32 terms; no absolute
floor) — and the inputs plant one key of softmax weight 0.5 and values +-8 per (row, head), so that ONE wrong key index is tens to
hundreds of tol (test_attn_decode_reference.py measures it on the CPU), and traps (score + 30, values +-64, or NaN bits) on every key
that must not be seen: masked prompt keys and the never-zeroed cache slots at and beyond kv_total.

form                                   selected by                                                     footprint in `part`
attn_decode1_kernel<10,12> / <8,8>     launcher 1, batch <= 8, cap <= 1024                             untouched
attn_decode_part_kernel<10,6>          launcher 2; launcher 0 below two workgroups per CU              128-key records
attn_decode_part_kernel<10,11,..,256>  eilev_debug_attn_part32(2)                                      256-key records (*)
attn_decode_loop_kernel<10,11,256>     batch * heads >= 2 CUs, or eilev_debug_attn_part32(3)           untouched
attn_decode_loop_kernel<8,8,256>       hd 64, batch * heads >= 2 CUs                                   untouched
attn_decode_part_kernel<10,6,true>     anc set, batch <= 8                                             128-key records
attn_decode_split_kernel               eilev_debug_attn_part32(0) / eilev_debug_beam_part(0) / rest    256-key records (*)
attn_decode_merge_kernel               every form that leaves records and is given `out`
(*) the 256-key range kernel and the split kernel leave the same records: between those two the test relies on the forcing switch.
The one-pass and the loop kernels both leave `part` untouched; they are told apart by the launcher (1 never reaches the loop) and by the
capacity (the cover and sweep cases of the loop go to 2048 keys, which the one-pass kernel cannot hold).

Not run on the GPU, checked by reading the code: ancestry entries outside [0, rows) (clamped in key_row of both beam kernels), a beam
state[0] of 0 or above cap_g (kv_total is clamped to seq_len + cap_g and slot_new becomes -1: no store), seq_len + state[0] > cap
(kv_total = min(cap, ...) in every kernel).  A broken guard would write out of bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_decode_ref as R
from attn_decode_ref import Spec

pytestmark = pytest.mark.gpu

EILEV_OK, EILEV_E_BADARG, EILEV_E_UNSUPPORTED, EILEV_E_WORKSPACE = 0, -1, -2, -3
SENT32 = 0x7FA5A5A5  # poison of `part` (a NaN as float)
SENT16 = 0x7FA5      # poison of `out` (a NaN as bf16)


class AttnDecodeArgs(C.Structure):
    """ctypes mirror of EilevDebugAttnDecodeArgs (csrc/attn_decode.hip, probe build): DecodeAttnArgs as plain pointers and integers."""
    _fields_ = [("qkv", C.c_void_p), ("ldq", C.c_int64), ("kc", C.c_void_p), ("vc", C.c_void_p), ("out", C.c_void_p), ("attn_mask", C.c_void_p),
                ("state", C.c_void_p), ("batch", C.c_int32), ("seq_len", C.c_int32), ("cap", C.c_int32), ("heads", C.c_int32), ("hd", C.c_int32),
                ("fuse_new", C.c_int32), ("part", C.c_void_p), ("part_bytes", C.c_uint64), ("rel_tab", C.c_void_p), ("rel_hs", C.c_int64),
                ("rel_off", C.c_int32), ("beams", C.c_int32), ("kg", C.c_void_p), ("vg", C.c_void_p), ("anc", C.c_void_p), ("cap_g", C.c_int32),
                ("out_frag", C.c_int32)]


_WORST: dict = {}
_VISITED: dict = {}


def _entry(lib):
    fn = lib.eilev_debug_attn_decode
    fn.argtypes = [C.POINTER(AttnDecodeArgs), C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    fn.restype = C.c_int
    return fn


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev_bits(a):
    """A bf16-exact float32 array (NaN allowed) -> device bf16 tensor with exactly those bits."""
    return torch.from_numpy(R.bf16_bits(a)).cuda().view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def part_bytes(sp: Spec, rng: int) -> int:
    keys = sp.seq_len + sp.cap_g if sp.beams else sp.cap
    return 4 * sp.batch * sp.heads * (-(-keys // rng)) * (sp.hd + 2)


class Launch:
    """The device buffers of one case, poisoned; launch() runs the entry under the case's switches (restored afterwards)."""

    def __init__(self, lib, c):
        sp = self.sp = c.spec
        self.lib, self.c = lib, c
        self.qkv = _dev_bits(c.qkv)
        self.kc, self.vc = _dev_bits(c.kc), _dev_bits(c.vc)
        self.kg = _dev_bits(c.kg) if c.beam else None
        self.vg = _dev_bits(c.vg) if c.beam else None
        self.anc = torch.from_numpy(c.anc).cuda().contiguous() if c.beam else None
        self.mask = torch.from_numpy(c.mask).cuda().contiguous() if c.mask is not None and c.mask.size else None
        self.state = None if sp.n_gen is None else torch.tensor([sp.n_gen], dtype=torch.int32, device="cuda")
        self.rel = torch.from_numpy(c.rel_tab).cuda().contiguous() if c.rel_tab is not None else None
        self.part = torch.full((part_bytes(sp, 128) // 4 + 64,), SENT32, dtype=torch.int32, device="cuda")
        self.out = torch.full(((32 if sp.out_frag else sp.batch) * c.d,), SENT16, dtype=torch.int16, device="cuda")
        self.nsplit = C.c_int(-1)
        a = self.args = AttnDecodeArgs()
        a.qkv, a.ldq = self.qkv.data_ptr(), (0 if sp.ldq_extra < 0 else c.ldq)
        a.kc, a.vc = self.kc.data_ptr(), self.vc.data_ptr()
        a.out = None if (sp.out_null or sp.launcher == 2) else self.out.data_ptr()
        a.attn_mask, a.state = _ptr(self.mask), _ptr(self.state)
        a.batch, a.seq_len, a.cap, a.heads, a.hd, a.fuse_new = sp.batch, sp.seq_len, sp.cap, sp.heads, sp.hd, sp.fuse_new
        a.part = self.part.data_ptr()
        a.part_bytes = part_bytes(sp, sp.part_short) - 1 if sp.part_short else part_bytes(sp, 128)
        a.rel_tab, a.rel_hs, a.rel_off = _ptr(self.rel), c.rel_hs, c.rel_off
        a.beams, a.cap_g = (sp.beams, sp.cap_g) if c.beam else (1, 0)
        a.kg, a.vg, a.anc = _ptr(self.kg), _ptr(self.vg), _ptr(self.anc)
        a.out_frag = sp.out_frag

    def launch(self, nsplit=True):
        sp = self.sp
        try:
            self.lib.eilev_debug_attn_part32(sp.part32)
            self.lib.eilev_debug_beam_part(sp.beam_part)
            rc = _entry(self.lib)(C.byref(self.args), C.sizeof(AttnDecodeArgs), sp.launcher, C.byref(self.nsplit) if nsplit else None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        finally:
            self.lib.eilev_debug_attn_part32(1)
            self.lib.eilev_debug_beam_part(1)
        return rc


def _check_footprint(L: Launch, rng: int):
    """Which kernel ran, from what it left in `part`: nothing (one-pass / loop), or (max, sum, o) records per range of `rng` keys with
    (-1e30, 0) and an unwritten o in the ranges beyond kv_total."""
    sp, c = L.sp, L.c
    part = L.part.cpu().numpy()
    if rng == 0:
        assert (part == SENT32).all(), f"{sp.name}: a kernel that leaves partials ran"
        return None
    keys = sp.seq_len + sp.cap_g if sp.beams else sp.cap
    ns, live = -(-keys // rng), -(-c.n // rng)
    total = sp.batch * sp.heads * ns * (sp.hd + 2)
    rec = part[:total].reshape(sp.batch, sp.heads, ns, sp.hd + 2)
    assert (rec[:, :, :live] != SENT32).all(), f"{sp.name}: unwritten records in ranges of {rng} keys"
    f = rec.view(np.float32)
    assert (f[:, :, live:, 0] == np.float32(-1e30)).all() and (f[:, :, live:, 1] == 0).all(), f"{sp.name}: empty ranges"
    assert (rec[:, :, live:, 2:] == SENT32).all() and (part[total:] == SENT32).all(), f"{sp.name}: writes beyond the records of {rng}-key ranges"
    return f


def run_case(lib, sp: Spec):
    """One launch, every check; returns the worst err / tol."""
    c = R.build_case(sp)
    ref, A = R.reference(c)
    L = Launch(lib, c)
    before = {n: _bits(getattr(L, n)) for n in ("kc", "vc", "kg", "vg") if getattr(L, n) is not None}
    rc = L.launch()
    torch.cuda.synchronize()
    assert rc == EILEV_OK, (sp.name, rc)
    rng = R.FORMS[sp.form]["rng"]
    f = _check_footprint(L, rng)
    out = L.out.cpu().numpy()
    if sp.out_null or sp.launcher == 2:  # the partials are the result: merged here in float64 (what the consumers' prologues do in fp32)
        assert L.nsplit.value == f.shape[2], (sp.name, L.nsplit.value)
        assert (out == SENT16).all()
        got = R.merge_ref(f)
    elif sp.out_frag:
        rows, cols = np.meshgrid(np.arange(sp.batch), np.arange(c.d), indexing="ij")
        idx = R.frag32_index(rows, cols)
        got = R.bits_to_f32(out[idx])
        rest = np.ones(out.shape, bool)
        rest[idx.ravel()] = False
        assert (out[rest] == SENT16).all(), f"{sp.name}: writes outside the rows of the row-block layout"
    else:
        got = R.bits_to_f32(out).reshape(sp.batch, c.d)
    ratio = R.worst_ratio(got, ref, A)
    if not ratio <= 1.0:
        err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e30) - ref) / R.tolerance(A)
        b, col = np.unravel_index(np.argmax(err), err.shape)
        pytest.fail(f"{sp.name}: err/tol {ratio:.3g} at row {b} head {col // sp.hd} dim {col % sp.hd} (got {got[b, col]}, ref {ref[b, col]}); "
                    f"kv_total {c.n}, that head's spike at key {c.spike_pos[b, col // sp.hd]}; heads beyond tol: {int((err.reshape(sp.batch, sp.heads, -1).max(-1) > 1).sum())}")
    # the caches: bit-identical, but for the newest slot of each (row, head), which holds the step's k / v
    d, n = c.d, c.n
    knew = R.bf16_bits(c.qkv[:, d:2 * d]).reshape(sp.batch, sp.heads, sp.hd) if sp.fuse_new else None
    vnew = R.bf16_bits(c.qkv[:, 2 * d:3 * d]).reshape(sp.batch, sp.heads, sp.hd) if sp.fuse_new else None
    for name in before:
        want = before[name]
        own = ("kg", "vg") if c.beam else ("kc", "vc")
        if sp.fuse_new and name in own:
            want = want.copy()
            want[:, :, (n - 1 - sp.seq_len) if c.beam else (n - 1)] = knew if name[0] == "k" else vnew
        assert np.array_equal(_bits(getattr(L, name)), want), f"{sp.name}: {name} changed outside the newest slot (or the newest slot is wrong)"
    _WORST[sp.form] = max(_WORST.get(sp.form, 0.0), ratio)
    if f is not None and not (sp.out_null or sp.launcher == 2):
        _WORST["merge"] = max(_WORST.get("merge", 0.0), ratio)
        _VISITED.setdefault("merge", sp.name)
    _VISITED.setdefault(sp.form, sp.name)
    return ratio


def _record():
    from hip_utils import record_parity

    record_parity("attn_decode", tol="(2^-8 + 2^-11) * sum_j p_j |v_ji| / sum_j p_j per element, no floor",
                  **{f"worst_err_over_tol_{k}": v for k, v in _WORST.items()}, **{f"first_case_{k}": v for k, v in _VISITED.items()})


def _run_all(lib, specs):
    assert specs
    try:
        for sp in specs:
            run_case(lib, sp)
    finally:
        _record()


COVER_FORMS = ("one80", "one64", "part128", "part128_l0", "part256", "loop80", "loop80_auto", "loop64", "split")


@pytest.mark.parametrize("form", COVER_FORMS)
def test_every_key_slot_is_the_spike_of_some_row_and_head(probes, form):
    """A full cache (kv_total == cap: 1024, 2048 or 2304 by form); launch k plants slot k * rows * heads + row * heads + head as the spike of
    (row, head), so over the launches of a form EVERY slot carries half of some row's weight: a key dropped, doubled or mis-addressed
    anywhere — range boundaries, the clamped owners of the ragged last group, the threads that own no key — fails its (row, head)."""
    _run_all(probes, [sp for sp in R.cover_specs(_num_cu()) if sp.name.startswith(f"cover-{form}-")])


@pytest.mark.parametrize("form", ("one80", "one64", "part128", "part256", "loop80", "loop64", "split"))
def test_kv_total_sweep_by_seq_len_and_by_state(probes, form):
    """kv_total = 1, 2, G-1, G, G+1, 127..129, 255..257, 511..513, 1023, 1024 (+ 1025, 2047, 2048, 2049 where the form holds them), reached
    once by seq_len and once by state[0] (read on the device); the spike on the newest key (from the q|k|v row) and on kv_total - 2;
    kv_total == cap at the range boundaries, traps in the slots beyond kv_total elsewhere."""
    _run_all(probes, [sp for sp in R.sweep_specs(_num_cu()) if sp.name.startswith(f"sweep-{form}-")])


@pytest.mark.parametrize("form", ("one80", "one64", "part128", "part256", "loop80", "loop80_auto", "loop64", "split"))
def test_masks_and_stale_slots(probes, form):
    """Left padding of 0, 1, 127, 128, 129 and 300 keys (a whole first range invisible: the online rescale after it), holes, a row with every
    prompt key masked; a trap on every masked key; traps, then NaN bits, in every slot at and beyond kv_total."""
    _run_all(probes, [sp for sp in R.mask_specs(_num_cu()) if sp.name.startswith(f"mask-{form}-")])


def test_beam_form_and_its_ancestry_table(probes):
    """beams 3 and 5, 1 or 2 samples, a random valid ancestry over 1, 2, 17 and cap_g generated tokens; spikes on prompt keys, on generated keys
    held by another row and on the newest key; the generation cache changes in the rows' own new slots only.  Both the 128-key beam
    kernel and the split kernel's beam form (eilev_debug_beam_part(0))."""
    _run_all(probes, R.beam_specs())


def test_t5_forms_bias_mask_and_row_stride(probes):
    """Head size 64: cross-attention over 960 keys (state == nullptr, fuse_new == 0, padding mask, a row with no visible key -> zeros), the
    self-attention with the position bias in both addressings (the spike's score includes its bias), ldq != 3 * heads * hd; through
    attn_decode_loop_kernel<8,8,256> at >= 2 workgroups per CU and through the split kernel at batch 4."""
    _run_all(probes, R.t5_specs(_num_cu()))


def test_what_the_other_forms_refuse_and_row_block_output(probes):
    """hd 8 / 40 / 64 / 96 / 128, cap 2304, partials left to the caller (out == nullptr), part_bytes one byte short of the 128-key size (falls
    through to the split kernel), launch_attn_decode's own choice of the 128-key ranges at batch 1 and of the loop at 2 workgroups per CU with
    out_frag 0 and 1."""
    _run_all(probes, R.other_specs(_num_cu()))


@pytest.mark.parametrize("launcher, batch", [(1, 2), (0, 2)])
def test_graph_replay_reads_state_on_the_device(probes, launcher, batch):
    """One launch captured once; replayed with state[0] = 1, 2, 3 and a new q|k|v row each time, it equals the eager launches bit for bit
    (outputs and caches).  A single launcher call: the graph has one branch."""
    sp = Spec("graph", "one80" if launcher == 1 else "part128", launcher=launcher, batch=batch, seq_len=200, cap=256, n_gen=1, mask="mixed", spikes="none", stale="nan")
    c = R.build_case(sp)
    rows = [_dev_bits(R.build_case(Spec("row", sp.form, batch=batch, seq_len=4, cap=8, seed=t, spikes="none", stale="rand")).qkv) for t in (1, 2, 3)]
    runs = []
    for graphed in (False, True):
        L = Launch(probes, c)
        g = None
        if graphed:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                rc = L.launch()
            assert rc == EILEV_OK
            for name in ("kc", "vc"):  # (the capture recorded, not ran; start from the same cache either way)
                getattr(L, name).copy_(_dev_bits(getattr(c, name)))
        outs = []
        for t in (1, 2, 3):
            L.state.fill_(t)
            L.qkv.copy_(rows[t - 1])
            L.out.fill_(SENT16)
            if graphed:
                g.replay()
            else:
                assert L.launch() == EILEV_OK
            torch.cuda.synchronize()
            outs.append(L.out.cpu().numpy().copy())
        runs.append((outs, _bits(L.kc), _bits(L.vc)))
    (eo, ek, ev), (go, gk, gv) = runs
    for t in range(3):
        assert (eo[t] != SENT16).all() and np.array_equal(eo[t], go[t]), f"replay {t + 1} differs from the eager launch"
        assert t == 0 or not np.array_equal(eo[t], eo[t - 1])
    assert np.array_equal(ek, gk) and np.array_equal(ev, gv)
    d = c.d
    for t in (1, 2, 3):  # the three new slots hold the three steps' keys
        assert np.array_equal(ek[:, :, 200 + t - 1].reshape(batch, d), _bits(rows[t - 1])[:, d:2 * d])


def test_refusals_launch_nothing(probes):
    """Host-side refusals: the code comes back and neither `out` nor `part` is written."""
    base = Spec("refuse", "split", batch=2, heads=4, hd=80, seq_len=30, cap=64, n_gen=2, spikes="none", stale="rand")

    def call(sp, nsplit=True, struct_bytes=None, **fields):
        L = Launch(probes, R.build_case(sp))
        for k, v in fields.items():
            setattr(L.args, k, v)
        if struct_bytes is None:
            rc = L.launch(nsplit)
        else:
            rc = _entry(probes)(C.byref(L.args), struct_bytes, sp.launcher, C.byref(L.nsplit), None)
        torch.cuda.synchronize()
        assert (L.out.cpu().numpy() == SENT16).all() and (L.part.cpu().numpy() == SENT32).all()
        return rc

    assert call(base, hd=136) == EILEV_E_UNSUPPORTED  # (the buffers are those of hd 80; nothing may be launched)
    assert call(base, hd=12) == EILEV_E_UNSUPPORTED
    assert call(base, nsplit=False, out=None) == EILEV_E_BADARG
    assert call(base, out_frag=1) == EILEV_E_UNSUPPORTED  # 8 (row, head) pairs: attn_decode_loop_ok is false
    assert call(base, part_bytes=part_bytes(base, 256) - 1) == EILEV_E_WORKSPACE
    assert call(base, struct_bytes=C.sizeof(AttnDecodeArgs) - 8) == EILEV_E_BADARG
    assert call(base, struct_bytes=C.sizeof(AttnDecodeArgs) + 8) == EILEV_E_BADARG
    assert call(Spec("r1", "one80", launcher=1, batch=2, heads=4, hd=80, seq_len=30, cap=1100, n_gen=2, spikes="none", stale="rand")) == EILEV_E_UNSUPPORTED
    assert call(Spec("r2", "part128", launcher=2, batch=2, heads=4, hd=64, seq_len=30, cap=64, n_gen=2, spikes="none", stale="rand")) == EILEV_E_UNSUPPORTED
    assert C.sizeof(AttnDecodeArgs) == 152
