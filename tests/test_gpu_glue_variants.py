"""The kernels between the pinned families on the device, one parametrised case per cell of tests/_glue_variants.py: the three tail
backward kernels a process reaches by its arguments (per-lane plain, matrix-core REDUCE, matrix-core REDUCE with dropout), the per-lane
REDUCE kernel in one child process (EGNN_TAIL_SCALAR=1), egnn_edge_pool_f32, the packed images of egnn_node_prep_hl / egnn_split_f16 /
egnn_split_scaled_f16 / egnn_split_scaled_both_f16 decoded WITH their pad rows, the column sums and egnn_sum_parts_f32 in their
restated order, egnn_silu_bwd_f32 with and without dropout, egnn_unsplit_words_f32 and egnn_node_mlp_fused_f32.

Toleranced comparisons use the bars of `_glue_variants` (derived from the float64 reference and torch fp32 on the same inputs, never
above the older test's bar of the same output); images, column sums, sum_rows, chunked dropout calls and second runs are compared bit
for bit.  Every output lies in front of sentinel rows that must stay untouched; refused calls leave every output untouched.  Each case
prints its worst error-to-bar ratio; the module prints the worst per kernel at its end."""
import os
import subprocess
import sys
from ctypes import byref

import numpy as np
import pytest
import torch

from tests import _glue_variants as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error / bar per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _note(kernel, err, bar):
    ratio = float(err) / max(float(bar), 1e-300) if float(err) > 0 else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    return ratio


def _lib():
    from egnn_pytorch_amd import _abi
    return _abi.load()


def _stream():
    from egnn_pytorch_amd import _ops
    return _ops._stream()


def _status_bits():
    """the forward status word as the range tests read it: after a synchronisation, then cleared"""
    from egnn_pytorch_amd import _ops
    st = _ops.status_word("cuda")
    torch.cuda.synchronize()
    bits = int(st.dev[0])
    st.dev.zero_()
    return bits


# ================================================================================================ the tail
TAIL_RUNS = [(c.id, mode) for c in V.TAIL_CELLS for mode in V.tail_modes(c) if mode != "scalar"]


@pytest.mark.parametrize("cid,mode", TAIL_RUNS, ids=[f"{cid}-{mode}" for cid, mode in TAIL_RUNS])
def test_tail_cell(cid, mode):
    d = V.prepare(cid)
    t, o = V.tail_run(d, mode)
    V.tail_check(d, mode, o, WORST)
    print(f"{cid} {mode}: worst error / bar so far {WORST.get(V.MODE_KERNEL[mode], 0.0):.3f}")
    _, again = V.tail_run(d, mode)
    assert all(torch.equal(o[name], again[name]) for name in o), (cid, mode, "two runs differ")
    _, bare = V.tail_run(d, mode, want_rel=False)                                # the by-products off: the same bits everywhere else
    assert "rel" in o and "rel" not in bare and all(torch.equal(o[name], bare[name]) for name in bare), (cid, mode, "rel / dist change the results")
    if d.drop is not None and d.b % 2 == 0:
        # the second half of the graphs as a call of its own, edges numbered on from the first half: the same bits per edge
        half = d.b // 2
        e0 = half * d.n * d.k
        oc = V.tail_outputs(d.e - e0, True, True)
        rc = V.tail_launch(V.tail_args(d, t, oc, True, d.drop, d.eid0 + e0, b=d.b - half, edge0=e0))
        torch.cuda.synchronize()
        assert rc == 0
        for name in ("gU", "g_rel", "rel", "dist"):
            assert torch.equal(oc[name][:d.e - e0], o[name][e0:d.e]), (cid, name, "chunked call differs")
            assert bool((oc[name][d.e - e0:] == V.SENTINEL).all())
        wrong = V.tail_outputs(d.e - e0, True, False)                            # (numbered from the cell's eid0 instead: another mask)
        assert V.tail_launch(V.tail_args(d, t, wrong, True, d.drop, d.eid0, b=d.b - half, edge0=e0)) == 0
        assert not torch.equal(wrong["gU"][:d.e - e0], o["gU"][e0:d.e])


def test_tail_per_lane_reduce_kernel_in_a_child_process():
    """edge_tail_bwd_kernel<true>: EGNN_TAIL_SCALAR is read once per process -- one fresh child with it set runs every REDUCE cell against
    the same specification and bars, and the launcher's refusal of dropout there."""
    env = dict(os.environ, EGNN_TAIL_SCALAR="1")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tests._glue_variants", "--scalar-child"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "scalar child:" in r.stdout


def test_tail_launcher_refusals_leave_every_output_untouched():
    """every branch of egnn_edge_tail_bwd_f32 that returns before a launch: its code, and the sentinel still in every output"""
    d = V.prepare("base_e80")
    t = V.tail_device_inputs(d)
    lib = _lib()

    def refused(code, reduce, edit, drop=None, want_rel=True, tt=t):
        o = V.tail_outputs(d.e, reduce, want_rel and reduce)
        a = V.tail_args(d, tt, o, reduce, drop, 0)
        edit(a)
        rc = lib.egnn_edge_tail_bwd_f32(byref(a), _stream())
        torch.cuda.synchronize()
        assert rc == code, (rc, code)
        for name, v in o.items():
            assert bool((v == (0x7fc00000 if name == "amax" else V.SENTINEL)).all()), name

    assert lib.egnn_edge_tail_bwd_f32(None, _stream()) == V.E_NULLPTR
    for field in ("u", "coors", "g_coors_out", "g_msum", "W3", "b3", "W4", "b4", "gU", "g_rel"):
        for reduce in (False, True):
            refused(V.E_NULLPTR, reduce, lambda a, f=field: setattr(a, f, None))
    for field in ("g_hid", "a3", "g_w", "g_scale", "g_gate"):                    # the plain mode's outputs (scale / gate: the cell has both)
        refused(V.E_NULLPTR, False, lambda a, f=field: setattr(a, f, None))
    refused(V.E_NULLPTR, True, lambda a: setattr(a, "scale", None))
    refused(V.E_NULLPTR, True, lambda a: setattr(a, "gate_b", None))
    refused(V.E_NULLPTR, True, lambda a: setattr(a, "dist_out", None))         # rel_out without dist_out
    refused(V.E_NULLPTR, True, lambda a: setattr(a, "rel_out", None))
    refused(V.E_SHAPE, True, lambda a: setattr(a, "idx", None))                # idx = NULL with K != N
    for field in ("B", "N", "K"):
        refused(V.E_SHAPE, True, lambda a, f=field: setattr(a, f, 0))
    for field in ("u", "gU", "g_rel", "part", "rel_out"):
        refused(V.E_ALIGN, True, lambda a, f=field: setattr(a, f, getattr(a, f) + 4))
    for field in ("g_hid", "a3"):
        refused(V.E_ALIGN, False, lambda a, f=field: setattr(a, f, getattr(a, f) + 4))
    refused(V.E_UNSUPPORTED, False, lambda a: None, drop=(0.5, 3))            # dropout without `part`
    refused(V.E_SHAPE, True, lambda a: setattr(a, "drop_inv_keep", 0.5), drop=(0.5, 3))
    refused(V.E_SHAPE, True, lambda a: setattr(a, "drop_inv_keep", float("nan")), drop=(0.5, 3))


def test_tail_wrapper_passes_a_zero_clamp_as_zero():
    """_ops.edge_tail_bwd with clamp = 0.0: everything is clamped (d/d w = 0 on every edge), not "no clamp" """
    from egnn_pytorch_amd import _ops
    d = V.prepare("clamp_zero")
    t = V.tail_device_inputs(d)
    args = (t["u"].view(d.b, d.n, d.k, 16), t["coors"], t["idx"], None, t["g_co"], t["g_msum"], t["W3"], t["b3"], t["W4"], t["b4"], t["scale"], V.EPS,
            0.0, d.b, d.n, d.k)
    out = _ops.edge_tail_bwd(*args, gate=(t["gate_w"], t["gate_b"]))
    assert not bool(out[4].any()) and not bool(out[2].any())                    # g_w, g_hid
    assert float((out[0][:, :d.m].double().cpu() - d.ref["g_u"]).abs().max()) <= float(torch.as_tensor(V.tail_bars(d.cell.id, "plain")["g_u"], dtype=torch.float64).max())
    free = _ops.edge_tail_bwd(*args[:12], None, *args[13:], gate=(t["gate_w"], t["gate_b"]))
    assert bool(free[4].any())                                                   # without a clamp the same cell has active weights


# ================================================================================================ the pool
@pytest.mark.parametrize("cell", V.POOL_CELLS, ids=[c["id"] for c in V.POOL_CELLS])
def test_pool_cell(cell):
    from egnn_pytorch_amd import _ops
    u, gate, pm, ref, bar = V.pool_case(cell)
    n, k = cell["n"], cell["k"]
    gd = None if gate is None else (gate[0].cuda(), gate[1].cuda())
    pm8 = None if pm is None else pm.cuda().contiguous().view(torch.uint8)
    out = torch.full((n + V.GUARD, 16), V.SENTINEL, device="cuda")
    ud = u.cuda()
    rc = _lib().egnn_edge_pool_f32(ud.data_ptr(), _ops._ptr(gd[0]) if gd else None, _ops._ptr(gd[1]) if gd else None, _ops._ptr(pm8), 1, n, k,
                                   out.data_ptr(), _stream())
    assert rc == 0
    err = float((out[:n].double().cpu() - ref[0]).abs().max())
    print(f"{cell['id']}: error / bar {_note('edge_pool_kernel', err, bar):.3f}")
    assert err <= bar, (err, bar)
    assert bool((out[n:] == V.SENTINEL).all())
    if pm is not None:
        dead = ~pm[0].any(dim=-1)
        assert bool(dead.any()) or cell["mask"] in ("scattered", "ragged")
        assert not bool(out[:n][dead.cuda()].any())                              # a fully masked node: exact 0
    assert torch.equal(_ops.edge_pool(ud, gd, pm8, 1, n, k)[0], out[:n])


# ================================================================================================ packed images
def _image(phl):
    return V.unpack_full(phl.hi, phl.rows, phl.kp), V.unpack_full(phl.lo, phl.rows, phl.kp)


def _assert_image(phl, want32, what, scale=1.0):
    """bit for bit: hi == fp16(s x), lo == fp16(s x - float32(hi)), zeros in every pad column and pad row"""
    hi, lo = _image(phl)
    rp = (phl.rows + 31) // 32 * 32
    assert hi.shape == (rp, phl.kp), what
    whi, wlo = V.split_image(want32, scale)
    assert V.same_bits(hi, V.padded(whi, rp, phl.kp)), (what, "hi")
    assert V.same_bits(lo, V.padded(wlo, rp, phl.kp)), (what, "lo")


@pytest.mark.parametrize("cell", V.PREP_CELLS, ids=[c["id"] for c in V.PREP_CELLS])
def test_node_prep_cell(cell):
    from egnn_pytorch_amd import _ops
    x, mi, gamma, beta = V.prep_case(cell)
    rows, dim = x.shape
    dv = lambda v: None if v is None else v.cuda()                                # noqa: E731
    out = _ops.node_prep_hl(dv(x), dv(mi), dv(gamma), dv(beta), 1e-5, 16, with_raw=cell["raw"])
    phl, raw = out if cell["raw"] else (out, None)
    assert _status_bits() == 0
    assert phl.kp == (dim + 16 + 31) // 32 * 32 and phl.rows == rows
    mi_np = mi.numpy() if mi is not None else np.zeros((rows, 16), dtype=np.float32)
    if raw is not None:
        _assert_image(raw, x.numpy(), (cell["id"], "raw"))
    if not cell["ln"]:
        _assert_image(phl, np.concatenate([x.numpy(), mi_np], axis=1), cell["id"])
        if not cell["mi"] and rows <= 300:                                       # the m_dim = 0 form is egnn_split_f16
            _assert_image(_ops.split_f16(x.cuda()), x.numpy(), (cell["id"], "split_f16"))
        return
    hi, lo = _image(phl)
    assert not hi[rows:].any() and not lo[rows:].any() and not hi[:, dim + 16:].any() and not lo[:, dim + 16:].any(), (cell["id"], "pad")
    mh, ml = V.split_image(mi_np)
    assert V.same_bits(hi[:rows, dim:dim + 16], mh) and V.same_bits(lo[:rows, dim:dim + 16], ml), (cell["id"], "m_i columns")
    ref = V.layer_norm_ref(x, gamma, beta, 1e-5, torch.float64).numpy()
    f32 = V.layer_norm_ref(x, gamma, beta, 1e-5, torch.float32)
    bar = V.bar_f32(torch.from_numpy(ref), f32, None)
    if cell["data"] != "mean1e4":                                                # (rows of mean 1e4: fp32 carries x - mean to 1e-3 of the deviation)
        bar = min(bar, 1e-5)                                                     # tests/test_gpu_kernels.py::test_node_prep_hl: atol 1e-5
    y = hi[:rows, :dim].astype(np.float64) + lo[:rows, :dim].astype(np.float64)
    err = np.abs(y - ref)
    assert np.isfinite(y).all()
    worst = float((err / (bar + 2.0 ** -22 * np.abs(ref))).max())
    print(f"{cell['id']}: error / bar {_note('node_prep_hl_kernel', worst, 1.0):.3f} (bar {bar:.2e})")
    assert worst <= 1.0, (cell["id"], worst, float(err.max()), bar)
    # the split of the row: lo is the rest behind the nearest fp16 -- at most half a unit in the last place of hi
    assert np.all(np.abs(lo[:rows, :dim].astype(np.float64)) <= 2.0 ** -11 * np.abs(hi[:rows, :dim].astype(np.float64)) + 2.0 ** -24)
    if cell["data"] == "const":
        assert np.array_equal(y[::3], np.broadcast_to(V.split_image(beta.numpy())[0].astype(np.float64) + V.split_image(beta.numpy())[1].astype(np.float64), y[::3].shape))


def test_node_prep_raw_image_of_another_width_through_the_c_entry():
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(5)
    rows, dim, m_dim = 33, 12, 16
    x = torch.randn(rows, dim, generator=g)
    gamma, beta = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    for kp, rkp in ((32, 96), (96, 32)):
        main = _ops.PackedHL(_ops._packed_empty(rows, kp, "cuda"), _ops._packed_empty(rows, kp, "cuda"), rows, kp)
        raw = _ops.PackedHL(_ops._packed_empty(rows, rkp, "cuda"), _ops._packed_empty(rows, rkp, "cuda"), rows, rkp)
        for t in (main.hi, main.lo, raw.hi, raw.lo):
            t.fill_(7.0)
        rc = _lib().egnn_node_prep_hl(xd.data_ptr(), None, None, None, 1e-5, main.hi.data_ptr(), main.lo.data_ptr(), kp, raw.hi.data_ptr(),
                                      raw.lo.data_ptr(), rkp, rows, dim, m_dim, None, _stream())
        assert rc == 0
        _assert_image(main, x.numpy(), ("main", kp))
        _assert_image(raw, x.numpy(), ("raw", rkp))
        rc = _lib().egnn_node_prep_hl(xd.data_ptr(), None, gd.data_ptr(), bd.data_ptr(), 1e-5, main.hi.data_ptr(), main.lo.data_ptr(), kp,
                                      raw.hi.data_ptr(), raw.lo.data_ptr(), rkp, rows, dim, m_dim, None, _stream())
        assert rc == 0
        _assert_image(raw, x.numpy(), ("raw beside LayerNorm", rkp))
    lib = _lib()
    h = main.hi.data_ptr()
    assert lib.egnn_node_prep_hl(None, None, None, None, 1e-5, h, h, 32, None, None, 0, rows, dim, m_dim, None, _stream()) == V.E_NULLPTR
    assert lib.egnn_node_prep_hl(xd.data_ptr(), None, gd.data_ptr(), None, 1e-5, h, h, 32, None, None, 0, rows, dim, m_dim, None, _stream()) == V.E_NULLPTR
    assert lib.egnn_node_prep_hl(xd.data_ptr(), None, None, None, 1e-5, h, h, 32, h, None, 32, rows, dim, m_dim, None, _stream()) == V.E_NULLPTR
    assert lib.egnn_node_prep_hl(xd.data_ptr(), None, None, None, 1e-5, h, h, 16, None, None, 0, rows, dim, m_dim, None, _stream()) == V.E_SHAPE
    assert lib.egnn_node_prep_hl(xd.data_ptr(), None, None, None, 1e-5, h, h, 48, None, None, 0, rows, dim, m_dim, None, _stream()) == V.E_SHAPE
    assert lib.egnn_node_prep_hl(xd.data_ptr(), None, None, None, 1e-5, h, h, 32, h, h, 8, rows, dim, m_dim, None, _stream()) == V.E_SHAPE


def test_packed_image_wrappers_take_views_of_any_layout():
    """_ops.split_f16 reads a view of rows of a wider matrix by its row stride and every other layout as a copy; _ops.node_prep_hl takes a
    strided operand as a copy: the image is the image of the values, whatever the layout."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(6)
    wide = torch.randn(70, 40, generator=g).cuda()
    views = {"row slice": wide[:, :24], "row slice, odd stride": torch.randn(70, 39, generator=g).cuda()[:, :24], "offset": wide[:, 1:25],
             "transposed": torch.randn(24, 70, generator=g).cuda().t(), "one row": wide[3:4, :24], "expanded": wide[:1, :24].expand(5, 24), "every other row": wide[::2, :24]}
    for name, v in views.items():
        assert not v.is_contiguous() or name == "one row"
        _assert_image(_ops.split_f16(v), v.cpu().numpy(), ("split_f16", name))
        _assert_image(_ops.node_prep_hl(v, None, None, None, 1e-5, 0), v.cpu().numpy(), ("node_prep_hl", name))
        mi = torch.randn(v.shape[0], 32, generator=g).cuda()[:, :16]
        _assert_image(_ops.node_prep_hl(v, mi, None, None, 1e-5, 16), np.concatenate([v.cpu().numpy(), mi.cpu().numpy()], axis=1), ("node_prep_hl + m_i", name))
    assert _status_bits() == 0


@pytest.mark.parametrize("value,flag", [(65504.0, 1), (-65504.0, 1), (1e30, 1), (65000.0, 0), (float("inf"), 0), (float("-inf"), 0), (float("nan"), 0)])
def test_packed_image_range_flag(value, flag):
    """one element with 65504 <= |y| < inf sets EGNN_RANGE_A_OPERAND; 65000, +-inf and NaN do not"""
    from egnn_pytorch_amd import _ops
    assert _status_bits() == 0
    x = torch.randn(33, 12, generator=torch.Generator().manual_seed(7))
    x[17, 5] = value
    _ops.node_prep_hl(x.cuda(), None, None, None, 1e-5, 16)
    assert _status_bits() == flag
    _ops.split_f16(x.cuda())
    assert _status_bits() == flag
    mi = torch.zeros(33, 16)
    mi[32, 15] = value
    _ops.node_prep_hl(torch.randn(33, 12, generator=torch.Generator().manual_seed(8)).cuda(), mi.cuda(), torch.ones(12).cuda(), torch.zeros(12).cuda(), 1e-5, 16)
    assert _status_bits() == flag
    _ops.node_prep_hl(x.cuda(), None, torch.ones(12).cuda(), torch.zeros(12).cuda(), 1e-5, 16, with_raw=True)      # the raw rows are checked too
    assert _status_bits() == flag
    _ops.split_scaled(torch.full((3, 5), value if value == value else 1.0).cuda(), 1.0)
    assert _status_bits() == (flag if value == value else 0)
    assert _status_bits() == 0                                                   # cleared


@pytest.mark.parametrize("cell", V.SPLIT_CELLS, ids=[c["id"] for c in V.SPLIT_CELLS])
def test_split_scaled_cell(cell):
    from egnn_pytorch_amd import _ops
    rows, cols, extra = cell["rows"], cell["cols"], cell["ldx_extra"]
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    store = (torch.randn(rows, cols + extra, generator=g) * 1e-3).cuda()
    x = store[:, :cols]                                                          # ldx > cols where extra > 0
    xn = x.cpu().numpy()
    assert extra == 0 or x.stride(0) > cols or rows == 1
    for scale in (2.0 ** 13, -1.4426950408889634):
        plain, alloc = _ops.split_scaled(x, scale)
        assert alloc == rows
        _assert_image(plain, xn, (cell["id"], "plain", scale), scale)
        tr, _ = _ops.split_scaled(x, scale, transposed=True)
        assert tr.rows == cols and tr.kp == (rows + 31) // 32 * 32
        _assert_image(tr, xn.T, (cell["id"], "transposed", scale), scale)
    scale = 2.0 ** 13
    wimg, alloc = _ops.split_scaled(x, scale, w_image=True)
    assert alloc == (rows + 127) // 128 * 128 and wimg.hi.numel() == alloc * wimg.kp
    whole = _ops.PackedHL(wimg.hi, wimg.lo, alloc, wimg.kp)                      # the whole 128-row tiles: zero behind the matrix
    _assert_image(whole, xn, (cell["id"], "w_image"), scale)
    bp, bt = _ops.split_scaled_both(x, scale)
    _assert_image(bp, xn, (cell["id"], "both, plain"), scale)
    _assert_image(bt, xn.T, (cell["id"], "both, transposed"), scale)
    # the column sums: the parts of the kernel and their sum, in the restated order, zero-filled columns in [cols, ld)
    ld = (cols + 3) // 4 * 4
    nblk = int(_lib().egnn_split_scaled_colsum_rows(rows, bt.kp))
    parts = torch.full((nblk + 2, ld), V.SENTINEL, device="cuda")
    rc = _lib().egnn_split_scaled_both_f16(x.data_ptr(), x.stride(0), rows, cols, scale, bp.hi.data_ptr(), bp.lo.data_ptr(), bp.kp, bt.hi.data_ptr(),
                                           bt.lo.data_ptr(), bt.kp, None, parts.data_ptr(), ld, _stream())
    assert rc == 0
    want_sum, want_parts = V.colsum_order(xn, scale, ld)
    assert want_parts.shape == (nblk, ld)
    assert np.array_equal(parts[:nblk].cpu().numpy().view(np.uint32), want_parts.view(np.uint32)), (cell["id"], "column-sum parts")
    assert bool((parts[nblk:] == V.SENTINEL).all())
    assert not want_parts[:, cols:].any()
    _assert_image(bp, xn, (cell["id"], "both + colsum, plain"), scale)
    cs = _ops.split_scaled_both(x, scale, colsum=True)[2]
    assert np.array_equal(cs.cpu().numpy().view(np.uint32), want_sum[:cols].view(np.uint32)), (cell["id"], "column sums")
    assert float(np.abs(want_sum[:cols].astype(np.float64) - xn.astype(np.float64).sum(0)).max()) <= 2e-6 * float(np.abs(xn.astype(np.float64)).sum(0).max())
    assert _status_bits() == 0


def test_split_scaled_refusals():
    lib = _lib()
    x = torch.randn(8, 8).cuda()
    h = torch.full((32 * 32,), 7.0, dtype=torch.float16, device="cuda")
    l, ht, lt = h.clone(), h.clone(), h.clone()
    p = x.data_ptr()
    both = lambda scale, xp=p, ldx=8, kp=32, kpt=32, hp=h.data_ptr(): lib.egnn_split_scaled_both_f16(        # noqa: E731
        xp, ldx, 8, 8, scale, hp, l.data_ptr(), kp, ht.data_ptr(), lt.data_ptr(), kpt, None, None, 0, _stream())
    one = lambda scale, xp=p, ldx=8, kp=32, tr=0: lib.egnn_split_scaled_f16(xp, ldx, 8, 8, scale, tr, h.data_ptr(), l.data_ptr(), kp, None, _stream())     # noqa: E731
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        assert both(scale) == V.E_SHAPE, scale
    for scale in (0.0, float("inf"), float("-inf"), float("nan")):
        assert one(scale) == V.E_SHAPE, scale
    assert both(2.0, xp=None) == V.E_NULLPTR and both(2.0, hp=None) == V.E_NULLPTR and one(2.0, xp=None) == V.E_NULLPTR
    assert both(2.0, ldx=7) == V.E_SHAPE and both(2.0, kp=16) == V.E_SHAPE and both(2.0, kpt=48) == V.E_SHAPE and both(2.0, kp=0) == V.E_SHAPE
    assert one(2.0, ldx=7) == V.E_SHAPE and one(2.0, kp=48) == V.E_SHAPE and one(2.0, kp=0, tr=1) == V.E_SHAPE
    parts = torch.zeros(1, 4, device="cuda")
    assert lib.egnn_split_scaled_both_f16(p, 8, 8, 8, 2.0, h.data_ptr(), l.data_ptr(), 32, ht.data_ptr(), lt.data_ptr(), 32, None, parts.data_ptr(), 4,
                                          _stream()) == V.E_SHAPE               # ld_colsum < cols
    torch.cuda.synchronize()
    for t in (h, l, ht, lt):
        assert bool((t == 7.0).all())
    assert one(-1.5) == 0 and both(2.0) == 0


# ================================================================================================ silu_bwd_, unsplit_words_, sum_rows
def _silu_bars(z, g, drop=None, row0=0):
    a64, gz64 = V.silu_spec(z, g, torch.float64, drop, row0)
    a32, gz32 = V.silu_spec(z, g, torch.float32, drop, row0)
    return a64, gz64, V.bar_f32(a64, a32, V.EDGE_CAP), V.bar_f32(gz64, gz32, V.EDGE_CAP)


@pytest.mark.parametrize("count", V.SILU_COUNTS)
@pytest.mark.parametrize("in_place", [True, False])
def test_silu_bwd_cell(count, in_place):
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(count)
    z = torch.randn(1, count, generator=g) * 4
    z[0, :4] = torch.tensor([100.0, -100.0, 0.0, -0.0])
    gr = torch.randn(1, count, generator=g)
    a64, gz64, bar_a, bar_g = _silu_bars(z, gr)
    zd, gd = z.cuda(), gr.cuda()
    if in_place:
        a, gz, bits = _ops.silu_bwd_(zd, gd)
        assert a.data_ptr() == zd.data_ptr()
    else:
        a, gz = torch.full((1, count + 64), V.SENTINEL, device="cuda"), torch.full((1, count + 64), V.SENTINEL, device="cuda")
        bits = torch.empty(2, dtype=torch.int32, device="cuda")
        assert _lib().egnn_silu_bwd_f32(zd.data_ptr(), gd.data_ptr(), a.data_ptr(), gz.data_ptr(), count, bits.data_ptr(), _stream()) == 0
        assert bool((a[:, count:] == V.SENTINEL).all()) and bool((gz[:, count:] == V.SENTINEL).all())
        assert torch.equal(zd.cpu(), z) and torch.equal(gd.cpu(), gr)
        a, gz = a[:, :count], gz[:, :count]
    ea, eg = float((a.double().cpu() - a64).abs().max()), float((gz.double().cpu() - gz64).abs().max())
    print(f"silu_bwd {count}: error / bar {_note('silu_bwd_kernel', ea, bar_a):.3f} {_note('silu_bwd_kernel', eg, bar_g):.3f}")
    assert ea <= bar_a and eg <= bar_g, (ea, bar_a, eg, bar_g)
    assert _ops.bits_to_floats(bits) == [float(a.abs().max()), float(gz.abs().max())]


def test_silu_bwd_beyond_the_grid_cap():
    """8192 x 1024 + 1024 quads (the grid-stride loop's second trip; 134 MB per tensor, in place): a 4096-element pattern repeated, every
    repetition against the pattern's float64 reference"""
    from egnn_pytorch_amd import _ops
    period, reps = 4096, 8193
    assert period * reps // 4 > 8192 * 1024
    g = torch.Generator().manual_seed(11)
    z, gr = torch.randn(period, generator=g) * 4, torch.randn(period, generator=g)
    a64, gz64, bar_a, bar_g = _silu_bars(z[None], gr[None])
    zd, gd = z.cuda().repeat(reps), gr.cuda().repeat(reps)
    a, gz, bits = _ops.silu_bwd_(zd, gd)
    a64d, gz64d = a64.cuda(), gz64.cuda()
    ea = eg = 0.0
    for r0 in range(0, reps, 1024):
        ea = max(ea, float((a.view(reps, period)[r0:r0 + 1024].double() - a64d).abs().max()))
        eg = max(eg, float((gz.view(reps, period)[r0:r0 + 1024].double() - gz64d).abs().max()))
    assert ea <= bar_a and eg <= bar_g, (ea, bar_a, eg, bar_g)
    assert torch.equal(a.view(reps, period)[-1], a.view(reps, period)[0]) and torch.equal(gz.view(reps, period)[-1], gz.view(reps, period)[0])
    assert _ops.bits_to_floats(bits) == [float(a.abs().max()), float(gz.abs().max())]


@pytest.mark.parametrize("cell", V.SILU_DROP, ids=[f"r{c['rows']}_c{c['cols']}_p{c['p']}" for c in V.SILU_DROP])
def test_silu_bwd_dropout_cell(cell):
    from egnn_pytorch_amd import _ops
    rows, cols, p = cell["rows"], cell["cols"], cell["p"]
    g = torch.Generator().manual_seed(rows * 131 + cols)
    z, gr = torch.randn(rows, cols, generator=g) * 3, torch.randn(rows, cols, generator=g)
    drop = (p, 999)
    a64, gz64, bar_a, bar_g = _silu_bars(z, gr, drop)
    kept = float((gz64 != 0).float().mean())
    assert 0.0 < kept < 1.0                                                      # the mask drops some and keeps some
    a, gz, bits = _ops.silu_bwd_(z.cuda(), gr.cuda(), drop=drop)
    ea, eg = float((a.double().cpu() - a64).abs().max()), float((gz.double().cpu() - gz64).abs().max())
    print(f"silu_bwd dropout: error / bar {_note('silu_bwd_kernel', ea, bar_a):.3f} {_note('silu_bwd_kernel', eg, bar_g):.3f}")
    assert ea <= bar_a and eg <= bar_g, (ea, bar_a, eg, bar_g)
    assert torch.equal((a == 0).cpu() | (z == 0), (a64 == 0) | (z == 0))        # the same units dropped, exactly zero
    assert _ops.bits_to_floats(bits) == [float(a.abs().max()), float(gz.abs().max())]
    # rows 4 .. as a call of their own, numbered on: the same bits
    a2, gz2, _ = _ops.silu_bwd_(z.cuda()[4:], gr.cuda()[4:], drop=drop, row0=4)
    assert torch.equal(a2, a[4:]) and torch.equal(gz2, gz[4:])
    a3_, _, _ = _ops.silu_bwd_(z.cuda()[4:], gr.cuda()[4:], drop=drop, row0=0)
    assert not torch.equal(a3_, a[4:])


def test_silu_bwd_refusals():
    lib = _lib()
    z = torch.full((16,), 3.0, device="cuda")
    g = z.clone()
    p, q = z.data_ptr(), g.data_ptr()
    call = lambda zp=p, gp=q, ap=p, bp=q, count=16, thr=0, inv=1.0, row0=0, cols=4: lib.egnn_silu_bwd_drop_f32(        # noqa: E731
        zp, gp, ap, bp, count, None, thr, 1, inv, row0, cols, _stream())
    assert call(zp=None) == V.E_NULLPTR and call(gp=None) == V.E_NULLPTR and call(ap=None) == V.E_NULLPTR and call(bp=None) == V.E_NULLPTR
    assert call(count=0) == V.E_SHAPE and call(count=6) == V.E_SHAPE
    assert call(zp=p + 4, count=8) == V.E_ALIGN and call(bp=q + 8, count=8) == V.E_ALIGN
    assert call(thr=5, inv=0.5) == V.E_SHAPE and call(thr=5, cols=3, count=12) == V.E_SHAPE and call(thr=5, cols=5) == V.E_SHAPE
    assert call(thr=5, row0=-1) == V.E_SHAPE and call(thr=5, row0=2 ** 32 - 4) == V.E_SHAPE
    torch.cuda.synchronize()
    assert bool((z == 3.0).all()) and bool((g == 3.0).all())
    assert call(thr=5, row0=2 ** 32 - 5) == 0


def test_unsplit_words_narrow_and_strided():
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(12)
    rows, ld = 37, 12
    halves = (torch.randn(rows, 4, 2, generator=g) * 100).half()
    table = torch.randn(rows + 2, ld, generator=g)
    table[:rows, :4] = halves.view(rows, 8).view(torch.float32)
    keep = table.clone()
    dev = table.cuda()
    _ops.unsplit_words_(dev[:rows], 4)
    want = keep.clone()
    want[:rows, :4] = halves[..., 0].float() + halves[..., 1].float()
    assert torch.equal(dev.cpu().view(torch.int32), want.view(torch.int32))       # the words decoded, every other element untouched
    lib = _lib()
    p = dev.data_ptr()
    assert lib.egnn_unsplit_words_f32(None, 12, 4, 4, _stream()) == V.E_NULLPTR
    for ldx, r, c in ((12, 0, 4), (12, 4, 0), (12, 4, 6), (3, 4, 4), (10, 4, 4)):
        assert lib.egnn_unsplit_words_f32(p, ldx, r, c, _stream()) == V.E_SHAPE, (ldx, r, c)
    assert lib.egnn_unsplit_words_f32(p + 4, 12, 4, 4, _stream()) == V.E_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("nparts", [1, 2, 5, 4096, 768, 6])
def test_sum_rows_order(nparts):
    """_ops.sum_rows on egnn_sum_parts_f32: the fp32 sum in the restated order, bit for bit, with a scale"""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(nparts)
    part = torch.randn(nparts, 8, generator=g) * torch.logspace(-3, 3, 8)
    pd = part.cuda()
    for scale in (1.0, 0.37, 2.0 ** -13):
        got = _ops.sum_rows(pd, scale).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), V.sum_rows_order(part.numpy(), scale).view(np.uint32)), (nparts, scale)
        out = torch.full((16,), V.SENTINEL, device="cuda")
        assert _lib().egnn_sum_parts_f32(pd.data_ptr(), nparts, 8, scale, out.data_ptr(), _stream()) == 0
        assert np.array_equal(out[:8].cpu().numpy().view(np.uint32), V.sum_parts_order(part.numpy(), scale).view(np.uint32))
        assert bool((out[8:] == V.SENTINEL).all())


def test_sum_parts_refusals():
    lib = _lib()
    part, out = torch.ones(4, 8, device="cuda"), torch.full((8,), V.SENTINEL, device="cuda")
    p, o = part.data_ptr(), out.data_ptr()
    assert lib.egnn_sum_parts_f32(None, 4, 8, 1.0, o, _stream()) == V.E_NULLPTR and lib.egnn_sum_parts_f32(p, 4, 8, 1.0, None, _stream()) == V.E_NULLPTR
    assert lib.egnn_sum_parts_f32(p, 0, 8, 1.0, o, _stream()) == V.E_SHAPE and lib.egnn_sum_parts_f32(p, 4, 0, 1.0, o, _stream()) == V.E_SHAPE
    assert lib.egnn_sum_parts_f32(p, 4, 6, 1.0, o, _stream()) == V.E_SHAPE
    assert lib.egnn_sum_parts_f32(p + 4, 2, 8, 1.0, o, _stream()) == V.E_ALIGN and lib.egnn_sum_parts_f32(p, 4, 4, 1.0, o + 8, _stream()) == V.E_ALIGN
    torch.cuda.synchronize()
    assert bool((out == V.SENTINEL).all())


# ================================================================================================ node_mlp_fused
def _nmf_device(dim, c):
    from egnn_pytorch_amd import _ops, _weights
    s5, s6 = _weights.split_f16(c.w5), _weights.split_f16(c.w6)
    s5d, s6d = tuple(t.cuda() if torch.is_tensor(t) else t for t in s5), tuple(t.cuda() if torch.is_tensor(t) else t for t in s6)
    img = _ops.node_mlp_fused_image(s5d, s6d, dim, 16)
    assert torch.equal(img.cpu(), _weights.node_mlp_fused_image(s5, s6, dim, 16))
    return s5d, s6d, img


def _nmf_call(node_in, img, s5d, s6d, b5, b6, res, out, rows, dim):
    from egnn_pytorch_amd import _ops
    return _lib().egnn_node_mlp_fused_f32(node_in.hi.data_ptr(), node_in.lo.data_ptr(), img.data_ptr(), float(s5d[2]), b5.data_ptr(), float(s6d[2]),
                                          b6.data_ptr(), res.data_ptr(), out.data_ptr(), rows, dim, 16, _ops._status_ptr("cuda"), _stream())


@pytest.mark.parametrize("rows", V.NMF_ROWS)
@pytest.mark.parametrize("dim", V.NMF_DIMS)
def test_node_mlp_fused_cell(dim, rows):
    from egnn_pytorch_amd import _ops
    assert V.nmf_supported(dim, 16) and _ops.node_mlp_fused_supported(dim, 16)
    c = V.nmf_case(dim, rows)
    s5d, s6d, img = _nmf_device(dim, c)
    node_in = _ops.split_f16(c.x.cuda())
    b5, b6, res = c.b5.cuda(), c.b6.cuda(), c.res.cuda()
    out = torch.full((rows + V.GUARD, dim), V.SENTINEL, device="cuda")
    assert _nmf_call(node_in, img, s5d, s6d, b5, b6, res, out, rows, dim) == 0
    assert _status_bits() == 0
    assert bool((out[rows:] == V.SENTINEL).all()), "guard rows behind M written"
    err = (out[:rows].double().cpu() - c.ref).abs()
    ratio = float((err / c.bar).max())
    print(f"node_mlp_fused dim {dim} rows {rows}: error / bar {_note(f'node_mlp_fused_kernel<{dim // 16}>', ratio, 1.0):.3f}")
    assert ratio <= 1.0, (ratio, float(err.max()))
    hid = _ops.linear_hl(node_in, s5d, 2 * dim, b5, act=1, out_f32=False, out_hl=True)
    two = _ops.linear_hl(hid, s6d, dim, b6, residual=res)
    assert float((out[:rows] - two).abs().max()) <= 1e-5 * max(1.0, float(c.ref.abs().max()))
    again = torch.full((rows + V.GUARD, dim), V.SENTINEL, device="cuda")
    assert _nmf_call(node_in, img, s5d, s6d, b5, b6, res, again, rows, dim) == 0
    assert torch.equal(out, again)
    assert torch.equal(_ops.node_mlp_fused(node_in, img, s5d[2], b5, s6d[2], b6, res, dim, 16), out[:rows])


@pytest.mark.parametrize("dim", V.NMF_DIMS)
def test_node_mlp_fused_range_flag_and_refusals(dim):
    from egnn_pytorch_amd import _ops
    rows = 17
    c = V.nmf_case(dim, rows)
    s5d, s6d, img = _nmf_device(dim, c)
    node_in = _ops.split_f16(c.x.cuda())
    b6, res = c.b6.cuda(), c.res.cuda()
    out = torch.full((rows + V.GUARD, dim), V.SENTINEL, device="cuda")
    for value, flag in ((65504.0 + 64, 1), (65000.0, 0)):                        # a hidden activation SiLU(b5 + ...) of that size in one unit
        b5 = c.b5.clone()
        b5[2 * dim - 1] = value
        assert _status_bits() == 0
        assert _nmf_call(node_in, img, s5d, s6d, b5.cuda(), b6, res, out, rows, dim) == 0
        assert _status_bits() == flag, (value, flag)
    b5 = c.b5.cuda()
    out.fill_(V.SENTINEL)
    lib = _lib()
    args = [node_in.hi.data_ptr(), node_in.lo.data_ptr(), img.data_ptr(), float(s5d[2]), b5.data_ptr(), float(s6d[2]), b6.data_ptr(), res.data_ptr(),
            out.data_ptr(), rows, dim, 16, None, _stream()]
    for at in (0, 1, 2, 4, 6, 7, 8):
        bad = list(args)
        bad[at] = None
        assert lib.egnn_node_mlp_fused_f32(*bad) == V.E_NULLPTR, at
    for at, value, code in ((9, 0, V.E_SHAPE), (10, dim + 16, V.E_UNSUPPORTED), (11, 8, V.E_UNSUPPORTED), (3, 0.0, V.E_SHAPE), (5, -1.0, V.E_SHAPE)):
        bad = list(args)
        bad[at] = value
        assert lib.egnn_node_mlp_fused_f32(*bad) == code, at
    torch.cuda.synchronize()
    assert bool((out == V.SENTINEL).all())
    assert not V.nmf_supported(dim + 16, 16) and not _ops.node_mlp_fused_supported(dim + 16, 16) and not _ops.node_mlp_fused_supported(dim, 8)
