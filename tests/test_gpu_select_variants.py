"""Every template instantiation and every run-time route of the neighbour selection kernels (csrc/knn_select.hip, knn_rows.hip,
knn_stream.hip, knn_segments.hip, knn_grid.hip) on the MI355X against the oracle's ranking, cell by cell (tests/_select_variants.py; its
host checks are tests/test_select_variants_table.py).  The contract is equality: indices equal, ranks equal on their bit patterns --
there is no tolerance in this file.  Outputs start poisoned (idx = -7, rank = NaN) and no poison may survive; a refused call returns
the code the restated launcher predicts and leaves the poison untouched."""
import numpy as np
import pytest
import torch

from tests import _select_variants as V

pytestmark = pytest.mark.gpu
POISON_IDX = -7


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _poisoned(*shape, dtype):
    idx = torch.full(shape, POISON_IDX, dtype=torch.int32, device="cuda")
    rank = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    return idx, rank


def _torch_dtype(t):
    return torch.float32 if t == "f" else torch.float64


def _bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _sparse(d):
    from egnn_pytorch_amd import SparseAdjacency
    return SparseAdjacency.from_dense(_dev(d.adj))


# The flagged streaming entries (csrc/egnn_common.h: egnn_knn_stream_flagged_*, defined in csrc/knn_stream.hip) are what the cell-grid
# selection calls for the rows it hands over.  They are internal C++ functions of the library, not part of the C ABI of
# include/egnn_hip.h, so they are looked up under their C++ symbol names: (coors, mask, [rowptr, col, rowptr_graph_stride,] B, N, K,
# rowflag, idx_out, rank_out, stream).
FLAGGED = {("stream", "f"): "_Z27egnn_knn_stream_flagged_f32PKfPKhiiiS2_PiPfPv", ("stream", "d"): "_Z27egnn_knn_stream_flagged_f64PKdPKhiiiS2_PiPdPv",
           ("csr", "f"): "_Z31egnn_knn_stream_flagged_csr_f32PKfPKhPKlPKiliiiS2_PiPfPv",
           ("csr", "d"): "_Z31egnn_knn_stream_flagged_csr_f64PKdPKhPKlPKiliiiS2_PiPdPv"}


def _call_flagged(c, d):
    """the flagged entry on the cell's operands and hand-made row flags -> (idx, rank) on the host, from poisoned outputs"""
    import ctypes
    from egnn_pytorch_amd import _abi, _ops
    fn = getattr(_abi.load(), FLAGGED[c.entry, c.t])
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fn.restype = i32
    fn.argtypes = [vp, vp] + ([vp, vp, i64] if c.entry == "csr" else []) + [i32, i32, i32, vp, vp, vp, vp]
    co, mask, flags = _dev(d.coors), _dev(d.mask).view(torch.uint8), _dev(d.flags)
    idx, rank = _poisoned(d.b, d.n, d.k, dtype=_torch_dtype(c.t))
    csr = ()
    if c.entry == "csr":
        sa = _sparse(d)
        csr = _ops._csr_args(sa, co)
    rc = fn(co.data_ptr(), mask.data_ptr(), *csr, d.b, d.n, d.k, flags.data_ptr(), idx.data_ptr(), rank.data_ptr(), _ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, (c.id, rc)
    return idx.cpu().numpy(), rank.cpu().numpy()


@pytest.mark.parametrize("cid", [c.id for c in V.RUN if c.group == "flagged"])
def test_flagged_stream_writes_the_flagged_rows_and_no_other(cid):
    """the FL contract: rows with a non-zero flag equal the oracle bit for bit, rows with a zero flag are untouched -- flags mixed inside
    a workgroup of R rows, a workgroup without a flag (it returns at once), a flagged masked row, two graphs with different flags"""
    c = V.BY_ID[cid]
    d = V.prepare(cid)
    idx, rank = _call_flagged(c, d)
    ref_idx, ref_rank = V.reference(cid)
    on = d.flags != 0
    assert on.any() and not on.all()
    assert (idx[~on] == POISON_IDX).all() and np.isnan(rank[~on]).all(), f"{cid}: a row with a zero flag was written"
    assert not (idx[on] == POISON_IDX).any() and not np.isnan(rank[on]).any(), f"{cid}: poison survives in a flagged row"
    np.testing.assert_array_equal(idx[on], ref_idx[on], err_msg=cid)
    np.testing.assert_array_equal(_bits(rank[on]), _bits(ref_rank[on]), err_msg=cid)


def _call(c, d, public=False):
    """the cell's call through its `_ops` wrapper (public: through `knn_select`, the dispatcher) -> (idx, rank, row flags or None) on the
    host, the outputs allocated here with the poison fill"""
    from egnn_pytorch_amd import GraphSegments, _abi, _ops
    dt = _torch_dtype(c.t)
    co, mask = _dev(d.coors), _dev(d.mask)
    flags = None
    if c.entry == "segments":
        out = _poisoned(d.n, d.k, dtype=dt)
        seg = GraphSegments.from_sizes(list(c.p["sizes"]), device="cuda")
        saved = _ops.KNN_SEGMENTS_LDS_NODES
        _ops.KNN_SEGMENTS_LDS_NODES = c.p["lds_nodes"] or None
        try:
            _ops.knn_select_segments(co, seg, d.k, out=out)
        finally:
            _ops.KNN_SEGMENTS_LDS_NODES = saved
            _abi.load().egnn_knn_segments_lds_nodes(0)
    else:
        out = _poisoned(d.b, d.n, d.k, dtype=dt)
        csr = c.entry in ("csr", "grid_csr")
        adj = None if d.adj is None else (_sparse(d) if csr else _dev(d.adj))
        if public or c.entry == "select":
            _ops.knn_select(co, mask, adj, d.k, out=out)
        elif c.entry == "stream":
            _ops.knn_select_stream(co, mask, adj, d.k, out=out)
        elif c.entry == "csr":
            _ops.knn_select_csr(co, mask, adj, d.k, out=out)
        else:
            lib = _abi.load()
            query = lib.egnn_knn_grid_workspace_bytes if c.t == "f" else lib.egnn_knn_grid_workspace_bytes_f64
            ws = torch.zeros(query(d.b, d.n, d.k), dtype=torch.uint8, device="cuda")        # the entry's own size
            _ops.knn_select_grid(co, mask, d.k, out=out, ws=ws, adj=adj)
            off = lib.egnn_knn_grid_rowflag_offset_f64(d.b, d.n)                            # (the same offset for both types)
            flags = ws[off:off + d.b * d.n].view(d.b, d.n).cpu().numpy()
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), flags


def _compare(c, idx, rank, what):
    ref_idx, ref_rank = V.reference(c.id)
    assert not (idx == POISON_IDX).any() and not np.isnan(rank).any(), f"{c.id} ({what}): poison survives in rows the entry owns"
    rows = V.compared_rows(c.id)
    if rows is not None:
        idx, rank = idx[:, rows], rank[:, rows]
    np.testing.assert_array_equal(idx, ref_idx, err_msg=f"{c.id} ({what})")
    np.testing.assert_array_equal(_bits(rank), _bits(ref_rank), err_msg=f"{c.id} ({what})")


@pytest.mark.parametrize("cid", [c.id for c in V.RUN if c.group != "flagged"])
def test_selection_cell_is_bit_equal_to_the_oracle(cid):
    from egnn_pytorch_amd import _ops
    c = V.BY_ID[cid]
    d = V.prepare(cid)
    if c.entry == "maxdeg":
        assert _ops.adj_max_degree(_dev(d.adj)) == int(V.reference(cid)[0])
        return
    idx, rank, flags = _call(c, d)
    _compare(c, idx, rank, "direct")
    if flags is not None:                                        # the grid's claims: who wrote the row
        for tag, where in c.claims:
            for g, row in where:
                assert flags[g, row] == (1 if tag == "handed_to_stream" else 0), (cid, tag, g, row)
        assert set(np.unique(flags).tolist()) <= {0, 1}
    if c.p["public"]:                                            # the same operands through the public dispatcher (at these sizes: ANOTHER kernel of the family): the same bits
        idx2, rank2, _ = _call(c, d, public=True)
        _compare(c, idx2, rank2, "public")
        np.testing.assert_array_equal(idx2, idx)
        np.testing.assert_array_equal(_bits(rank2), _bits(rank))


# ------------------------------------------------------------------------------------------------ refusals: raw arguments
def _raw_call(c):
    """the cell's entry through the C ABI with the raw arguments its wrapper would check away -> (code, idx, rank)"""
    from egnn_pytorch_amd import _abi, _ops
    lib = _abi.load()
    p, raw = c.p, c.p["raw"]
    null = set(raw.get("null", ()))
    dt = _torch_dtype(c.t)
    sfx = "_f32" if c.t == "f" else "_f64"
    ptr = lambda name, t: None if name in null else t.data_ptr()                  # noqa: E731
    st = _ops._stream()
    if c.entry == "maxdeg":
        b, n = raw.get("b", p["b"]), p["n"]
        adj = torch.ones(max(b, 1), n, n, dtype=torch.uint8, device="cuda")
        out = torch.full((1,), POISON_IDX, dtype=torch.int32, device="cuda")
        rc = lib.egnn_adj_max_degree_u8(ptr("adj", adj), b * n, n, ptr("out", out), st)
        return rc, out, None
    if c.entry == "segments":
        sizes = list(p["sizes"])
        t_nodes, k, cd = sum(sizes), raw.get("k", p["k"]), raw.get("c", p["c"])
        co = torch.randn(t_nodes, max(cd, 1), dtype=dt, device="cuda")
        off = torch.from_numpy(V.segment_offsets(sizes)).cuda()
        seg_of = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).cuda()
        idx, rank = _poisoned(t_nodes, max(k, 1), dtype=dt)
        rc = getattr(lib, "egnn_knn_select_segments" + sfx)(ptr("coors", co), ptr("offsets", off), ptr("segment_of", seg_of), raw.get("g", len(sizes)),
                                                            t_nodes, k, cd, raw.get("max_segment", max(sizes)), idx.data_ptr(), rank.data_ptr(), st)
        return rc, idx, rank
    b, n, k, cd = raw.get("b", p["b"]), raw.get("n", p["n"]), raw.get("k", p["k"]), raw.get("c", p["c"])
    co = torch.randn(max(b, 1), n, max(cd, 1), dtype=dt, device="cuda")
    idx, rank = _poisoned(max(b, 1), n, max(k, 1), dtype=dt)
    tail = (b, n, k, cd, ptr("idx", idx), ptr("rank", rank))
    csr = ()
    if c.entry in ("csr", "grid_csr"):
        rowptr = torch.arange(n + 1, dtype=torch.int64, device="cuda")                       # every node adjacent to itself
        col = torch.arange(n, dtype=torch.int32, device="cuda")
        csr = (ptr("rowptr", rowptr), col.data_ptr(), raw.get("rp_stride", 0))
    if c.entry in ("select", "stream"):
        rc = getattr(lib, ("egnn_knn_select" if c.entry == "select" else "egnn_knn_select_stream") + sfx)(ptr("coors", co), None, None, 0, *tail, st)
    elif c.entry == "csr":
        rc = getattr(lib, "egnn_knn_select_csr" + sfx)(ptr("coors", co), None, *csr, *tail, st)
    else:
        query = lib.egnn_knn_grid_workspace_bytes if c.t == "f" else lib.egnn_knn_grid_workspace_bytes_f64
        total = query(max(b, 1), n, max(k, 1))
        ws = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
        ws_ptr = None if "ws" in null else ws.data_ptr() + raw.get("ws_misalign", 0)
        name = ("egnn_knn_select_grid_csr" if csr else "egnn_knn_select_grid") + sfx
        rc = getattr(lib, name)(ptr("coors", co), None, *csr, *tail, ws_ptr, total - raw.get("ws_short", 0), st)
    return rc, idx, rank


@pytest.mark.parametrize("cid", [c.id for c in V.REFUSED])
def test_refused_call_returns_the_predicted_code_and_writes_nothing(cid):
    c = V.BY_ID[cid]
    rc, idx, rank = _raw_call(c)
    torch.cuda.synchronize()
    assert rc == c.expect, (cid, rc)
    assert bool((idx == POISON_IDX).all()) and (rank is None or bool(torch.isnan(rank).all())), cid
