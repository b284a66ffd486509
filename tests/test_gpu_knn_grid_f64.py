"""The cell-grid k-NN selection for float64 coordinates on the MI355X (csrc/knn_grid.hip; egnn_knn_select_grid_f64 / _grid_csr_f64):
bit-identical to the pinned float64 selection (`_ops.knn_select`, with and without a `SparseAdjacency`) on every shape, mask, adjacency
and geometry of the fp32 grid's tests, and on three geometries only float64 can get wrong; the row flags show that the grid itself
answered (not the streaming kernel it hands rows to); against the oracle on sampled rows at 70 000 and 262 144 nodes; float64 layers,
a training step and a call with a SparseAdjacency routed to it from 65 537 nodes; the entries' argument checks.  Every comparison is
bit equality: indices equal, ranks equal as int64 views."""
import numpy as np
import pytest
import torch

from tests.test_gpu_knn_grid import GEOMETRIES as GEOMETRIES_F32
from tests.test_gpu_knn_grid import SHAPES, _geometry, _ragged
from tests.test_gpu_knn_grid_csr import ADJ, _edges, _mask, _SA, _sparse
from tests.test_gpu_knn_grid_csr import SHAPES as CSR_SHAPES
from tests.test_gpu_large_graphs import _dev, _sampled_topk

pytestmark = pytest.mark.gpu


def _assert_same(got, ref):
    assert got[1].dtype == ref[1].dtype == torch.float64 and got[0].dtype == torch.int32
    assert torch.equal(got[0], ref[0])
    assert torch.equal(got[1].view(torch.int64), ref[1].view(torch.int64))


def _grid_with_flags(c, m, k, sa=None):
    """the selection on a workspace of the test's own, and the (B, N) row flags it left there: 0 = the grid wrote the row itself,
    1 = it handed the row to the streaming kernel"""
    from egnn_pytorch_amd import _abi, _ops
    lib = _abi.load()
    b, n = c.shape[:2]
    ws = torch.zeros(lib.egnn_knn_grid_workspace_bytes_f64(b, n, k), dtype=torch.uint8, device="cuda")
    out = _ops.knn_select_grid(c, m, k, ws=ws, adj=sa)
    off = lib.egnn_knn_grid_rowflag_offset_f64(b, n)
    return out, ws[off:off + b * n].view(b, n).clone()


def _grid_twice_equals_pinned(coors, mask, k, sa=None):
    """-> the row flags of the first call"""
    from egnn_pytorch_amd import _ops
    assert coors.dtype == np.float64
    c, m = _dev(coors), _dev(mask)
    ref = _ops.knn_select(c, m, sa, k)
    got, flags = _grid_with_flags(c, m, k, sa)
    got2 = _ops.knn_select_grid(c, m, k, adj=sa)
    _assert_same(got, ref)
    _assert_same(got2, got)
    return flags


def _valid(mask, b, n):
    return torch.ones(b, n, dtype=torch.bool, device="cuda") if mask is None else _dev(mask)


# ------------------------------------------------------------------ a. the grid equals the pinned float64 selection, bit for bit
def _check_shape_flags(flags, mask, b, n, k):
    """unit-normal coordinates: a graph with fewer than K valid nodes (none at all included) is handed over whole -- fewer_than_k, the
    empty graph of one_graph_empty, K = N = 33 with the hub masked -- and in every other graph no valid row is: about 16 nodes per cell,
    K-th d^2 far below 1e5"""
    valid = _valid(mask, b, n)
    whole = 0
    for g in range(b):
        if int(valid[g].sum()) < k:
            assert bool((flags[g] == 1).all())
            whole += 1
        else:
            assert not bool(flags[g][valid[g]].any())
    return whole


@pytest.mark.parametrize("b,n,k,kind", SHAPES, ids=[f"b{b}-n{n}-k{k}-{kind}" for b, n, k, kind in SHAPES])
def test_knn_select_grid_f64_equals_the_pinned_selection(b, n, k, kind):
    rng = np.random.default_rng(n * 7 + k * 3 + b)
    coors = rng.standard_normal((b, n, 3))
    mask = _mask(kind, rng, b, n, k)
    if kind == "few_hundred":                                             # only 500-600 valid nodes in the graph
        mask = _ragged(rng, b, n, k, 500, 600)
    flags = _grid_twice_equals_pinned(coors, mask, k)
    assert _check_shape_flags(flags, mask, b, n, k) == {"fewer_than_k": 1, "one_graph_empty": 1}.get(kind, 0)


CSR_CASES = [(b, n, k, kind, adj) for b, n, k, kind in CSR_SHAPES for adj in ADJ if not (adj == "hub_masked" and kind is None)]


@pytest.mark.parametrize("b,n,k,kind,adj", CSR_CASES, ids=[f"b{b}-n{n}-k{k}-{kind}-{adj}" for b, n, k, kind, adj in CSR_CASES])
def test_knn_select_grid_csr_f64_equals_the_pinned_csr_selection(b, n, k, kind, adj):
    rng = np.random.default_rng(n * 7 + k * 3 + b)
    coors = rng.standard_normal((b, n, 3))
    mask = _mask(kind, rng, b, n, k)
    if mask is not None and adj == "hub":
        mask[mask.any(axis=1), 0] = True                                  # (the hub is a real node of every graph that has one)
    if adj == "hub_masked":
        mask[:, 0] = False
    if adj == "random6_batched":
        sa = _sparse("random6", n, rng, graphs=b)
        assert sa.batched and sa.num_graphs == b
    else:
        sa = _sparse(adj, n, rng)
        assert sa.shared
    flags = _grid_twice_equals_pinned(coors, mask, k, sa)
    whole = _check_shape_flags(flags, mask, b, n, k)
    assert whole == {"fewer_than_k": 1, "one_graph_empty": 1}.get(kind, 0) + (b if (adj == "hub_masked" and k == n) else 0)


# ------------------------------------------------------------------ b. geometries, c. the grid answers them itself
def _geometry_f64(name, rng, b, n):
    if name == "below_f32":                                               # neighbours decided by bits a cast to float destroys
        base = rng.integers(1, 10, size=(b, n, 3)).astype(np.float32) * np.float32(0.125)         # (no zero: 1e-10 survives a cast there)
        return base.astype(np.float64) + 1e-10 * rng.standard_normal((b, n, 3))
    if name == "offset_1e7":
        return rng.standard_normal((b, n, 3)) + 1e7
    if name == "extent_1e30":                                             # one real node at 1e30: the graph is handed over whole
        c = rng.standard_normal((b, n, 3))
        c[:, 7] = 1e30
        return c
    return _geometry(name, rng, b, n).astype(np.float64)


GEOMETRIES = GEOMETRIES_F32 + ("below_f32", "offset_1e7", "extent_1e30")
# no valid row may be left to the streaming kernel: 16 nodes per cell on average, no cell near max(4096, N / 64) nodes, K-th d^2 far below
# 1e5 (one_point: a single cell of at most 2000 nodes, every d^2 = 0)
ANSWERED_BY_THE_GRID = ("normal", "uniform", "one_point", "below_f32", "offset_1e7")
HANDED_OVER_WHOLE = ("extent_1e30",)                                      # exempt, and asserted to BE flagged: an extent beyond 1e18


@pytest.mark.parametrize("with_adj", [False, True], ids=["no_adjacency", "csr"])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_knn_select_grid_f64_on_geometries(name, with_adj):
    b, n, k = 2, 2000, 16
    rng = np.random.default_rng(GEOMETRIES.index(name) + 100)
    coors = _geometry_f64(name, rng, b, n)
    assert coors.dtype == np.float64
    if name == "below_f32":                                               # (the cast collapses the lattice's points onto each other)
        assert np.unique(coors[0].astype(np.float32), axis=0).shape[0] < n // 2 < np.unique(coors[0], axis=0).shape[0]
    mask = _ragged(rng, b, n, k)
    mask[:, 7] = True                                                     # (the outlier is a real node)
    sa = None
    if with_adj:
        ei = np.concatenate([_edges("random6", n, rng), _edges("chain", n, rng)], axis=1)
        sa = _SA().from_edge_index(torch.from_numpy(ei), n).to("cuda")
    flags = _grid_twice_equals_pinned(coors, mask, k, sa)
    if name in ANSWERED_BY_THE_GRID:
        assert not bool(flags[_dev(mask)].any())
    if name in HANDED_OVER_WHOLE:
        assert bool((flags == 1).all())


# ------------------------------------------------------------------ d. beyond the pinned kernels' comfort: sampled rows against the oracle
@pytest.mark.parametrize("n", [70000, 262144])
def test_knn_select_grid_f64_large_sampled_rows(n):
    from egnn_pytorch_amd import _ops
    k = 32
    rng = np.random.default_rng(n + k)
    coors = rng.standard_normal((1, n, 3))
    mask = (np.arange(n) < n - 1234)[None, :]                            # ragged: the tail is padding
    rows = np.sort(np.concatenate([rng.choice(n, 256, replace=False), [0, n - 1, n - 1234, n - 1235, 5, 6]]))
    c, m = _dev(coors), _dev(mask)
    (idx, rank), flags = _grid_with_flags(c, m, k)
    assert not bool(flags[m].any())                                       # every valid row answered by the grid
    got_idx, got_rank = idx.cpu().numpy()[0, rows], rank.cpu().numpy()[0, rows]
    for lo in range(0, rows.size, 64):                                    # (64 rows of the (rows, N, 3) differences at a time)
        ref_val, ref_idx = _sampled_topk(coors, mask, None, rows[lo:lo + 64], k)
        assert ref_val.dtype == np.float64
        np.testing.assert_array_equal(ref_idx.astype(np.int32), got_idx[lo:lo + 64])
        np.testing.assert_array_equal(ref_val.view(np.uint64), got_rank[lo:lo + 64].view(np.uint64))
    if n == 70000:
        _assert_same((idx, rank), _ops.knn_select_stream(c, m, None, k))


# ------------------------------------------------------------------ e. float64 layers
def _layer_and_inputs(n, dim=16, k=8, seed=0):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed)
    layer = EGNN(dim=dim, num_nearest_neighbors=k).cuda().double()
    feats = torch.randn(1, n, dim, device="cuda", dtype=torch.float64)
    coors = torch.randn(1, n, 3, device="cuda", dtype=torch.float64)
    return layer, feats, coors


@pytest.mark.parametrize("with_adj", [False, True], ids=["no_adjacency", "chain"])
def test_float64_layer_at_70000_nodes_takes_the_grid_and_equals_the_all_pairs_route(with_adj, monkeypatch):
    from egnn_pytorch_amd import _ops, layer as L
    n = 70000
    layer, feats, coors = _layer_and_inputs(n)
    sa = _sparse("chain", n, None) if with_adj else None
    with torch.no_grad():
        with _ops.phase_timer() as t:
            node, co = layer(feats, coors, adj_mat=sa)
        names = t.summary()
        assert "knn_select_grid" in names and "knn_select" not in names
        node2, co2 = layer(feats, coors, adj_mat=sa)                      # (untimed)
        monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
        with _ops.phase_timer() as t:
            ref_node, ref_co = layer(feats, coors, adj_mat=sa)
        names = t.summary()
        assert "knn_select" in names and "knn_select_grid" not in names
    assert node.dtype == co.dtype == torch.float64
    assert torch.equal(node, ref_node) and torch.equal(co, ref_co)
    assert torch.equal(node2, ref_node) and torch.equal(co2, ref_co)


def test_float64_training_step_at_70000_nodes_equals_the_all_pairs_route(monkeypatch):
    from egnn_pytorch_amd import layer as L
    n = 70000
    layer, feats, coors = _layer_and_inputs(n, seed=1)

    def step():
        f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        node, co = layer(f, c)
        (node.square().mean() + co.square().mean()).backward()
        return [node.detach(), co.detach(), f.grad, c.grad] + [p.grad for p in layer.parameters()]

    assert L.EGNN._use_grid(layer, coors, None, 8)                        # (forward and backward share the one list)
    got = step()
    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
    assert not L.EGNN._use_grid(layer, coors, None, 8)
    ref = step()
    assert len(got) == len(ref) and all(g is not None for g in got[:4])
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == torch.float64 and torch.equal(g, r)


def test_float64_layer_at_40000_nodes_keeps_the_all_pairs_selection():
    from egnn_pytorch_amd import _ops
    layer, feats, coors = _layer_and_inputs(40000)
    with torch.no_grad(), _ops.phase_timer() as t:
        layer(feats, coors)
    names = t.summary()
    assert "knn_select" in names and "knn_select_grid" not in names


def test_other_dtypes_are_refused():
    from egnn_pytorch_amd import _ops
    c = torch.randn(1, 64, 3, device="cuda")
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            _ops.knn_select_grid(c.to(dtype), None, 4)
        with pytest.raises(TypeError):
            _ops.knn_grid_workspace(1, 64, 4, c.device, dtype)
    assert _ops.knn_grid_workspace(1, 64, 4, c.device).numel() < _ops.knn_grid_workspace(1, 64, 4, c.device, torch.float64).numel()


# ------------------------------------------------------------------ f. argument checks on the device
def test_grid_f64_entries_argument_checks_launch_nothing():
    from egnn_pytorch_amd import _abi, _ops
    lib = _abi.load()
    n, k = 500, 8
    coors = torch.randn(1, n, 3, device="cuda", dtype=torch.float64)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    idx = torch.full((1, n, k), -7, dtype=torch.int32, device="cuda")
    rank = torch.full((1, n, k), -7.0, device="cuda", dtype=torch.float64)
    nbytes = lib.egnn_knn_grid_workspace_bytes_f64(1, n, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = _ops._stream()

    def call(c=coors, i=idx, r=rank, w=ws, nn=n, kk=k, cdim=3, wb=nbytes):
        return lib.egnn_knn_select_grid_f64(_ops._ptr(c), None, 1, nn, kk, cdim, _ops._ptr(i), _ops._ptr(r), _ops._ptr(w), wb, st)

    def call_csr(c=coors, rp=rowptr, stride=0, i=idx, r=rank, w=ws, nn=n, kk=k, cdim=3, wb=nbytes):
        return lib.egnn_knn_select_grid_csr_f64(_ops._ptr(c), None, _ops._ptr(rp), None, stride, 1, nn, kk, cdim, _ops._ptr(i), _ops._ptr(r),
                                                _ops._ptr(w), wb, st)

    for f in (call, call_csr):
        assert f(c=None) == -1 and f(i=None) == -1 and f(r=None) == -1 and f(w=None) == -1                # EGNN_E_NULLPTR
        assert f(kk=n + 1) == -2 and f(nn=0) == -2 and f(kk=0) == -2                                      # EGNN_E_SHAPE
        assert f(wb=nbytes - 1) == -2                                                                     # one byte short
        assert f(wb=lib.egnn_knn_grid_workspace_bytes(1, n, k)) == -2                                     # (the fp32 size)
        assert f(cdim=2) == -3 and f(kk=_ops.KNN_GRID_KMAX + 1) == -3                                     # EGNN_E_UNSUPPORTED
        assert f(w=ws[4:]) == -4                                                                          # EGNN_E_ALIGN
    assert call_csr(rp=None) == -1 and call_csr(stride=n) == -2
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((rank == -7.0).all()) and not bool(ws.any())
    assert call() == 0
    torch.cuda.synchronize()
    ref = _ops.knn_select(coors, None, None, k)
    _assert_same((idx, rank), ref)
    assert call_csr() == 0 and call_csr(stride=n + 1) == 0                # col = NULL, every row empty
    torch.cuda.synchronize()
    empty = _SA().from_edge_index(torch.zeros(2, 0, dtype=torch.int64), n).to("cuda")
    _assert_same((idx, rank), _ops.knn_select(coors, None, empty, k))
