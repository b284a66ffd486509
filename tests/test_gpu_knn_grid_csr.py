"""The cell-grid k-NN selection with a `SparseAdjacency` on the MI355X (csrc/knn_grid.hip; egnn_knn_select_grid_csr_f32): bit-identical
to the CSR selection of the all-pairs kernels (`_ops.knn_select` with the same object, itself pinned to the dense-adjacency kernels) on
every shape, mask, adjacency and geometry; against the oracle on sampled rows of a 70 000-node graph; layers, training steps, networks
and captured graphs routed to it.  Every comparison is bit equality: indices equal, ranks equal as int32 views."""
import numpy as np
import pytest
import torch

from tests.test_gpu_large_graphs import _dev, _sampled_topk

pytestmark = pytest.mark.gpu


def _SA():
    from egnn_pytorch_amd import SparseAdjacency
    return SparseAdjacency


def _assert_same(got, ref):
    assert torch.equal(got[0], ref[0])
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def _grid_twice_equals_pinned(coors, mask, sa, k):
    from egnn_pytorch_amd import _ops
    c, m = _dev(coors), _dev(mask)
    ref = _ops.knn_select(c, m, sa, k)
    got = _ops.knn_select_grid(c, m, k, adj=sa)
    got2 = _ops.knn_select_grid(c, m, k, adj=sa)
    _assert_same(got, ref)
    _assert_same(got2, got)


def _ragged(rng, b, n, k):
    lens = rng.integers(max(k, n // 2), n + 1, size=b)
    return np.arange(n)[None, :] < lens[:, None]


def _edges(kind, n, rng):
    """(2, E) int64 directed edges of one graph"""
    i = np.arange(n)
    if kind == "empty":
        src = dst = i[:0]
    elif kind == "chain":
        src, dst = np.concatenate([i, i[:-1], i[1:]]), np.concatenate([i, i[1:], i[:-1]])
    elif kind == "chain_nodiag":
        src, dst = np.concatenate([i[:-1], i[1:]]), np.concatenate([i[1:], i[:-1]])
    elif kind == "random6":                                               # over ALL indices: to and from masked nodes too
        src, dst = np.repeat(i, 6), rng.integers(0, n, 6 * n)
    elif kind in ("hub", "hub_masked"):                                   # row 0 bonded to every other node, and back
        src, dst = np.concatenate([np.zeros(n - 1, dtype=np.int64), i[1:]]), np.concatenate([i[1:], np.zeros(n - 1, dtype=np.int64)])
    else:
        raise KeyError(kind)
    return np.stack([src, dst]).astype(np.int64)


def _sparse(kind, n, rng, graphs=None):
    """the adjacency `kind` on the device: one graph's rows shared by the batch (graphs=None) or `graphs` graphs of their own"""
    if graphs is None:
        return _SA().from_edge_index(torch.from_numpy(_edges(kind, n, rng)), n).to("cuda")
    per = [_edges(kind, n, rng) for _ in range(graphs)]
    gid = np.concatenate([np.full(e.shape[1], g, dtype=np.int64) for g, e in enumerate(per)])
    return _SA().from_edge_index(torch.from_numpy(np.concatenate(per, axis=1)), n, graph=torch.from_numpy(gid), num_graphs=graphs).to("cuda")


# ------------------------------------------------------------------ a. the grid with CSR rows equals the pinned CSR selection
SHAPES = [
    # (B, N, K, mask kind)
    (1, 1, 1, None), (3, 16, 4, None), (3, 33, 33, "ragged"), (3, 100, 7, "ragged"), (2, 1000, 32, "scattered"),
    (1, 9000, 128, None), (2, 300, 40, "one_graph_empty"), (1, 600, 32, "fewer_than_k"),
]
ADJ = ("empty", "chain", "chain_nodiag", "random6", "random6_batched", "hub", "hub_masked")
CASES = [(b, n, k, kind, adj) for b, n, k, kind in SHAPES for adj in ADJ if not (adj == "hub_masked" and kind is None)]


def _mask(kind, rng, b, n, k):
    if kind == "ragged":
        return _ragged(rng, b, n, k)
    if kind == "scattered":
        return rng.random((b, n)) < 0.6
    if kind == "one_graph_empty":
        mask = rng.random((b, n)) < 0.7
        mask[1] = False
        return mask
    if kind == "fewer_than_k":                                            # every selection holds padded nodes
        mask = np.zeros((b, n), dtype=bool)
        mask[0, rng.permutation(n)[:k - 5]] = True
        return mask
    return None


@pytest.mark.parametrize("b,n,k,kind,adj", CASES, ids=[f"b{b}-n{n}-k{k}-{kind}-{adj}" for b, n, k, kind, adj in CASES])
def test_knn_select_grid_csr_equals_the_pinned_csr_selection(b, n, k, kind, adj):
    rng = np.random.default_rng(n * 7 + k * 3 + b)
    coors = rng.standard_normal((b, n, 3)).astype(np.float32)
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
    if adj == "empty":
        assert sa.col.numel() == 0                                        # (the entry receives col = NULL)
    if adj.startswith("hub") and n > 1:
        assert sa.max_degree() == n - 1
    _grid_twice_equals_pinned(coors, mask, sa, k)


# ------------------------------------------------------------------ b. geometries
def _geometry(name, rng, b, n):
    if name == "normal":
        return rng.standard_normal((b, n, 3))
    if name == "uniform":
        return rng.random((b, n, 3))
    if name == "clusters_and_outlier":                                    # two clusters 1e3 apart and one node at 1e6
        c = rng.standard_normal((b, n, 3))
        c[:, n // 2:, 0] += 1e3
        c[:, 7] = 1e6
        return c
    if name == "one_point":                                               # adjacent nodes (0) and every other node (d^2 = 0) tie by index
        return np.full((b, n, 3), 0.75)
    if name == "lattice_x40":                                             # long runs of equal keys across the K boundary
        base = rng.integers(-3, 4, size=(b, n // 40, 3)).astype(np.float64)
        c = np.repeat(base, 40, axis=1)
        return np.stack([c[g, rng.permutation(n)] for g in range(b)])
    if name == "collinear":                                               # zero box extent on two axes
        c = np.zeros((b, n, 3))
        c[..., 1] = rng.standard_normal((b, n))
        c[..., 0], c[..., 2] = 2.5, -1.0
        return c
    if name == "normal_x400":                                             # valid rows handed over to the flagged CSR streaming kernel
        return rng.standard_normal((b, n, 3)) * 400.0
    raise KeyError(name)


GEOMETRIES = ("normal", "uniform", "clusters_and_outlier", "one_point", "lattice_x40", "collinear", "normal_x400")
GEO_CASES = [(name, 16) for name in GEOMETRIES] + [("one_point", 1), ("one_point", 2)]


@pytest.mark.parametrize("name,k", GEO_CASES, ids=[f"{name}-k{k}" for name, k in GEO_CASES])
def test_knn_select_grid_csr_on_geometries(name, k):
    b, n = 2, 2000
    rng = np.random.default_rng(GEOMETRIES.index(name) + 100)
    coors = _geometry(name, rng, b, n).astype(np.float32)
    mask = _ragged(rng, b, n, 16)
    mask[:, 7] = True                                                     # (the outlier is a real node)
    ei = np.concatenate([_edges("random6", n, rng), _edges("chain", n, rng)], axis=1)
    sa = _SA().from_edge_index(torch.from_numpy(ei), n).to("cuda")
    _grid_twice_equals_pinned(coors, mask, sa, k)


# ------------------------------------------------------------------ c. 70 000 nodes: sampled rows against the oracle, all rows against the CSR kernel
def test_knn_select_grid_csr_on_70000_nodes():
    from egnn_pytorch_amd import _ops
    n, k = 70000, 32
    rng = np.random.default_rng(n)
    coors = rng.standard_normal((1, n, 3)).astype(np.float32)
    mask = (np.arange(n) < n - 1234)[None, :]                            # the tail is padding
    src = np.concatenate([np.repeat(np.arange(n), 3), rng.integers(0, n, 3 * n), np.arange(n)])
    dst = np.concatenate([rng.integers(0, n, 3 * n), np.repeat(np.arange(n), 3), np.arange(n)])
    sa = _SA().from_edge_index(torch.from_numpy(np.stack([src, dst])), n).to("cuda")
    rows = np.sort(np.concatenate([rng.choice(n, 250, replace=False), [0, n - 1, n - 1234, n - 1235, 5, 6]]))
    rp, col = sa.rowptr.cpu().numpy()[0], sa.col.cpu().numpy()
    adj_rows = np.zeros((rows.size, n), dtype=bool)
    for r, i in enumerate(rows):
        adj_rows[r, col[rp[i]:rp[i + 1]]] = True
    ref_val, ref_idx = _sampled_topk(coors, mask, adj_rows, rows, k)
    c, m = _dev(coors), _dev(mask)
    idx, rank = _ops.knn_select_grid(c, m, k, adj=sa)
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy()[0, rows])
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy()[0, rows].view(np.uint32))
    _assert_same((idx, rank), _ops.knn_select(c, m, sa, k))


# ------------------------------------------------------------------ d. routing
def _chain_contacts(n, diag=True):
    """a chain with sparse contacts (about 3 bonds per row), as (2, E) int64"""
    i = torch.arange(n)
    a = torch.arange(0, n - 40, 97)
    src = torch.cat([i[:-1], i[1:], a, a + 31] + ([i] if diag else []))
    dst = torch.cat([i[1:], i[:-1], a + 31, a] + ([i] if diag else []))
    return torch.stack([src, dst])


LAYERS = {
    "knn_with_adjacency": (dict(num_nearest_neighbors=8), False),
    "only_sparse_neighbors": (dict(only_sparse_neighbors=True), False),
    "radius_norm_mean_masked": (dict(num_nearest_neighbors=6, valid_radius=1.5, norm_coors=True, m_pool_method="mean"), True),
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_with_sparse_adjacency_takes_the_grid_and_equals_the_all_pairs_route(name, monkeypatch):
    from egnn_pytorch_amd import EGNN, _ops, layer as L
    kw, with_mask = LAYERS[name]
    n, dim = 4096, 16
    torch.manual_seed(3)
    layer = EGNN(dim=dim, **kw).cuda()
    feats = torch.randn(1, n, dim, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    mask = (torch.rand(1, n, device="cuda") < 0.8) if with_mask else None
    sa = _SA().from_edge_index(_chain_contacts(n), n).to("cuda")
    dense = sa.to_dense()

    def run(adj):
        with torch.no_grad(), _ops.phase_timer() as t:
            out = layer(feats, coors, mask=mask, adj_mat=adj)
        return out, t.summary()

    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", 64)
    if hasattr(L, "_KNN_GRID_ADJ_MIN_N"):
        monkeypatch.setattr(L, "_KNN_GRID_ADJ_MIN_N", 64)
    (node, co), names = run(sa)
    assert "knn_select_grid" in names and "knn_select" not in names
    (dn, dc), names = run(dense)
    assert "knn_select" in names and "knn_select_grid" not in names
    assert torch.equal(node, dn) and torch.equal(co, dc)
    with torch.no_grad():
        node2, co2 = layer(feats, coors, mask=mask, adj_mat=sa)           # (untimed: the selection on the side stream)
    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
    if hasattr(L, "_KNN_GRID_ADJ_MIN_N"):
        monkeypatch.setattr(L, "_KNN_GRID_ADJ_MIN_N", n + 1)
    (rn, rc), names = run(sa)
    assert "knn_select" in names and "knn_select_grid" not in names
    assert torch.equal(node, rn) and torch.equal(co, rc)
    assert torch.equal(node2, rn) and torch.equal(co2, rc)


def test_layer_at_262144_nodes_with_sparse_adjacency_takes_the_grid_by_default():
    from egnn_pytorch_amd import EGNN, _ops
    n, dim = 262144, 16
    torch.manual_seed(4)
    layer = EGNN(dim=dim, num_nearest_neighbors=8).cuda()
    feats = torch.randn(1, n, dim, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    sa = _SA().from_edge_index(_chain_contacts(n), n).to("cuda")
    with torch.no_grad(), _ops.phase_timer() as t:
        node, co = layer(feats, coors, adj_mat=sa)
    names = t.summary()
    assert "knn_select_grid" in names and "knn_select" not in names
    assert node.shape == (1, n, dim) and co.shape == (1, n, 3)
    assert torch.isfinite(node).all() and torch.isfinite(co).all()


# ------------------------------------------------------------------ e. training
def test_training_step_at_70000_nodes_with_sparse_adjacency_equals_the_all_pairs_route(monkeypatch):
    from egnn_pytorch_amd import EGNN, layer as L
    n, dim = 70000, 16
    torch.manual_seed(1)
    layer = EGNN(dim=dim, num_nearest_neighbors=8).cuda()
    feats = torch.randn(1, n, dim, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    sa = _sparse("chain", n, None)

    def step():
        f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        node, co = layer(f, c, adj_mat=sa)
        (node.square().mean() + co.square().mean()).backward()
        return [node.detach(), co.detach(), f.grad, c.grad] + [p.grad for p in layer.parameters()]

    assert L.EGNN._use_grid(layer, coors, sa, 8)
    got = step()
    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
    if hasattr(L, "_KNN_GRID_ADJ_MIN_N"):
        monkeypatch.setattr(L, "_KNN_GRID_ADJ_MIN_N", n + 1)
    assert not L.EGNN._use_grid(layer, coors, sa, 8)
    ref = step()
    assert len(got) == len(ref) and all(g is not None for g in got[:4])
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert torch.equal(g, r)


# ------------------------------------------------------------------ f. networks with adjacency degrees
@pytest.mark.parametrize("kw", [dict(num_nearest_neighbors=6), dict(num_nearest_neighbors=6, only_sparse_neighbors=True)],
                         ids=["knn", "only_sparse_neighbors"])
def test_network_with_adjacency_degrees_grid_route_equals_the_all_pairs_route(kw, monkeypatch):
    from egnn_pytorch_amd import EGNN_Network, _ops, layer as L
    n = 8192
    torch.manual_seed(5)
    net = EGNN_Network(num_tokens=20, dim=16, depth=2, num_adj_degrees=2, adj_dim=4, **kw).cuda()
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    sa = _sparse("chain", n, None)

    def run():
        with torch.no_grad(), _ops.phase_timer() as t:
            out = net(tokens, coors, adj_mat=sa)
        return out, t.summary()

    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", 64)
    if hasattr(L, "_KNN_GRID_ADJ_MIN_N"):
        monkeypatch.setattr(L, "_KNN_GRID_ADJ_MIN_N", 64)
    (h, x), names = run()
    assert "knn_select_grid" in names and "knn_select" not in names
    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
    if hasattr(L, "_KNN_GRID_ADJ_MIN_N"):
        monkeypatch.setattr(L, "_KNN_GRID_ADJ_MIN_N", n + 1)
    (rh, rx), names = run()
    assert "knn_select" in names and "knn_select_grid" not in names
    assert torch.equal(h, rh) and torch.equal(x, rx)


# ------------------------------------------------------------------ g. graphed(): no host synchronisation in the selection
def test_graphed_layer_at_70000_nodes_with_sparse_adjacency_replays_to_the_eager_result():
    from egnn_pytorch_amd import EGNN, graphed
    n, dim = 70000, 16
    torch.manual_seed(2)
    layer = EGNN(dim=dim, num_nearest_neighbors=8).cuda()
    feats = torch.randn(1, n, dim, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    sa = _SA().from_edge_index(_chain_contacts(n), n).to("cuda")
    assert sa.shared
    with torch.no_grad():
        ref_node, ref_co = layer(feats, coors, adj_mat=sa)
        g = graphed(layer, feats, coors, adj_mat=sa)
        out = g(feats, coors, adj_mat=sa)
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref_node) and torch.equal(out[1], ref_co)


# ------------------------------------------------------------------ h. the entry on the device
def test_grid_csr_entry_argument_checks_launch_nothing_and_null_col_is_an_empty_adjacency():
    from egnn_pytorch_amd import _abi, _ops
    lib = _abi.load()
    n, k = 500, 8
    coors = torch.randn(1, n, 3, device="cuda")
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    idx = torch.full((1, n, k), -7, dtype=torch.int32, device="cuda")
    rank = torch.full((1, n, k), -7.0, device="cuda")
    nbytes = lib.egnn_knn_grid_workspace_bytes(1, n, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = _ops._stream()

    def call(c=coors, rp=rowptr, stride=0, i=idx, r=rank, w=ws, nn=n, kk=k, cdim=3, wb=nbytes):
        return lib.egnn_knn_select_grid_csr_f32(_ops._ptr(c), None, _ops._ptr(rp), None, stride, 1, nn, kk, cdim, _ops._ptr(i), _ops._ptr(r),
                                                _ops._ptr(w), wb, st)

    assert call(c=None) == -1 and call(rp=None) == -1 and call(i=None) == -1 and call(r=None) == -1 and call(w=None) == -1
    assert call(kk=n + 1) == -2 and call(nn=0) == -2 and call(kk=0) == -2 and call(wb=nbytes - 1) == -2 and call(stride=n) == -2
    assert call(cdim=2) == -3 and call(kk=_ops.KNN_GRID_KMAX + 1) == -3
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((rank == -7.0).all()) and not bool(ws.any())
    assert call() == 0                                                    # col = NULL, every row empty
    assert call(stride=n + 1) == 0
    torch.cuda.synchronize()
    empty = _SA().from_edge_index(torch.zeros(2, 0, dtype=torch.int64), n).to("cuda")
    _assert_same((idx, rank), _ops.knn_select(coors, None, empty, k))
