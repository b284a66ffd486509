"""The cell-grid k-NN selection on the MI355X (csrc/knn_grid.hip; egnn_knn_select_grid_f32): bit-identical to the pinned selection
kernels on every shape, mask and geometry they run; against the oracle on sampled rows beyond them; whole layers routed to it from
65 537 nodes, in eager mode, under autograd and inside a captured graph; the entry's argument checks."""
import numpy as np
import pytest
import torch

from tests.test_gpu_large_graphs import _dev, _sampled_topk

pytestmark = pytest.mark.gpu


def _assert_same(got, ref):
    assert torch.equal(got[0], ref[0])
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def _grid_twice_equals_pinned(coors, mask, k):
    from egnn_pytorch_amd import _ops
    c, m = _dev(coors), _dev(mask)
    ref = _ops.knn_select(c, m, None, k)
    got = _ops.knn_select_grid(c, m, k)
    got2 = _ops.knn_select_grid(c, m, k)
    _assert_same(got, ref)
    _assert_same(got2, got)


def _ragged(rng, b, n, k, lo=None, hi=None):
    lens = rng.integers(max(k, n // 2) if lo is None else lo, (n + 1) if hi is None else hi, size=b)
    return np.arange(n)[None, :] < lens[:, None]


# ------------------------------------------------------------------ a. the grid equals the pinned kernels, bit for bit
SHAPES = [
    # (B, N, K, mask kind)
    (1, 1, 1, None), (3, 16, 4, None), (3, 33, 33, "ragged"), (3, 100, 7, "ragged"), (2, 1000, 32, "scattered"),
    (1, 9000, 128, None), (1, 8300, 64, "few_hundred"), (2, 300, 40, "one_graph_empty"), (1, 600, 32, "fewer_than_k"),
]


@pytest.mark.parametrize("b,n,k,kind", SHAPES, ids=[f"b{b}-n{n}-k{k}-{kind}" for b, n, k, kind in SHAPES])
def test_knn_select_grid_equals_the_pinned_kernels(b, n, k, kind):
    rng = np.random.default_rng(n * 7 + k * 3 + b)
    coors = rng.standard_normal((b, n, 3)).astype(np.float32)
    mask = None
    if kind == "ragged":
        mask = _ragged(rng, b, n, k)
    elif kind == "scattered":
        mask = rng.random((b, n)) < 0.6
    elif kind == "few_hundred":                                           # only 500-600 valid nodes in the graph
        mask = _ragged(rng, b, n, k, 500, 600)
    elif kind == "one_graph_empty":
        mask = rng.random((b, n)) < 0.7
        mask[1] = False
    elif kind == "fewer_than_k":                                          # every selection holds padded nodes
        mask = np.zeros((b, n), dtype=bool)
        mask[0, rng.permutation(n)[:k - 5]] = True
    _grid_twice_equals_pinned(coors, mask, k)


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
    if name == "one_point":
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
    if name == "normal_x400":                                             # valid pairs beyond d^2 = 1e5, masked pairs at exactly 1e5
        return rng.standard_normal((b, n, 3)) * 400.0
    raise KeyError(name)


GEOMETRIES = ("normal", "uniform", "clusters_and_outlier", "one_point", "lattice_x40", "collinear", "normal_x400")


@pytest.mark.parametrize("name", GEOMETRIES)
def test_knn_select_grid_on_geometries(name):
    b, n, k = 2, 2000, 16
    rng = np.random.default_rng(GEOMETRIES.index(name) + 100)
    coors = _geometry(name, rng, b, n).astype(np.float32)
    mask = _ragged(rng, b, n, k)
    mask[:, 7] = True                                                     # (the outlier is a real node)
    _grid_twice_equals_pinned(coors, mask, k)


# ------------------------------------------------------------------ b. beyond every other kernel: sampled rows against the oracle
@pytest.mark.parametrize("n", [70000, 262144])
def test_knn_select_grid_large_sampled_rows(n):
    from egnn_pytorch_amd import _ops
    k = 32
    rng = np.random.default_rng(n + k)
    coors = rng.standard_normal((1, n, 3)).astype(np.float32)
    mask = (np.arange(n) < n - 1234)[None, :]                            # ragged: the tail is padding
    rows = np.sort(np.concatenate([rng.choice(n, 250, replace=False), [0, n - 1, n - 1234, n - 1235, 5, 6]]))
    c, m = _dev(coors), _dev(mask)
    idx, rank = _ops.knn_select_grid(c, m, k)
    ref_val, ref_idx = _sampled_topk(coors, mask, None, rows, k)
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy()[0, rows])
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy()[0, rows].view(np.uint32))
    if n == 70000:
        _assert_same((idx, rank), _ops.knn_select_stream(c, m, None, k))


# ------------------------------------------------------------------ c. layers
def _layer_and_inputs(n, dim=16, k=8, seed=0):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed)
    layer = EGNN(dim=dim, num_nearest_neighbors=k).cuda()
    feats = torch.randn(1, n, dim, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    return layer, feats, coors


def test_layer_at_70000_nodes_takes_the_grid_and_equals_the_streaming_route(monkeypatch):
    from egnn_pytorch_amd import _ops, layer as L
    n = 70000
    layer, feats, coors = _layer_and_inputs(n)
    with torch.no_grad():
        with _ops.phase_timer() as t:
            node, co = layer(feats, coors)
        assert "knn_select_grid" in t.summary()
        node2, co2 = layer(feats, coors)                                  # (untimed: the one-call C forward declines, two streams)
        monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
        with _ops.phase_timer() as t:
            ref_node, ref_co = layer(feats, coors)
        names = t.summary()
        assert "knn_select" in names and "knn_select_grid" not in names
    assert torch.equal(node, ref_node) and torch.equal(co, ref_co)
    assert torch.equal(node2, ref_node) and torch.equal(co2, ref_co)


def test_training_step_at_70000_nodes_equals_the_streaming_route(monkeypatch):
    from egnn_pytorch_amd import layer as L
    n = 70000
    layer, feats, coors = _layer_and_inputs(n, seed=1)

    def step():
        f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        node, co = layer(f, c)
        (node.square().mean() + co.square().mean()).backward()
        return [node.detach(), co.detach(), f.grad, c.grad] + [p.grad for p in layer.parameters()]

    got = step()
    monkeypatch.setattr(L, "_KNN_GRID_MIN_N", n + 1)
    ref = step()
    assert len(got) == len(ref) and all(g is not None for g in got[:4])
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert torch.equal(g, r)


def test_layer_at_40000_nodes_keeps_the_all_pairs_selection():
    from egnn_pytorch_amd import _ops
    layer, feats, coors = _layer_and_inputs(40000)
    with torch.no_grad(), _ops.phase_timer() as t:
        layer(feats, coors)
    names = t.summary()
    assert "knn_select" in names and "knn_select_grid" not in names


def test_layer_at_262144_nodes_returns_finite_outputs():
    layer, feats, coors = _layer_and_inputs(262144)
    with torch.no_grad():
        node, co = layer(feats, coors)
    torch.cuda.synchronize()
    assert node.shape == (1, 262144, 16) and co.shape == (1, 262144, 3)
    assert torch.isfinite(node).all() and torch.isfinite(co).all()


# ------------------------------------------------------------------ d. graphed(): no host synchronisation in the new path
def test_graphed_layer_at_70000_nodes_replays_to_the_eager_result():
    from egnn_pytorch_amd import graphed
    layer, feats, coors = _layer_and_inputs(70000, seed=2)
    with torch.no_grad():
        ref_node, ref_co = layer(feats, coors)
        g = graphed(layer, feats, coors)
        out = g(feats, coors)
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref_node) and torch.equal(out[1], ref_co)


# ------------------------------------------------------------------ e. argument checks
def test_grid_entry_argument_checks_launch_nothing():
    from egnn_pytorch_amd import _abi, _ops
    lib = _abi.load()
    n, k = 500, 8
    coors = torch.randn(1, n, 3, device="cuda")
    idx = torch.full((1, n, k), -7, dtype=torch.int32, device="cuda")
    rank = torch.full((1, n, k), -7.0, device="cuda")
    nbytes = lib.egnn_knn_grid_workspace_bytes(1, n, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = _ops._stream()

    def call(c=coors, i=idx, r=rank, w=ws, nn=n, kk=k, cdim=3, wb=nbytes):
        return lib.egnn_knn_select_grid_f32(_ops._ptr(c), None, 1, nn, kk, cdim, _ops._ptr(i), _ops._ptr(r), _ops._ptr(w), wb, st)

    assert call(c=None) == -1 and call(i=None) == -1 and call(r=None) == -1 and call(w=None) == -1     # EGNN_E_NULLPTR
    assert call(kk=n + 1) == -2 and call(nn=0) == -2 and call(kk=0) == -2                                 # EGNN_E_SHAPE
    assert call(wb=nbytes - 1) == -2                                                                      # one byte short
    assert call(cdim=2) == -3 and call(kk=_ops.KNN_GRID_KMAX + 1) == -3                                   # EGNN_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((rank == -7.0).all()) and not bool(ws.any())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((idx >= 0).all())
    sizes = lib.egnn_knn_grid_workspace_bytes
    assert isinstance(sizes(1, 1, 1), int) and sizes(1, 1, 1) > 0
    for b, nn, kk in ((1, 1, 1), (3, 100, 7), (1, 70000, 32)):
        assert sizes(b, nn, kk) <= sizes(b + 1, nn, kk) and sizes(b, nn, kk) <= sizes(b, nn + 1, kk) <= sizes(b, nn * 2, kk)
        assert sizes(b, nn, kk) <= sizes(b, nn, kk + 1)
