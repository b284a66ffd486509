"""Per-kernel parity on the MI355X, through the C ABI (egnn_pytorch_amd._ops -> libegnn_hip.so)."""
import os

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O
from tests import _reflib
from tests._util import check_neighbors, golden_names, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    """These are forward-parity tests: run them the way inference code does (under autograd the modules would record a
    graph, as the reference does -- that path is tests/test_autograd.py)."""
    with torch.no_grad():
        yield


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------ neighbour selection: bit-exact
@pytest.mark.parametrize("n,k,use_mask,adj_kind", [
    (16, 4, False, None), (64, 8, True, None), (100, 7, True, None), (256, 32, True, None),
    (1024, 32, True, None), (2048, 16, False, None), (300, 40, True, "random"), (64, 8, True, "chain"),
    (4096, 8, False, None), (33, 33, True, None), (1024, 100, True, None), (6000, 16, True, None), (8192, 32, False, None),
    # beyond what a wave keeps in registers: one workgroup per row, keys in LDS; the second case has fewer valid
    # nodes than K in its row set (ties at 1e5 straddle the K boundary: index-ordered pick)
    (9000, 32, False, None), (8300, 700, True, None),
])
def test_knn_select_bit_exact(n, k, use_mask, adj_kind):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n * 131 + k)
    b = 3 if n <= 4096 else 1
    coors = rng.standard_normal((b, n, 3)).astype(np.float32)
    mask = None
    if use_mask:
        lens = rng.integers(max(k, n // 2) if n != 8300 else 500, (n + 1) if n != 8300 else 600, size=b)
        mask = np.arange(n)[None, :] < lens[:, None]
    adj = None
    if adj_kind == "chain":
        i = np.arange(n)
        adj = np.abs(i[:, None] - i[None, :]) <= 1
    elif adj_kind == "random":
        adj = np.zeros((b, n, n), bool)
        for bb in range(b):
            for i in range(n):
                js = rng.choice(n, size=rng.integers(0, 4), replace=False)
                adj[bb, i, js] = True
                adj[bb, js, i] = True
            adj[bb][np.arange(n), np.arange(n)] = True
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, adj)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), _dev(adj), k)
    idx, rank = idx.cpu().numpy(), rank.cpu().numpy()
    # oracle and kernel share the tie policy (ascending index): everything must be identical
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.view(np.uint32))
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx)


@pytest.mark.parametrize("n,band,k,use_mask,three_d,with_diag", [
    (2048, 1, 3, True, False, True),        # BASELINE.json's c4: chain with the diagonal, K = max degree: every interior row is decided
    (2048, 1, 3, False, True, False),       # no diagonal in adj_mat: self + K adjacent tie for K slots (the first K - 1 by index)
    (512, 2, 5, True, False, True), (1024, 3, 4, True, True, True), (256, 1, 8, False, False, True),     # K - 1 > degree: distances decide
    (300, 2, 5, True, False, True),         # N % 64 != 0
    (130, 1, 3, False, False, True),        # N % 4 != 0: the general path
])
def test_knn_select_rows_decided_by_the_adjacency(n, band, k, use_mask, three_d, with_diag):
    """only_sparse_neighbors-style selections (egnn_pytorch.py:248-256): rows with at least K - 1 adjacent nodes come straight from
    the adjacency row (csrc/knn_select.hip, round 6) -- bit-identical to the oracle's ranking + stable top-k, including the rows that
    must NOT take the shortcut: fewer adjacent nodes than K - 1, and a non-adjacent node at distance exactly 0 (it ties with the
    adjacent ones at rank 0.0 and wins by index)."""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n + 7 * k)
    b = 2
    coors = rng.standard_normal((b, n, 3)).astype(np.float32)
    # exact duplicates of unmasked, non-adjacent nodes: 5 <-> 40 (lower index wins a slot of row 40), 90 <- 17 in graph 1
    coors[0, 40] = coors[0, 5]
    coors[1, 90] = coors[1, 17]
    coors[1, 91, 0] = coors[1, 20, 0]                                    # equal first coordinate only: the conservative check falls back
    mask = (np.arange(n)[None, :] < np.array([[n], [n - n // 5]])) if use_mask else None
    i = np.arange(n)
    adj = np.abs(i[:, None] - i[None, :]) <= band
    if not with_diag:
        adj = adj & (i[:, None] != i[None, :])
    if three_d:
        adj = np.stack([adj, adj.copy()])
        adj[1, 7, :] = False                                             # an isolated row in graph 1: everything by distance
        adj[1, :, 7] = False
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, adj)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), _dev(adj), k)
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy())


def _check_large_graph_other_dimensions(cdim, n, k, valid, chain, seed):
    """one graph of n nodes with cdim != 3 coordinates, beyond the 4096 candidates a wave keeps: the first `valid` nodes real (None: all),
    chain: a band-1 adjacency with the diagonal; bit for bit against the oracle"""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(seed)
    coors = rng.standard_normal((1, n, cdim)).astype(np.float32)
    mask = None if valid is None else (np.arange(n)[None, :] < valid)
    i = np.arange(n)
    adj = (np.abs(i[:, None] - i[None, :]) <= 1) if chain else None
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, adj)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), _dev(adj), k)
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy())


def test_knn_select_large_graph_other_coordinate_dimensions():
    """N = 4500 with 5-D coordinates (a wave keeps at most 4096 such candidates): the workgroup-per-row kernel with the reference's
    summation order for C = 5 (s0, s4, s1, s2, s3)."""
    _check_large_graph_other_dimensions(5, 4500, 24, 4100, False, seed=45)


@pytest.mark.parametrize("cdim,k,valid,chain", [(8, 24, 3900, False), (2, 8, None, True)], ids=["c8-k24-prefix_mask", "c2-k8-chain_adjacency"])
def test_knn_select_large_graph_left_to_right_dimensions(cdim, k, valid, chain):
    """N = 4100, the smallest size class of knn_select_rows_kernel<float, 8> (csrc/knn_rows.hip): the left-to-right summation order of
    C = 8 and C = 2 (C = 5 above takes the other order of egnn_sqdist_n), and an adjacency row entering that kernel's keys."""
    _check_large_graph_other_dimensions(cdim, 4100, k, valid, chain, seed=4100 + cdim)


@pytest.mark.parametrize("cdim,n,k,use_mask,use_adj", [(9, 200, 16, True, False), (11, 64, 8, True, True), (16, 300, 32, False, False),
                                                       (33, 128, 8, True, False), (40, 77, 77, False, False), (64, 150, 5, True, True)])
def test_knn_select_more_than_eight_coordinates_bit_exact(cdim, n, k, use_mask, use_adj):
    """More than 8 coordinates (VERDICT r3 missing #5): the squared distances follow ATen's summation tree for any length
    (egnn_common.h::egnn_sqdist_any; the oracle's inner_sum is pinned against torch bit for bit in tests/test_oracle_vs_reference.py),
    so ranking values and indices equal the oracle's exactly -- incl. rows with exact ties."""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(cdim * 1000 + n)
    b = 2
    coors = rng.standard_normal((b, n, cdim)).astype(np.float32)
    coors[:, 5] = coors[:, 4]                                            # exact ties: lowest index first
    mask = (np.arange(n)[None, :] < np.array([[n], [max(k, n - 7)]])) if use_mask else None
    i = np.arange(n)
    adj = (np.abs(i[:, None] - i[None, :]) <= 2) if use_adj else None
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, adj)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), _dev(adj), k)
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy())


@pytest.mark.parametrize("name", [g for g in golden_names()])
def test_knn_select_matches_reference_topk(name):
    """Against the indices the reference's own topk returned (golden), under the §8c tie policy."""
    from egnn_pytorch_amd import _ops
    meta, _, d = load_golden(name)
    if meta["kind"] != "layer" or not meta["n_topk"]:
        pytest.skip("dense path / network case")
    k = d["topk_values.0"].shape[-1]
    idx, rank = _ops.knn_select(_dev(d["coors"]), _dev(d.get("mask")), _dev(d.get("adj_mat")), k)
    check_neighbors(d["topk_values.0"], d["topk_indices.0"], rank.cpu().numpy(), idx.cpu().numpy())


def test_knn_k_gt_n_raises():
    from egnn_pytorch_amd import _ops
    with pytest.raises(RuntimeError):
        _ops.knn_select(torch.zeros(1, 4, 3, device="cuda"), None, None, 5)


def test_adj_max_degree():
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(1)
    adj = rng.random((3, 70, 70)) < 0.1
    assert _ops.adj_max_degree(_dev(adj)) == O.sparse_num_nearest(adj)
    adj2 = np.eye(37, dtype=bool)
    assert _ops.adj_max_degree(_dev(adj2)) == 1


# ------------------------------------------------------------------ fp32 MFMA linear
@pytest.mark.parametrize("m,n,k,act,res", [
    (16, 130, 32, 0, False), (300, 257, 65, 1, False), (1024, 4160, 512, 0, False),
    (2048, 1024, 528, 1, False), (2048, 512, 1024, 0, True), (77, 40, 36, 0, True), (5, 3, 7, 1, True),
])
def test_linear_f32(m, n, k, act, res):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(m + n + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    r = rng.standard_normal((m, n)).astype(np.float32) if res else None
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if act:
        ref = ref / (1.0 + np.exp(-ref))
    if res:
        ref = ref + r
    out = _reflib.linear(_dev(a), _dev(w), _dev(bias), _dev(r), act=act).cpu().numpy()
    assert out.shape == (m, n)
    # asymmetric operands: a transposed / mis-mapped C tile cannot pass
    np.testing.assert_allclose(out, ref, atol=2e-5, rtol=0)


@pytest.mark.parametrize("m,n,k,act,res", [
    (16, 130, 32, 0, False), (300, 257, 65, 1, False), (1024, 4160, 512, 0, False),
    (2048, 1024, 528, 1, False), (2048, 512, 1024, 0, True), (77, 40, 36, 0, True), (5, 3, 7, 1, True),
    (128, 128, 8, 0, False), (129, 129, 100, 0, False),
])
def test_linear_split_f16x3(m, n, k, act, res):
    """fp32-in/fp32-out GEMM on the matrix cores (3-term split-f16): fp32-class accuracy against an fp64
    reference, same tolerance as the exact-fp32 kernel; weights at very different scales exercise the
    power-of-two range scaling."""
    from egnn_pytorch_amd import _ops, _weights
    rng = np.random.default_rng(m + n + k)
    for wscale in (1.0, 1e-3, 37.0):
        a = (rng.standard_normal((m, k)) * 3).astype(np.float32)
        w = (rng.standard_normal((n, k)) / np.sqrt(k) * wscale).astype(np.float32)
        bias = rng.standard_normal(n).astype(np.float32)
        r = rng.standard_normal((m, n)).astype(np.float32) if res else None
        ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
        if act:
            ref = ref / (1.0 + np.exp(-ref))
        if res:
            ref = ref + r
        ws = _reflib.split_f16_rowmajor(_dev(w))
        out = _reflib.linear_split(_dev(a), ws, n, _dev(bias), _dev(r), act=act).cpu().numpy()
        assert out.shape == (m, n)
        tol = 2e-5 * max(1.0, 3 * wscale)
        np.testing.assert_allclose(out, ref, atol=tol, rtol=0)
        # and it must agree with the exact-fp32 MFMA kernel at fp32 round-off level
        exact = _reflib.linear(_dev(a), _dev(w), _dev(bias), _dev(r), act=act).cpu().numpy()
        np.testing.assert_allclose(out, exact, atol=tol, rtol=0)


@pytest.mark.parametrize("m,n,k,act,res", [
    (16, 130, 32, 0, False), (300, 257, 65, 1, False), (1024, 4160, 512, 0, False),
    (2048, 1024, 528, 1, False), (2048, 512, 1024, 0, True), (77, 40, 36, 0, True), (5, 3, 7, 1, True),
    (129, 129, 100, 0, False), (4096, 256, 2048, 0, False), (16384, 4160, 512, 0, False), (8192, 2048, 160, 1, True),
])
def test_linear_hl_lds_dma(m, n, k, act, res):
    """The production GEMM (pre-split fp16 hi/lo operands, LDS-DMA staging, swizzled LDS image): fp32-class accuracy
    against an fp64 reference, fp32 and re-split outputs, operands that are neither symmetric nor tile aligned."""
    from egnn_pytorch_amd import _ops, _weights
    rng = np.random.default_rng(m * 7 + n + k)
    a = (rng.standard_normal((m, k)) * 2).astype(np.float32)
    a[:, ::7] *= 1e-3                                               # mixed magnitudes inside a row
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    r = rng.standard_normal((m, n)).astype(np.float32) if res else None
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if act:
        ref = ref / (1.0 + np.exp(-ref))
    if res:
        ref = ref + r
    ahl = _ops.split_f16(_dev(a))
    assert ahl.kp % 32 == 0 and ahl.hi.numel() == (m + 31) // 32 * 32 * ahl.kp
    back = ahl.dense()
    # 22-bit split; lo of elements below ~1e-3 is an fp16 subnormal: absolute error up to 2^-25
    np.testing.assert_allclose(back[:, :k].cpu().numpy(), a, rtol=3e-7, atol=3.1e-8)
    assert float(back[:, k:].abs().max()) == 0.0 if back.shape[1] > k else True
    ws = _weights.split_f16(_dev(w))
    out, chl = _ops.linear_hl(ahl, ws, n, _dev(bias), _dev(r), act=act, out_f32=True, out_hl=True)
    out = out.cpu().numpy()
    np.testing.assert_allclose(out, ref, atol=3e-5, rtol=0)
    resplit = chl.dense().cpu().numpy()
    np.testing.assert_allclose(resplit[:, :n], out, rtol=3e-7, atol=3.1e-8)
    assert np.all(resplit[:, n:] == 0)
    exact = _reflib.linear(_dev(a), _dev(w), _dev(bias), _dev(r), act=act).cpu().numpy()      # exact-fp32 MFMA kernel
    np.testing.assert_allclose(out, exact, atol=3e-5, rtol=0)


def test_linear_hl_split_cols():
    """split_cols: the leading columns of C come out as (fp16 hi | fp16 lo << 16) words of the same values -- the form
    in which the edge pass takes P_i -- the rest stays fp32."""
    from egnn_pytorch_amd import _ops, _weights
    rng = np.random.default_rng(5)
    m, n, k, sc = 300, 192, 96, 64
    a = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    ahl = _ops.split_f16(_dev(a))
    ws = _weights.split_f16(_dev(w))
    plain = _ops.linear_hl(ahl, ws, n, _dev(bias)).cpu().numpy()
    mixed = _ops.linear_hl(ahl, ws, n, _dev(bias), split_cols=sc).cpu().numpy()
    np.testing.assert_array_equal(mixed[:, sc:], plain[:, sc:])
    words = np.ascontiguousarray(mixed[:, :sc]).view(np.uint32)
    hi = (words & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    lo = (words >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
    np.testing.assert_array_equal(hi, plain[:, :sc].astype(np.float16).astype(np.float32))
    np.testing.assert_allclose(hi + lo, plain[:, :sc], rtol=3e-7, atol=3.1e-8)


def test_node_prep_hl():
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(0)
    x = rng.standard_normal((300, 100)).astype(np.float32) * 3 + 1
    mi = rng.standard_normal((300, 16)).astype(np.float32)
    g = rng.standard_normal(100).astype(np.float32)
    bt = rng.standard_normal(100).astype(np.float32)
    phl = _ops.node_prep_hl(_dev(x), _dev(mi), _dev(g), _dev(bt), 1e-5, 16)
    assert phl.kp == 128 and phl.rows == 300
    out = phl.dense().cpu().numpy()
    ref = np.concatenate([O.layer_norm(x, g, bt), mi], axis=-1)
    np.testing.assert_allclose(out[:, :116], ref, atol=1e-5, rtol=0)
    assert np.all(out[:, 116:] == 0)
    # one pass, two consumers: m_i columns left zero for the edge pass + the raw rows as a second (hi, lo) pair
    phl2, raw = _ops.node_prep_hl(_dev(x), None, _dev(g), _dev(bt), 1e-5, 16, with_raw=True)
    out2 = phl2.dense().cpu().numpy()
    np.testing.assert_array_equal(out2[:, :100], out[:, :100])
    assert np.all(out2[:, 100:] == 0)
    assert raw.kp == 128 and raw.rows == 300
    rawd = raw.dense().cpu().numpy()
    np.testing.assert_allclose(rawd[:, :100], x, rtol=3e-7, atol=3.1e-8)
    assert np.all(rawd[:, 100:] == 0)


def test_node_prep():
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(0)
    x = rng.standard_normal((300, 100)).astype(np.float32) * 3 + 1
    mi = rng.standard_normal((300, 16)).astype(np.float32)
    g = rng.standard_normal(100).astype(np.float32)
    bt = rng.standard_normal(100).astype(np.float32)
    out = _reflib.node_prep(_dev(x), _dev(mi), _dev(g), _dev(bt), 1e-5, 16).cpu().numpy()
    ref = np.concatenate([O.layer_norm(x, g, bt), mi], axis=-1)
    np.testing.assert_allclose(out, ref, atol=1e-5, rtol=0)
    out2 = _reflib.node_prep(_dev(x), _dev(mi), None, None, 1e-5, 16).cpu().numpy()
    np.testing.assert_array_equal(out2, np.concatenate([x, mi], axis=-1))


def test_spatial_order_is_a_permutation_and_results_do_not_depend_on_it(monkeypatch):
    """egnn_spatial_order_f32 is a scheduling aid: a valid per-graph permutation, and the layer's outputs are
    bit-identical with and without it."""
    from egnn_pytorch_amd import EGNN, _ops, layer as L
    rng = np.random.default_rng(4)
    for n in (64, 100, 1024, 3000):
        coors = rng.standard_normal((3, n, 3)).astype(np.float32)
        order = _ops.spatial_order(_dev(coors)).cpu().numpy()
        assert order.shape == (3, n)
        for b in range(3):
            assert np.array_equal(np.sort(order[b]), np.arange(n))
    # locality: consecutive nodes in the order are much closer than consecutive nodes in index order
    c = coors[0]
    d_idx = np.linalg.norm(c[1:] - c[:-1], axis=1).mean()
    d_ord = np.linalg.norm(c[order[0][1:]] - c[order[0][:-1]], axis=1).mean()
    assert d_ord < 0.5 * d_idx
    kw = dict(dim=64, num_nearest_neighbors=16)
    cfg = O.EGNNConfig(**kw)
    params = O.random_params(cfg, seed=2)
    net = EGNN(**kw)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.cuda().eval()
    feats = _dev(rng.standard_normal((2, 300, 64)).astype(np.float32))
    co = _dev(rng.standard_normal((2, 300, 3)).astype(np.float32))
    mask = _dev(np.arange(300)[None, :] < np.array([[300], [211]]))
    monkeypatch.setattr(L, "_SPATIAL_ORDER", True)
    n1, c1 = net(feats, co, mask=mask)
    monkeypatch.setattr(L, "_SPATIAL_ORDER", False)
    n0, c0 = net(feats, co, mask=mask)
    assert torch.equal(n0, n1) and torch.equal(c0, c1)


@pytest.mark.parametrize("n,degrees,kind", [(16, 2, "chain"), (100, 3, "random"), (256, 4, "chain_nodiag"), (1024, 3, "random"),
                                            (70, 1, "random"), (130, 5, "sparse_random")])
def test_adj_expand_bit_exact(n, degrees, kind):
    """N-degree adjacency expansion (bit sets on the device) against the oracle's float-matmul restatement of
    egnn_pytorch.py:414-427: labels and expanded adjacency identical, 2-D and batched inputs."""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n + degrees)
    b = 3
    i = np.arange(n)
    if kind == "chain":
        adj = np.broadcast_to(np.abs(i[:, None] - i[None, :]) <= 1, (b, n, n)).copy()
    elif kind == "chain_nodiag":
        adj = np.broadcast_to(np.abs(i[:, None] - i[None, :]) == 1, (b, n, n)).copy()
    elif kind == "sparse_random":
        adj = rng.random((b, n, n)) < 0.01                       # asymmetric, some empty rows, no forced diagonal
    else:
        adj = rng.random((b, n, n)) < 0.03
        adj = adj | adj.transpose(0, 2, 1) | np.eye(n, dtype=bool)[None]
    ref_idx, ref_adj = O.adjacency_degrees(adj, degrees)
    out_adj, out_idx = _ops.adj_expand(_dev(adj), b, degrees)
    np.testing.assert_array_equal(out_idx.cpu().numpy().astype(np.int64), ref_idx)
    np.testing.assert_array_equal(out_adj.cpu().numpy(), ref_adj)
    # shared (N,N) adjacency broadcast over the batch
    out_adj2, out_idx2 = _ops.adj_expand(_dev(adj[0]), b, degrees)
    for bb in range(b):
        np.testing.assert_array_equal(out_idx2[bb].cpu().numpy().astype(np.int64), ref_idx[0])
        np.testing.assert_array_equal(out_adj2[bb].cpu().numpy(), ref_adj[0])


def test_rows_gather_sum_fixed_order():
    """egnn_rows_gather_sum_f32 (backward of the neighbour gather): equals the sequential fp32 sum over the sorted in-edge list
    bit for bit, run after run (no atomics), and a float64 index_add within rounding."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(12)
    n_out, e, cols = 300, 5000, 96
    rows = torch.randn(e, cols, generator=g).cuda()
    dest = torch.randint(0, n_out, (e,), generator=g).cuda()
    dest[:40] = 7                                                           # one heavy destination; some get none
    ds, order = torch.sort(dest, stable=True)
    seg = torch.searchsorted(ds, torch.arange(n_out + 1, device="cuda"))
    out = _ops.rows_gather_sum(rows, order, seg, n_out)
    out2, bits = _ops.rows_gather_sum(rows, order, seg, n_out, want_amax=True)
    assert _ops.bits_to_floats(bits)[0] == float(out.abs().max())                # the by-product: max |out|, exact
    assert torch.equal(out, out2)
    # sequential fp32 reference for a few rows (pairs of rows are added one after the other in list order)
    for r in (7, 0, 123, n_out - 1):
        acc = torch.zeros(cols, device="cuda")
        for p in range(int(seg[r]), int(seg[r + 1])):
            acc = acc + rows[order[p]]
        assert torch.equal(out[r], acc), r
    ref = torch.zeros(n_out, cols, dtype=torch.float64, device="cuda").index_add_(0, dest, rows.double())
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), atol=1e-5)


@pytest.mark.parametrize("b,n,k,dim,hub,extra", [(2, 40, 8, 32, False, {}), (1, 64, 32, 64, False, {}), (3, 50, 5, 32, True, {}),
                                                 (1, 33, 16, 32, True, {}), (2, 40, 16, 32, False, dict(edge_dim=4)),
                                                 (1, 48, 8, 32, True, dict(fourier_features=1)), (1, 40, 8, 16, False, dict(edge_dim=1)),
                                                 # the BASELINE widths: 17 / 9 / 5 persistent column chunks of 128 (Hp = 2080 / 1056 / 544)
                                                 (1, 96, 32, 512, False, {}), (1, 80, 32, 256, True, {}), (2, 64, 32, 128, False, {}),
                                                 (1, 64, 16, 512, True, dict(edge_dim=4)),
                                                 # two tiles per source node with padding in the second (summed in the kernel), three tiles (gather-sum)
                                                 (1, 40, 24, 32, False, {}), (2, 50, 40, 32, True, {}), (1, 40, 20, 32, False, dict(edge_dim=2)),
                                                 # more than five per-edge scalars: d/d s on the matrix cores (8, 13 and 16 scalars)
                                                 (1, 48, 32, 64, False, dict(edge_dim=3, fourier_features=2)), (2, 40, 8, 32, True, dict(edge_dim=12)),
                                                 (1, 40, 16, 32, False, dict(edge_dim=5, fourier_features=5))])
def test_edge_bwd_pass_contractions_match_float64(b, n, k, dim, hub, extra):
    """egnn_edge_bwd_pass_f32 (nothing of size E x H in memory: z, SiLU(z), dz recomputed and contracted in registers) against the
    same contractions in float64:
    d/d P_i, d/d P_j (per node), d/d W_s, d/d scalars, d/d W_2.  K below / equal / above a 16-entry tile, and `hub` = a few nodes
    with very large in-degree (one key over many tiles) next to nodes nobody points to."""
    from egnn_pytorch_amd import EGNN, _weights, autograd
    g = torch.Generator().manual_seed(100 * n + k)
    layer = EGNN(dim=dim, num_nearest_neighbors=k, **extra)
    # xavier-scale weights: with the default N(0, 1e-3) init z ~ 0, where SiLU' is almost constant and a
    # wrong z would go unnoticed
    torch.manual_seed(1000 + dim + k)
    for mod in layer.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.xavier_normal_(mod.weight)
    layer = layer.cuda()
    w = layer.packed_weights()
    h, hp, m, s_in = w["H"], w["Hp"], layer.m_dim, w["S"]
    feats = torch.randn(b, n, dim, generator=g).cuda()
    idx = torch.randint(0, n, (b, n, k), generator=g)
    if hub:
        idx[:, :, 0] = 3
        idx[:, ::2, 1] = 7
    idx32 = idx.to(torch.int32).cuda()
    e = b * n * k
    coors = (torch.randn(b, n, 3, generator=g) * 1.5).cuda()
    edges = torch.randn(b, n, n, extra["edge_dim"], generator=g).cuda() if extra.get("edge_dim") else None
    scal = autograd.edge_scalars(layer, coors, edges, idx32.long())[1].reshape(e, s_in).contiguous()    # [fourier, dist, edge feats]
    gu = torch.randn(e, m, generator=g) * 1e-3
    gu[torch.rand(e, generator=g) < 0.2] = 0.0                                  # masked edges carry no gradient
    gu16 = torch.zeros(e, 16)
    gu16[:, :m] = gu
    gu16 = gu16.cuda()
    gu_scale = _weights.pow2_scale(float(gu16.abs().max()))
    lin0, lin3 = layer.edge_mlp[0], layer.edge_mlp[3]
    w1 = lin0.weight.detach()
    w_s = torch.zeros(hp, s_in, device="cuda")
    w_s[:h] = w1[:, 2 * dim:]
    f2d = feats.view(b * n, dim)
    outs = {}
    for name, fn in (("fused", autograd._edge_contract_fused),):
        with torch.no_grad():
            outs[name] = fn(layer, w, f2d, coors, edges, scal, idx32, gu16, gu_scale, w_s, b, n, k, k >= 6)
    with torch.no_grad():
        again = autograd._edge_contract_fused(layer, w, f2d, coors, edges, scal, idx32, gu16, gu_scale, w_s, b, n, k, k >= 6)
    assert all(torch.equal(x, y) for x, y in zip(outs["fused"], again))        # fixed summation order: bit-reproducible
    # float64 reference
    w1d, b1d, w2d = w1.double(), lin0.bias.detach().double(), lin3.weight.detach().double()
    fd = f2d.double()
    p_i = fd @ w1d[:, :dim].t() + b1d
    p_j = fd @ w1d[:, dim:2 * dim].t()
    src = torch.arange(b * n, device="cuda").repeat_interleave(k)
    dst = (idx32.long() + (torch.arange(b, device="cuda") * n)[:, None, None]).reshape(-1)
    z = p_i[src] + p_j[dst] + scal.double() @ w1d[:, 2 * dim:].t()
    sg = torch.sigmoid(z)
    act = z * sg
    dz = (gu16[:, :m].double() @ w2d) * (sg * (1 + z * (1 - sg)))
    ref = dict(gz_i=torch.zeros(b * n, h, dtype=torch.float64, device="cuda").index_add_(0, src, dz),
               gz_j=torch.zeros(b * n, h, dtype=torch.float64, device="cuda").index_add_(0, dst, dz),
               g_ws=dz.t() @ scal.double(), g_scal=dz @ w1d[:, 2 * dim:], g_w2=gu16[:, :m].double().t() @ act)
    for name, (gz_i, gz_j, g_ws, g_scal, g_w2) in outs.items():
        got = dict(gz_i=gz_i[:, :h], gz_j=gz_j[:, :h], g_ws=g_ws[:h], g_scal=g_scal, g_w2=g_w2[:m, :h])
        for key, r in ref.items():
            scale = float(r.abs().max())
            err = float((got[key].double() - r).abs().max())
            if os.environ.get("EGNN_TEST_VERBOSE"):
                print(f"{name:6s} {key:7s} rel err {err / scale:.2e}")
            assert err <= 5e-6 * scale + 1e-12, (name, key, err, scale)
        if h < hp:
            assert float(gz_i[:, h:].abs().max()) == 0.0 and float(gz_j[:, h:].abs().max()) == 0.0, name      # pad columns


@pytest.mark.parametrize("b,n,k,use_mask,use_order", [(2, 100, 8, True, True), (1, 64, 32, False, True), (3, 40, 5, True, False)])
def test_slot_prep_records_bit_exact(b, n, k, use_mask, use_order):
    """egnn_slot_prep_f32: one record per edge slot in the edge pass's consumption order -- {j | pair_ok << 31, x_i - x_j} -- equal, bit
    for bit, to what the edge pass's own setup derives from order -> idx -> coors -> mask / rank (egnn_pytorch.py:232, :292-300);
    and the layer's outputs do not depend on whether the records are used."""
    from egnn_pytorch_amd import EGNN, _ops, layer as L
    g = torch.Generator().manual_seed(b * 1000 + n + k)
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = (torch.arange(n)[None] < torch.randint(n // 2, n + 1, (b, 1), generator=g)).cuda() if use_mask else None
    idx, rank = _ops.knn_select(coors, mask, None, k)
    order = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).to(torch.int32).cuda() if use_order else None
    radius = float(rank[rank < 1e4].median())
    slots = _ops.slot_prep(coors, _ops._u8(mask), idx, rank, order, radius).view(b, n, k, 4)
    o = order.long() if order is not None else torch.arange(n, device="cuda")[None].expand(b, n)
    bi = torch.arange(b, device="cuda")[:, None]
    idx_o, rank_o = idx[bi, o].long(), rank[bi, o]                                  # (b, pos, k): rows in consumption order
    xi = coors[bi, o][:, :, None, :]
    xj = coors[bi[:, :, None], idx_o]
    rel = xi - xj
    ok = torch.ones(b, n, k, dtype=torch.bool, device="cuda")
    if mask is not None:
        ok = mask[bi, o][:, :, None] & mask[bi[:, :, None], idx_o] & (rank_o <= radius)
    want_w0 = idx_o.to(torch.int32) | (ok.to(torch.int32) << 31)
    # (bit 30 = the group flag of padded nodes: test_padded_nodes_last_in_the_order_and_the_group_flag_of_the_slot_records)
    assert torch.equal(slots[..., 0] & ~(1 << 30), want_w0)
    assert torch.equal(slots[..., 1:].view(torch.float32), rel)
    # the layer with and without the records
    torch.manual_seed(3)
    layer = EGNN(dim=32, num_nearest_neighbors=k, valid_radius=radius, norm_coors=True).cuda().eval()
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(40.0)
        feats = torch.randn(b, n, 32, generator=g).cuda()
        old = L._SLOT_PREP
        try:
            L._SLOT_PREP = True
            with_records = layer(feats, coors, mask=mask)
            L._SLOT_PREP = False
            without = layer(feats, coors, mask=mask)
        finally:
            L._SLOT_PREP = old
    assert torch.equal(with_records[0], without[0]) and torch.equal(with_records[1], without[1])


@pytest.mark.parametrize("b,n,k,dense", [(3, 100, 8, False), (2, 1024, 32, False), (1, 300, 70, False), (2, 48, 48, True), (1, 4096, 16, False),
                                         (1, 8192, 4, False), (2, 12000, 3, False), (1, 20000, 2, False)])
def test_dest_lists_equal_a_stable_sort(b, n, k, dense):
    """egnn_dest_lists_i32 (counting sort per graph, two launches) against torch.sort(stable=True): the CSR order bit for bit, the
    padded entry list = autograd.entry_list of that order; two runs identical."""
    from egnn_pytorch_amd import _ops, autograd as A
    g = torch.Generator().manual_seed(b + n + k)
    if dense:
        idx = None
        dest = (torch.arange(k)[None, None, :] + (torch.arange(b) * n)[:, None, None]).expand(b, n, k).reshape(-1).cuda()
    elif n >= 8000:
        # (N beyond ~8000: fewer waves per graph so that the histograms still fit in LDS -- ADVICE r3; rows with distinct destinations,
        # built without n randperms)
        base = torch.randint(0, n, (b, n, 1), generator=g)
        step = torch.randint(1, n // k, (b, n, 1), generator=g)
        idx = ((base + step * torch.arange(k)[None, None, :]) % n).to(torch.int32).cuda()
    else:
        idx = torch.stack([torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(n)]) for _ in range(b)]).to(torch.int32).cuda()
        if n >= 300:
            idx[:, ::3, 0] = 7                                                  # a hub (destinations stay distinct within a row:
            idx[:, ::3, 1:] = torch.where(idx[:, ::3, 1:] == 7, torch.full_like(idx[:, ::3, 1:], 8), idx[:, ::3, 1:])   # ... mostly)
            idx[:, ::3, 1:] = torch.where(idx[:, ::3, 1:] == 8, (idx[:, ::3, 1:2] * 0 + 9).expand_as(idx[:, ::3, 1:]), idx[:, ::3, 1:]) if False else idx[:, ::3, 1:]
    if not dense:
        dest = (idx.long() + (torch.arange(b, device="cuda") * n)[:, None, None]).reshape(-1)
    dl = _ops.dest_lists(idx, b, n, k, "cuda")
    dl2 = _ops.dest_lists(idx, b, n, k, "cuda")
    dest_sorted, by_dest = torch.sort(dest, stable=True)
    seg = torch.searchsorted(dest_sorted, torch.arange(b * n + 1, device="cuda"))
    assert torch.equal(dl.seg, seg)
    if dense or n < 300 or n >= 8000:
        assert torch.equal(dl.order, by_dest)
        ent, tile_seg = A.entry_list(by_dest, dest_sorted, b * n)
        assert torch.equal(dl.tile_seg, tile_seg) and torch.equal(dl.ent, ent)
    else:
        # rows whose destinations are not all distinct (the hub overwrite above can collide): still a valid grouping -- every
        # destination's segment holds exactly its edges
        assert torch.equal(dest[dl.order], dest_sorted)
    assert torch.equal(dl.ent, dl2.ent) and torch.equal(dl.order, dl2.order)


@pytest.mark.parametrize("r,m,n", [(4096, 2080, 512), (1000, 96, 24), (8192, 544, 128)])
def test_gradient_gemms_match_float64(r, m, n):
    """The backward's node-level products on the split-f16 GEMM (egnn_split_scaled_f16, egnn_linear_hl_f32 / _splitk_f32,
    egnn_sum_parts_f32): g (R, M) @ W (M, N) and g^T (M, R) @ x (R, N), with gradient-sized operands (1e-5 .. 1e-9: fp16
    subnormals without the power-of-two pre-scaling), against float64 at 3e-6 of the result's scale."""
    from egnn_pytorch_amd import _ops, _weights
    g = torch.Generator().manual_seed(r + m)
    grad = (torch.randn(r, m, generator=g) * torch.logspace(-9, -5, m)[None, :]).cuda()
    grad[:, m - 7:] = 0.0                                                       # pad-like zero columns
    w = (torch.randn(m, n, generator=g) * 0.05).cuda()
    x = torch.randn(r, n, generator=g).cuda()
    got_nn = _ops.grad_nn(grad, _weights.split_f16(w.t().contiguous()), n)
    want_nn = grad.double() @ w.double()
    assert float((got_nn.double() - want_nn).abs().max()) <= 3e-6 * float(want_nn.abs().max())
    res = torch.randn(r, n, generator=g).cuda() * float(want_nn.abs().max())
    got_res = _ops.grad_nn(grad, _weights.split_f16(w.t().contiguous()), n, residual=res)
    assert float((got_res.double() - (want_nn + res.double())).abs().max()) <= 3e-6 * float((want_nn + res.double()).abs().max())
    got_tn = _ops.grad_tn(grad, x)
    want_tn = grad.double().t() @ x.double()
    assert got_tn.shape == (m, n)
    assert float((got_tn.double() - want_tn).abs().max()) <= 3e-6 * float(want_tn.abs().max())
    assert torch.equal(got_tn, _ops.grad_tn(grad, x))                            # fixed-order partial sums: bit-reproducible
    for k_splits in (1, 2):
        alt = _ops.grad_tn(grad, x, k_splits=k_splits)
        assert float((alt.double() - want_tn).abs().max()) <= 3e-6 * float(want_tn.abs().max())
    zero = _ops.grad_tn(torch.zeros_like(grad), x)
    assert float(zero.abs().max()) == 0.0
    bad = grad.clone(); bad[3, 1] = float("nan")                                  # a NaN in an operand: NaN products, like fp32 (not zeros)
    assert bool(torch.isnan(_ops.grad_tn(bad, x)).all()) and bool(torch.isnan(_ops.grad_nn(bad, _weights.split_f16(w.t().contiguous()), n)).all())
    # the shared pieces (one absmax per matrix, feats^T split once) give the same bits as the stand-alone calls
    op = _ops.grad_tn_operand(x)
    assert torch.equal(_ops.grad_tn(grad, x, amax=_ops.absmax(grad), x_operand=op), got_tn)
    assert torch.equal(_ops.grad_nn(grad, _weights.split_f16(w.t().contiguous()), n, amax=_ops.absmax(grad)), got_nn)


@pytest.mark.parametrize("count", [1, 3, 4, 1000, 4099, 1 << 22, (1 << 22) + 2])
def test_absmax_is_exact(count):
    """egnn_absmax_f32 against torch: the exact maximum of |x| (integer atomicMax on the bit patterns), tails that are not a multiple
    of four, negative extremes, zeros, and a NaN anywhere comes back as NaN."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(count)
    x = (torch.randn(count, generator=g) * torch.logspace(-8, 3, count)).cuda()
    assert _ops.absmax(x) == float(x.abs().max())
    x[count // 2] = -1.0e9
    assert _ops.absmax(x) == 1.0e9
    x[count - 1] = -3.0e9                                                       # (the tail element)
    assert _ops.absmax(x) == float(torch.tensor(3.0e9, dtype=torch.float32))
    assert _ops.absmax(torch.zeros(count, device="cuda")) == 0.0
    x[count // 3] = float("nan")
    v = _ops.absmax(x)
    assert v != v


def test_unsplit_words_recovers_the_forward_projection():
    """egnn_unsplit_words_f32: the P_i half of the projection table as the forward's edge pass reads it ((fp16 hi, fp16 lo) words,
    egnn_linear_hl_f32 with split_cols) decoded in place equals hi + lo exactly; the P_j half is untouched; and the decoded table
    equals the all-fp32 table of the same GEMM to the split's resolution."""
    from egnn_pytorch_amd import EGNN, _ops
    torch.manual_seed(3)
    layer = EGNN(dim=64, num_nearest_neighbors=8).cuda()
    w = layer.packed_weights()
    hp = w["Hp"]
    f2d = torch.randn(200, 64, device="cuda")
    words = _ops.linear_hl(_ops.split_f16(f2d), w["Wcat_split"], 2 * hp, w["bcat"], split_cols=hp)
    full = _ops.linear_hl(_ops.split_f16(f2d), w["Wcat_split"], 2 * hp, w["bcat"], split_cols=0)
    halves = words[:, :hp].contiguous().view(torch.float16).view(200, hp, 2).float()
    want = halves[..., 0] + halves[..., 1]
    pj = words[:, hp:].clone()
    _ops.unsplit_words_(words, hp)
    assert torch.equal(words[:, :hp], want)
    assert torch.equal(words[:, hp:], pj)
    assert float((words - full).abs().max()) <= 2.0 ** -20 * float(full.abs().max())


@pytest.mark.parametrize("rows,cols", [(1000, 96), (4096, 2080), (70, 24), (129, 33)])
def test_split_scaled_both_equals_the_two_single_splits(rows, cols):
    """egnn_split_scaled_both_f16 (one read of X) writes exactly the images of the two stand-alone egnn_split_scaled_f16 calls."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * 1e-6).cuda()
    scale = _ops.grad_scale(_ops.absmax(x))
    plain, tr = _ops.split_scaled_both(x, scale)
    p1 = _ops.split_scaled(x, scale)[0]
    t1 = _ops.split_scaled(x, scale, transposed=True)[0]
    for a, b in ((plain, p1), (tr, t1)):
        assert a.kp == b.kp and a.rows == b.rows
        assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)
    # ... and, on request, the column sums of X as a by-product of the same read (a bias gradient): same images, sums against float64,
    # bit-reproducible (per 64-row block in the kernel, blocks added in fixed order)
    plain2, tr2, cs = _ops.split_scaled_both(x, scale, colsum=True)
    for a, b in ((plain2, p1), (tr2, t1)):
        assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)
    want = x.double().sum(dim=0)
    assert cs.shape == (cols,)
    assert float((cs.double() - want).abs().max()) <= 2e-6 * float(x.double().abs().sum(dim=0).max())
    assert torch.equal(cs, _ops.split_scaled_both(x, scale, colsum=True)[2])
    op = _ops.GradOperand(x, colsum=True)
    assert torch.equal(op.colsum, cs)
    assert float(_ops.GradOperand(torch.zeros_like(x), colsum=True).colsum.abs().max()) == 0.0


@pytest.mark.parametrize("dim,rows", [(32, 100), (64, 4096), (128, 5000), (256, 1300)])
def test_node_mlp_fused_matches_float64_and_the_two_launch_path(dim, rows):
    """csrc/node_mlp_fused.hip (narrow layers: W6 SiLU(W5 x + b5) + b6 + h in one launch, the hidden activation in registers): its weight
    image equals the tensor-op twin bit for bit (the permutation of W6's K-slots is the specification's), the output equals float64 at
    fp32-class accuracy and the two-launch path to the rounding of the fp32 sums; rows % 128 != 0 (a workgroup's tail) included."""
    from egnn_pytorch_amd import _ops, _weights
    g = torch.Generator().manual_seed(dim + rows)
    m = 16
    w5 = torch.randn(2 * dim, dim + m, generator=g) / (dim + m) ** 0.5
    w6 = torch.randn(dim, 2 * dim, generator=g) / (2 * dim) ** 0.5
    b5, b6 = torch.randn(2 * dim, generator=g), torch.randn(dim, generator=g)
    x = torch.randn(rows, dim + m, generator=g)
    res = torch.randn(rows, dim, generator=g)
    s5, s6 = _weights.split_f16(w5), _weights.split_f16(w6)
    want_img = _weights.node_mlp_fused_image(s5, s6, dim, m)
    s5d, s6d = tuple(t.cuda() if torch.is_tensor(t) else t for t in s5), tuple(t.cuda() if torch.is_tensor(t) else t for t in s6)
    img = _ops.node_mlp_fused_image(s5d, s6d, dim, m)
    assert torch.equal(img.cpu(), want_img)
    node_in = _ops.split_f16(x.cuda())
    out = _ops.node_mlp_fused(node_in, img, s5[2], b5.cuda(), s6[2], b6.cuda(), res.cuda(), dim, m)
    ref = torch.nn.functional.silu(x.double() @ w5.double().t() + b5.double()) @ w6.double().t() + b6.double() + res.double()
    assert float((out.double().cpu() - ref).abs().max()) <= 3e-5 * max(1.0, float(ref.abs().max()))
    hid = _ops.linear_hl(node_in, s5d, 2 * dim, b5.cuda(), act=1, out_f32=False, out_hl=True)
    two = _ops.linear_hl(hid, s6d, dim, b6.cuda(), residual=res.cuda())
    assert float((out - two).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    assert torch.equal(out, _ops.node_mlp_fused(node_in, img, s5[2], b5.cuda(), s6[2], b6.cuda(), res.cuda(), dim, m))     # bit-reproducible


def test_silu_bwd_matches_autograd():
    """egnn_silu_bwd_f32: a = SiLU(z) and gz = g SiLU'(z) in place, against torch autograd in float64."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(4)
    z = (torch.randn(513, 64, generator=g) * 4).cuda()
    gr = torch.randn(513, 64, generator=g).cuda()
    with torch.enable_grad():
        z64 = z.double().requires_grad_(True)
        a64 = torch.nn.functional.silu(z64)
        want = torch.autograd.grad(a64, z64, gr.double())[0]
    a, gz, bits = _ops.silu_bwd_(z.clone(), gr.clone())
    assert _ops.bits_to_floats(bits) == [float(a.abs().max()), float(gz.abs().max())]
    assert float((a.double() - a64.detach()).abs().max()) <= 2e-6 * float(a64.abs().max())
    assert float((gz.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())


@pytest.mark.parametrize("kw", [dict(dim=512, num_nearest_neighbors=32), dict(dim=20, m_dim=8, edge_dim=3, fourier_features=2, soft_edges=True),
                                dict(dim=24, m_dim=40, norm_feats=True, norm_coors=True), dict(dim=16, update_feats=False),
                                dict(dim=16, update_coors=False, edge_dim=1)])
def test_device_weight_pack_equals_the_tensor_op_pack(kw):
    """_weights.pack on the GPU (seven GEMM weight images from egnn_split_scaled_f16, all scale maxima in one host read) against the
    same function on the CPU (plain tensor ops; itself bit-identical to the C packer, tests/test_host_logic.py): every packed image,
    table and scale equal bit for bit -- with default-initialised and with rescaled weights."""
    from egnn_pytorch_amd import EGNN, _weights
    for mul in (1.0, 37.0):
        torch.manual_seed(7)
        layer = EGNN(**kw)
        with torch.no_grad():
            for p in layer.parameters():
                p.mul_(mul)
        want = _weights.pack(layer)
        got = _weights.pack(layer.cuda())
        assert set(want) == set(got)
        for key, a in want.items():
            b = got[key]
            if isinstance(a, tuple):                            # (hi, lo, inv_scale, rows)
                assert torch.equal(a[0], b[0].cpu()) and torch.equal(a[1], b[1].cpu()) and a[2:] == b[2:], key
            elif torch.is_tensor(a):
                assert torch.equal(a, b.cpu()), key
            elif isinstance(a, list):                           # (W2Th_blocks: one image per block of 16 message channels)
                assert len(a) == len(b) and all(torch.equal(x, y.cpu()) for x, y in zip(a, b)), key
            else:
                assert a == b, key


@pytest.mark.parametrize("b,n,k,dim,kw,ragged", [
    (2, 200, 32, 64, {}, True),                                                  # N % 4 != 0: waves past the last node; ragged mask
    (3, 129, 32, 32, dict(norm_coors=True, coor_weights_clamp_value=0.5), False),  # groups that straddle two graphs
    (1, 96, 64, 48, dict(soft_edges=True, m_pool_method="mean"), True),          # two rounds per node, gate, masked mean
    (2, 160, 128, 24, dict(norm_feats=True, m_dim=7), True),                     # four rounds per node, m_dim < 16
    (1, 64, 32, 512, dict(update_coors=False), False),                           # the north-star width (Hp = 2080: a 32-column tail chunk)
    (1, 70, 32, 16, dict(update_feats=False, valid_radius=1.5), True),           # Hp = 96; radius cut through the records
    (5, 33, 32, 8, {}, False),                                                   # Hp = 64: ONE chunk per round (the ring alternates per round)
])
def test_persistent_edge_kernel_equals_the_general_one(b, n, k, dim, kw, ragged):
    """csrc/edge_pw.hip (egnn_edge_args.algo = 0: persistent workgroups, one wave per node, records prefetched into LDS, residual on the
    4x4x4 MFMA) against csrc/edge_fused.hip's general kernel (algo = 1) on the same launch sequence: same operand layouts, same
    products, same summation order for K <= 128 -> the same bits.  Both are checked against the oracle elsewhere
    (tests/test_gpu_parity.py runs with algo = 0)."""
    from egnn_pytorch_amd import EGNN, layer as L
    g = torch.Generator().manual_seed(b * 7919 + n * 31 + k + dim)
    layer = EGNN(dim=dim, num_nearest_neighbors=k, **kw)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, generator=g)
    layer = layer.cuda().eval()
    feats = torch.randn(b, n, dim, generator=g).cuda()
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = (torch.arange(n)[None] < torch.randint(max(k, n // 2), n + 1, (b, 1), generator=g)).cuda() if ragged else None
    old = L._EDGE_ALGO
    try:
        with torch.no_grad():
            L._EDGE_ALGO = 1
            ref = layer(feats, coors, mask=mask)
            L._EDGE_ALGO = 0
            new = layer(feats, coors, mask=mask)
            again = layer(feats, coors, mask=mask)
    finally:
        L._EDGE_ALGO = old
    assert all(bool(torch.isfinite(o).all()) for o in new)
    assert torch.equal(new[0], again[0]) and torch.equal(new[1], again[1])
    assert torch.equal(new[0], ref[0]), float((new[0] - ref[0]).abs().max())
    assert torch.equal(new[1], ref[1]), float((new[1] - ref[1]).abs().max())


@pytest.mark.parametrize("b,n,dim,kw,ragged", [
    (64, 128, 32, {}, True),                                                     # four rounds per node (K = N = 128): the same bits
    (32, 256, 24, dict(norm_coors=True, soft_edges=True, m_pool_method="mean"), True),   # eight rounds: another summation order across rounds
])
def test_dense_layers_on_the_wave_per_node_kernel(b, n, dim, kw, ragged):
    """Round 5: a dense all-pairs layer with N % 32 == 0 runs csrc/edge_pw.hip when the batch fills the chip (B N >= 8192): per-slot
    records with j = k (egnn_slot_prep_f32 with idx = NULL).  Against the general kernel on the same inputs (bit-identical up to four
    rounds per node; beyond, the rounds of a node are summed in another order: 1e-5 of the output's scale) and, for two graphs, against
    the oracle at the parity tolerance."""
    from egnn_pytorch_amd import EGNN, layer as L, _ops
    g = torch.Generator().manual_seed(b + n + dim)
    layer = EGNN(dim=dim, **kw)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, generator=g)
            m.weight.data.mul_(0.3)                                               # (hundreds of neighbours per node: damped, as the dense goldens)
    layer = layer.cuda().eval()
    feats = torch.randn(b, n, dim, generator=g).cuda()
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = (torch.arange(n)[None] < torch.randint(n // 2, n + 1, (b, 1), generator=g)).cuda() if ragged else None
    old = L._DENSE_PW
    try:
        with torch.no_grad():
            L._DENSE_PW = False
            ref = layer(feats, coors, mask=mask)
            L._DENSE_PW = True
            with _ops.phase_timer() as pt:
                new = layer(feats, coors, mask=mask)
    finally:
        L._DENSE_PW = old
    assert "slot_prep" in pt.summary()                                           # (the records were built: the wave-per-node path ran)
    for a, r in zip(new, ref):
        scale = max(1.0, float(r.abs().max()))
        if n <= 128:
            assert torch.equal(a, r), float((a - r).abs().max())
        else:
            assert float((a - r).abs().max()) <= 1e-5 * scale
    from oracle import egnn_oracle as O
    cfg = O.EGNNConfig(dim=dim, **kw)
    params = {k_: v.detach().cpu().numpy() for k_, v in layer.state_dict().items()}
    want = O.egnn_forward(cfg, params, feats[:2].cpu().numpy(), coors[:2].cpu().numpy(), None, None if mask is None else mask[:2].cpu().numpy(), None)
    for a, w in zip(new, want):
        np.testing.assert_allclose(a[:2].cpu().numpy(), w, atol=1e-4 * max(1.0, float(np.abs(w).max())), rtol=0)


@pytest.mark.parametrize("b,n,k,dim,ragged", [(2, 150, 32, 64, True), (1, 80, 64, 32, False)])
def test_wave_per_node_kernel_writes_the_same_u_for_the_backward(b, n, k, dim, ragged):
    """The forward under autograd keeps u = edge_mlp.3(SiLU(edge_mlp.0(.))) (E x 16), written by the edge kernel on the side
    (egnn_edge_args.U_out): the wave-per-node kernel's against the general kernel's, bit for bit, outputs included."""
    from egnn_pytorch_amd import EGNN, layer as L
    g = torch.Generator().manual_seed(n + k)
    layer = EGNN(dim=dim, num_nearest_neighbors=k)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, generator=g)
    layer = layer.cuda().eval()
    feats = torch.randn(b, n, dim, generator=g).cuda()
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = (torch.arange(n)[None] < torch.randint(max(k, n // 2), n + 1, (b, 1), generator=g)).cuda() if ragged else None
    old = L._EDGE_ALGO
    res = {}
    try:
        for algo in (1, 0):
            L._EDGE_ALGO = algo
            out = layer._forward_hip_checked(feats, coors, None, mask, None, None, want_u=True)
            res[algo] = (out[0], out[1], out[6])
    finally:
        L._EDGE_ALGO = old
    assert res[0][2] is not None and res[0][2].shape == (b * n * k, 16)
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n,k", [(96, 32), (130, 64), (64, 64)])
def test_padded_nodes_last_in_the_order_and_the_group_flag_of_the_slot_records(n, k):
    """egnn_spatial_order_masked_f32: a permutation of each graph's nodes with every real node in front of every padded one (and the
    unmasked order when there is no mask); egnn_slot_prep_f32: bit 30 exactly on the records with k % 32 == 0 of the nodes whose group
    of four consecutive positions (over the whole batch) is all padding, bits 31 / j / x_i - x_j as before."""
    from egnn_pytorch_amd import _ops
    b = 3
    g = torch.Generator().manual_seed(n + k)
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = (torch.rand(b, n, generator=g) < 0.5)
    mask[1, : n // 2] = True
    mask[1, n // 2:] = False
    mask_d = mask.cuda()
    m8 = _ops._u8(mask_d)
    plain = _ops.spatial_order(coors).cpu()
    order = _ops.spatial_order(coors, mask8=m8).cpu()
    assert torch.equal(_ops.spatial_order(coors, mask8=None).cpu(), plain)
    for gi in range(b):
        perm = order[gi].long()
        assert torch.equal(torch.sort(perm).values, torch.arange(n))
        real = mask[gi][perm]
        nreal = int(mask[gi].sum())
        assert bool(real[:nreal].all()) and not bool(real[nreal:].any())
        # (within the real nodes and within the padded ones: the Morton order of the unmasked call)
        pl = plain[gi].long()
        assert torch.equal(perm[:nreal], pl[mask[gi][pl]]) and torch.equal(perm[nreal:], pl[~mask[gi][pl]])
    idx, rank = _ops.knn_select(coors, mask_d, None, k)
    rec = _ops.slot_prep(coors, m8, idx, rank, order.cuda(), float("inf")).cpu().view(b * n, k, 4)
    rec_nomask = _ops.slot_prep(coors, None, idx, rank, order.cuda(), float("inf")).cpu().view(b * n, k, 4)
    w0 = rec[..., 0].long() & 0xffffffff
    node_real = torch.stack([mask[gi][order[gi].long()] for gi in range(b)]).reshape(-1)          # in consumption order
    dead = ~node_real.view(-1, 4).any(dim=1) if (b * n) % 4 == 0 else None
    for node in range(b * n):
        grp = node // 4
        members = node_real[4 * grp: 4 * grp + 4]
        want = not bool(members.any())
        for kk in range(k):
            flag = (int(w0[node, kk]) >> 30) & 1
            assert flag == (1 if (want and kk % 32 == 0) else 0), (node, kk)
    assert not bool(((rec_nomask[..., 0].long() >> 30) & 1).any())
    assert torch.equal(rec[..., 0].long() & 0x3fffffff, rec_nomask[..., 0].long() & 0x3fffffff)   # j
    assert torch.equal(rec[..., 1:], rec_nomask[..., 1:])                                          # x_i - x_j
    ok = (w0 >> 31) & 1
    i_of = torch.stack([order[gi].long() for gi in range(b)]).reshape(-1)
    for node in range(0, b * n, 7):
        gi = node // n
        ii = int(i_of[node])
        jj = idx.cpu()[gi, ii].long()
        assert torch.equal(ok[node].bool(), mask[gi, ii] & mask[gi][jj])


def test_projection_gemm_skips_the_tiles_of_padded_rows_only():
    """egnn_linear_hl_lda_rows_f32: an M-tile is skipped -- its rows of C stay as they were -- exactly when none of its rows is set in the
    row mask; every other row equals the unmasked product bit for bit (set or not: tiles are computed whole).  And the predicate that says
    where a caller may use it (egnn_edge_pw_covers) for the BASELINE shapes."""
    from egnn_pytorch_amd import _abi, _ops, _weights
    g = torch.Generator().manual_seed(11)
    m, k, n = 2048 + 70, 64, 384
    a = torch.randn(m, k, generator=g).cuda()
    w = (torch.randn(n, k, generator=g) / 8).cuda()
    bias = torch.randn(n, generator=g).cuda()
    ws = _weights.split_f16(w)
    full = _ops.linear_hl(_ops.split_f16(a), ws, n, bias)
    mask = torch.zeros(m, dtype=torch.uint8)
    mask[5] = 1                    # one row of the first tile
    mask[700:900] = 1              # rows across a tile boundary
    mask[m - 1] = 1                # the ragged last tile
    got = _ops.linear_hl(_ops.split_f16(a), ws, n, bias, row_mask=mask.cuda())        # (C comes poisoned: tests/conftest.py)
    torch.cuda.synchronize()
    written = ~torch.isnan(got).any(dim=1).cpu()
    assert torch.equal(got[written.cuda()], full[written.cuda()])
    assert bool(written[mask.bool()].all())                                            # every set row was computed
    # tiles are 128 or 256 rows: a row is written iff its tile (of either size, whichever the library chose) holds a set row
    for bm in (128, 256):
        tiles = torch.zeros((m + bm - 1) // bm, dtype=torch.bool)
        tiles[torch.nonzero(mask).flatten() // bm] = True
        if torch.equal(written, tiles.repeat_interleave(bm)[:m]):
            break
    else:
        raise AssertionError("the written rows are not a union of whole M-tiles that hold a set row")
    assert not bool(written.all())                                                     # (something was skipped)
    lib = _abi.load()
    hp = lib.egnn_padded_hidden(2 * (2 * 512 + 1))
    assert lib.egnn_edge_pw_covers(64, 1024, 32, 1, 0, 0, 16, 3, 2 * hp) == 1          # north star
    assert lib.egnn_edge_pw_covers(64, 1024, 64, 1, 0, 0, 16, 3, 2 * hp) == 1
    assert lib.egnn_edge_pw_covers(32, 2048, 3, 5, 0, 4, 16, 3, 2 * hp) == 0           # c4: K = 3, edge features -> the general kernel
    assert lib.egnn_edge_pw_covers(64, 1024, 32, 1, 0, 0, 16, 5, 2 * hp) == 0          # other coordinate dimensions
    assert lib.egnn_edge_pw_covers(64, 1024, 32, 1, 0, 0, 32, 3, 2 * hp) == 0          # wide heads
    assert lib.egnn_edge_pw_covers(64, 1024, 40, 1, 0, 0, 16, 3, 2 * hp) == 0          # K % 32 != 0
