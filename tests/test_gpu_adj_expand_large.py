"""N-degree adjacency expansion (csrc/adj_expand.hip) beyond 4 096 nodes on the MI355X: the any-N kernel
(egnn_adj_expand_wide_u8, taken by egnn_adj_expand_u8 above 4 096 nodes) bit-exact against the oracle and against the reference's
recipe restated in torch, equal to the one-word-per-lane kernel where both run, and EGNN_Network(num_adj_degrees=...) on graphs of
far-apart clusters against the same network run on each cluster alone."""
import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O

pytestmark = pytest.mark.gpu


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _adj_kind(kind, n, b, rng):
    """(B, N, N) bool: the kinds of test_gpu_kernels.py::test_adj_expand_bit_exact."""
    i = np.arange(n)
    if kind == "chain":
        return np.broadcast_to(np.abs(i[:, None] - i[None, :]) <= 1, (b, n, n)).copy()
    if kind == "chain_nodiag":
        return np.broadcast_to(np.abs(i[:, None] - i[None, :]) == 1, (b, n, n)).copy()
    if kind == "sparse_random":                                          # asymmetric, empty rows, no forced diagonal
        return rng.random((b, n, n)) < min(0.01, 2.0 / n)
    adj = rng.random((b, n, n)) < min(0.03, 4.0 / n)
    return adj | adj.transpose(0, 2, 1) | np.eye(n, dtype=bool)[None]


KINDS = ["chain", "chain_nodiag", "random", "sparse_random"]


# ------------------------------------------------------------------ 1. above 4 096 nodes the expansion and the network run
def test_network_with_adjacency_degrees_on_5000_nodes_returns():
    from egnn_pytorch_amd import EGNN_Network, _ops
    n = 5000
    torch.manual_seed(0)
    net = EGNN_Network(num_tokens=10, dim=16, depth=2, num_nearest_neighbors=8, num_adj_degrees=3, adj_dim=4).cuda()
    tokens = torch.randint(0, 10, (1, n), device="cuda")
    coors = torch.randn(1, n, 3, device="cuda")
    i = torch.arange(n, device="cuda")
    adj = (i[:, None] - i[None, :]).abs() <= 1
    with torch.no_grad():
        h, x = net(tokens, coors, adj_mat=adj)
    torch.cuda.synchronize()
    assert h.shape == (1, n, 16) and x.shape == (1, n, 3)
    assert torch.isfinite(h).all() and torch.isfinite(x).all()
    out_adj, deg = _ops.adj_expand(adj[:4097, :4097], 1, 2)
    assert out_adj.shape == (1, 4097, 4097) and deg.shape == (1, 4097, 4097)


# ------------------------------------------------------------------ 2. bit-exact against the oracle just above the old limit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4097, 4160, 5000])
def test_adj_expand_beyond_4096_bit_exact(n, kind):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n + len(kind))
    b = 2
    adj = _adj_kind(kind, n, b, rng)
    a_dev = _dev(adj)
    for degrees in (1, 2, 3, 4):
        ref_idx, ref_adj = O.adjacency_degrees(adj, degrees)
        out_adj, out_idx = _ops.adj_expand(a_dev, b, degrees)
        np.testing.assert_array_equal(out_idx.cpu().numpy().astype(np.int64), ref_idx)
        np.testing.assert_array_equal(out_adj.cpu().numpy(), ref_adj)
        out_adj2, out_idx2 = _ops.adj_expand(a_dev[0], b, degrees)          # shared (N,N) adjacency broadcast over the batch
        for bb in range(b):
            np.testing.assert_array_equal(out_idx2[bb].cpu().numpy().astype(np.int64), ref_idx[0])
            np.testing.assert_array_equal(out_adj2[bb].cpu().numpy(), ref_adj[0])
        del out_adj, out_idx, out_adj2, out_idx2


# ------------------------------------------------------------------ 3. bit-exact at 40 000 / 65 536 nodes against the recipe in torch
def _recipe_step(cur, blk=4096):
    """(cur @ cur) > 0 for an (N, N) bool matrix: 0/1 operands in bf16 with fp32 accumulation (the products are exact and a sum of
    non-negative terms cannot round to zero: exact for N < 2^24), in row blocks."""
    a = cur.to(torch.bfloat16)
    nxt = torch.empty_like(cur)
    for lo in range(0, cur.shape[0], blk):
        nxt[lo:lo + blk] = (a[lo:lo + blk] @ a) > 0
    del a
    return nxt


def _large_adj(kind, n, seed):
    """(N, N) bool on the device: a chain without its diagonal (edges disappear: the XOR), or ~2 random out-edges per row with some
    empty rows (asymmetric, no diagonal)."""
    i = torch.arange(n, device="cuda")
    if kind == "chain_nodiag":
        adj = torch.zeros(n, n, dtype=torch.bool, device="cuda")
        adj[i[1:], i[:-1]] = True
        adj[i[:-1], i[1:]] = True
        return adj
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = i.repeat_interleave(2)
    dst = torch.randint(0, n, (2 * n,), device="cuda", generator=g)
    keep = src % 7 != 3                                                  # every 7th row stays empty
    adj = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    adj[src[keep], dst[keep]] = True
    return adj


@pytest.mark.parametrize("kind", ["chain_nodiag", "sparse_random"])
@pytest.mark.parametrize("n", [40000, 65536])
def test_adj_expand_large_bit_exact_against_the_recipe(n, kind):
    from egnn_pytorch_amd import _ops
    adj = _large_adj(kind, n, n + 1)
    labels = adj.to(torch.uint8)
    cur = adj
    for degrees in (2, 3, 4):
        nxt = _recipe_step(cur)
        labels[nxt != cur] = degrees
        cur = nxt
        out_adj, out_idx = _ops.adj_expand(adj, 1, degrees)
        assert torch.equal(out_idx[0], labels)
        assert torch.equal(out_adj[0], cur)
        del out_adj, out_idx
    del adj, labels, cur, nxt
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. the any-N kernel equals the one-word-per-lane kernel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [16, 70, 1024, 4096])
def test_adj_expand_wide_equals_the_pinned_kernel(n, kind):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(3 * n + len(kind))
    b = 3
    adj = _dev(_adj_kind(kind, n, b, rng))
    for degrees in (1, 2, 3, 4, 9):
        for a in (adj, adj[1]):
            ref_adj, ref_idx = _ops.adj_expand(a, b, degrees)
            got_adj, got_idx = _ops.adj_expand_wide(a, b, degrees)
            assert torch.equal(got_idx, ref_idx) and torch.equal(got_adj, ref_adj)


# ------------------------------------------------------------------ 5. EGNN_Network on graphs of far-apart clusters
CL = 4096


def _cluster_adj(n_clusters):
    """(N, N) bool, block-diagonal: every cluster the same chain (with its diagonal) plus the same fixed contacts, so that the
    global maximum degree is each cluster's (only_sparse_neighbors takes K from it)."""
    i = torch.arange(CL, device="cuda")
    blk = (i[:, None] - i[None, :]).abs() <= 1
    a = torch.arange(0, CL - 40, 97, device="cuda")
    blk[a, a + 31] = True
    blk[a + 31, a] = True
    adj = torch.zeros(n_clusters * CL, n_clusters * CL, dtype=torch.bool, device="cuda")
    for c in range(n_clusters):
        adj[c * CL:(c + 1) * CL, c * CL:(c + 1) * CL] = blk
    return adj


def _clusters(n_clusters, dtype, seed, k):
    """Coordinates (1, n_clusters * 4096, 3): unit-normal clusters on a 3 x 2 x 2 grid of spacing 40; a ragged mask that leaves
    every cluster >= 3 K real nodes at its end (as tests/test_gpu_large_graphs.py)."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in range(3) for y in range(2) for z in range(2)], dtype=np.float64)[:n_clusters] * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None].astype(dtype)
    real = CL - rng.integers(0, CL - 3 * k, size=n_clusters)
    real[0] = CL
    mask = np.concatenate([np.arange(CL) < real[c] for c in range(n_clusters)])[None]
    return coors, mask


@pytest.mark.parametrize("mode", ["c_forward", "python_launch", "sparse_only", "float64"])
def test_network_with_adjacency_degrees_on_clustered_graph_matches_each_cluster_alone(mode, monkeypatch):
    from egnn_pytorch_amd import EGNN_Network, layer as L
    n_clusters = 6 if mode == "float64" else 10                          # 24 576 (float64) / 40 960 nodes
    k = 16
    coors, mask = _clusters(n_clusters, np.float64 if mode == "float64" else np.float32, 21, k)
    torch.manual_seed(5)
    net = EGNN_Network(num_tokens=20, dim=32, depth=2, num_nearest_neighbors=k, num_adj_degrees=3, adj_dim=4,
                       only_sparse_neighbors=mode == "sparse_only").cuda()
    if mode == "float64":
        net = net.double()
    if mode == "python_launch":
        monkeypatch.setattr(L, "_C_FORWARD", False)
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    c, m = _dev(coors), _dev(mask)
    adj = _cluster_adj(n_clusters)
    with torch.no_grad():
        big = net(tokens, c, adj_mat=adj, mask=m)
        alone = []
        for cl in range(n_clusters):
            s = slice(cl * CL, (cl + 1) * CL)
            alone.append(net(tokens[:, s], c[:, s], adj_mat=adj[s, s], mask=m[:, s]))
    del adj
    for t, x in enumerate(big):
        torch.testing.assert_close(x, torch.cat([a[t] for a in alone], 1), rtol=1e-5, atol=1e-5)


def test_network_with_adjacency_degrees_exact_arithmetic_on_clustered_graph():
    from egnn_pytorch_amd import EGNN_Network, exact_arithmetic
    n_clusters, k = 10, 16
    coors, mask = _clusters(n_clusters, np.float32, 22, k)
    torch.manual_seed(6)
    net = EGNN_Network(num_tokens=20, dim=32, depth=2, num_nearest_neighbors=k, num_adj_degrees=3, adj_dim=4).cuda()
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    c, m = _dev(coors), _dev(mask)
    adj = _cluster_adj(n_clusters)
    with torch.no_grad(), exact_arithmetic():
        big = net(tokens, c, adj_mat=adj, mask=m)
        alone = [net(tokens[:, cl * CL:(cl + 1) * CL], c[:, cl * CL:(cl + 1) * CL], adj_mat=adj[cl * CL:(cl + 1) * CL, cl * CL:(cl + 1) * CL],
                     mask=m[:, cl * CL:(cl + 1) * CL]) for cl in range(n_clusters)]
    del adj
    for t, x in enumerate(big):
        torch.testing.assert_close(x, torch.cat([a[t] for a in alone], 1), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ 6. training above the old limit
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_network_training_with_adjacency_degrees_on_8192_nodes_matches_each_cluster_alone(dtype):
    """Forward + backward on 2 clusters (8 192 nodes) with edge tokens: the (1,N,N,edge_dim+adj_dim) edge tensor is materialised
    under autograd (2 GB in fp32); gradients of the coordinates and of every parameter equal the per-cluster sums."""
    from egnn_pytorch_amd import EGNN_Network
    n_clusters, k = 2, 16
    coors, mask = _clusters(n_clusters, np.float32 if dtype == torch.float32 else np.float64, 23, k)
    torch.manual_seed(7)
    net = EGNN_Network(num_tokens=20, num_edge_tokens=6, edge_dim=4, dim=16, depth=2, num_nearest_neighbors=k, num_adj_degrees=3,
                       adj_dim=4).cuda().to(dtype)
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    edge_tok = torch.randint(0, 6, (1, n, n), device="cuda")           # int64: 0.5 GB
    wn = torch.randn(1, n, 16, dtype=dtype, device="cuda")
    wc = torch.randn(1, n, 3, dtype=dtype, device="cuda")
    c, m = _dev(coors), _dev(mask)
    adj = _cluster_adj(n_clusters)

    def grads(s):
        net.zero_grad()
        x = c[:, s].clone().requires_grad_(True)
        h, co = net(tokens[:, s], x, adj_mat=adj[s, s], edges=edge_tok[:, s, s].contiguous(), mask=m[:, s])
        ((h * wn[:, s]).sum() + (co * wc[:, s]).sum()).backward()
        out = (h.detach(), co.detach(), x.grad, {name: p.grad.clone() for name, p in net.named_parameters() if p.grad is not None})
        del h, co
        torch.cuda.empty_cache()
        return out

    hb, cb, gc, gp = grads(slice(0, n))
    gp_sum = None
    for cl in range(n_clusters):
        s = slice(cl * CL, (cl + 1) * CL)
        h1, c1, gc1, p1 = grads(s)
        torch.testing.assert_close(hb[:, s], h1, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(cb[:, s], c1, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(gc[:, s], gc1, rtol=1e-4, atol=1e-4)
        gp_sum = p1 if gp_sum is None else {name: gp_sum[name] + p1[name] for name in p1}
    assert gp.keys() == gp_sum.keys()
    assert {"adj_emb.weight", "token_emb.weight", "edge_emb.weight"} <= gp.keys()
    for name in gp:
        torch.testing.assert_close(gp[name], gp_sum[name], rtol=1e-4, atol=1e-4)
    del edge_tok, adj
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 7. determinism
def test_network_with_adjacency_degrees_on_40000_nodes_is_deterministic():
    from egnn_pytorch_amd import EGNN_Network, _ops
    n = 40000
    torch.manual_seed(8)
    net = EGNN_Network(num_tokens=10, dim=16, depth=2, num_nearest_neighbors=8, num_adj_degrees=3, adj_dim=4).cuda()
    tokens = torch.randint(0, 10, (1, n), device="cuda")
    coors = torch.randn(1, n, 3, device="cuda") * 4
    mask = (torch.arange(n, device="cuda") < n - 777)[None]
    adj = _large_adj("sparse_random", n, 9)
    adj |= adj.T.clone()
    with torch.no_grad():
        r1 = net(tokens, coors, adj_mat=adj, mask=mask)
        r2 = net(tokens, coors, adj_mat=adj, mask=mask)
    assert torch.isfinite(r1[0]).all() and torch.isfinite(r1[1]).all()
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    a1, d1 = _ops.adj_expand(adj, 1, 3)
    a2, d2 = _ops.adj_expand(adj, 1, 3)
    assert torch.equal(a1, a2) and torch.equal(d1, d2)
