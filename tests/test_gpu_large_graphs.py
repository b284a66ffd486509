"""Graphs beyond the LDS-resident kernels on the MI355X: the streaming k-NN selection (csrc/knn_stream.hip, N > 32 768 with C <= 8,
beyond the LDS check otherwise and in float64) and the banded destination lists (csrc/entry_lists.hip, N > 20 415), and whole layers
on them.  No N x N oracle: the selection is checked on sampled rows, the layers on graphs of far-apart clusters against the same
layer run on each cluster alone."""
import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O

pytestmark = pytest.mark.gpu


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _sampled_topk(coors, mask, adj_rows, rows, k):
    """The oracle's ranking + stable top-k for the rows `rows` of graph 0 only (adj_rows: those rows of the (N, N) adjacency)."""
    c = coors[0]
    n = c.shape[0]
    dist = O.inner_sum((c[rows, None] - c[None]) ** 2)                    # (R, N), the order of O.pairwise
    ranking = dist.copy()
    if mask is not None:
        m = mask[0]
        ranking[~(m[rows, None] & m[None, :])] = dist.dtype.type(O.RANK_MASKED)
    if adj_rows is not None:
        diag = rows[:, None] == np.arange(n)[None, :]
        ranking[diag] = dist.dtype.type(O.RANK_SELF)
        ranking[adj_rows & ~diag] = dist.dtype.type(O.RANK_ADJ)
    return O.topk_smallest(ranking, k)


def _random_sym_adj(n, per_row, seed):
    """(N, N) bool on the device: a random symmetric adjacency (~2 per_row neighbours per node) with the diagonal set."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    adj = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    i = torch.arange(n, device="cuda").repeat_interleave(per_row)
    j = torch.randint(0, n, (n * per_row,), device="cuda", generator=g)
    adj[i, j] = True
    adj[j, i] = True
    adj[torch.arange(n, device="cuda"), torch.arange(n, device="cuda")] = True
    return adj


# ------------------------------------------------------------------ 1. a k-NN layer beyond 32 768 nodes runs
def test_knn_layer_on_40000_nodes_returns():
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(0)
    layer = EGNN(dim=32, num_nearest_neighbors=16).cuda()
    feats = torch.randn(1, 40000, 32, device="cuda")
    coors = torch.randn(1, 40000, 3, device="cuda")
    with torch.no_grad():
        node, co = layer(feats, coors)
    torch.cuda.synchronize()
    assert node.shape == (1, 40000, 32) and co.shape == (1, 40000, 3)
    assert torch.isfinite(node).all() and torch.isfinite(co).all()


# ------------------------------------------------------------------ 2. selection beyond the limits, bit-exact on sampled rows
@pytest.mark.parametrize("n,k,cdim,dtype,adj_kind", [
    (40000, 32, 3, np.float32, None), (65536, 32, 3, np.float32, None), (40000, 32, 3, np.float32, "random"),
    (24000, 32, 3, np.float64, None), (42000, 16, 12, np.float32, None),
])
def test_knn_select_beyond_the_lds_limit_sampled_rows(n, k, cdim, dtype, adj_kind):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n + k + cdim)
    coors = rng.standard_normal((1, n, cdim)).astype(dtype)
    mask = (np.arange(n) < n - 1234)[None, :]                            # ragged: the tail is padding
    adj = _random_sym_adj(n, 3, n) if adj_kind else None
    rows = np.sort(np.concatenate([rng.choice(n, 250, replace=False), [0, n - 1, n - 1234, n - 1235, 5, 6]]))
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), adj, k)
    idx2, rank2 = _ops.knn_select(_dev(coors), _dev(mask), adj, k)
    adj_rows = adj[torch.from_numpy(rows).cuda()].cpu().numpy() if adj is not None else None
    ref_val, ref_idx = _sampled_topk(coors, mask, adj_rows, rows, k)
    idx, rank = idx.cpu().numpy()[0, rows], rank.cpu().numpy()[0, rows]
    view = np.uint64 if dtype == np.float64 else np.uint32
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx)
    np.testing.assert_array_equal(ref_val.view(view), rank.view(view))
    assert torch.equal(idx2.cpu()[0, rows], torch.from_numpy(idx)) and torch.equal(rank2.cpu()[0, rows], torch.from_numpy(rank))


# ------------------------------------------------------------------ 3. the streaming entry equals the pinned kernels where they run
@pytest.mark.parametrize("n,k,cdim,dtype,use_mask,adj_kind,b", [
    # the parametrisations of test_gpu_kernels.py::test_knn_select_bit_exact
    (16, 4, 3, np.float32, False, None, 3), (64, 8, 3, np.float32, True, None, 3), (100, 7, 3, np.float32, True, None, 3),
    (256, 32, 3, np.float32, True, None, 3), (1024, 32, 3, np.float32, True, None, 3), (2048, 16, 3, np.float32, False, None, 3),
    (300, 40, 3, np.float32, True, "random", 3), (64, 8, 3, np.float32, True, "chain", 3), (4096, 8, 3, np.float32, False, None, 3),
    (33, 33, 3, np.float32, True, None, 3), (1024, 100, 3, np.float32, True, None, 3), (6000, 16, 3, np.float32, True, None, 1),
    (8192, 32, 3, np.float32, False, None, 1), (9000, 32, 3, np.float32, False, None, 1), (8300, 700, 3, np.float32, True, None, 1),
    # other coordinate dimensions, float64, K = 1024, (B, N, N) adjacency
    (3000, 16, 2, np.float32, True, None, 2), (2000, 24, 12, np.float32, True, "random", 2), (1500, 20, 5, np.float32, False, "chain", 2),
    (3000, 16, 3, np.float64, True, None, 2), (1200, 40, 7, np.float64, True, "random", 2), (4000, 1024, 3, np.float32, True, None, 1),
    (2500, 1024, 3, np.float64, True, None, 1), (12000, 8, 3, np.float32, True, None, 1),
])
def test_knn_select_stream_equals_the_pinned_kernels(n, k, cdim, dtype, use_mask, adj_kind, b):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n * 7 + k * 3 + cdim)
    coors = rng.standard_normal((b, n, cdim)).astype(dtype)
    mask = None
    if use_mask:
        lens = rng.integers(max(k, n // 2) if n != 8300 else 500, (n + 1) if n != 8300 else 600, size=b)
        mask = np.arange(n)[None, :] < lens[:, None]
    adj = None
    if adj_kind == "chain":
        i = np.arange(n)
        adj = _dev(np.abs(i[:, None] - i[None, :]) <= 1)
    elif adj_kind == "random":
        adj = torch.stack([_random_sym_adj(n, 2, n + bb) for bb in range(b)])        # (B, N, N)
    ci, cm = _dev(coors), _dev(mask)
    ref_idx, ref_rank = _ops.knn_select(ci, cm, adj, k)
    idx, rank = _ops.knn_select_stream(ci, cm, adj, k)
    idx2, rank2 = _ops.knn_select_stream(ci, cm, adj, k)
    assert torch.equal(idx, ref_idx)
    assert torch.equal(rank.view(torch.int64 if dtype == np.float64 else torch.int32),
                       ref_rank.view(torch.int64 if dtype == np.float64 else torch.int32))
    assert torch.equal(idx2, idx) and torch.equal(rank2, rank)


def test_knn_select_stream_with_duplicated_coordinates():
    """Rows with many exactly equal distances (every node repeated 40 times, a coarse grid): long runs of equal keys straddle K, the
    index digits of the radix select decide."""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(5)
    base = rng.integers(-3, 4, size=(1, 150, 3)).astype(np.float32)
    coors = np.repeat(base, 40, axis=1)[:, rng.permutation(6000)]
    mask = (np.arange(6000) < 5800)[None]
    for k in (16, 100, 1024):
        ref = _ops.knn_select(_dev(coors), _dev(mask), None, k)
        got = _ops.knn_select_stream(_dev(coors), _dev(mask), None, k)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


# ------------------------------------------------------------------ 4. destination lists beyond 20 415 nodes
@pytest.mark.parametrize("b,n,k", [(1, 24000, 16), (2, 40000, 32), (1, 40000, 80)])
def test_dest_lists_beyond_the_lds_limit_equal_a_stable_sort(b, n, k):
    from egnn_pytorch_amd import _ops, autograd as A
    g = torch.Generator().manual_seed(b + n + k)
    base = torch.randint(0, n, (b, n, 1), generator=g)
    step = torch.randint(1, n // k, (b, n, 1), generator=g)
    idx = ((base + step * torch.arange(k)[None, None, :]) % n).to(torch.int32)
    idx[:, ::5, 0] = 7                                                    # a hub: 1 / 5 of the rows lead to node 7 ...
    hit = (idx[:, ::5, 1:] == 7)
    idx[:, ::5, 1:] = torch.where(hit, torch.full_like(idx[:, ::5, 1:], n - 1), idx[:, ::5, 1:])
    rows_ok = (idx.sort(dim=-1).values.diff(dim=-1) != 0).all(dim=-1)     # ... keep the rows whose destinations stay distinct
    idx = torch.where(rows_ok[..., None], idx, ((base + step * torch.arange(k)[None, None, :]) % n).to(torch.int32)).cuda()
    dest = (idx.long() + (torch.arange(b, device="cuda") * n)[:, None, None]).reshape(-1)
    dl = _ops.dest_lists(idx, b, n, k, "cuda")
    dl2 = _ops.dest_lists(idx, b, n, k, "cuda")
    dest_sorted, by_dest = torch.sort(dest, stable=True)
    seg = torch.searchsorted(dest_sorted, torch.arange(b * n + 1, device="cuda"))
    assert torch.equal(dl.seg, seg)
    assert torch.equal(dl.order, by_dest)
    ent, tile_seg = A.entry_list(by_dest, dest_sorted, b * n)
    assert torch.equal(dl.tile_seg, tile_seg) and torch.equal(dl.ent, ent)
    assert torch.equal(dl.ent, dl2.ent) and torch.equal(dl.order, dl2.order)


# ------------------------------------------------------------------ 5. layers on graphs of far-apart clusters
CL = 4096


def _clusters(n_clusters, dtype, seed, k):
    """(1, n_clusters * 4096, 3) coordinates: unit-normal clusters on a 3 x 2 x 2 grid of spacing 40 (squared distances across clusters
    > ~900, within a cluster < ~150, all < 1e5), a ragged mask that leaves every cluster >= 3 K real nodes at its end."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in range(3) for y in range(2) for z in range(2)], dtype=np.float64)[:n_clusters] * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None].astype(dtype)
    real = CL - rng.integers(0, CL - 3 * k, size=n_clusters)
    real[0] = CL
    mask = np.concatenate([np.arange(CL) < real[c] for c in range(n_clusters)])[None]
    return coors, mask


def _per_cluster_forward(layer, feats, coors, mask, n_clusters):
    outs = []
    for c in range(n_clusters):
        s = slice(c * CL, (c + 1) * CL)
        outs.append(layer(feats[:, s], coors[:, s], mask=mask[:, s]))
    return torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)


@pytest.mark.parametrize("mode", ["c_forward", "python_launch", "exact", "float64"])
def test_layer_on_clustered_graph_matches_each_cluster_alone(mode, monkeypatch):
    from egnn_pytorch_amd import EGNN, exact_arithmetic, layer as L
    n_clusters = 6 if mode == "float64" else 10                         # 24 576 (float64) / 40 960 nodes
    k = 16
    dtype = np.float64 if mode == "float64" else np.float32
    coors, mask = _clusters(n_clusters, dtype, 11, k)
    torch.manual_seed(1)
    layer = EGNN(dim=32, num_nearest_neighbors=k).cuda()
    if mode == "float64":
        layer = layer.double()
    if mode == "python_launch":
        monkeypatch.setattr(L, "_C_FORWARD", False)
    feats = torch.randn(1, coors.shape[1], 32, dtype=torch.float64 if mode == "float64" else torch.float32).cuda()
    c, m = _dev(coors), _dev(mask)
    with torch.no_grad():
        if mode == "exact":
            with exact_arithmetic():
                big = layer(feats, c, mask=m)
                alone = _per_cluster_forward(layer, feats, c, m, n_clusters)
        else:
            big = layer(feats, c, mask=m)
            alone = _per_cluster_forward(layer, feats, c, m, n_clusters)
    for x, y in zip(big, alone):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layer_backward_on_clustered_graph_matches_each_cluster_alone(dtype):
    from egnn_pytorch_amd import EGNN
    k = 16
    n_clusters = 10 if dtype == torch.float32 else 6                     # 40 960 / 24 576 nodes
    coors, mask = _clusters(n_clusters, np.float32 if dtype == torch.float32 else np.float64, 12, k)
    torch.manual_seed(2)
    layer = EGNN(dim=32, num_nearest_neighbors=k).cuda().to(dtype)
    n = coors.shape[1]
    feats = torch.randn(1, n, 32, dtype=dtype, device="cuda")
    wn = torch.randn(1, n, 32, dtype=dtype, device="cuda")
    wc = torch.randn(1, n, 3, dtype=dtype, device="cuda")
    c, m = _dev(coors), _dev(mask)

    def grads(s):
        layer.zero_grad()
        f = feats[:, s].clone().requires_grad_(True)
        x = c[:, s].clone().requires_grad_(True)
        node, co = layer(f, x, mask=m[:, s])
        ((node * wn[:, s]).sum() + (co * wc[:, s]).sum()).backward()
        return f.grad, x.grad, {name: p.grad.clone() for name, p in layer.named_parameters() if p.grad is not None}

    gf, gc, gp = grads(slice(0, n))
    gp_sum = None
    for cl in range(n_clusters):
        s = slice(cl * CL, (cl + 1) * CL)
        f1, c1, p1 = grads(s)
        torch.testing.assert_close(gf[:, s], f1, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(gc[:, s], c1, rtol=1e-4, atol=1e-4)
        gp_sum = p1 if gp_sum is None else {name: gp_sum[name] + p1[name] for name in p1}
    assert gp.keys() == gp_sum.keys()
    for name in gp:
        torch.testing.assert_close(gp[name], gp_sum[name], rtol=1e-4, atol=1e-4)


def test_training_with_dropout_and_network_beyond_32768_nodes():
    """Training with dropout, and EGNN_Network (no num_adj_degrees), on a 40 000-node k-NN graph: they run, deterministically."""
    from egnn_pytorch_amd import EGNN, EGNN_Network
    n = 40000
    torch.manual_seed(3)
    layer = EGNN(dim=16, num_nearest_neighbors=8, dropout=0.1).cuda().train()
    feats = torch.randn(1, n, 16, device="cuda")
    coors = torch.randn(1, n, 3, device="cuda") * 4
    mask = (torch.arange(n, device="cuda") < n - 999)[None]
    res = []
    for _ in range(2):
        torch.manual_seed(4)
        layer.zero_grad()
        f = feats.clone().requires_grad_(True)
        node, co = layer(f, coors, mask=mask)
        (node.square().mean() + co.square().mean()).backward()
        res.append((node.detach(), f.grad, [p.grad.clone() for p in layer.parameters() if p.grad is not None]))
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))

    net = EGNN_Network(num_tokens=10, dim=16, depth=2, num_nearest_neighbors=8).cuda()
    tokens = torch.randint(0, 10, (1, n), device="cuda")
    with torch.no_grad():
        h, x = net(tokens, coors, mask=mask)
    assert h.shape == (1, n, 16) and x.shape == (1, n, 3)
    assert torch.isfinite(h).all() and torch.isfinite(x).all()
