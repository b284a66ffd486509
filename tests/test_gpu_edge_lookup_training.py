"""EGNN_Network training on edge look-up tables: under autograd the layers read the embedding rows of the K selected pairs
(egnn_edge_features_gather_f32) and the embedding gradients come from egnn_edge_features_grad_f32 (csrc/segment_sum.hip), a
fixed-order reduction over the selected pairs.  Nothing of size B N^2 D is allocated, except the gradient of dense float edges the
caller passed in.  Checked against the materialised recipe (the dense (B,N,N,D) tensor fed to each EGNN layer), against float64,
the reduction against a float64 index_add_, and at 49 152 nodes against each cluster trained alone."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = 4096


# ------------------------------------------------------------------ helpers
def _chain_adj(n, seed):
    """(N, N) bool: a chain with its diagonal plus a few random symmetric contacts."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    adj = (i[:, None] - i[None, :]).abs() <= 1
    a = torch.randint(0, n, (max(1, n // 16),), generator=g)
    b = torch.randint(0, n, (max(1, n // 16),), generator=g)
    adj[a, b] = True
    adj[b, a] = True
    return adj.cuda()


def _cluster_adj(n_clusters):
    """(N, N) bool, block-diagonal: the same chain plus fixed contacts in every cluster of CL nodes."""
    i = torch.arange(CL, device="cuda")
    blk = (i[:, None] - i[None, :]).abs() <= 1
    a = torch.arange(0, CL - 40, 97, device="cuda")
    blk[a, a + 31] = True
    blk[a + 31, a] = True
    adj = torch.zeros(n_clusters * CL, n_clusters * CL, dtype=torch.bool, device="cuda")
    for c in range(n_clusters):
        adj[c * CL:(c + 1) * CL, c * CL:(c + 1) * CL] = blk
    return adj


def _clusters(n_clusters, seed, k):
    """Coordinates (1, n_clusters * CL, 3): unit-normal clusters 40 apart on a 3 x 2 x 2 grid; a ragged mask that leaves every
    cluster >= 3 K real nodes."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in range(3) for y in range(2) for z in range(2)], dtype=np.float64)[:n_clusters] * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None].astype(np.float32)
    real = CL - rng.integers(0, CL - 3 * k, size=n_clusters)
    real[0] = CL
    mask = np.concatenate([np.arange(CL) < real[c] for c in range(n_clusters)])[None]
    return torch.from_numpy(coors).cuda(), torch.from_numpy(mask).cuda()


def _materialised(net, tokens, coors, adj, edge_tok=None, dense_edges=None, mask=None):
    """EGNN_Network's forward with the (B,N,N,edge_dim+adj_dim) edge tensor built densely in torch and handed to each EGNN layer."""
    from egnn_pytorch_amd import _ops
    b, n = tokens.shape[:2]
    feats = net.token_emb(tokens) if net.token_emb is not None else tokens
    if net.pos_emb is not None:
        feats = feats + net.pos_emb(torch.arange(n, device=feats.device))[None]
    parts = []
    if edge_tok is not None:
        parts.append(net.edge_emb(edge_tok))
    elif dense_edges is not None:
        parts.append(dense_edges)
    adj_mat = adj
    if net.num_adj_degrees is not None:
        adj_mat, deg = _ops.adj_expand(adj, b, net.num_adj_degrees)
        if net.adj_emb is not None:
            parts.append(net.adj_emb(deg.long()))
    edges = torch.cat(parts, dim=-1) if len(parts) > 1 else (parts[0] if parts else None)
    gt = net.global_tokens[None].expand(b, -1, -1) if net.global_tokens is not None else None
    for attn, egnn in net.layers:
        if attn is not None:
            feats, gt = attn(feats, gt, mask=mask)
        feats, coors = egnn(feats, coors, edges=edges, mask=mask, adj_mat=adj_mat)
    return feats, coors


EDGES = {                                                   # network keyword arguments of each edge-feature kind
    "tok": dict(num_edge_tokens=6, edge_dim=4),
    "deg": dict(num_adj_degrees=3, adj_dim=4),
    "both": dict(num_edge_tokens=6, edge_dim=4, num_adj_degrees=3, adj_dim=4),
    "dense_deg": dict(edge_dim=3, num_adj_degrees=2, adj_dim=4),
}
MODES = {
    "knn": dict(num_nearest_neighbors=8),
    "sparse": dict(only_sparse_neighbors=True),
    "dense": dict(),
}


def _setup(n, edges, mode, extra="plain", seed=0):
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(seed)
    kw = dict(num_tokens=11, dim=16, depth=2, norm_coors=True, **EDGES[edges], **MODES[mode])
    if extra == "attn":
        kw.update(num_positions=n, global_linear_attn_every=1, global_linear_attn_heads=2, global_linear_attn_dim_head=8)
    if extra == "dropout":
        kw.update(dropout=0.2)
    net = EGNN_Network(**kw).cuda()
    if extra == "dropout":
        net.train()
    tokens = torch.randint(0, 11, (2, n), device="cuda")
    coors = torch.randn(2, n, 3, device="cuda")
    mask = torch.ones(2, n, dtype=torch.bool, device="cuda")
    mask[1, n - n // 5:] = False
    adj = _chain_adj(n, seed + n)
    inp = dict(edge_tok=None, dense_edges=None)
    if "num_edge_tokens" in EDGES[edges]:
        inp["edge_tok"] = torch.randint(0, 6, (2, n, n), device="cuda")
    if edges == "dense_deg":
        inp["dense_edges"] = torch.randn(2, n, n, 3, device="cuda")
    return net, tokens, coors, mask, adj, inp


def _step(fn, coors, wn, wc, params, extra_leaf=None, seed=123):
    """one forward + backward of fn(x) -> (h, co); returns (h, co, d/d coors, {name: grad}, d/d extra_leaf)"""
    x = coors.clone().requires_grad_(True)
    for _, p in params:
        p.grad = None
    if extra_leaf is not None:
        extra_leaf.grad = None
    torch.manual_seed(seed)                                 # (the dropout seeds come from the CPU generator)
    h, co = fn(x)
    ((h * wn).sum() + (co * wc).sum()).backward()
    grads = {name: p.grad.clone() for name, p in params if p.grad is not None}
    return h.detach(), co.detach(), x.grad, grads, None if extra_leaf is None else extra_leaf.grad.clone()


def _compare(net, tokens, coors, mask, adj, inp, ctx=None):
    import contextlib
    ctx = ctx or contextlib.nullcontext
    n = tokens.shape[1]
    wn = torch.randn(2, n, 16, device="cuda")
    wc = torch.randn(2, n, 3, device="cuda")
    params = list(net.named_parameters())
    de = inp["dense_edges"]
    leaf = de.clone().requires_grad_(True) if de is not None else None
    with ctx():
        got = _step(lambda x: net(tokens, x, adj_mat=adj, edges=inp["edge_tok"] if leaf is None else leaf, mask=mask), coors, wn, wc,
                    params, leaf)
        want = _step(lambda x: _materialised(net, tokens, x, adj, inp["edge_tok"], leaf, mask), coors, wn, wc, params, leaf)
    torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[1], want[1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[2], want[2], rtol=1e-4, atol=1e-4)
    assert got[3].keys() == want[3].keys()
    for name in want[3]:
        torch.testing.assert_close(got[3][name], want[3][name], rtol=1e-4, atol=1e-4, msg=name)
    if leaf is not None:
        torch.testing.assert_close(got[4], want[4], rtol=1e-4, atol=1e-4)
    return got, want


# ------------------------------------------------------------------ 1. memory: nothing of size B N^2 D
def test_training_step_on_8192_nodes_allocates_no_dense_edge_tensor():
    from egnn_pytorch_amd import EGNN_Network
    n_clusters, k = 2, 16
    coors, mask = _clusters(n_clusters, 31, k)
    torch.manual_seed(8)
    net = EGNN_Network(num_tokens=20, num_edge_tokens=6, edge_dim=8, dim=16, depth=2, num_nearest_neighbors=k, num_adj_degrees=3,
                       adj_dim=8).cuda()
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    edge_tok = torch.randint(0, 6, (1, n, n), device="cuda")
    adj = _cluster_adj(n_clusters)
    x = coors.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h, co = net(tokens, x, adj_mat=adj, edges=edge_tok, mask=mask)
    (h.sum() + co.sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert net.edge_emb.weight.grad is not None and net.adj_emb.weight.grad is not None
    assert peak < (1 << 30), f"peak {peak / 2**30:.2f} GiB above the inputs"


# ------------------------------------------------------------------ 2. equal to the materialised recipe
@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [64, 300, 1024])
def test_network_training_equals_the_materialised_recipe(n, mode, edges):
    _compare(*_setup(n, edges, mode))


@pytest.mark.parametrize("edges", ["both", "dense_deg"])
@pytest.mark.parametrize("extra", ["attn", "exact", "dropout"])
def test_network_training_equals_the_materialised_recipe_variants(extra, edges):
    from egnn_pytorch_amd import exact_arithmetic
    net, *rest = _setup(300, edges, "knn", extra)
    _compare(net, *rest, ctx=exact_arithmetic if extra == "exact" else None)


# ------------------------------------------------------------------ 3. against float64
@pytest.mark.parametrize("mode", ["knn", "dense"])
def test_embedding_gradients_match_float64(mode):
    net, tokens, coors, mask, adj, inp = _setup(64, "both", mode, seed=3)
    net64 = copy.deepcopy(net).double()
    wn = torch.randn(2, 64, 16, device="cuda", dtype=torch.float64)
    wc = torch.randn(2, 64, 3, device="cuda", dtype=torch.float64)
    got = _step(lambda x: net(tokens, x, adj_mat=adj, edges=inp["edge_tok"], mask=mask), coors, wn.float(), wc.float(),
                list(net.named_parameters()))
    want = _step(lambda x: net64(tokens, x, adj_mat=adj, edges=inp["edge_tok"], mask=mask), coors.double(), wn, wc,
                 list(net64.named_parameters()))
    for name in ("edge_emb.weight", "adj_emb.weight"):
        torch.testing.assert_close(got[3][name].double(), want[3][name], rtol=1e-4, atol=1e-4, msg=name)


# ------------------------------------------------------------------ 4. the reduction kernel
def _reduction_case(v, d, with_idx, b=2, n=150, k=7, seed=0):
    from egnn_pytorch_amd.layer import EdgeLookup
    g = torch.Generator(device="cuda").manual_seed(seed)
    kk = k if with_idx else n
    tok = torch.randint(0, v, (b, n, n), device="cuda", generator=g)
    v2 = min(v, 256)
    deg = torch.randint(0, v2, (b, n, n), device="cuda", generator=g).to(torch.uint8)
    lookup = EdgeLookup(tok=tok, tok_emb=torch.zeros(v, d, device="cuda"), deg=deg, deg_emb=torch.zeros(v2, d, device="cuda"))
    idx = torch.stack([torch.randperm(n, device="cuda", generator=g)[:k] for _ in range(b * n)]).view(b, n, k).int() if with_idx else None
    e = b * n * kk
    wide = torch.randn(e, 2 * d + 5, device="cuda", generator=g)
    rows = wide[:, 3:3 + 2 * d]                              # (strided rows: ld = 2 d + 5)
    return lookup, idx, tok, deg, rows, b, n, kk, v2


def _assert_sum_close(got, want, abs_sum):
    """fp32 sums of many terms against float64: |error| <= 1e-5 |want| + 1e-6 (sum of |terms|) -- a missing or doubled edge still
    shows (it moves an element by the size of one term)."""
    err = (got.double() - want).abs()
    bound = 1e-5 * want.abs() + 1e-6 * abs_sum + 1e-6
    assert bool((err <= bound).all()), f"max error {float(err.max())}, max excess {float((err - bound).max())}"


def _labels(lab, idx, b, n, k):
    if idx is None:
        return lab.reshape(-1)
    return torch.gather(lab, 2, idx.long()).reshape(-1)


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("d", [1, 4, 8, 16, 48])
@pytest.mark.parametrize("v", [1, 3, 256, 5000])
def test_edge_features_grad_matches_index_add(v, d, with_idx):
    from egnn_pytorch_amd import _ops
    lookup, idx, tok, deg, rows, b, n, k, v2 = _reduction_case(v, d, with_idx)
    g_tok, g_deg = _ops.edge_features_grad(lookup, idx, b, n, k, rows)
    want_tok = torch.zeros(v, d, dtype=torch.float64, device="cuda").index_add_(0, _labels(tok, idx, b, n, k), rows[:, :d].double())
    want_deg = torch.zeros(v2, d, dtype=torch.float64, device="cuda").index_add_(0, _labels(deg.long(), idx, b, n, k),
                                                                                  rows[:, d:].double())
    lt, ld = _labels(tok, idx, b, n, k), _labels(deg.long(), idx, b, n, k)
    abs_tok = torch.zeros(v, d, dtype=torch.float64, device="cuda").index_add_(0, lt, rows[:, :d].double().abs())
    abs_deg = torch.zeros(v2, d, dtype=torch.float64, device="cuda").index_add_(0, ld, rows[:, d:].double().abs())
    _assert_sum_close(g_tok, want_tok, abs_tok)
    _assert_sum_close(g_deg, want_deg, abs_deg)
    # bit-identical from call to call
    g_tok2, g_deg2 = _ops.edge_features_grad(lookup, idx, b, n, k, rows)
    assert torch.equal(g_tok, g_tok2) and torch.equal(g_deg, g_deg2)
    # chunked over graphs: the parts sum to the whole
    parts = [_ops.edge_features_grad(lookup.graphs(q, q + 1), None if idx is None else idx[q:q + 1].contiguous(), 1, n, k,
                                     rows[q * n * k:(q + 1) * n * k]) for q in range(b)]
    _assert_sum_close(parts[0][0] + parts[1][0], want_tok, abs_tok)
    _assert_sum_close(parts[0][1] + parts[1][1], want_deg, abs_deg)


@pytest.mark.parametrize("with_idx", [True, False])
def test_edge_features_grad_stores_dense_edge_rows(with_idx):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    b, n, k, d1, d2 = 2, 90, 5, 3, 4
    edges = torch.randn(b, n, n, d1, device="cuda")
    deg = torch.randint(0, 4, (b, n, n), device="cuda").to(torch.uint8)
    lookup = EdgeLookup(edges=edges, deg=deg, deg_emb=torch.zeros(4, d2, device="cuda"))
    idx = torch.stack([torch.randperm(n, device="cuda")[:k] for _ in range(b * n)]).view(b, n, k).int() if with_idx else None
    kk = k if with_idx else n
    rows = torch.randn(b * n * kk, d1 + d2, device="cuda")
    g_edges = torch.zeros(b, n, n, d1, device="cuda")
    g_tok, g_deg = _ops.edge_features_grad(lookup, idx, b, n, kk, rows, g_edges=g_edges)
    assert g_tok is None
    want = torch.zeros(b, n, n, d1, device="cuda")
    if idx is None:
        want = rows[:, :d1].reshape(b, n, n, d1)
    else:
        want.scatter_(2, idx.long()[..., None].expand(b, n, k, d1), rows[:, :d1].reshape(b, n, k, d1))
    assert torch.equal(g_edges, want)
    want_deg = torch.zeros(4, d2, dtype=torch.float64, device="cuda").index_add_(0, _labels(deg.long(), idx, b, n, kk), rows[:, d1:].double())
    torch.testing.assert_close(g_deg.double(), want_deg, rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------ 5. scale: 49 152 nodes
def test_network_training_on_49152_nodes_matches_each_cluster_alone():
    """One training step on 12 clusters (49 152 nodes) with edge tokens and 3 adjacency degrees: the materialised recipe would need
    ~309 GB in its forward.  Gradients equal the sum of the 12 per-cluster steps; the embedding gradients are bit-reproducible."""
    from egnn_pytorch_amd import EGNN_Network
    n_clusters, k = 12, 16
    coors, mask = _clusters(n_clusters, 41, k)
    torch.manual_seed(9)
    net = EGNN_Network(num_tokens=20, num_edge_tokens=6, edge_dim=8, dim=16, depth=2, num_nearest_neighbors=k, num_adj_degrees=3,
                       adj_dim=8).cuda()
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    edge_tok = torch.randint(0, 6, (1, n, n), device="cuda")           # int64: 19 GB
    wn = torch.randn(1, n, 16, device="cuda")
    wc = torch.randn(1, n, 3, device="cuda")
    adj = _cluster_adj(n_clusters)
    params = list(net.named_parameters())

    def step(s, tok):
        return _step(lambda x: net(tokens[:, s], x, adj_mat=adj[s, s], edges=tok, mask=mask[:, s]), coors[:, s], wn[:, s], wc[:, s],
                     params)

    hb, cb, gc, gp, _ = step(slice(0, n), edge_tok)
    _, _, _, gp2, _ = step(slice(0, n), edge_tok)
    assert torch.equal(gp["edge_emb.weight"], gp2["edge_emb.weight"]) and torch.equal(gp["adj_emb.weight"], gp2["adj_emb.weight"])
    del gp2
    gp_sum = None
    for cl in range(n_clusters):
        s = slice(cl * CL, (cl + 1) * CL)
        h1, c1, gc1, p1, _ = step(s, edge_tok[:, s, s].contiguous())
        torch.testing.assert_close(hb[:, s], h1, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(cb[:, s], c1, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(gc[:, s], gc1, rtol=1e-4, atol=1e-4)
        gp_sum = p1 if gp_sum is None else {name: gp_sum[name] + p1[name] for name in p1}
    assert gp.keys() == gp_sum.keys()
    assert {"adj_emb.weight", "token_emb.weight", "edge_emb.weight"} <= gp.keys()
    for name in gp:
        torch.testing.assert_close(gp[name], gp_sum[name], rtol=1e-4, atol=1e-4, msg=name)
    del edge_tok, adj
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. only the edge embedding trains
def test_frozen_network_still_trains_the_edge_embedding():
    net, tokens, coors, mask, adj, inp = _setup(300, "both", "knn", seed=4)
    got_full, want = _compare(net, tokens, coors, mask, adj, inp)
    for name, p in net.named_parameters():
        p.requires_grad_(name == "edge_emb.weight")
    net.edge_emb.weight.grad = None
    h, co = net(tokens, coors, adj_mat=adj, edges=inp["edge_tok"], mask=mask)
    wn = torch.randn(2, 300, 16, device="cuda")
    wc = torch.randn(2, 300, 3, device="cuda")
    ((h * wn).sum() + (co * wc).sum()).backward()
    g = net.edge_emb.weight.grad
    assert g is not None and g.abs().sum() > 0
    net.edge_emb.weight.grad = None
    torch.manual_seed(0)
    want = _step(lambda x: _materialised(net, tokens, x, adj, inp["edge_tok"], None, mask), coors, wn, wc,
                 [("edge_emb.weight", net.edge_emb.weight)])
    torch.testing.assert_close(g, want[3]["edge_emb.weight"], rtol=1e-4, atol=1e-4)
