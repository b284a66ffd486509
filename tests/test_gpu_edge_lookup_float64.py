"""Float64 layers and networks on edge look-up tables: a `.double()` EGNN / EGNN_Network reads the embedding rows of the K selected
pairs through egnn_edge_features_gather_f64 and reduces their gradients over the same pairs through egnn_edge_features_grad_f64
(csrc/segment_sum.hip: the _f32 kernels instantiated for double) -- in inference, in training and under create_graph=True.  No
(B,N,N,D) float tensor is built, except the gradient of dense float edges the caller passed in.  Checked: the two kernels on their
own, a layer against the same layer on the materialised float64 tensor, networks against the materialised float64 recipe (first and
second order), and the memory of a step at 4 096 nodes and of inference at 16 384."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = 4096
F64 = torch.float64


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
    """Float64 coordinates (1, n_clusters * CL, 3): unit-normal clusters 40 apart on a 3 x 2 x 2 grid; a ragged mask that leaves every
    cluster >= 3 K real nodes (the first one whole)."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in range(3) for y in range(2) for z in range(2)], dtype=np.float64)[:n_clusters] * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None]
    real = CL - rng.integers(0, CL - 3 * k, size=n_clusters)
    real[0] = CL
    mask = np.concatenate([np.arange(CL) < real[c] for c in range(n_clusters)])[None]
    return torch.from_numpy(coors).cuda(), torch.from_numpy(mask).cuda()


def _materialised(net, tokens, coors, adj, edge_tok=None, dense_edges=None, mask=None):
    """EGNN_Network's forward with the (B,N,N,edge_dim+adj_dim) edge tensor built densely in torch (float64 embeddings) and handed to
    each EGNN layer."""
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


def _big_net(k=16):
    from egnn_pytorch_amd import EGNN_Network
    return EGNN_Network(num_tokens=20, num_edge_tokens=6, edge_dim=8, dim=16, depth=2, num_nearest_neighbors=k, num_adj_degrees=3,
                        adj_dim=8).cuda().double()


def _neighbours(b, n, k, gen):
    """(B,N,K) int32: K distinct neighbours per node"""
    return torch.stack([torch.randperm(n, device="cuda", generator=gen)[:k] for _ in range(b * n)]).view(b, n, k).int()


# ------------------------------------------------------------------ 2. the gather kernel: a copy
GATHER = {                                                  # (tokens?, dense float edges?, degrees?)
    "tok_deg": (True, False, True),
    "tok": (True, False, False),
    "deg": (False, False, True),
    "dense_deg": (False, True, True),
}


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("kind", list(GATHER))
def test_gather_equals_indexing_the_float64_tables(kind, with_idx):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    has_tok, has_dense, has_deg = GATHER[kind]
    b, n, v, d1, d2 = 2, 5, 4, 3, 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    kw, cols = {}, []
    if has_tok:
        kw.update(tok=torch.randint(0, v, (b, n, n), device="cuda", generator=gen),
                  tok_emb=torch.randn(v, d1, device="cuda", dtype=F64, generator=gen))
        cols.append(kw["tok_emb"][kw["tok"]])
    if has_dense:
        kw.update(edges=torch.randn(b, n, n, d1, device="cuda", dtype=F64, generator=gen))
        cols.append(kw["edges"])
    if has_deg:
        kw.update(deg=torch.randint(0, 3, (b, n, n), device="cuda", generator=gen).to(torch.uint8),
                  deg_emb=torch.randn(3, d2, device="cuda", dtype=F64, generator=gen))
        cols.append(kw["deg_emb"][kw["deg"].long()])
    lookup = EdgeLookup(dtype=F64, **kw)
    full = torch.cat(cols, dim=-1)                          # (B,N,N,D): tiny here
    idx = _neighbours(b, n, 3, gen) if with_idx else None
    k = 3 if with_idx else n
    got = _ops.edge_features_gather(lookup, idx, b, n, k)
    want = full if idx is None else torch.gather(full, 2, idx.long()[..., None].expand(b, n, k, full.shape[-1]))
    assert got.dtype == F64 and tuple(got.shape) == (b, n, k, lookup.width)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 3. the gradient reduction kernel
def _reduction_case(v, d, with_idx, b=2, n=150, k=7, seed=0, dtype=F64):
    from egnn_pytorch_amd.layer import EdgeLookup
    g = torch.Generator(device="cuda").manual_seed(seed)
    kk = k if with_idx else n
    tok = torch.randint(0, v, (b, n, n), device="cuda", generator=g)
    v2 = min(v, 256)
    deg = torch.randint(0, v2, (b, n, n), device="cuda", generator=g).to(torch.uint8)
    lookup = EdgeLookup(tok=tok, tok_emb=torch.zeros(v, d, device="cuda", dtype=dtype), deg=deg,
                        deg_emb=torch.zeros(v2, d, device="cuda", dtype=dtype), dtype=dtype)
    idx = _neighbours(b, n, k, g) if with_idx else None
    e = b * n * kk
    wide = torch.randn(e, 2 * d + 5, device="cuda", dtype=F64, generator=g)
    rows = wide[:, 3:3 + 2 * d]                              # (strided rows: ld = 2 d + 5)
    return lookup, idx, tok, deg, rows, b, n, kk, v2


def _labels(lab, idx):
    return lab.reshape(-1) if idx is None else torch.gather(lab, 2, idx.long()).reshape(-1)


def _index_add(v, lab, terms, exact=True):
    """(V, d) float64 index_add_ of `terms` (E, d) on the labels `lab` (E,), labels outside [0, V) dropped.  exact: the terms are
    split into three pieces on grids q, q 2^-30, q 2^-60 (q a power of two with |terms| < 2^30 q) and a residue below q 2^-61; a piece
    is a multiple of its grid below 2^30 times it, so any sum of fewer than 2^16 of them stays below 2^46 grid steps and is exact
    in float64 whatever order the device adds in.  What is left is the residue's own sum (below 1e-30 absolute here) and the three
    additions that join the pieces: the reference is within 3 u of the exact sum."""
    keep = (lab >= 0) & (lab < v)
    lab, terms = lab[keep], terms[keep]
    add = lambda t: torch.zeros(v, terms.shape[1], dtype=F64, device=terms.device).index_add_(0, lab, t)      # noqa: E731
    if not exact or lab.numel() == 0:
        return add(terms)
    assert lab.numel() < 1 << 16
    q = 2.0 ** (math.frexp(float(terms.abs().max()))[1] - 30)
    parts, rest = [], terms
    for _ in range(3):
        piece = torch.round(rest / q) * q
        parts.append(add(piece))
        rest = rest - piece
        q *= 2.0 ** -30
    return parts[0] + (parts[1] + (parts[2] + add(rest)))


def _assert_sum_close(got, v, lab, terms):
    want, abs_sum = _index_add(v, lab, terms), _index_add(v, lab, terms.abs(), exact=False)
    err = (got - want).abs()
    bound = 1e-13 * abs_sum + 1e-300
    worst = float((err / (abs_sum + 1e-300)).max())
    print(f"max |err| / sum|terms| = {worst:.3e}")
    assert got.dtype == F64
    assert bool((err <= bound).all()), f"max |err| / sum|terms| = {worst:.3e}"


# (V, d): every branch of the kernel for double -- a wave's LDS table holds 1024 doubles, P = 64 // d lane groups of d lanes,
# Vb = 1024 // (P d) labels per block
BRANCHES = [
    (3, 16),            # d divides 64: P = 4 lane groups, all 64 lanes busy, one label block
    (3, 3),             # d = 3: P = 21, lane 63 idle
    (3, 80),            # d > 64: one lane group, each lane walks columns c and c + 64; Vb = 12
    (300, 80),          # ... in 25 label blocks
    (256, 8),           # P = 8, Vb = 16: 16 label blocks for each of the two tables (the degree table has 256 labels as well)
    (5000, 16),         # 313 label blocks, most labels with no edge at all when K = 7
    (1, 4),             # V = 1: every edge lands on the one row
]


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("v,d", BRANCHES)
def test_edge_features_grad_f64_matches_index_add(v, d, with_idx):
    """|err| <= 1e-13 sum|terms| + 1e-300 per element, against a float64 index_add_ on the gathered labels.

    Where the bound comes from (u = 2^-53 = 1.11e-16; a sum of terms computed by any chain of L additions is within L u sum|terms|
    of the exact sum, to first order).  The kernel: a workgroup takes at most 2048 edges, a wave a quarter (512), a lane group every
    P-th of those; the 4 P tables are added in order, then the G <= 22 partials (E = 2 100 with the neighbour list, 45 000 dense):
    L <= 512 / P + 4 P + G, largest at P = 1 (d = 80): 538.  The reference (`_index_add`) sums exactly representable pieces, so it
    adds 3 u whatever the device's order.  Together at most 541 u = 6.0e-14 of sum|terms|, below 1e-13.  A missing or doubled edge
    moves an element by a whole term, about 1e13 times the bound."""
    from egnn_pytorch_amd import _ops
    lookup, idx, tok, deg, rows, b, n, k, v2 = _reduction_case(v, d, with_idx)
    g_tok, g_deg = _ops.edge_features_grad(lookup, idx, b, n, k, rows)
    lt, ld = _labels(tok, idx), _labels(deg.long(), idx)
    _assert_sum_close(g_tok, v, lt, rows[:, :d])
    _assert_sum_close(g_deg, v2, ld, rows[:, d:])
    # bit-identical from call to call
    g_tok2, g_deg2 = _ops.edge_features_grad(lookup, idx, b, n, k, rows)
    assert torch.equal(g_tok, g_tok2) and torch.equal(g_deg, g_deg2)
    # chunked over graphs (what the backward does): the parts sum to the whole
    parts = [_ops.edge_features_grad(lookup.graphs(q, q + 1), None if idx is None else idx[q:q + 1].contiguous(), 1, n, k,
                                     rows[q * n * k:(q + 1) * n * k]) for q in range(b)]
    _assert_sum_close(parts[0][0] + parts[1][0], v, lt, rows[:, :d])
    _assert_sum_close(parts[0][1] + parts[1][1], v2, ld, rows[:, d:])


def test_edge_features_grad_f64_ignores_labels_outside_the_tables():
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    b, n, k, v, v2, d = 2, 150, 7, 5, 4, 8
    gen = torch.Generator(device="cuda").manual_seed(2)
    tok = torch.randint(-2, v + 3, (b, n, n), device="cuda", generator=gen)                 # -2 .. v + 2
    deg = torch.randint(0, 200, (b, n, n), device="cuda", generator=gen).to(torch.uint8)    # mostly >= v2
    lookup = EdgeLookup(tok=tok, tok_emb=torch.zeros(v, d, device="cuda", dtype=F64), deg=deg,
                        deg_emb=torch.zeros(v2, d, device="cuda", dtype=F64), dtype=F64)
    idx = _neighbours(b, n, k, gen)
    rows = torch.randn(b * n * k, 2 * d, device="cuda", dtype=F64, generator=gen)
    g_tok, g_deg = _ops.edge_features_grad(lookup, idx, b, n, k, rows)
    lt, ld = _labels(tok, idx), _labels(deg.long(), idx)
    assert bool(((lt < 0) | (lt >= v)).any()) and bool((ld >= v2).any())
    _assert_sum_close(g_tok, v, lt, rows[:, :d])
    _assert_sum_close(g_deg, v2, ld, rows[:, d:])


@pytest.mark.parametrize("with_idx", [True, False])
def test_edge_features_grad_f64_stores_dense_edge_rows(with_idx):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    b, n, k, d1, d2 = 2, 90, 5, 3, 4
    gen = torch.Generator(device="cuda").manual_seed(3)
    edges = torch.randn(b, n, n, d1, device="cuda", dtype=F64, generator=gen)
    deg = torch.randint(0, 4, (b, n, n), device="cuda", generator=gen).to(torch.uint8)
    lookup = EdgeLookup(edges=edges, deg=deg, deg_emb=torch.zeros(4, d2, device="cuda", dtype=F64), dtype=F64)
    idx = _neighbours(b, n, k, gen) if with_idx else None
    kk = k if with_idx else n
    rows = torch.randn(b * n * kk, d1 + d2, device="cuda", dtype=F64, generator=gen)
    g_edges = torch.zeros(b, n, n, d1, device="cuda", dtype=F64)
    g_tok, g_deg = _ops.edge_features_grad(lookup, idx, b, n, kk, rows, g_edges=g_edges)
    assert g_tok is None
    want = torch.zeros(b, n, n, d1, device="cuda", dtype=F64)
    if idx is None:
        want = rows[:, :d1].reshape(b, n, n, d1)
    else:
        want.scatter_(2, idx.long()[..., None].expand(b, n, k, d1), rows[:, :d1].reshape(b, n, k, d1))
    assert torch.equal(g_edges, want)
    _assert_sum_close(g_deg, 4, _labels(deg.long(), idx), rows[:, d1:])


def test_edge_features_grad_rejects_mixed_dtypes():
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    lookup32, idx, _, _, rows, b, n, k, _ = _reduction_case(3, 4, True, dtype=torch.float32)
    with pytest.raises(TypeError, match="matching the tables"):
        _ops.edge_features_grad(lookup32, idx, b, n, k, rows)                               # fp32 tables, float64 g
    with pytest.raises(TypeError, match="matching the tables"):
        _ops.edge_features_grad(lookup32.to(F64), idx, b, n, k, rows.float())               # float64 tables, fp32 g
    mixed = EdgeLookup(tok=lookup32.tok, tok_emb=lookup32.tok_emb, deg=lookup32.deg, deg_emb=lookup32.deg_emb)
    mixed.deg_emb = mixed.deg_emb.double()
    with pytest.raises(TypeError, match="all be float32 or all float64"):
        _ops.edge_features_gather(mixed, idx, b, n, k)


# ------------------------------------------------------------------ 4. a float64 layer given the tables
def _layer_case(edge_dim, d1, seed=5):
    from egnn_pytorch_amd import EGNN
    from egnn_pytorch_amd.layer import EdgeLookup
    torch.manual_seed(seed)
    b, n, d2 = 2, 12, edge_dim - d1
    layer = EGNN(dim=8, edge_dim=edge_dim, m_dim=16, num_nearest_neighbors=4, norm_coors=True).cuda().double()
    feats = torch.randn(b, n, 8, device="cuda", dtype=F64)
    coors = torch.randn(b, n, 3, device="cuda", dtype=F64)
    mask = torch.ones(b, n, dtype=torch.bool, device="cuda")
    mask[1, 9:] = False
    tok = torch.randint(0, 4, (b, n, n), device="cuda")
    deg = torch.randint(0, 3, (b, n, n), device="cuda").to(torch.uint8)
    tok_emb = torch.randn(4, d1, device="cuda", dtype=F64, requires_grad=True)
    deg_emb = torch.randn(3, d2, device="cuda", dtype=F64, requires_grad=True)
    lookup = lambda: EdgeLookup(tok=tok, tok_emb=tok_emb, deg=deg, deg_emb=deg_emb, dtype=F64)                  # noqa: E731
    dense = lambda: torch.cat((tok_emb[tok], deg_emb[deg.long()]), dim=-1)                                       # noqa: E731
    return layer, feats, coors, mask, tok_emb, deg_emb, lookup, dense


def test_float64_layer_on_lookup_equals_the_materialised_tensor():
    """The gathered operands are the tables' own bits and the same kernel (egnn_edge_exact_f64) consumes them -- its two edge-read
    modes differ in the address of a pair's features only -- so the outputs are equal bit for bit."""
    layer, feats, coors, mask, _, _, lookup, dense = _layer_case(edge_dim=5, d1=3)
    with torch.no_grad():
        got = layer(feats, coors, edges=lookup(), mask=mask)
        want = layer(feats, coors, edges=dense(), mask=mask)
    assert got[0].dtype == F64 and got[1].dtype == F64
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a look-up built with the default dtype over float64 tensors and handed to a float64 layer: `EdgeLookup.to` converts from the
    # caller's tensors, not from its fp32 copies, so nothing is rounded -- the same bits again
    from egnn_pytorch_amd.layer import EdgeLookup
    lk = lookup()
    lk32 = EdgeLookup(tok=lk.tok, tok_emb=lk.live[1], deg=lk.deg, deg_emb=lk.live[2])
    assert lk32.dtype == torch.float32 and lk32.tok_emb.dtype == torch.float32
    with torch.no_grad():
        got32 = layer(feats, coors, edges=lk32, mask=mask)
    assert torch.equal(got32[0], want[0]) and torch.equal(got32[1], want[1])
    assert lk32.to(F64) is lk32.to(F64) and lk32.to(torch.float32) is lk32


@pytest.mark.parametrize("edge_dim,d1", [(5, 3), (40, 24)])
def test_float64_layer_on_lookup_trains_the_tables(edge_dim, d1):
    """d/d feats, coors, both tables and every parameter against the same layer on the materialised tensor, at 1e-10 (float64, fixed
    summation orders that differ: the tables' gradients are reductions over the K selected pairs here, over all N^2 there).
    edge_dim = 5: the float64 kernels' own backward (`_backward_exact`); edge_dim = 40: 41 per-edge scalars, beyond what it carries,
    so the ATen recompute backward (`_backward_recompute`)."""
    layer, feats, coors, mask, tok_emb, deg_emb, lookup, dense = _layer_case(edge_dim, d1)
    wn, wc = torch.randn_like(feats), torch.randn_like(coors)
    res = []
    for edges in (lookup, dense):
        f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        for p in list(layer.parameters()) + [tok_emb, deg_emb]:
            p.grad = None
        h, co = layer(f, c, edges=edges(), mask=mask)
        ((h * wn).sum() + (co * wc).sum()).backward()
        res.append([h.detach(), co.detach(), f.grad, c.grad, tok_emb.grad.clone(), deg_emb.grad.clone()] +
                   [p.grad.clone() for p in layer.parameters()])
    assert res[0][4].dtype == F64 and float(res[0][4].abs().sum()) > 0 and float(res[0][5].abs().sum()) > 0
    for got, want in zip(*res):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)


# ------------------------------------------------------------------ 5. networks against the materialised float64 recipe
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
    net = EGNN_Network(**kw).cuda().double()
    if extra == "dropout":
        net.train()
    tokens = torch.randint(0, 11, (2, n), device="cuda")
    coors = torch.randn(2, n, 3, device="cuda", dtype=F64)
    mask = torch.ones(2, n, dtype=torch.bool, device="cuda")
    mask[1, n - n // 5:] = False
    adj = _chain_adj(n, seed + n)
    inp = dict(edge_tok=None, dense_edges=None)
    if "num_edge_tokens" in EDGES[edges]:
        inp["edge_tok"] = torch.randint(0, 6, (2, n, n), device="cuda")
    if edges == "dense_deg":
        inp["dense_edges"] = torch.randn(2, n, n, 3, device="cuda", dtype=F64)
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


def _compare(net, tokens, coors, mask, adj, inp, tol=1e-10):
    n = tokens.shape[1]
    wn = torch.randn(2, n, 16, device="cuda", dtype=F64)
    wc = torch.randn(2, n, 3, device="cuda", dtype=F64)
    params = list(net.named_parameters())
    de = inp["dense_edges"]
    leaf = de.clone().requires_grad_(True) if de is not None else None
    got = _step(lambda x: net(tokens, x, adj_mat=adj, edges=inp["edge_tok"] if leaf is None else leaf, mask=mask), coors, wn, wc,
                params, leaf)
    want = _step(lambda x: _materialised(net, tokens, x, adj, inp["edge_tok"], leaf, mask), coors, wn, wc, params, leaf)
    assert got[0].dtype == F64
    torch.testing.assert_close(got[0], want[0], rtol=tol, atol=tol)
    torch.testing.assert_close(got[1], want[1], rtol=tol, atol=tol)
    torch.testing.assert_close(got[2], want[2], rtol=tol, atol=tol)
    assert got[3].keys() == want[3].keys()
    for name in ("edge_emb.weight", "adj_emb.weight"):
        if getattr(net, name.split(".")[0]) is not None:
            assert name in got[3] and got[3][name].dtype == F64 and float(got[3][name].abs().sum()) > 0, name
    for name in want[3]:
        torch.testing.assert_close(got[3][name], want[3][name], rtol=tol, atol=tol, msg=name)
    if leaf is not None:
        assert got[4].dtype == F64
        torch.testing.assert_close(got[4], want[4], rtol=tol, atol=tol)


@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("mode", list(MODES))
def test_float64_network_training_equals_the_materialised_recipe(mode, edges):
    """Outputs, d/d coors, every parameter gradient and the dense-edge gradient at rtol = atol = 1e-10: float64 arithmetic with
    different but fixed summation orders over chains of O(1e3) operations gives about 1e-13; the bound leaves three orders of margin
    and stays six below any real defect."""
    _compare(*_setup(64, edges, mode))


@pytest.mark.parametrize("extra", ["dropout", "attn"])
def test_float64_network_training_equals_the_materialised_recipe_variants(extra):
    """training-mode dropout (the same seed on both sides: the same hash masks) / a global attention block before every layer"""
    _compare(*_setup(64, "both", "knn", extra))


# ------------------------------------------------------------------ 6. second order
def test_float64_force_matching_gradient_equals_the_materialised_recipe():
    """F = -d(h.sum())/dx under create_graph=True, loss = |F|^2, differentiated with respect to every parameter -- the two embedding
    tables among them -- against the materialised float64 recipe at 1e-9."""
    net, tokens, coors, mask, adj, inp = _setup(32, "both", "knn", seed=6)
    params = [p for p in net.parameters()]
    names = [name for name, _ in net.named_parameters()]

    def force_grads(fn):
        x = coors.clone().requires_grad_(True)
        h, _ = fn(x)
        force = -torch.autograd.grad(h.sum(), x, create_graph=True)[0]
        loss = force.pow(2).sum()
        return loss.detach(), torch.autograd.grad(loss, params, allow_unused=True)

    loss_g, got = force_grads(lambda x: net(tokens, x, adj_mat=adj, edges=inp["edge_tok"], mask=mask))
    loss_w, want = force_grads(lambda x: _materialised(net, tokens, x, adj, inp["edge_tok"], None, mask))
    torch.testing.assert_close(loss_g, loss_w, rtol=1e-9, atol=1e-9)
    assert float(loss_w) > 0
    for name, g, w in zip(names, got, want):
        if name in ("edge_emb.weight", "adj_emb.weight"):
            assert g is not None and w is not None and float(w.abs().sum()) > 0, name
        assert (g is None) == (w is None), name
        if w is not None:
            torch.testing.assert_close(g, w, rtol=1e-9, atol=1e-9, msg=name)


# ------------------------------------------------------------------ 7. memory of a training step
def test_float64_training_step_on_4096_nodes_allocates_no_dense_edge_tensor():
    """One forward + backward of a float64 network on one graph of 4 096 nodes: the peak above the inputs stays below HALF the bytes
    of the (1, N, N, 16) float64 edge tensor (2 GiB), which the materialised recipe allocates several times over.  What is left: the
    N^2 byte maps of the degree expansion (16 MiB), the (E, 16) float64 features (8 MiB), the exact backward's (H, E) tables."""
    k = 16
    coors, mask = _clusters(1, 31, k)
    torch.manual_seed(8)
    net = _big_net(k)
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    edge_tok = torch.randint(0, 6, (1, n, n), device="cuda")
    adj = _cluster_adj(1)
    x = coors.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h, co = net(tokens, x, adj_mat=adj, edges=edge_tok, mask=mask)
    (h.sum() + co.sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense_bytes = n * n * 16 * 8
    print(f"peak {peak / 2**20:.1f} MiB above the inputs; the dense tensor {dense_bytes / 2**20:.0f} MiB")
    assert h.dtype == F64 and bool(torch.isfinite(h).all()) and bool(torch.isfinite(co).all())
    for w in (net.edge_emb.weight, net.adj_emb.weight):
        assert w.grad is not None and w.grad.dtype == F64 and bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().sum()) > 0
    assert peak < dense_bytes // 2, f"peak {peak / 2**30:.2f} GiB above the inputs"


# ------------------------------------------------------------------ 8. a large graph, inference
def test_float64_inference_on_16384_nodes_matches_the_first_cluster_alone():
    """Four clusters 40 apart with a block-diagonal adjacency: no neighbour list crosses clusters, so the first cluster's outputs equal
    those of that cluster run alone (1e-10).  The dense float64 tensor would be 32 GiB; the peak above the inputs stays below 2 GiB."""
    n_clusters, k = 4, 16
    coors, mask = _clusters(n_clusters, 41, k)
    torch.manual_seed(9)
    net = _big_net(k)
    n = coors.shape[1]
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    edge_tok = torch.randint(0, 6, (1, n, n), device="cuda")           # int64: 2 GiB
    adj = _cluster_adj(n_clusters)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        h, co = net(tokens, coors, adj_mat=adj, edges=edge_tok, mask=mask)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 2**20:.1f} MiB above the inputs")
    assert h.dtype == F64 and bool(torch.isfinite(h).all()) and bool(torch.isfinite(co).all())
    assert peak < (2 << 30), f"peak {peak / 2**30:.2f} GiB above the inputs"
    s = slice(0, CL)
    with torch.no_grad():
        h1, c1 = net(tokens[:, s], coors[:, s], adj_mat=adj[s, s], edges=edge_tok[:, s, s].contiguous(), mask=mask[:, s])
    torch.testing.assert_close(h[:, s], h1, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(co[:, s], c1, rtol=1e-10, atol=1e-10)
    del edge_tok, adj
    torch.cuda.empty_cache()
