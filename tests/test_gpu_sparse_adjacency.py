"""`SparseAdjacency` on the MI355X: a call with the CSR object returns the same bits as the same call with its `to_dense()` -- neighbour
lists (egnn_knn_select_csr_f32 / _f64 against the pinned dense-adjacency kernels), layer and network outputs, every gradient.  The dense
call is what the other test files pin to the reference; the one graph too large for a dense image is checked against the oracle on
sampled rows, and a 262 144-node graph of clusters against each cluster run alone with its dense adjacency."""
import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O

pytestmark = pytest.mark.gpu


def _SA():
    from egnn_pytorch_amd import SparseAdjacency
    return SparseAdjacency


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _adjacency(g, n, k, diag, gen):
    """(g, n, n) bool on the device, directed: rows of about k entries (shorter and longer than K - 1), row 2 full, row 3 empty, the
    last row a single entry; the diagonal all set or all clear."""
    adj = torch.rand(g, n, n, device="cuda", generator=gen) < min(1.0, k / max(n, 1))
    if n > 4:
        adj[:, 2] = True
        adj[:, 3] = False
        adj[:, n - 1] = False
        adj[:, n - 1, 0] = True
    eye = torch.eye(n, dtype=torch.bool, device="cuda")
    return (adj | eye) if diag else (adj & ~eye)


# ------------------------------------------------------------------ 1. selection: the CSR kernel against the dense-adjacency entry
@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("dtype,cdim", [(torch.float32, 3), (torch.float32, 2), (torch.float32, 12), (torch.float64, 3)])
@pytest.mark.parametrize("b,n,k", [(1, 1, 1), (2, 70, 8), (3, 257, 33)])
def test_csr_selection_equals_the_dense_adjacency_selection(b, n, k, dtype, cdim, batched):
    from egnn_pytorch_amd import _ops
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * cdim + batched)
    coors = torch.randn(b, n, cdim, device="cuda", generator=gen, dtype=dtype)
    # duplicated coordinates: every odd node sits exactly on the even node before it -- for an odd row i the node i - 1 is at distance 0,
    # adjacent or not: where it is not, it ties with the adjacent nodes at rank 0 and wins by its lower index
    dup = coors.clone()
    dup[:, 1::2] = dup[:, 0:2 * (n // 2):2]
    scattered = torch.rand(b, n, device="cuda", generator=gen) < 0.7
    scattered[-1] = False                                            # an all-masked graph
    for diag in (False, True):
        adj = _adjacency(b if batched else 1, n, k, diag, gen)
        if not batched:
            adj = adj[0]
        sa = _SA().from_dense(adj)
        assert sa.shared != batched and tuple(sa.shape) == tuple(adj.shape)
        if n > 4:
            lens = sa.row_lengths()
            assert int(lens.min()) == int(diag) and int(lens.max()) >= n - 1 and bool((lens < k - 1).any()) and bool((lens > k - 1).any())
            odd = torch.arange(1, n, 2, device="cuda")
            a2 = adj if adj.dim() == 2 else adj[0]
            assert bool((~a2[odd, odd - 1]).any())                   # non-adjacent lower-index duplicates exist
        for c in (coors, dup):
            for mask in (None, scattered):
                ref_idx, ref_rank = _ops.knn_select(c, mask, adj, k)
                idx, rank = _ops.knn_select(c, mask, sa, k)
                assert _same(idx, ref_idx) and _same(rank, ref_rank), (diag, c is dup, mask is not None)
    # a batched object sliced by graphs: absolute offsets into the shared column array
    if batched and b > 1:
        part = sa.graphs(1, b)
        ref = _ops.knn_select(coors[1:], None, adj[1:], k)
        got = _ops.knn_select(coors[1:], None, part, k)
        assert _same(got[0], ref[0]) and _same(got[1], ref[1])


def test_csr_selection_k_equal_n_and_empty_adjacency():
    from egnn_pytorch_amd import _ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    coors = torch.randn(2, 33, 3, device="cuda", generator=gen)
    mask = torch.rand(2, 33, device="cuda", generator=gen) < 0.8
    for adj in (torch.zeros(33, 33, dtype=torch.bool, device="cuda"), _adjacency(2, 33, 5, False, gen)):
        sa = _SA().from_dense(adj)
        for k in (1, 33):
            ref = _ops.knn_select(coors, mask, adj, k)
            got = _ops.knn_select(coors, mask, sa, k)
            assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    with pytest.raises(RuntimeError, match="out of range"):
        _ops.knn_select(coors, mask, sa, 34)
    with pytest.raises(ValueError):
        _ops.knn_select(coors[:, :32], None, sa, 4)


def test_csr_selection_on_70000_nodes_sampled_rows():
    """No dense image: the oracle's ranking and stable top-k on sampled rows of one 70 000-node graph with a random directed adjacency
    of about six bonds per node, diagonal set."""
    from egnn_pytorch_amd import _ops
    n, k = 70000, 32
    rng = np.random.default_rng(n)
    coors = rng.standard_normal((1, n, 3)).astype(np.float32)
    mask = (np.arange(n) < n - 1234)[None, :]
    src = np.concatenate([np.repeat(np.arange(n), 3), rng.integers(0, n, 3 * n), np.arange(n)])
    dst = np.concatenate([rng.integers(0, n, 3 * n), np.repeat(np.arange(n), 3), np.arange(n)])
    sa = _SA().from_edge_index(torch.from_numpy(np.stack([src, dst])), n).to("cuda")
    rows = np.sort(np.concatenate([rng.choice(n, 250, replace=False), [0, n - 1, n - 1234, n - 1235, 5, 6]]))
    rp, col = sa.rowptr.cpu().numpy()[0], sa.col.cpu().numpy()
    adj_rows = np.zeros((rows.size, n), dtype=bool)
    for r, i in enumerate(rows):
        adj_rows[r, col[rp[i]:rp[i + 1]]] = True
    c = coors[0]
    dist = O.inner_sum((c[rows, None] - c[None]) ** 2)
    ranking = dist.copy()
    ranking[~(mask[0][rows, None] & mask[0][None, :])] = np.float32(O.RANK_MASKED)
    diag = rows[:, None] == np.arange(n)[None, :]
    ranking[diag] = np.float32(O.RANK_SELF)
    ranking[adj_rows & ~diag] = np.float32(O.RANK_ADJ)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    cd, md = torch.from_numpy(coors).cuda(), torch.from_numpy(mask).cuda()
    idx, rank = _ops.knn_select(cd, md, sa, k)
    idx2, rank2 = _ops.knn_select(cd, md, sa, k)
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx.cpu().numpy()[0, rows])
    np.testing.assert_array_equal(ref_val.view(np.uint32), rank.cpu().numpy()[0, rows].view(np.uint32))
    assert _same(idx, idx2) and _same(rank, rank2)


# ------------------------------------------------------------------ 2. layers: sparse call against dense call, outputs and gradients
def _layer_run(layer, feats, coors, mask, adj, mode, second_order=False):
    from egnn_pytorch_amd import exact_arithmetic
    import contextlib
    layer.zero_grad()
    f = feats.clone().requires_grad_(True)
    c = coors.clone().requires_grad_(True)
    gen = torch.Generator(device="cuda").manual_seed(77)
    with exact_arithmetic() if mode == "exact" else contextlib.nullcontext():
        node, co = layer(f, c, mask=mask, adj_mat=adj)
        loss = (node * torch.randn(node.shape, device="cuda", generator=gen, dtype=node.dtype)).sum() + \
               (co * torch.randn(co.shape, device="cuda", generator=gen, dtype=co.dtype)).sum()
        params = [p for p in layer.parameters()]
        if second_order:
            g1 = torch.autograd.grad(loss, [f, c], create_graph=True)
            (g1[0].square().sum() + g1[1].square().sum()).backward()
            first = [g.detach() for g in g1]
        else:
            loss.backward()
            first = []
    grads = [f.grad, c.grad] + [p.grad for p in params if p.grad is not None]
    return [node.detach(), co.detach()] + first + [g.clone() for g in grads]


@pytest.mark.parametrize("mode", ["fast", "exact", "float64"])
@pytest.mark.parametrize("kw", [dict(only_sparse_neighbors=True), dict(num_nearest_neighbors=6),
                                dict(num_nearest_neighbors=9, only_sparse_neighbors=True, norm_coors=True, soft_edges=True)],
                         ids=["sparse_only", "knn_with_adj", "both"])
def test_layer_sparse_call_equals_dense_call(kw, mode):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(3)
    dtype = torch.float64 if mode == "float64" else torch.float32
    b, n, dim = 3, 70, 16
    layer = EGNN(dim=dim, **kw).cuda().to(dtype)
    gen = torch.Generator(device="cuda").manual_seed(9)
    feats = torch.randn(b, n, dim, device="cuda", generator=gen, dtype=dtype)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen, dtype=dtype)
    mask = torch.rand(b, n, device="cuda", generator=gen) < 0.85
    for batched in (False, True):
        adj = _adjacency(b if batched else 1, n, 4, True, gen)
        adj[:, 2] = False                                            # (no full row: K stays well below N)
        adj = adj if batched else adj[0]
        sa = _SA().from_dense(adj)
        dense = _layer_run(layer, feats, coors, mask, adj, mode)
        sparse = _layer_run(layer, feats, coors, mask, sa, mode)
        assert len(dense) == len(sparse) > 4
        for x, y in zip(dense, sparse):
            assert _same(x, y)
        assert all(torch.isfinite(x).all() for x in sparse)
        with torch.no_grad():                                        # inference: the dense call takes the one-call C forward in fp32
            for x, y in zip(layer(feats, coors, mask=mask, adj_mat=adj), layer(feats, coors, mask=mask, adj_mat=sa)):
                assert _same(x, y)


def _second_order_layer():
    """dense and sparse create_graph=True runs of one sparse-neighbour layer: (names, dense tensors, sparse tensors)"""
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(4)
    b, n, dim = 2, 40, 8
    layer = EGNN(dim=dim, only_sparse_neighbors=True).cuda()
    gen = torch.Generator(device="cuda").manual_seed(10)
    feats = torch.randn(b, n, dim, device="cuda", generator=gen)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen)
    adj = _adjacency(b, n, 3, False, gen)
    adj[:, 2] = False
    dense = _layer_run(layer, feats, coors, None, adj, "fast", second_order=True)
    sparse = _layer_run(layer, feats, coors, None, _SA().from_dense(adj), "fast", second_order=True)
    names = ["node", "coors", "d/d feats", "d/d coors", "feats.grad", "coors.grad"]
    return names + [f"param {i}" for i in range(len(dense) - len(names))], dense, sparse


def _second_order_network():
    """the same through EGNN_Network(num_adj_degrees=3, adj_dim=4): the second backward gathers adj_emb's rows for the selected pairs
    from the label CSR (autograd.py::_lookup_rows) -- a force-matching step, d/d parameters of |d energy / d coors|^2"""
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(7)
    b, n, dim = 2, 30, 8
    net = EGNN_Network(depth=2, dim=dim, num_tokens=5, num_adj_degrees=3, adj_dim=4, only_sparse_neighbors=True).cuda()
    gen = torch.Generator(device="cuda").manual_seed(13)
    tokens = torch.randint(0, 5, (b, n), device="cuda", generator=gen)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen)
    adj = _adjacency(b, n, 2, False, gen)
    adj[:, 2] = False
    named = [name for name, _ in net.named_parameters()]

    def run(a):
        net.zero_grad()
        c = coors.clone().requires_grad_(True)
        h, x = net(tokens, c, adj_mat=a)
        force = torch.autograd.grad(h.square().sum() + x.sum(), c, create_graph=True)[0]
        force.square().sum().backward()
        return [h.detach(), x.detach(), force.detach(), c.grad] + [p.grad.clone() for p in net.parameters() if p.grad is not None], \
               [name for name, p in net.named_parameters() if p.grad is not None]

    (dense, got), (sparse, _) = run(adj), run(_SA().from_dense(adj))
    assert "adj_emb.weight" in got and set(got) <= set(named)
    return ["h", "x", "force", "coors.grad"] + got, dense, sparse


_SECOND_ORDER = {"layer": _second_order_layer, "network": _second_order_network}


@pytest.mark.parametrize("case", sorted(_SECOND_ORDER))
def test_second_order_sparse_call_equals_dense_call_bit_for_bit(case):
    """create_graph=True: outputs, first-order gradients and every gradient of the second backward of the sparse call carry the bits of
    the dense call's.  The pair runs in a fresh process of its own: the create_graph backward (autograd.py::_backward_twice, ATen under
    autograd) does not reproduce its last bits run to run once other layers have run in the process -- the same DENSE call, twice,
    differed in 8 of its 13 second-order gradients (by at most 2.4e-7) inside this file's run, DESIGN.md section 9 item 8 -- so a
    comparison made there would measure that, not the adjacency's form.  In a fresh process it reproduces."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=root, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", "")))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tensors compared" in r.stdout


def test_layer_sparse_call_first_order_under_create_graph_and_empty_adjacency():
    """In this process: outputs and the first-order gradients taken with create_graph=True, bit for bit (they are reproducible here; the
    second backward is compared in test_second_order_sparse_call_equals_dense_call_bit_for_bit), and K = 0."""
    from egnn_pytorch_amd import EGNN
    names, dense, sparse = _second_order_layer()
    for name, x, y in list(zip(names, dense, sparse))[:4]:
        assert _same(x, y), name
    layer = EGNN(dim=8, only_sparse_neighbors=True).cuda()
    feats, coors = torch.randn(2, 40, 8, device="cuda"), torch.randn(2, 40, 3, device="cuda")
    # no bond at all: K = 0, no messages -- on both forms
    none = torch.zeros(40, 40, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        for x, y in zip(layer(feats, coors, adj_mat=none), layer(feats, coors, adj_mat=_SA().from_dense(none))):
            assert _same(x, y)


# ------------------------------------------------------------------ 3. networks without num_adj_degrees
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kw", [dict(), dict(num_edge_tokens=5, edge_dim=4), dict(global_linear_attn_every=1, global_linear_attn_heads=2,
                                                                                 global_linear_attn_dim_head=8)],
                         ids=["plain", "edge_tokens", "attention"])
def test_network_sparse_call_equals_dense_call(kw, dtype):
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(6)
    b, n, dim = 2, 48, 16
    net = EGNN_Network(depth=2, dim=dim, num_tokens=7, only_sparse_neighbors=True, **kw).cuda().to(dtype)
    gen = torch.Generator(device="cuda").manual_seed(12)
    tokens = torch.randint(0, 7, (b, n), device="cuda", generator=gen)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen, dtype=dtype)
    mask = torch.rand(b, n, device="cuda", generator=gen) < 0.9
    edges = torch.randint(0, 5, (b, n, n), device="cuda", generator=gen) if "num_edge_tokens" in kw else None
    adj = _adjacency(b, n, 4, False, gen)
    adj[:, 2] = False
    wn = torch.randn(b, n, dim, device="cuda", generator=gen, dtype=dtype)

    def run(a):
        net.zero_grad()
        c = coors.clone().requires_grad_(True)
        h, x = net(tokens, c, adj_mat=a, edges=edges, mask=mask)
        ((h * wn).sum() + x.square().sum()).backward()
        return [h.detach(), x.detach(), c.grad] + [p.grad.clone() for p in net.parameters() if p.grad is not None]

    dense, sparse = run(adj), run(_SA().from_dense(adj))
    assert len(dense) == len(sparse) > 10
    for x, y in zip(dense, sparse):
        assert _same(x, y)


# ------------------------------------------------------------------ 4. the N-degree expansion on CSR rows
def _adj_kind(kind, n, b, rng):
    """(B, N, N) bool: the kinds of test_gpu_adj_expand_large.py"""
    i = np.arange(n)
    if kind == "chain":
        return np.broadcast_to(np.abs(i[:, None] - i[None, :]) <= 1, (b, n, n)).copy()
    if kind == "chain_nodiag":
        return np.broadcast_to(np.abs(i[:, None] - i[None, :]) == 1, (b, n, n)).copy()
    if kind == "sparse_random":                                          # asymmetric, empty rows, no forced diagonal
        return rng.random((b, n, n)) < min(0.01, 2.0 / n)
    adj = rng.random((b, n, n)) < min(0.03, 4.0 / n)
    return adj | adj.transpose(0, 2, 1) | np.eye(n, dtype=bool)[None]


@pytest.mark.parametrize("kind", ["chain", "chain_nodiag", "random", "sparse_random"])
@pytest.mark.parametrize("n", [16, 70, 1024, 4160])
def test_csr_expansion_equals_the_dense_expansion(n, kind):
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(n + len(kind))
    b = 2
    adj = torch.from_numpy(_adj_kind(kind, n, b, rng)).cuda()
    for batched in (True, False):
        a = adj if batched else adj[0]
        sa = _SA().from_dense(a)
        for degrees in (1, 2, 3, 4):
            ref_adj, ref_lab = _ops.adj_expand(a, b, degrees)
            out, lab = _ops.adj_expand_csr(sa, b, degrees)
            assert out.num_graphs == lab.num_graphs == (b if batched else 1)
            _SA()(out.rowptr, out.col, n, validate=True)                 # sorted rows, offsets in range
            _SA()(lab.rowptr, lab.col, n, validate=True)
            dense = out.to_dense()
            assert torch.equal(dense if batched else dense.expand(b, n, n), ref_adj), (batched, degrees)
            assert torch.equal(lab.to_dense(b), ref_lab), (batched, degrees)
            assert int(lab.val.min()) >= 1 if lab.val.numel() else True
            if (n == 70 and degrees in (2, 4)) or (n == 4160 and degrees == 2):   # ... the global-memory bit maps, and a second run
                out2, lab2 = _ops.adj_expand_csr(sa, b, degrees, force_global=True)
                out3, lab3 = _ops.adj_expand_csr(sa, b, degrees)
                for x, y in ((out2, out), (out3, out)):
                    assert torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col)
                for x, y in ((lab2, lab), (lab3, lab)):
                    assert torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col) and torch.equal(x.val, y.val)
            del ref_adj, ref_lab


def test_csr_expansion_of_a_star_with_17000_leaves():
    """Degree 2 of a star without diagonal: the centre row (17 000 entries) and every output row (17 000 or 17 001 entries) are longer
    than 64 KB of int32 -- no workgroup holds one as a list; the centre's own bond to itself appears and the leaves lose the centre
    (relabelled 2 by the XOR although it leaves the adjacency)."""
    from egnn_pytorch_amd import _ops
    n = 17001
    leaves = torch.arange(1, n)
    ei = torch.cat([torch.stack([torch.zeros_like(leaves), leaves]), torch.stack([leaves, torch.zeros_like(leaves)])], dim=1)
    sa = _SA().from_edge_index(ei, n).to("cuda")
    ref_adj, ref_lab = _ops.adj_expand(sa.to_dense(), 1, 2)
    for force in (False, True):
        out, lab = _ops.adj_expand_csr(sa, 1, 2, force_global=force)
        lens, lab_lens = out.row_lengths()[0], lab.rowptr[0, 1:] - lab.rowptr[0, :-1]
        assert int(lens[0]) == 1 and int(lens[1:].min()) == n - 1 > 16384   # (the centre keeps only itself; a leaf gets every leaf)
        assert int(lab_lens.min()) == n                                  # every label row holds every column
        assert torch.equal(out.to_dense()[None], ref_adj)
        assert torch.equal(lab.to_dense(), ref_lab)
    assert bool(ref_lab[0, 1, 0] == 2) and not bool(ref_adj[0, 1, 0])    # the quirk is in this graph


def test_csr_expansion_under_capture_says_why_not():
    from egnn_pytorch_amd import _ops
    sa = _SA().from_dense(torch.eye(8, dtype=torch.bool, device="cuda"))
    _ops.adj_expand_csr(sa, 1, 2)                                        # (warm: library loaded, allocator primed)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(g):
            _ops.adj_expand_csr(sa, 1, 2)


# ------------------------------------------------------------------ 5. slot labels, gather and gradients by slot
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("use_idx", [True, False], ids=["knn", "dense_layer"])
def test_slot_labels_gather_and_grad_equal_the_dense_label_map(use_idx, dtype):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    gen = torch.Generator(device="cuda").manual_seed(31)
    b, n, k, d1, d2, degrees = 3, 70, 9, 3, 4, 3
    adj = _adjacency(b, n, 3, False, gen)
    adj[:, 2] = False
    coors = torch.randn(b, n, 3, device="cuda", generator=gen)
    for batched in (True, False):
        a = adj if batched else adj[0]
        _, lab_dense = _ops.adj_expand(a, b, degrees)
        _, lab = _ops.adj_expand_csr(_SA().from_dense(a), b, degrees)
        if use_idx:
            idx, _ = _ops.knn_select(coors, None, a, k)
            kk = k
        else:
            idx, kk = None, n
        slot = _ops.csr_slot_labels(lab, idx, b, n, kk)
        want = lab_dense if idx is None else torch.gather(lab_dense, 2, idx.long())
        assert torch.equal(slot, want)
        assert int(slot.max()) == degrees and int(slot.min()) == 0
        tok = torch.randint(0, 5, (b, n, n), device="cuda", generator=gen)
        tok_emb = torch.randn(5, d1, device="cuda", generator=gen, dtype=dtype)
        deg_emb = torch.randn(degrees + 1, d2, device="cuda", generator=gen, dtype=dtype)
        dense_lk = EdgeLookup(tok=tok, tok_emb=tok_emb, deg=lab_dense, deg_emb=deg_emb, dtype=dtype)
        csr_lk = EdgeLookup(tok=tok, tok_emb=tok_emb, deg=lab, deg_emb=deg_emb, dtype=dtype)
        assert _same(_ops.edge_features_gather(csr_lk, idx, b, n, kk), _ops.edge_features_gather(dense_lk, idx, b, n, kk))
        g = torch.randn(b * n * kk, d1 + d2 + 2, device="cuda", generator=gen, dtype=dtype)
        for lo, hi in ((0, b), (1, b)):                                  # (the chunked backward slices the look-up by graphs)
            rows = g[lo * n * kk:hi * n * kk]
            i32 = None if idx is None else idx[lo:hi].contiguous()
            ref = _ops.edge_features_grad(dense_lk.graphs(lo, hi), i32, hi - lo, n, kk, rows)
            got = _ops.edge_features_grad(csr_lk.graphs(lo, hi), i32, hi - lo, n, kk, rows)
            assert _same(got[0], ref[0]) and _same(got[1], ref[1])


# ------------------------------------------------------------------ 6. networks with adjacency degrees
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kw", [dict(), dict(num_edge_tokens=5, edge_dim=4), dict(global_linear_attn_every=1, global_linear_attn_heads=2,
                                                                                 global_linear_attn_dim_head=8),
                                dict(only_sparse_neighbors=False)],
                         ids=["plain", "edge_tokens", "attention", "dense_layers"])
def test_network_with_adjacency_degrees_sparse_call_equals_dense_call(kw, dtype):
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(6)
    b, n, dim = 2, 48, 16
    kw = dict(dict(only_sparse_neighbors=True), **kw)
    net = EGNN_Network(depth=2, dim=dim, num_tokens=7, num_adj_degrees=3, adj_dim=4, **kw).cuda().to(dtype)
    gen = torch.Generator(device="cuda").manual_seed(12)
    tokens = torch.randint(0, 7, (b, n), device="cuda", generator=gen)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen, dtype=dtype)
    mask = torch.rand(b, n, device="cuda", generator=gen) < 0.9
    edges = torch.randint(0, 5, (b, n, n), device="cuda", generator=gen) if "num_edge_tokens" in kw else None
    wn = torch.randn(b, n, dim, device="cuda", generator=gen, dtype=dtype)

    def run(a):
        net.zero_grad()
        c = coors.clone().requires_grad_(True)
        h, x = net(tokens, c, adj_mat=a, edges=edges, mask=mask)
        ((h * wn).sum() + x.square().sum()).backward()
        named = {name: p.grad.clone() for name, p in net.named_parameters() if p.grad is not None}
        return [h.detach(), x.detach(), c.grad], named

    for batched in (True, False):
        adj = _adjacency(b if batched else 1, n, 2, False, gen)
        adj[:, 2] = False
        adj = adj if batched else adj[0]
        (dense, dg), (sparse, sg) = run(adj), run(_SA().from_dense(adj))
        for x, y in zip(dense, sparse):
            assert _same(x, y)
        assert dg.keys() == sg.keys() and "adj_emb.weight" in sg
        for name in dg:
            assert _same(dg[name], sg[name]), name
        assert float(sg["adj_emb.weight"].abs().max()) > 0
        with torch.no_grad():
            for x, y in zip(net(tokens, coors, adj_mat=adj, edges=edges, mask=mask),
                            net(tokens, coors, adj_mat=_SA().from_dense(adj), edges=edges, mask=mask)):
                assert _same(x, y)


# ------------------------------------------------------------------ 7. scale: 262 144 nodes, no N^2 byte map anywhere
CL = 4096


def test_network_on_262144_nodes_equals_each_cluster_alone_without_an_n2_map():
    """64 well-separated clusters of 4 096 nodes, every cluster the same chain (with its diagonal) plus fixed contacts: the dense
    adjacency would be 64 GiB, and the dense expansion two more maps of that size.  One inference forward of
    EGNN_Network(num_adj_degrees=3, adj_dim=4, only_sparse_neighbors=True, depth=1) equals each cluster run alone with its dense adjacency
    (the tolerance of the 40 960-node test in test_gpu_adj_expand_large.py), and the device memory the call takes above its inputs stays
    below N^2 / 16 bytes (4 GiB): no room for any N^2 byte map."""
    from egnn_pytorch_amd import EGNN_Network
    n_clusters = 64
    n = n_clusters * CL
    rng = np.random.default_rng(21)
    grid = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], dtype=np.float64) * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None].astype(np.float32)
    i = torch.arange(CL)
    a = torch.arange(0, CL - 40, 97)
    src = torch.cat([i, i[:-1], i[1:], a, a + 31])
    dst = torch.cat([i, i[1:], i[:-1], a + 31, a])
    local = torch.stack([src, dst])
    ei = torch.cat([local + c * CL for c in range(n_clusters)], dim=1)
    torch.manual_seed(8)
    net = EGNN_Network(num_tokens=20, dim=16, depth=1, num_adj_degrees=3, adj_dim=4, only_sparse_neighbors=True).cuda()
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    c = torch.from_numpy(coors).cuda()
    sa = _SA().from_edge_index(ei, n).to("cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        h, x = net(tokens, c, adj_mat=sa)
    torch.cuda.synchronize()
    above = torch.cuda.max_memory_allocated() - before
    print(f"262144 nodes: peak device memory above the inputs {above / 2 ** 20:.0f} MiB")
    assert above < n * n // 16
    assert torch.isfinite(h).all() and torch.isfinite(x).all()
    blk = torch.zeros(CL, CL, dtype=torch.bool)
    blk[local[0], local[1]] = True
    blk = blk.cuda()
    with torch.no_grad():
        for cl in range(n_clusters):
            s = slice(cl * CL, (cl + 1) * CL)
            h1, x1 = net(tokens[:, s], c[:, s], adj_mat=blk)
            torch.testing.assert_close(h[:, s], h1, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(x[:, s], x1, rtol=1e-5, atol=1e-5)


if __name__ == "__main__":
    # one second-order case in a process of its own (test_second_order_sparse_call_equals_dense_call_bit_for_bit)
    import sys
    names, dense, sparse = _SECOND_ORDER[sys.argv[1]]()
    bad = 0
    for name, x, y in zip(names, dense, sparse):
        ok = _same(x, y)
        bad += not ok
        print(f"{name}: {'same bits' if ok else 'DIFFERENT'}  max |difference| {float((x - y).abs().max()):.3e}  max |value| {float(x.abs().max()):.3e}")
    assert len(names) == len(dense) == len(sparse)
    print(f"{len(names)} tensors compared, {bad} different")
    sys.exit(1 if bad else 0)
