"""`SparseEdges` on the MI355X: a call with bond features / bond tokens on CSR rows returns the same bits as the same call with its
`to_dense()` -- the two entries alone (csrc/edge_csr.hip, csrc/segment_sum.hip) against their dense siblings, layers and networks with
every gradient, the second-order path in a fresh process -- and a 70 000-node network, whose dense token map would be 39 GB, against
each of its clusters run alone.  The dense call is what the other test files pin to the reference; one configuration is compared with
the float64 oracle on the dense image here as well."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O
from tests._util import ATOL

pytestmark = pytest.mark.gpu


def _SE():
    from egnn_pytorch_amd import SparseEdges
    return SparseEdges


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _keep(dense, pat):
    """dense float edges with +0.0 outside the pattern: the dense image of a SparseEdges (a product with the pattern would leave -0.0)"""
    return torch.where(pat[..., None], dense, torch.zeros_like(dense))


def _pattern(b, n, gen, density=0.06):
    """(b, n, n) bool on the device: a sparse random directed pattern with its diagonal, and in graph 0 rows of exactly 0, 1, 3, 64, 65
    and 200 entries (as far as n allows: 64 and 65 sit on either side of one wave's lanes)"""
    pat = torch.rand(b, n, n, device="cuda", generator=gen) < density
    pat |= torch.eye(n, dtype=torch.bool, device="cuda")
    for row, length in enumerate((0, 1, 3, 64, 65, 200)):
        if row < n and length <= n:
            pat[0, row] = False
            cols = torch.randperm(n, device="cuda", generator=gen)[:length]
            pat[0, row, cols] = True
    return pat


def _selection(b, n, k, gen):
    """(b, n, k) int32: k distinct columns per node, in random order (a neighbour list is not sorted)"""
    return torch.rand(b, n, n, device="cuda", generator=gen).topk(k, dim=-1).indices.to(torch.int32).contiguous()


# ------------------------------------------------------------------ 1. the entries alone, against the dense entries
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["float", "tokens"])
@pytest.mark.parametrize("n", [1, 70, 257])
def test_csr_gather_and_grad_equal_the_dense_entries(n, kind, dtype):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    gen = torch.Generator(device="cuda").manual_seed(100 * n + (kind == "tokens"))
    b, vocab, degrees, d2 = 2, 5, 3, 3
    pat = _pattern(b, n, gen)
    if n >= 200:
        lens = pat[0].sum(-1)[:6].tolist()
        assert lens == [0, 1, 3, 64, 65, 200]
    bi, ri, ci = pat.nonzero(as_tuple=True)
    posmap = torch.full((b, n, n), -1, dtype=torch.int32, device="cuda")
    posmap[bi, ri, ci] = torch.arange(bi.numel(), dtype=torch.int32, device="cuda")
    deg = torch.randint(0, degrees + 1, (b, n, n), device="cuda", generator=gen, dtype=torch.uint8)
    deg_emb = torch.randn(degrees + 1, d2, device="cuda", generator=gen, dtype=dtype)
    for d1 in (1, 4, 15, 40):
        if kind == "tokens":
            dense = torch.randint(0, vocab, (b, n, n), device="cuda", generator=gen) * pat      # (token 0 inside the pattern too)
            tok_emb = torch.randn(vocab, d1, device="cuda", generator=gen, dtype=dtype)
        else:
            dense = _keep(torch.randn(b, n, n, d1, device="cuda", generator=gen, dtype=dtype), pat)
            tok_emb = None
        se = _SE().from_dense(dense, pattern=pat)
        assert se.col.numel() == bi.numel() and torch.equal(se.to_dense(), dense)
        for k in (1, 8, 33, None):                                   # (None: the dense layer, idx NULL, K = N)
            if k is not None and k > n:
                continue
            idx = None if k is None else _selection(b, n, k, gen)
            kk = n if k is None else k
            want_pos = posmap if idx is None else torch.gather(posmap, 2, idx.long())
            if n >= 70 and k != 1:
                assert bool((want_pos < 0).any()) and bool((want_pos >= 0).any())   # selected pairs the rows do not hold, and held ones
            for with_deg in (False, True):
                extra = dict(deg=deg, deg_emb=deg_emb) if with_deg else {}
                if kind == "tokens":
                    dense_lk = EdgeLookup(tok=dense, tok_emb=tok_emb, dtype=dtype, **extra)
                else:
                    dense_lk = EdgeLookup(edges=dense, dtype=dtype, **extra)
                csr_lk = EdgeLookup(csr=se, tok_emb=tok_emb, dtype=dtype, **extra)
                ref = _ops.edge_features_gather(dense_lk, idx, b, n, kk)
                out, pos = _ops.edge_features_gather(csr_lk, idx, b, n, kk, with_pos=True)
                assert torch.equal(pos, want_pos), (d1, k, with_deg)
                assert _same(out, ref), (d1, k, with_deg)
                w = d1 + (d2 if with_deg else 0)
                g = torch.randn(b * n * kk, w + 2, device="cuda", generator=gen, dtype=dtype)
                for lo, hi in ((0, b), (1, b)):                      # (the chunked backward slices the look-up by graphs)
                    rows = g[lo * n * kk:hi * n * kk]
                    i32 = None if idx is None else idx[lo:hi].contiguous()
                    ge = torch.zeros(hi - lo, n, n, d1, device="cuda", dtype=dtype) if kind == "float" else None
                    gv = torch.zeros(se.col.numel(), d1, device="cuda", dtype=dtype) if kind == "float" else None
                    r_tok, r_deg = _ops.edge_features_grad(dense_lk.graphs(lo, hi), i32, hi - lo, n, kk, rows, g_edges=ge)
                    g_tok, g_deg = _ops.edge_features_grad(csr_lk.graphs(lo, hi), i32, hi - lo, n, kk, rows, g_edges=gv,
                                                           pos=pos[lo:hi])
                    assert (g_tok is None) == (kind == "float") and (g_deg is None) == (not with_deg)
                    if kind == "tokens":
                        assert _same(g_tok, r_tok), (d1, k, with_deg, lo)
                    else:
                        full = torch.zeros(b, n, n, d1, device="cuda", dtype=dtype)
                        full[lo:hi] = ge
                        assert _same(gv, full[bi, ri, ci]), (d1, k, with_deg, lo)    # the dense entry read at the held pairs
                        held_unselected = torch.ones(b, n, n, dtype=torch.bool, device="cuda")
                        if idx is not None:
                            held_unselected.scatter_(2, idx.long(), False)
                            assert bool((gv[held_unselected[bi, ri, ci]] == 0).all())
                    if with_deg:
                        assert _same(g_deg, r_deg), (d1, k, with_deg, lo)
                # the positions looked up again when the caller does not pass them
                if kind == "tokens" and with_deg:
                    again = _ops.edge_features_grad(csr_lk, idx, b, n, kk, g)
                    first = _ops.edge_features_grad(csr_lk, idx, b, n, kk, g, pos=pos)
                    assert _same(again[0], first[0]) and _same(again[1], first[1])   # and two runs give the same bits


def test_csr_entries_on_an_empty_pattern_and_a_wrong_batch():
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.layer import EdgeLookup
    b, n, k = 2, 9, 4
    gen = torch.Generator(device="cuda").manual_seed(2)
    idx = _selection(b, n, k, gen)
    tok_emb = torch.randn(5, 3, device="cuda", generator=gen)
    for dense in (torch.zeros(b, n, n, 3, device="cuda"), torch.zeros(b, n, n, dtype=torch.int64, device="cuda")):
        se = _SE().from_dense(dense)
        assert se.col.numel() == 0
        lk = EdgeLookup(csr=se, tok_emb=tok_emb if se.is_tokens else None)
        out, pos = _ops.edge_features_gather(lk, idx, b, n, k, with_pos=True)
        assert bool((pos == -1).all())
        want = tok_emb[0].expand(b, n, k, 3) if se.is_tokens else torch.zeros(b, n, k, 3, device="cuda")
        assert _same(out, want.contiguous())
    with pytest.raises(ValueError, match="per graph"):
        _ops.edge_features_gather(lk.graphs(0, 1), idx, b, n, k)


# ------------------------------------------------------------------ 2. layers: sparse call against dense call, outputs and gradients
def _layer_run(layer, feats, coors, mask, adj, edges, mode, held=None, second_order=False):
    """edges: a dense (B,N,N,D) tensor or a SparseEdges.  Returns outputs, gradients of feats / coors / the edge values (for dense edges:
    `edges.grad` read at the `held` pairs, the order of the CSR entries) and of the parameters."""
    from egnn_pytorch_amd import exact_arithmetic
    SE = _SE()
    layer.zero_grad()
    torch.manual_seed(1234)                                          # (training-mode dropout draws its mask seed from it)
    f = feats.clone().requires_grad_(True)
    c = coors.clone().requires_grad_(True)
    if isinstance(edges, SE):
        leaf = edges.values.detach().clone().requires_grad_(True)
        e = SE(edges.rowptr, edges.col, leaf, edges.n, validate=False)
    else:
        leaf = e = edges.clone().requires_grad_(True)
    gen = torch.Generator(device="cuda").manual_seed(77)
    with exact_arithmetic() if mode == "exact" else contextlib.nullcontext():
        node, co = layer(f, c, e, mask=mask, adj_mat=adj)
        loss = (node * torch.randn(node.shape, device="cuda", generator=gen, dtype=node.dtype)).sum() + \
               (co * torch.randn(co.shape, device="cuda", generator=gen, dtype=co.dtype)).sum()
        first = []
        if second_order:
            g1 = list(torch.autograd.grad(loss, [f, c, leaf], create_graph=True))
            if not isinstance(edges, SE):
                # the values of a SparseEdges are the held pairs only: the dense call's second-order objective takes d/d edges there too
                # (a selected pair the rows do not hold has a gradient in the dense tensor that no SparseEdges value stands for)
                g1[2] = g1[2][held]
            sum(g.square().sum() for g in g1).backward()
            first = [g.detach() for g in g1]
        else:
            loss.backward()
    eg = leaf.grad if isinstance(edges, SE) else leaf.grad[held]
    assert leaf.grad.shape == leaf.shape
    return [node.detach(), co.detach()] + first + [f.grad, c.grad, eg] + [p.grad.clone() for p in layer.parameters() if p.grad is not None]


def _layer_inputs(b, n, dim, edge_dim, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    feats = torch.randn(b, n, dim, device="cuda", generator=gen, dtype=dtype)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen, dtype=dtype)
    mask = torch.rand(b, n, device="cuda", generator=gen) < 0.85
    pat = _pattern(b, n, gen, density=0.15)
    dense = _keep(torch.randn(b, n, n, edge_dim, device="cuda", generator=gen, dtype=dtype), pat)
    adj = torch.rand(b, n, n, device="cuda", generator=gen) < 4.0 / n       # a pattern of its own, not the edges'
    adj |= torch.eye(n, dtype=torch.bool, device="cuda")
    return feats, coors, mask, pat, dense, adj


@pytest.mark.parametrize("mode", ["fast", "exact", "float64"])
@pytest.mark.parametrize("case", ["knn", "sparse_adjacency", "dense_layer", "wide_edges", "dropout"])
def test_layer_sparse_edges_call_equals_dense_call(case, mode):
    from egnn_pytorch_amd import EGNN, SparseAdjacency
    torch.manual_seed(3)
    dtype = torch.float64 if mode == "float64" else torch.float32
    kw = dict(knn=dict(num_nearest_neighbors=6), sparse_adjacency=dict(only_sparse_neighbors=True), dense_layer=dict(),
              wide_edges=dict(num_nearest_neighbors=6), dropout=dict(num_nearest_neighbors=6, dropout=0.2))[case]
    edge_dim = 40 if case == "wide_edges" else 4                    # (40 per-edge scalars: the plain kernels)
    b, n, dim = 2, 24 if case == "dense_layer" else 70, 16
    layer = EGNN(dim=dim, edge_dim=edge_dim, **kw).cuda().to(dtype)
    layer.train(case == "dropout")
    feats, coors, mask, pat, dense, adj = _layer_inputs(b, n, dim, edge_dim, dtype, 9)
    adj_arg = SparseAdjacency.from_dense(adj) if case == "sparse_adjacency" else None
    se = _SE().from_dense(dense, pattern=pat)
    held = pat.nonzero(as_tuple=True)
    ref = _layer_run(layer, feats, coors, mask, adj_arg, dense, mode, held)
    got = _layer_run(layer, feats, coors, mask, adj_arg, se, mode)
    assert len(ref) == len(got) > 6
    for i, (x, y) in enumerate(zip(ref, got)):
        assert _same(x, y), i
    assert all(torch.isfinite(x).all() for x in got) and float(got[4].abs().max()) > 0
    if case != "dropout":
        with torch.no_grad():                                        # inference: the dense call takes the one-call C forward in fp32
            for x, y in zip(layer(feats, coors, dense, mask=mask, adj_mat=adj_arg), layer(feats, coors, se, mask=mask, adj_mat=adj_arg)):
                assert _same(x, y)


def test_layer_sparse_edges_call_rerun_on_the_plain_kernels_equals_dense_call():
    """bond features x 1e9 leave the split-fp16 range: the call is re-run on the plain-fp32 kernels automatically, inference and
    training, and returns the dense call's bits there too"""
    import warnings
    from egnn_pytorch_amd import EGNN, _ops
    torch.manual_seed(5)
    layer = EGNN(dim=16, edge_dim=4, num_nearest_neighbors=6).cuda()
    feats, coors, mask, pat, dense, _ = _layer_inputs(2, 70, 16, 4, torch.float32, 11)
    dense = dense * 1e9
    se = _SE().from_dense(dense, pattern=pat)
    held = pat.nonzero(as_tuple=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # (the once-per-process notice of the re-run)
        with torch.no_grad(), _ops.phase_timer() as pt:
            got = layer(feats, coors, se, mask=mask)
        launched = set(pt.summary())
        assert "edge_fused" in launched and "edge_exact" in launched, launched      # the fast attempt, then the re-run
        with torch.no_grad():
            ref = layer(feats, coors, dense, mask=mask)
        for x, y in zip(ref, got):
            assert _same(x, y) and bool(torch.isfinite(y).all())
        for x, y in zip(_layer_run(layer, feats, coors, mask, None, dense, "fast", held),
                        _layer_run(layer, feats, coors, mask, None, se, "fast")):
            assert _same(x, y) and bool(torch.isfinite(y).all())


def test_layer_refuses_a_sparse_edges_of_another_width_or_batch_and_graphed_says_no():
    from egnn_pytorch_amd import EGNN, graphed
    layer = EGNN(dim=16, edge_dim=4, num_nearest_neighbors=6).cuda()
    feats, coors, mask, pat, dense, adj = _layer_inputs(2, 30, 16, 4, torch.float32, 4)
    se = _SE().from_dense(dense, pattern=pat)
    with torch.no_grad():
        with pytest.raises(ValueError):
            layer(feats, coors, _SE().from_dense(dense[..., :3], pattern=pat))
        with pytest.raises(ValueError, match="per graph"):
            layer(feats, coors, se.graphs(0, 1))
        with pytest.raises(RuntimeError, match="same device"):
            layer(feats, coors, se.to("cpu"))
        with pytest.raises(NotImplementedError, match="SparseEdges"):
            graphed(layer, feats, coors, se)


# ------------------------------------------------------------------ 3. networks
_NETS = {
    "edge_tokens": dict(num_edge_tokens=5, edge_dim=4, num_nearest_neighbors=6),
    "float_edges": dict(edge_dim=4, num_nearest_neighbors=6),
    "adj_degrees_tokens": dict(num_edge_tokens=5, edge_dim=4, num_adj_degrees=2, adj_dim=4, only_sparse_neighbors=True),
    "adj_degrees_float": dict(edge_dim=4, num_adj_degrees=2, adj_dim=4, num_nearest_neighbors=6),
    "attention": dict(num_edge_tokens=5, edge_dim=4, num_nearest_neighbors=6, global_linear_attn_every=1, global_linear_attn_heads=2,
                      global_linear_attn_dim_head=8),
}


def _network_case(name, dtype, b=2, n=48, dim=16):
    """(net, run): run(edges, adj) -> (tensors, named parameter gradients); edges dense or SparseEdges, adj dense or SparseAdjacency"""
    from egnn_pytorch_amd import EGNN_Network
    SE = _SE()
    kw = _NETS[name]
    torch.manual_seed(6)
    net = EGNN_Network(depth=2, dim=dim, num_tokens=7, **kw).cuda().to(dtype)
    gen = torch.Generator(device="cuda").manual_seed(12)
    tokens = torch.randint(0, 7, (b, n), device="cuda", generator=gen)
    coors = torch.randn(b, n, 3, device="cuda", generator=gen, dtype=dtype)
    mask = torch.rand(b, n, device="cuda", generator=gen) < 0.9
    pat = _pattern(b, n, gen, density=0.15)
    if "num_edge_tokens" in kw:
        dense = torch.randint(0, 5, (b, n, n), device="cuda", generator=gen) * pat
    else:
        dense = _keep(torch.randn(b, n, n, 4, device="cuda", generator=gen, dtype=dtype), pat)
    adj = torch.rand(b, n, n, device="cuda", generator=gen) < 3.0 / n
    wn = torch.randn(b, n, dim, device="cuda", generator=gen, dtype=dtype)
    held = pat.nonzero(as_tuple=True)

    def run(edges, a, second_order=False):
        net.zero_grad()
        c = coors.clone().requires_grad_(True)
        leaf = None
        if isinstance(edges, SE) and not edges.is_tokens:
            leaf = edges.values.detach().clone().requires_grad_(True)
            edges = SE(edges.rowptr, edges.col, leaf, edges.n, validate=False)
        elif torch.is_tensor(edges) and edges.is_floating_point():
            leaf = edges = edges.clone().requires_grad_(True)
        h, x = net(tokens, c, adj_mat=a, edges=edges, mask=mask)
        loss = (h * wn).sum() + x.square().sum()
        out = [h.detach(), x.detach()]
        if second_order:
            force = torch.autograd.grad(loss, c, create_graph=True)[0]
            force.square().sum().backward()
            out.append(force.detach())
        else:
            loss.backward()
        out.append(c.grad)
        if leaf is not None:
            out.append(leaf.grad if leaf.dim() == 2 else leaf.grad[held])
        return out, {name: p.grad.clone() for name, p in net.named_parameters() if p.grad is not None}

    return net, run, dense, pat, adj, (tokens, coors, mask)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(_NETS))
def test_network_sparse_edges_call_equals_dense_call(name, dtype):
    from egnn_pytorch_amd import SparseAdjacency
    net, run, dense, pat, adj, (tokens, coors, mask) = _network_case(name, dtype)
    se = _SE().from_dense(dense, pattern=pat)
    needs_adj = "num_adj_degrees" in _NETS[name] or _NETS[name].get("only_sparse_neighbors")
    forms = [(adj, SparseAdjacency.from_dense(adj)), (adj, adj)] if needs_adj else [(None, None)]
    for a_dense, a_other in forms:                                   # (with a sparse and with a dense adjacency next to it)
        (ref, rg), (got, gg) = run(dense, a_dense), run(se, a_other)
        assert len(ref) == len(got)
        for i, (x, y) in enumerate(zip(ref, got)):
            assert _same(x, y), i
        assert rg.keys() == gg.keys() and len(gg) > 10
        for key in rg:
            assert _same(rg[key], gg[key]), key
        if "num_edge_tokens" in _NETS[name]:
            assert float(gg["edge_emb.weight"].abs().max()) > 0
        with torch.no_grad():
            for x, y in zip(net(tokens, coors, adj_mat=a_dense, edges=dense, mask=mask),
                            net(tokens, coors, adj_mat=a_other, edges=se, mask=mask)):
                assert _same(x, y)


def test_network_with_sparse_float_edges_against_the_float64_oracle_on_the_dense_image():
    """EGNN_Network(depth=2, edge_dim=4, only_sparse_neighbors=True) on a chain, bond features from a SparseEdges whose pattern is the
    chain's: the oracle evaluates the dense image in float64; the tolerance is the one tests/test_gpu_parity.py holds its network
    configurations to against the oracle (ATOL)."""
    from egnn_pytorch_amd import EGNN_Network, SparseAdjacency
    depth, dim, b, n = 2, 16, 2, 40
    cfg = O.EGNNConfig(dim=dim, edge_dim=4, only_sparse_neighbors=True, norm_feats=True)
    params = {}
    for layer in range(depth):
        params.update(O.random_params(cfg, seed=70 + layer, prefix=f"layers.{layer}.1."))
    net = EGNN_Network(depth=depth, dim=dim, edge_dim=4, only_sparse_neighbors=True)
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(b, n, dim, generator=g)
    coors = torch.randn(b, n, 3, generator=g)
    i = torch.arange(n)
    adj = (i[:, None] - i[None, :]).abs() <= 1
    dense = _keep(torch.randn(b, n, n, 4, generator=g), adj[None].expand(b, n, n))
    mask = torch.arange(n)[None] < torch.tensor([[n], [n - 9]])
    se = _SE().from_dense(dense).cuda()
    with torch.no_grad():
        h, x = net(feats.cuda(), coors.cuda(), adj_mat=SparseAdjacency.from_dense(adj.cuda()), edges=se, mask=mask.cuda())
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    rh, rx = O.egnn_network_forward(depth, cfg, p64, feats.double().numpy(), coors.double().numpy(), adj_mat=adj.numpy(),
                                    edges=dense.double().numpy(), mask=mask.numpy())
    print(f"max |difference| to the float64 oracle: feats {np.abs(h.cpu().numpy() - rh).max():.2e}, coors {np.abs(x.cpu().numpy() - rx).max():.2e}")
    np.testing.assert_allclose(h.cpu().numpy(), rh, atol=ATOL, rtol=0)
    np.testing.assert_allclose(x.cpu().numpy(), rx, atol=ATOL, rtol=0)


# ------------------------------------------------------------------ 4. second order, in a fresh process
def _second_order_layer():
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(4)
    b, n, dim = 2, 40, 8
    layer = EGNN(dim=dim, edge_dim=4, num_nearest_neighbors=5).cuda()
    feats, coors, _, pat, dense, _ = _layer_inputs(b, n, dim, 4, torch.float32, 10)
    held = pat.nonzero(as_tuple=True)
    ref = _layer_run(layer, feats, coors, None, None, dense, "fast", held, second_order=True)
    got = _layer_run(layer, feats, coors, None, None, _SE().from_dense(dense, pattern=pat), "fast", second_order=True)
    names = ["node", "coors", "d/d feats", "d/d coors", "d/d values", "feats.grad", "coors.grad", "values.grad"]
    return names + [f"param {i}" for i in range(len(ref) - len(names))], ref, got


def _second_order_tokens():
    """a force-matching step through EGNN_Network(num_edge_tokens=5, num_adj_degrees=2): the second backward gathers edge_emb's rows
    through the positions (autograd.py::_lookup_rows)"""
    from egnn_pytorch_amd import SparseAdjacency
    net, run, dense, pat, adj, _ = _network_case("adj_degrees_tokens", torch.float32, n=30, dim=8)
    (ref, rg), (got, gg) = run(dense, adj, True), run(_SE().from_dense(dense, pattern=pat), SparseAdjacency.from_dense(adj), True)
    assert rg.keys() == gg.keys() and "edge_emb.weight" in gg and "adj_emb.weight" in gg
    keys = sorted(rg)
    return ["h", "x", "force", "coors.grad"] + keys, ref + [rg[k] for k in keys], got + [gg[k] for k in keys]


_SECOND_ORDER = {"layer": _second_order_layer, "tokens": _second_order_tokens}


@pytest.mark.parametrize("case", sorted(_SECOND_ORDER))
def test_second_order_sparse_edges_call_equals_dense_call_bit_for_bit(case):
    """create_graph=True: outputs, first-order gradients and every gradient of the second backward carry the bits of the dense call's.
    In a fresh process of its own, like test_second_order_sparse_call_equals_dense_call_bit_for_bit (the
    create_graph backward does not reproduce its last bits run to run once other layers have run in the process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=root, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", "")))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tensors compared" in r.stdout


# ------------------------------------------------------------------ 5. scale: 70 000 nodes, no N^2 tensor anywhere
CL = 1000


def test_network_on_70000_nodes_with_bond_tokens_equals_each_cluster_alone_without_an_n2_tensor():
    """70 clusters of 1 000 nodes, every cluster the same chain (with its diagonal) plus fixed contacts, every bond with a token: the
    dense token map would be 8 N^2 = 39 GB.  One inference forward of EGNN_Network(num_edge_tokens=5, edge_dim=4,
    only_sparse_neighbors=True, depth=1) equals each cluster run alone with its dense token map and dense adjacency (the tolerance of
    the 262 144-node test in test_gpu_sparse_adjacency.py), the device memory the call takes above its inputs stays below N^2 bytes --
    one byte per pair -- and one training step runs."""
    from egnn_pytorch_amd import EGNN_Network, SparseAdjacency
    n_clusters = 70
    n = n_clusters * CL
    rng = np.random.default_rng(21)
    coors = np.concatenate([rng.standard_normal((CL, 3)) + 40.0 * np.array([c % 5, (c // 5) % 5, c // 25])
                            for c in range(n_clusters)])[None].astype(np.float32)
    i = torch.arange(CL)
    a = torch.arange(0, CL - 40, 97)
    src = torch.cat([i, i[:-1], i[1:], a, a + 31])
    dst = torch.cat([i, i[1:], i[:-1], a + 31, a])
    local = torch.stack([src, dst])
    local_tok = torch.randint(0, 5, (local.shape[1],), generator=torch.Generator().manual_seed(3))    # (token 0 on some bonds)
    ei = torch.cat([local + c * CL for c in range(n_clusters)], dim=1)
    torch.manual_seed(8)
    net = EGNN_Network(num_tokens=20, dim=16, depth=1, num_edge_tokens=5, edge_dim=4, only_sparse_neighbors=True).cuda()
    tokens = torch.randint(0, 20, (1, n), device="cuda")
    c = torch.from_numpy(coors).cuda()
    sa = SparseAdjacency.from_edge_index(ei, n).to("cuda")
    se = _SE().from_edge_index(ei, local_tok.repeat(n_clusters), n).to("cuda")
    assert se.col.numel() == ei.shape[1] and se.shape == (1, n, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        h, x = net(tokens, c, adj_mat=sa, edges=se)
    torch.cuda.synchronize()
    above = torch.cuda.max_memory_allocated() - before
    print(f"70000 nodes: peak device memory above the inputs {above / 2 ** 20:.0f} MiB")
    assert above < n * n
    assert torch.isfinite(h).all() and torch.isfinite(x).all()
    blk = torch.zeros(CL, CL, dtype=torch.bool)
    blk[local[0], local[1]] = True
    blk_tok = torch.zeros(1, CL, CL, dtype=torch.int64)
    blk_tok[0, local[0], local[1]] = local_tok
    blk, blk_tok = blk.cuda(), blk_tok.cuda()
    with torch.no_grad():
        for cl in range(n_clusters):
            s = slice(cl * CL, (cl + 1) * CL)
            h1, x1 = net(tokens[:, s], c[:, s], adj_mat=blk, edges=blk_tok)
            torch.testing.assert_close(h[:, s], h1, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(x[:, s], x1, rtol=1e-5, atol=1e-5)
    # one backward of it
    torch.cuda.reset_peak_memory_stats()
    cg = c.clone().requires_grad_(True)
    h, x = net(tokens, cg, adj_mat=sa, edges=se)
    (h.square().sum() + x.sum()).backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < n * n
    assert torch.isfinite(cg.grad).all() and float(net.edge_emb.weight.grad.abs().max()) > 0
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)


if __name__ == "__main__":
    # one second-order case in a process of its own (test_second_order_sparse_edges_call_equals_dense_call_bit_for_bit)
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
