"""Second-order autograd (create_graph=True) on the MI355X: the kernels of csrc/edge_hidden.hip against their specification, gradgradcheck
through EdgeHidden and through float64 layers, force matching against the reference's float64 results (single layers, the
denoise_sparse.py network, an fp32 network on edge look-up tables with global attention), training-mode dropout, no E x H tensor in
ATen, first-order values under create_graph, and the errors that remain."""
import contextlib
import math

import pytest
import torch

from tests._reference import check_state, pack_grads, reference_result, state_digest, unpack_grads
from tests.test_second_order import HVP_CASE, _CPU_CASES, _block_inputs, _layer_case, force_matching_grads, second_order_products

pytestmark = pytest.mark.gpu


def _close(got, want, rel, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    assert err <= rel * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------ 4. kernels against the specification
@pytest.mark.parametrize("dtype,dense,m,s_dim,drop", [
    (torch.float64, False, 16, 1, False), (torch.float64, True, 16, 5, True), (torch.float64, False, 70, 21, False),
    (torch.float64, False, 24, 3, True), (torch.float32, False, 16, 5, True), (torch.float32, False, 40, 1, False),
    (torch.float32, True, 70, 21, False),
])
def test_kernels_match_specification(monkeypatch, dtype, dense, m, s_dim, drop):
    from egnn_pytorch_amd import autograd as A
    (p_i, p_j, s, w_s, w2, b2), idx, dims, g_u = _block_inputs(3, 20, 6, 24, m, s_dim, dense, seed=m)
    dr = (0.5, 4321, 5) if drop else None
    g = torch.Generator().manual_seed(1)
    cot = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (p_i, p_j, s, w_s, w2, b2)]
    want_u = A.edge_hidden_torch(p_i, p_j, s, w_s, w2, b2, idx, dr, dims)
    want1 = A.edge_hidden_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, dr, dims)
    want2 = A.edge_hidden_double_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, dr, dims, cot)
    dv = lambda t: None if t is None else t.to(device="cuda", dtype=dtype if t.is_floating_point() else t.dtype)   # noqa: E731
    ins = [dv(t) for t in (p_i, p_j, s, w_s, w2)]
    i_d, gu_d, cot_d = dv(idx), dv(g_u), [dv(c) for c in cot]
    rel = 1e-12 if dtype == torch.float64 else 1e-5
    _close(A._edge_hidden_fwd_gpu(*ins, dv(b2), i_d, dr, dims), want_u, rel, "u")
    monkeypatch.setattr(A, "_TWICE_BLOCK_EDGES", 1)               # (one contraction block per graph: chunk-independent bits)
    got1 = A._edge_hidden_bwd_gpu(gu_d, *ins, i_d, dr, dims)
    got2 = A._edge_hidden_bwd_gpu(gu_d, *ins, i_d, dr, dims, cot=cot_d)
    for name, got, want in zip(("dPi", "dPj", "ds", "dWs", "dW2", "db2"), got1, want1):
        _close(got, want, rel, name)
    for name, got, want in zip(("ggU", "gPi", "gPj", "gs", "gWs", "gW2"), got2, want2):
        _close(got, want, rel, name)
    again = A._edge_hidden_bwd_gpu(gu_d, *ins, i_d, dr, dims, cot=cot_d)
    monkeypatch.setattr(A, "_TWICE_MAX_GRAPHS", 1)                # forced chunking: one graph per chunk
    chunked1 = A._edge_hidden_bwd_gpu(gu_d, *ins, i_d, dr, dims)
    chunked2 = A._edge_hidden_bwd_gpu(gu_d, *ins, i_d, dr, dims, cot=cot_d)
    for a, b in zip(got2, again):                                 # a repeat: the same bits
        assert torch.equal(a, b)
    for a, b in zip(got1 + got2, chunked1 + chunked2):            # forced chunking: the same bits as one chunk
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. gradgradcheck
def test_gradgradcheck_edge_hidden():
    from egnn_pytorch_amd import autograd as A
    (p_i, p_j, s, w_s, w2, b2), idx, dims, _ = _block_inputs(2, 5, 3, 6, 3, 2, False, seed=9)
    ins = tuple(t.cuda().requires_grad_(True) for t in (p_i, p_j, s, w_s, w2, b2))
    i_d = idx.cuda()
    for dr in (None, (0.5, 77, 3)):
        fn = lambda *t: A.EdgeHidden.apply(*t, i_d, dr, dims)    # noqa: E731
        assert torch.autograd.gradcheck(fn, ins)
        assert torch.autograd.gradgradcheck(fn, ins)


_GGC_CASES = [
    ("knn_all", dict(dim=4, num_nearest_neighbors=3, norm_coors=True, coor_weights_clamp_value=2.0, soft_edges=True, fourier_features=1,
                     edge_dim=2), 3, dict(mask=True, edges=True)),
    ("dense", dict(dim=4), 3, dict()),
    ("mean_pool", dict(dim=4, num_nearest_neighbors=3, m_pool_method="mean"), 3, dict(mask=True)),
    ("no_coors_update", dict(dim=4, num_nearest_neighbors=3, update_coors=False), 3, dict()),
    ("coor_dim5", dict(dim=4, num_nearest_neighbors=3), 5, dict()),
]


@pytest.mark.parametrize("name,kw,cdim,flags", _GGC_CASES, ids=[c[0] for c in _GGC_CASES])
def test_gradgradcheck_float64_layers(name, kw, cdim, flags):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(3)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(30.0)
    layer = layer.double().cuda()
    b, n = 1, 6
    g = torch.Generator().manual_seed(4)
    # well separated: distinct lattice points, so that no top-k choice flips under the finite differences
    base = torch.randperm(4 * n, generator=g)[:n].double()
    coors = torch.cat((base[:, None] * 0.7, torch.randn(n, cdim - 1, generator=g, dtype=torch.float64) * 0.05), dim=-1)[None]
    feats = torch.randn(b, n, kw["dim"], generator=g, dtype=torch.float64)
    mask = (torch.arange(n)[None] < n - 1).cuda() if flags.get("mask") else None
    ins = [feats.cuda().requires_grad_(True), coors.cuda().requires_grad_(True)]
    if flags.get("edges"):
        ins.append(torch.randn(b, n, n, kw["edge_dim"], generator=g, dtype=torch.float64).cuda().requires_grad_(True))
    fn = lambda *t: layer(t[0], t[1], t[2] if len(t) > 2 else None, mask)    # noqa: E731
    assert torch.autograd.gradgradcheck(fn, tuple(ins), atol=1e-5, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ 6. force matching against the reference
@pytest.mark.parametrize("name,kw,n,flags", _CPU_CASES, ids=[c[0] for c in _CPU_CASES])
def test_force_matching_layer_matches_reference(name, kw, n, flags):
    """The same fixtures as tests/test_second_order.py (the reference's float64 autograd), here on the float64 kernels."""
    layer, feats, coors, mask, edges = _layer_case(kw, n, flags)
    stored = reference_result(f"second_order_{name}", _no_record)
    check_state(layer, stored)
    want = unpack_grads(stored)
    layer = layer.cuda()
    mk = lambda t: None if t is None else t.cuda().requires_grad_(True)      # noqa: E731
    f, c, e = mk(feats), mk(coors), mk(edges)
    m = None if mask is None else mask.cuda()
    wrt = [c, f] + ([e] if e is not None else []) + list(layer.parameters())
    got = force_matching_grads(layer, lambda: layer(f, c, e, m), c, wrt)
    tol = 1e-7 if kw.get("norm_coors") else 1e-9                   # (tests/test_second_order.py: CoorsNorm's self pair)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is not None:
            _close(g, w, tol, i)


def _no_record(ref):
    raise RuntimeError("recorded by tests/test_second_order.py")


@contextlib.contextmanager
def _finite_coors_norm(ref):
    """While recording: the reference's CoorsNorm with |x| written as sqrt(max(|x|^2, tiny)) (0 below) instead of coors.norm() -- the same
    values and first derivatives, but a finite second derivative at the self pair (torch's norm gives NaN there, which a stack of
    norm_coors layers carries into every gradient).  Written out here rather than imported, and restored afterwards."""
    cls = ref.EGNN_Network.__init__.__globals__["CoorsNorm"]                  # (the reference module's namespace)
    original = cls.forward

    def forward(self, coors):
        sq = (coors * coors).sum(dim=-1, keepdim=True)
        tiny = torch.finfo(coors.dtype).tiny
        norm = torch.where(sq > tiny, sq.clamp(min=tiny).sqrt(), torch.zeros_like(sq))
        return coors / norm.clamp(min=self.eps) * self.scale
    cls.forward = forward
    try:
        yield
    finally:
        cls.forward = original


def _net_case(kw, n, seed=6, scale=20.0, attn_scale=4.0):
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(seed)
    net = EGNN_Network(**kw)
    with torch.no_grad():
        for attn, egnn in net.layers:                              # (the EGNN layers away from their vacuous default init)
            for p in egnn.parameters():
                p.mul_(scale)
            if attn is not None:                                   # (attention logits that are not near-uniform: its query gradients
                for name, p in attn.named_parameters():            #  are not vacuous)
                    if "to_q" in name or "to_kv" in name:
                        p.mul_(attn_scale)
        if net.global_tokens is not None:
            net.global_tokens.mul_(attn_scale)
    return net


_DENOISE = dict(num_tokens=21, num_positions=48, depth=3, dim=8, num_nearest_neighbors=4, fourier_features=2, norm_coors=True,
                coor_weights_clamp_value=2.0)
# (K = 6: self + the at most four pairs within two hops, which all rank 0 -- no tie at the top-k boundary -- + one by distance)
_LOOKUP = dict(depth=2, dim=8, num_nearest_neighbors=6, num_adj_degrees=2, adj_dim=2, num_edge_tokens=5, edge_dim=3,
               global_linear_attn_every=1, global_linear_attn_heads=2, global_linear_attn_dim_head=8, num_global_tokens=2)


@pytest.mark.parametrize("name,kw,dtype,tol", [
    ("denoise_net", _DENOISE, torch.float64, 1e-7),
    ("lookup_attn_net", _LOOKUP, torch.float32, 1e-4),
])
def test_force_matching_network_matches_reference(name, kw, dtype, tol):
    """EGNN_Network: the denoise_sparse.py network (depth 3, adj_mat) in float64, and an fp32 network on edge look-up tables (edge tokens,
    adjacency degrees) with global attention, against the reference's float64 autograd of the same force-matching loss, every gradient at
    `tol` of its own scale.  The denoise fixture is recorded with the reference's CoorsNorm patched (`_finite_coors_norm`): unpatched,
    its second-order gradients are NaN."""
    net = _net_case(kw, 12)
    b, n = 2, 12
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, 21, (b, n), generator=g)
    base = torch.stack([torch.randperm(4 * n, generator=g)[:n] for _ in range(b)]).double()
    coors = torch.cat((base[..., None] * 0.45, torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 0.05), dim=-1)
    i = torch.arange(n)
    adj = (i[:, None] >= i[None, :] - 1) & (i[:, None] <= i[None, :] + 1)
    mask = torch.arange(n)[None] < torch.tensor([[n], [n - 2]])
    if "num_tokens" in kw:
        feats, edges = tok, None
    else:
        feats = torch.randn(b, n, kw["dim"], generator=g, dtype=torch.float64)
        edges = torch.randint(0, kw["num_edge_tokens"], (b, n, n), generator=g)

    def run(model, f, c, dev):
        f = f.to(dev) if not f.is_floating_point() else f.to(dev).requires_grad_(True)
        c = c.to(dev).requires_grad_(True)
        wrt = [c] + ([f] if f.is_floating_point() else []) + list(model.parameters())
        call = lambda: model(f, c, adj_mat=adj.to(dev), edges=None if edges is None else edges.to(dev), mask=mask.to(dev))   # noqa: E731
        return force_matching_grads(model, call, c, wrt)

    def reference(ref):
        rn = ref.EGNN_Network(**kw)
        rn.load_state_dict(net.state_dict(), strict=True)
        rn = rn.double()
        with _finite_coors_norm(ref):
            out = pack_grads(run(rn, feats if not feats.is_floating_point() else feats.double(), coors, "cpu"))
        out["state_sha256"] = state_digest(rn.float() if dtype == torch.float32 else rn)
        return out
    stored = reference_result(f"second_order_{name}", reference, gpu=True)
    ours = net.to(dtype)
    check_state(ours, stored)
    ours = ours.cuda()
    got = run(ours, feats if not feats.is_floating_point() else feats.to(dtype), coors.to(dtype), "cuda")
    want = unpack_grads(stored)
    assert len(got) == len(want)
    for k, (gg, w) in enumerate(zip(got, want)):
        assert (gg is None) == (w is None), k
        if gg is not None:
            _close(gg, w, tol, k)


# ------------------------------------------------------------------------------------------------ 7. training-mode dropout
def test_dropout_matches_torch_double_backward():
    from egnn_pytorch_amd import EGNN, _dropout
    from egnn_pytorch_amd.autograd import layer_given_neighbors
    torch.manual_seed(3)
    layer = EGNN(dim=6, dropout=0.5)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(30.0)
    layer = layer.double().cuda().train()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 7, 6, generator=g, dtype=torch.float64).cuda()
    coors = torch.randn(2, 7, 3, generator=g, dtype=torch.float64).cuda()
    wrt_of = lambda c, f: [c, f] + list(layer.parameters())        # noqa: E731
    torch.manual_seed(11)
    f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
    got = force_matching_grads(layer, lambda: layer(f, c), c, wrt_of(c, f))
    torch.manual_seed(11)
    seed = _dropout.draw_seed()                                    # (the seed that forward drew)
    f2, c2 = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
    want = force_matching_grads(layer, lambda: layer_given_neighbors(layer, f2, c2, None, None, None, None, math.inf, drop=(0.5, seed)),
                                c2, wrt_of(c2, f2))
    for k, (gg, w) in enumerate(zip(got, want)):
        assert (gg is None) == (w is None), k
        if gg is not None:
            _close(gg, w, 1e-9, k)


# ------------------------------------------------------------------------------------------------ 8. no E x H tensor in ATen
def test_no_edge_by_hidden_tensor_in_aten():
    from torch.utils._python_dispatch import TorchDispatchMode
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(0)
    layer = EGNN(dim=64, num_nearest_neighbors=16).cuda()
    b, n = 2, 64
    feats = torch.randn(b, n, 64, device="cuda", requires_grad=True)
    coors = torch.randn(b, n, 3, device="cuda", requires_grad=True)
    h = layer.edge_mlp[0].weight.shape[0]
    limit = b * n * 16 * h // 2
    alloc = ("empty", "empty_strided", "new_empty", "new_empty_strided", "zeros", "new_zeros", "zero_", "fill_", "full", "new_full",
             "empty_like", "zeros_like")
    big = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = func.overloadpacket.__name__
            if func.is_view:                                        # (a view produces no tensor: slices of the kernels' transient tables)
                return out
            for t in (out if isinstance(out, (tuple, list)) else (out,)):
                if isinstance(t, torch.Tensor) and t.numel() >= limit and name not in alloc:
                    big.append((name, tuple(t.shape)))
            return out
    with Watch():
        node, co = layer(feats, coors)
        energy = (node * node).sum() + co.sum()
        force = torch.autograd.grad(energy, coors, create_graph=True)[0]
        loss = force.square().sum()
        loss.backward()
    torch.cuda.synchronize()
    assert not big, big
    assert feats.grad is not None and layer.edge_mlp[0].weight.grad is not None


# ------------------------------------------------------------------------------------------------ 9. first order under create_graph
@pytest.mark.parametrize("dtype,rel", [(torch.float32, 1e-4), (torch.float64, 1e-10)])
def test_first_order_values_under_create_graph(dtype, rel):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(1)
    layer = EGNN(dim=16, num_nearest_neighbors=6, edge_dim=2, fourier_features=1, norm_feats=True)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(30.0)
    layer = layer.to(dtype).cuda()
    g = torch.Generator().manual_seed(2)
    b, n = 2, 20
    feats = torch.randn(b, n, 16, generator=g).to(dtype).cuda().requires_grad_(True)
    coors = torch.randn(b, n, 3, generator=g).to(dtype).cuda().requires_grad_(True)
    edges = torch.randn(b, n, n, 2, generator=g).to(dtype).cuda().requires_grad_(True)
    mask = (torch.arange(n)[None] < torch.tensor([[n], [n - 4]])).cuda()
    rn = torch.randn(b, n, 16, generator=g).to(dtype).cuda()
    rc = torch.randn(b, n, 3, generator=g).to(dtype).cuda()
    wrt = [feats, coors, edges] + list(layer.parameters())
    res = []
    for cg in (False, True):
        node, co = layer(feats, coors, edges, mask)
        res.append(torch.autograd.grad((node * rn).sum() + (co * rc).sum(), wrt, create_graph=cg))
    assert res[1][1].requires_grad and not res[0][1].requires_grad
    for k, (a, b_) in enumerate(zip(*res)):
        _close(b_, a, rel, k)


# ------------------------------------------------------------------------------------------------ 10. clear errors
def test_third_order_raises():
    from egnn_pytorch_amd import EGNN
    layer = EGNN(dim=8, num_nearest_neighbors=4).double().cuda()
    coors = torch.randn(1, 10, 3, dtype=torch.float64, device="cuda", requires_grad=True)
    feats = torch.randn(1, 10, 8, dtype=torch.float64, device="cuda")
    node, _ = layer(feats, coors)
    first = torch.autograd.grad(node.square().sum(), coors, create_graph=True)[0]
    second = torch.autograd.grad(first.square().sum(), coors, create_graph=True)[0]
    with pytest.raises(RuntimeError, match="third-order"):
        torch.autograd.grad(second.sum(), coors)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_module_under_create_graph_raises(dtype):
    from egnn_pytorch_amd import EGNN
    layer = EGNN(dim=8, num_nearest_neighbors=4).to(dtype).cuda()
    coors = torch.randn(1, 10, 3, device="cuda").to(dtype).requires_grad_(True)
    feats = torch.randn(1, 10, 8, device="cuda").to(dtype)
    node, _ = layer(feats, coors)
    with pytest.raises(NotImplementedError, match="float32 or float64"):
        torch.autograd.grad(node.float().square().sum(), coors, create_graph=True)


# ------------------------------------------------------------------------------------------------ hvp / vhp / hessian, K = 0, wide scalars
@pytest.mark.parametrize("name,kw,n,flags", [HVP_CASE], ids=[HVP_CASE[0]])
def test_hvp_vhp_hessian_match_reference(name, kw, n, flags):
    """torch.autograd.functional.hvp (double-backward trick: the second-order backward differentiated with respect to its cotangents),
    vhp and hessian of a float64 layer on the device against the reference's (tests/test_second_order.py records them)."""
    layer, feats, coors, mask, _ = _layer_case(kw, n, flags)
    stored = reference_result(f"second_order_{name}", _no_record)
    check_state(layer, stored)
    layer = layer.cuda()
    got = second_order_products(layer, feats.cuda(), coors.cuda(), None if mask is None else mask.cuda())
    for key, g in zip(("hvp", "vhp", "hessian"), got):
        _close(g, torch.from_numpy(stored[key]), 1e-9, key)


def test_create_graph_with_no_neighbours():
    """K = 0 (only_sparse_neighbors and an empty adjacency) under create_graph=True on the device, against `layer_given_neighbors`."""
    from egnn_pytorch_amd.autograd import layer_given_neighbors
    layer, feats, coors, _, _ = _layer_case(dict(dim=8, only_sparse_neighbors=True), 6, {})
    layer, feats = layer.cuda(), feats.cuda()
    adj = torch.zeros(6, 6, dtype=torch.bool, device="cuda")
    c1, c2 = coors.cuda().requires_grad_(True), coors.cuda().requires_grad_(True)
    wrt = lambda c: [c] + list(layer.parameters())                 # noqa: E731
    got = force_matching_grads(layer, lambda: layer(feats, c1, adj_mat=adj), c1, wrt(c1))
    idx = torch.empty(2, 6, 0, dtype=torch.long, device="cuda")
    want = force_matching_grads(layer, lambda: layer_given_neighbors(layer, feats, c2, None, None, idx, idx.double(), 0.0), c2, wrt(c2))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), k
        if g is not None:
            _close(g, w, 1e-12, k)


@pytest.mark.parametrize("edge_dim", [30, 60])
def test_more_scalars_than_the_kernels_take(edge_dim):
    """31 / 61 per-edge scalars in float64 -- beyond the 26 the kernels keep in LDS: the block runs as its torch expression
    (`edge_hidden_kernels_fit`), against torch's double backward of `layer_given_neighbors` on the same neighbours."""
    from egnn_pytorch_amd import autograd as A
    from egnn_pytorch_amd.autograd import layer_given_neighbors
    kw = dict(dim=6, edge_dim=edge_dim, num_nearest_neighbors=4)
    layer, feats, coors, _, edges = _layer_case(kw, 8, dict(edges=True))
    assert not A.edge_hidden_kernels_fit(2 * layer.fourier_features + 1 + edge_dim, torch.float64)
    layer, feats, edges = layer.cuda(), feats.cuda(), edges.cuda()
    c1, c2 = coors.cuda().requires_grad_(True), coors.cuda().requires_grad_(True)
    wrt = lambda c: [c] + list(layer.parameters())                 # noqa: E731
    got = force_matching_grads(layer, lambda: layer(feats, c1, edges), c1, wrt(c1))
    d = ((coors[:, :, None] - coors[:, None]) ** 2).sum(-1).cuda()
    rank, idx = d.topk(4, dim=-1, largest=False)
    want = force_matching_grads(layer, lambda: layer_given_neighbors(layer, feats, c2, edges, None, idx, rank, math.inf), c2, wrt(c2))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), k
        if g is not None:
            _close(g, w, 1e-9, k)
