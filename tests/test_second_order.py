"""Second-order autograd (create_graph=True) without a GPU: the closed forms of the E x H block (autograd.py::EdgeHidden /
EdgeHiddenGrad, the specification of csrc/edge_hidden.hip) against torch's own double backward of the literal expression, the whole
layer through autograd.EGNNFunction on the CPU stand-in against the reference's float64 second-order results.  (The argument
struct of the C entries against the header: tests/test_abi_agreement.py.)"""
import pytest
import torch

from tests._reference import check_state, pack_grads, reference_result, state_digest, unpack_grads


def _block_inputs(b, n, k, h, m, s_dim, dense, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)    # noqa: E731
    if dense:
        idx = None
        k = n
    else:
        idx = torch.randint(0, n, (b, n, k), generator=g)
        idx[:, :, 0] = torch.arange(n)                       # self pairs
        idx[:, :, 1] = 2                                     # one node chosen by every row
        idx = idx.to(torch.int32)
    e = b * n * k
    return (rnd(b * n, h), rnd(b * n, h), rnd(e, s_dim), 0.5 * rnd(h, s_dim), 0.3 * rnd(m, h), rnd(m)), idx, (b, n, k), rnd(e, m)


@pytest.mark.parametrize("dense,m,s_dim,drop", [
    (False, 16, 1, False), (True, 16, 5, False), (False, 1, 21, False), (False, 70, 5, False), (True, 1, 1, True), (False, 16, 5, True),
    (False, 70, 21, True),
])
def test_closed_forms_match_torch_double_backward(dense, m, s_dim, drop):
    from egnn_pytorch_amd import autograd as A
    (p_i, p_j, s, w_s, w2, b2), idx, dims, g_u = _block_inputs(2, 6, 4, 12, m, s_dim, dense, seed=m + s_dim)
    dr = (0.5, 1234, 17) if drop else None
    ins = [t.clone().requires_grad_(True) for t in (p_i, p_j, s, w_s, w2, b2)]
    gu = g_u.clone().requires_grad_(True)
    u = A.edge_hidden_torch(*ins, idx, dr, dims)
    first = torch.autograd.grad(u, ins, gu, create_graph=True)
    spec1 = A.edge_hidden_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, dr, dims)
    for got, want in zip(spec1, first):
        want = want.detach()
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-300), (got - want).abs().max()
    g = torch.Generator().manual_seed(7)
    cot = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in first]
    second = torch.autograd.grad(first, [gu] + ins[:5], cot, allow_unused=True)
    spec2 = A.edge_hidden_double_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, dr, dims, cot)
    for got, want in zip(spec2, second):
        want = torch.zeros_like(got) if want is None else want
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-300)


def test_edge_hidden_functions_are_twice_differentiable_on_the_host():
    """EdgeHidden / EdgeHiddenGrad on host tensors (the closed forms) under gradcheck / gradgradcheck; a third order raises."""
    from egnn_pytorch_amd import autograd as A
    (p_i, p_j, s, w_s, w2, b2), idx, dims, _ = _block_inputs(1, 4, 3, 5, 3, 2, False, seed=3)
    ins = tuple(t.clone().requires_grad_(True) for t in (p_i, p_j, s, w_s, w2, b2))
    fn = lambda *t: A.EdgeHidden.apply(*t, idx, (0.5, 99, 0), dims)       # noqa: E731
    assert torch.autograd.gradcheck(fn, ins)
    assert torch.autograd.gradgradcheck(fn, ins)
    u = fn(*ins)
    gu = torch.randn(u.shape, dtype=torch.float64, requires_grad=True)
    first = torch.autograd.grad(u, ins, gu, create_graph=True)
    second = torch.autograd.grad(first[0].sum(), ins[0], create_graph=True)[0]
    with pytest.raises(RuntimeError, match="third-order"):
        torch.autograd.grad(second.sum(), ins[1])


# ------------------------------------------------------------------------------------------------ the layer on the CPU stand-in
@pytest.fixture
def cpu_layer_stub(monkeypatch):
    """tests/_cpu_stub.py's forward, wrapped for the `selection=` keyword that autograd.EGNNFunction.forward passes."""
    from egnn_pytorch_amd import _ops, layer as L
    from tests import _cpu_stub
    monkeypatch.setattr(L.EGNN, "_forward_with_hint", L.EGNN._forward_with_hint)        # (restored afterwards)
    monkeypatch.setattr(_ops, "RANGE_CHECK", _ops.RANGE_CHECK)
    _cpu_stub.install()
    stub = L.EGNN._forward_with_hint

    def forward(self, *args, selection=False, **kw):
        return stub(self, *args, **kw)
    monkeypatch.setattr(L.EGNN, "_forward_with_hint", forward)


def force_matching_grads(net, call, coors, wrt, seed=0):
    """d/d (wrt) of a force-matching loss: E = node_out . w, F = -dE/d coors (create_graph=True),
    loss = mean (F - F_ref)^2 + sum coors_out * r."""
    node, co = call()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(node.shape, generator=g).to(node)
    f_ref = torch.randn(coors.shape, generator=g).to(node)
    r = torch.randn(co.shape, generator=g).to(node)
    energy = (node * w).sum()
    force = -torch.autograd.grad(energy, coors, create_graph=True)[0]
    loss = ((force - f_ref) ** 2).mean() + (co * r).sum()
    return torch.autograd.grad(loss, wrt, allow_unused=True)


def _layer_case(kw, n, flags, seed=5):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(60.0)                                  # away from the vacuous default init (std 1e-3)
    layer = layer.double()
    g = torch.Generator().manual_seed(2)
    b = 2
    feats = torch.randn(b, n, kw["dim"], generator=g, dtype=torch.float64)
    # well separated: every node on its own lattice point (no top-k tie under small perturbations)
    coors = (torch.randperm(n * 4, generator=g)[:b * n] if b * n <= n * 4 else torch.arange(b * n)).view(b, n, 1).double()
    coors = torch.cat((coors * 0.37, torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 0.05), dim=-1)
    mask = (torch.arange(n)[None] < torch.tensor([[n], [n - 3]])) if flags.get("mask") else None
    edges = torch.randn(b, n, n, kw.get("edge_dim", 0), generator=g, dtype=torch.float64) if flags.get("edges") else None
    return layer, feats, coors, mask, edges


_CPU_CASES = [
    ("knn4_normcoors", dict(dim=8, num_nearest_neighbors=4, norm_coors=True), 10, dict()),
    ("knn5_mask_fourier", dict(dim=8, num_nearest_neighbors=5, fourier_features=2, coor_weights_clamp_value=3.0), 12, dict(mask=True)),
    ("dense_all_flags", dict(dim=8, edge_dim=2, fourier_features=1, soft_edges=True, norm_coors=True, norm_feats=True, m_pool_method="mean",
                             coor_weights_clamp_value=2.0), 7, dict(mask=True, edges=True)),
]


@pytest.mark.parametrize("name,kw,n,flags", _CPU_CASES, ids=[c[0] for c in _CPU_CASES])
def test_force_matching_through_the_layer_matches_reference(cpu_layer_stub, name, kw, n, flags):
    """create_graph=True through autograd.EGNNFunction (CPU stand-in forward, `_backward_twice` with EdgeHidden's closed forms) against
    the reference's float64 autograd of the same force-matching loss."""
    layer, feats, coors, mask, edges = _layer_case(kw, n, flags)
    mk = lambda t: None if t is None else t.clone().requires_grad_(True)      # noqa: E731

    def reference(ref):
        rl = ref.EGNN(**kw)
        rl.load_state_dict(layer.state_dict(), strict=True)
        rl = rl.double()
        f, c, e = mk(feats), mk(coors), mk(edges)
        wrt = [c, f] + ([e] if e is not None else []) + list(rl.parameters())
        out = pack_grads(force_matching_grads(rl, lambda: rl(f, c, e, mask), c, wrt))
        out["state_sha256"] = state_digest(rl)
        return out
    stored = reference_result(f"second_order_{name}", reference)
    check_state(layer, stored)
    want = unpack_grads(stored)
    f, c, e = mk(feats), mk(coors), mk(edges)
    wrt = [c, f] + ([e] if e is not None else []) + list(layer.parameters())
    got = force_matching_grads(layer, lambda: layer(f, c, e, mask), c, wrt)
    assert len(got) == len(want)
    # (norm_coors: the self pair's x / clamp(|x|, 1e-8) has a Jacobian of scale / 1e-8, which turns float64 rounding -- in the reference's
    # gradient as much as in ours -- into ~1e-8 of the scale at second order (tests/test_autograd.py: the same at first order))
    tol = 1e-7 if kw.get("norm_coors") else 1e-9
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is not None:
            scale = max(float(w.abs().max()), 1e-30)
            assert float((g - w).abs().max()) <= tol * scale, (i, float((g - w).abs().max()), scale)


def test_first_order_is_unchanged_without_create_graph(cpu_layer_stub, monkeypatch):
    """create_graph=False keeps the first-order path (`_backward_twice` is not called, no graph) and the same values as create_graph=True,
    which goes through `_backward_twice` and EdgeHidden."""
    from egnn_pytorch_amd import autograd as A
    calls = []
    twice_fn = A._backward_twice
    monkeypatch.setattr(A, "_backward_twice", lambda *a: calls.append(1) or twice_fn(*a))
    layer, feats, coors, mask, edges = _layer_case(dict(dim=8, num_nearest_neighbors=4), 9, {})
    c = coors.clone().requires_grad_(True)
    node, co = layer(feats, c)
    plain = torch.autograd.grad(node.sum() + co.sum(), c, retain_graph=True)[0]
    assert not calls and not plain.requires_grad
    twice = torch.autograd.grad(node.sum() + co.sum(), c, create_graph=True)[0]
    assert calls and twice.requires_grad
    names, todo, seen = set(), [twice.grad_fn], set()
    while todo:                                                   # the graph of the gradient holds EdgeHidden's backward
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    assert "EdgeHiddenGradBackward" in names, names
    assert float((plain - twice).abs().max()) <= 1e-12 * float(plain.abs().max())


def _energy_fn(layer, feats, mask, seed=4):
    g = torch.Generator().manual_seed(seed)
    w = None

    def energy(c):
        nonlocal w
        node, co = layer(feats, c, None, mask)
        if w is None:
            w = torch.randn(node.shape, generator=g, dtype=node.dtype).to(node.device)
            w2 = torch.randn(co.shape, generator=g, dtype=node.dtype).to(node.device)
            energy.w2 = w2
        return (node * w).sum() + (co * co * energy.w2).sum()
    return energy


def second_order_products(layer, feats, coors, mask, seed=4):
    """hvp, vhp and the Hessian of a scalar energy of (node_out, coors_out) with respect to the coordinates"""
    energy = _energy_fn(layer, feats, mask, seed)
    v = torch.randn(coors.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=coors.dtype).to(coors.device)
    hvp = torch.autograd.functional.hvp(energy, coors, v)[1]
    vhp = torch.autograd.functional.vhp(energy, coors, v)[1]
    hess = torch.autograd.functional.hessian(energy, coors)
    return hvp, vhp, hess


HVP_CASE = ("hvp_knn5_mask", dict(dim=8, num_nearest_neighbors=5, fourier_features=1, soft_edges=True, coor_weights_clamp_value=3.0), 8,
            dict(mask=True))


def test_hvp_vhp_hessian_of_edge_hidden():
    """The second-order products torch.autograd.functional builds (hvp: the double-backward trick, which differentiates the second-order
    backward with respect to its cotangents) through EdgeHidden equal those of the literal expression."""
    from egnn_pytorch_amd import autograd as A
    (p_i, p_j, s, w_s, w2, b2), idx, dims, g_u = _block_inputs(2, 5, 3, 7, 4, 3, False, seed=11)
    dr = (0.5, 5, 0)

    def scalar(fn):
        return lambda *t: (fn(*t, idx, dr, dims) * g_u).sum()
    ins = (p_i, p_j, s, w_s, w2, b2)
    vs = tuple(torch.randn(t.shape, generator=torch.Generator().manual_seed(i), dtype=torch.float64) for i, t in enumerate(ins))
    for product in (torch.autograd.functional.hvp, torch.autograd.functional.vhp):
        got = product(scalar(A.EdgeHidden.apply), ins, vs)[1]
        want = product(scalar(A.edge_hidden_torch), ins, vs)[1]
        for g, w in zip(got, want):
            assert float((g - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-300)


@pytest.mark.parametrize("name,kw,n,flags", [HVP_CASE], ids=[HVP_CASE[0]])
def test_hvp_vhp_hessian_through_the_layer_match_reference(cpu_layer_stub, name, kw, n, flags):
    layer, feats, coors, mask, _ = _layer_case(kw, n, flags)

    def reference(ref):
        rl = ref.EGNN(**kw)
        rl.load_state_dict(layer.state_dict(), strict=True)
        rl = rl.double()
        hvp, vhp, hess = second_order_products(rl, feats, coors.clone(), mask)
        return {"hvp": hvp.numpy(), "vhp": vhp.numpy(), "hessian": hess.numpy(), "state_sha256": state_digest(rl)}
    stored = reference_result(f"second_order_{name}", reference)
    check_state(layer, stored)
    for key, got in zip(("hvp", "vhp", "hessian"), second_order_products(layer, feats, coors.clone(), mask)):
        want = torch.from_numpy(stored[key])
        assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()), key


def test_create_graph_with_no_neighbours(cpu_layer_stub):
    """K = 0 (only_sparse_neighbors and an empty adjacency: no messages) under create_graph=True, against the same loss through
    `layer_given_neighbors` with an empty neighbour list."""
    from egnn_pytorch_amd.autograd import layer_given_neighbors
    layer, feats, coors, _, _ = _layer_case(dict(dim=8, only_sparse_neighbors=True), 6, {})
    adj = torch.zeros(6, 6, dtype=torch.bool)
    c1, c2 = coors.clone().requires_grad_(True), coors.clone().requires_grad_(True)
    wrt = lambda c: [c] + list(layer.parameters())                 # noqa: E731
    got = force_matching_grads(layer, lambda: layer(feats, c1, adj_mat=adj), c1, wrt(c1))
    idx = torch.empty(2, 6, 0, dtype=torch.long)
    want = force_matching_grads(layer, lambda: layer_given_neighbors(layer, feats, c2, None, None, idx, idx.double(), 0.0), c2, wrt(c2))
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert torch.allclose(g, w, rtol=1e-12, atol=1e-14)
