"""Step 1 of the backward, "behind u" (autograd._behind_u_route): the smallest layers that reach every arm -- the standard tail kernel
whole, in chunks of one graph, with dropout, dense, with more per-edge scalars; the closed form on wider heads, other coordinate
dimensions and layers without coors_mlp / node_mlp, on the native and on the exact path; `layer_tail` through autograd -- each on the
route it is meant for and only that one, every gradient against the float64 `_backward_recompute` of a `.double()` copy of the layer over
the neighbour list the forward selected: within 1e-4 of each tensor's maximum in fp32, 1e-9 for a float64 module (the bars of
tests/test_autograd.py's device gradient tests).

The m_dim 80 case is the one route through fp32 autograd (`layer_tail`): under CoorsNorm its d/d coors carried the self pair's rounding
noise (2.7e-2 of its maximum) until `_behind_u_autograd` took the self pair's x_i - x_i out of the graph, as the closed-form kernels write
its term as the zero it sums to."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, K = 3, 37, 8
BASE = dict(dim=24, num_nearest_neighbors=K, norm_coors=True, coor_weights_clamp_value=0.6, soft_edges=True, m_pool_method="mean", m_dim=16)

# name: (constructor arguments over BASE, options, the backward that runs, the route of step 1, calls of it)
CASES = {
    "standard": ({}, {}, "native", "standard", 1),
    "standard_chunked": ({}, dict(max_graphs=1), "native", "standard", B),
    "standard_dropout": (dict(dropout=0.1), dict(train=True), "native", "standard", 1),
    "standard_dense": (dict(num_nearest_neighbors=0), dict(n=20, mask=False), "native", "standard", 1),
    "standard_scalars9": (dict(fourier_features=2, edge_dim=4), dict(edges=True), "native", "standard", 1),
    "closed_m20": (dict(m_dim=20), {}, "native", "closed", 1),
    "closed_c5": ({}, dict(cdim=5), "native", "closed", 1),
    "closed_no_coors_mlp": (dict(update_coors=False), {}, "native", "closed", 1),
    "closed_no_node_mlp": (dict(update_feats=False), {}, "native", "closed", 1),
    "exact_autograd_m80": (dict(m_dim=80), {}, "exact", "autograd", 1),
    "exact_closed_double": ({}, dict(double=True), "exact", "closed", 1),
}


def scale_parameters(layer):
    """The reference's init is 1e-3-sized, a nearly linear layer: xavier-scale weights instead (biases as they are), under which the
    messages are alive and the gate is not saturated; coors_mlp's last Linear six times that, which puts the coordinate weights on both
    sides of the clamp (12 ... 40 % of the pairs beyond it; nearly all with m_dim 20 and without node_mlp).  No gradient vanishes."""
    for mod in layer.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.xavier_normal_(mod.weight)
    if layer.coors_mlp is not None:
        with torch.no_grad():
            layer.coors_mlp[3].weight.mul_(6.0)


@pytest.mark.parametrize("name", list(CASES))
def test_route_taken_and_gradients(name, monkeypatch):
    from egnn_pytorch_amd import EGNN, autograd as A
    over, opt, path, route, n_calls = CASES[name]
    kw = dict(BASE, **over)
    n, cdim = opt.get("n", N), opt.get("cdim", 3)
    dt = torch.float64 if opt.get("double") else torch.float32
    torch.manual_seed(11)
    layer = EGNN(**kw)
    scale_parameters(layer)
    layer = layer.to(device="cuda", dtype=dt).train(bool(opt.get("train")))
    g = torch.Generator().manual_seed(12)
    feats = torch.randn(B, n, kw["dim"], generator=g, dtype=dt).cuda().requires_grad_(True)
    coors = torch.randn(B, n, cdim, generator=g, dtype=dt).cuda().requires_grad_(True)
    edges = torch.randn(B, n, n, kw["edge_dim"], generator=g, dtype=dt).cuda().requires_grad_(True) if opt.get("edges") else None
    mask = (torch.arange(n)[None] < torch.tensor([[n], [n - 5], [n // 2 + 3]])).cuda() if opt.get("mask", True) else None
    g_node = torch.randn(B, n, kw["dim"], generator=g, dtype=dt).cuda()
    g_coors = torch.randn(B, n, cdim, generator=g, dtype=dt).cuda()

    # plain attribute replacement: the three routes counted, the backward that ran and what it was handed kept
    calls, seen = {"standard": 0, "closed": 0, "autograd": 0}, {}
    recompute = A._backward_recompute
    for r in calls:
        def counted(*a, _r=r, _f=getattr(A, "_behind_u_" + r), **k):
            calls[_r] += 1
            return _f(*a, **k)
        monkeypatch.setattr(A, "_behind_u_" + r, counted)
    for tag in ("native", "exact", "recompute"):
        def kept(ctx, gn, gc, _t=tag, _f=getattr(A, "_backward_" + tag)):
            seen[_t] = (ctx, tuple(ctx.saved_tensors[:6]))
            return _f(ctx, gn, gc)
        monkeypatch.setattr(A, "_backward_" + tag, kept)
    monkeypatch.setattr(A, "_FUSED_MAX_GRAPHS", opt.get("max_graphs", 0))

    params = list(layer.parameters())
    leaves = [feats, coors] + ([edges] if edges is not None else [])
    torch.manual_seed(13)                                              # (the dropout seed is drawn from the CPU generator)
    node, co = layer(feats, coors, edges, mask)
    got = torch.autograd.grad([node, co], leaves + params, [g_node, g_coors], allow_unused=True)
    torch.cuda.synchronize()
    assert list(seen) == [path], (name, list(seen))
    assert calls == {r: (n_calls if r == route else 0) for r in calls}, (name, calls)

    # the float64 recompute of a .double() copy over the same neighbour list
    ctx, saved = seen[path]
    l64 = copy.deepcopy(layer).double()
    ctx64 = types.SimpleNamespace(layer=l64, saved_tensors=tuple(t.double() if t.is_floating_point() else t for t in saved), flags=ctx.flags,
                                  has_edges=ctx.has_edges, valid_radius=ctx.valid_radius, needs_input_grad=ctx.needs_input_grad,
                                  table_inputs=True, edges_by_k=False, drop=ctx.drop, dead_outputs=(False, False))
    want = recompute(ctx64, g_node.double(), g_coors.double())
    want = [want[4], want[5]] + ([want[6]] if edges is not None else []) + list(want[7:])
    bar = 1e-9 if opt.get("double") else 1e-4
    names = ["feats", "coors"] + (["edges"] if edges is not None else []) + [nm for nm, _ in layer.named_parameters()]
    worst = {}
    for nm, a, r in zip(names, got, want):
        assert (a is None) == (r is None), (name, nm)
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), (name, nm)
        scale = float(r.abs().max())
        assert scale > 0, (name, nm)                                   # (a vanishing gradient would make the comparison vacuous)
        worst[nm] = float((a.double() - r).abs().max()) / scale
    print(name, {k_: f"{v:.2e}" for k_, v in worst.items()})
    bad = {k_: v for k_, v in worst.items() if not v <= bar}
    assert not bad, (name, bad)
