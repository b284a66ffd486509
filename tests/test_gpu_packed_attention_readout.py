"""A packed k-NN EGNN layer into a learned readout: scores from a Linear(32, H = 2) (without a bias: a softmax does not see a shift of its
scores, so the gradient of one is zero by identity and both routes return rounding noise for it), `GraphSegments.attention_pool`, a
squared loss and backward -- against the padded call with the prefix mask, a masked_fill(-inf) torch softmax over the node axis and an einsum; then once
more under create_graph=True with a gradient penalty on coors.  The bars of tests/test_gpu_packed_layers.py, as in
test_packed_layer_into_the_readout_matches_the_padded_route: ATOL / 1e-4 in fp32, 1e-9 / 1e-8 in float64."""
import math

import pytest
import torch

from tests._util import ATOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
def test_packed_layer_into_the_attention_readout_matches_the_padded_route(dtype):
    from egnn_pytorch_amd import EGNN, GraphSegments
    f64 = dtype == torch.float64
    tol_f, tol_g = (1e-9, 1e-8) if f64 else (ATOL, 1e-4)
    sizes, heads = (7, 1, 12, 5), 2
    torch.manual_seed(11)
    layer, score = EGNN(dim=32, num_nearest_neighbors=4), torch.nn.Linear(32, heads, bias=False)
    layer, score = ((layer.double(), score.double()) if f64 else (layer, score))
    layer, score = layer.cuda(), score.cuda()
    seg = GraphSegments.from_sizes(list(sizes), device="cuda")
    g = torch.Generator().manual_seed(12)
    t = sum(sizes)
    feats, coors = torch.randn(t, 32, generator=g).to(dtype).cuda(), torch.randn(t, 3, generator=g).to(dtype).cuda()
    target = torch.randn(len(sizes), heads, 16, generator=g).to(dtype).cuda()
    mask = seg.prefix_mask()
    params = list(layer.parameters()) + list(score.parameters())

    def packed(f, x):
        node, co = layer(f, x, mask=seg)
        return seg.attention_pool(score(node), node.reshape(t, heads, 16)), co

    def padded(f, x):
        node, co = layer(seg.unpack(f), seg.unpack(x), mask=mask)
        w = torch.softmax(score(node).masked_fill(~mask[..., None], -math.inf), 1)                          # (G, N, H)
        return torch.einsum("gnh,gnhd->ghd", w, node.reshape(len(sizes), -1, heads, 16)), seg.pack(co)

    def run(route, penalty):
        f, x = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        pooled, co = route(f, x)
        loss = ((pooled - target) ** 2).sum() + (co ** 2).sum()
        if penalty:
            force = torch.autograd.grad(loss, x, create_graph=True)[0]
            loss = loss + (force ** 2).sum()
        grads = torch.autograd.grad(loss, [f, x] + params, allow_unused=True)
        return pooled.detach(), [torch.zeros_like(p) if g_ is None else g_ for p, g_ in zip([f, x] + params, grads)]

    names = ["feats", "coors"] + [k for k, _ in layer.named_parameters()] + ["score." + k for k, _ in score.named_parameters()]
    for penalty in (False, True):
        got, ggrads = run(packed, penalty)
        want, wgrads = run(padded, penalty)
        assert got.shape == (len(sizes), heads, 16) and torch.isfinite(got).all() and float((got - want).abs().max()) <= tol_f
        live = 0
        for name, a, b in zip(names, ggrads, wgrads):
            scale, err = float(b.abs().max()), float((a - b).abs().max())
            print(f"attention readout {dtype} penalty={penalty}: d/d {name} error / scale {err / max(scale, 1e-30):.3e} (bar {tol_g:g})")
            assert torch.isfinite(a).all() and err <= tol_g * max(scale, 1e-30), (name, err, scale)
            live += scale > 0
        assert live >= 7
