"""Oracle vs the reference module itself (its outputs stored by tests/_reference.py: tests/golden/reference/).
This is the differential pin of SURVEY.md §8c at BASELINE.json-like layer widths."""
import numpy as np
import pytest
import torch

from egnn_pytorch_amd import EGNN
from oracle import egnn_oracle as O
from tests._reference import case_key, check_state, reference_result, state_digest
from tests._util import check_neighbors


def _xavier(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            if p.ndim == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[0] + p.shape[1])) ** 0.5)


@pytest.mark.parametrize("kwargs,b,n,use_mask", [
    (dict(dim=512, num_nearest_neighbors=32), 1, 192, True),      # north-star layer, reduced N
    (dict(dim=512), 1, 48, False),                                # config 2 layer, reduced N
    (dict(dim=128, num_nearest_neighbors=32, norm_feats=True), 2, 128, True),   # config 3 layer
    (dict(dim=256, num_nearest_neighbors=32, norm_feats=True, norm_coors=True), 1, 128, True),  # config 5 layer
])
def test_layer(kwargs, b, n, use_mask, request):
    def build(cls):
        torch.manual_seed(0)
        m = cls(**kwargs).eval()
        _xavier(m, 11)
        return m
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(b, n, kwargs["dim"], generator=g)
    coors = torch.randn(b, n, 3, generator=g)
    mask = None
    if use_mask:
        lens = torch.randint(n // 2, n + 1, (b,), generator=g)
        mask = torch.arange(n)[None] < lens[:, None]

    def reference(ref):
        rlayer = build(ref.EGNN)
        captured = []
        orig = torch.Tensor.topk

        def spy(t, *a, **kw):
            out = orig(t, *a, **kw)
            captured.append(out)
            return out

        torch.Tensor.topk = spy
        try:
            with torch.no_grad():
                rn, rc = rlayer(feats, coors, mask=mask)
        finally:
            torch.Tensor.topk = orig
        out = dict(node=rn.numpy(), coors=rc.numpy(), state_sha256=state_digest(rlayer))
        if captured:
            out.update(topk_values=captured[0][0].numpy(), topk_indices=captured[0][1].numpy())
        return out
    want = reference_result(case_key(request), reference)
    layer = build(EGNN)
    check_state(layer, want)
    rn, rc = want["node"], want["coors"]
    params = {k: v.numpy() for k, v in layer.state_dict().items()}
    cfg = O.EGNNConfig(**kwargs)
    node, co, nr, ni = O.egnn_forward(cfg, params, feats.numpy(), coors.numpy(),
                                      mask=None if mask is None else mask.numpy(), return_neighbors=True)
    if "topk_values" in want:
        check_neighbors(want["topk_values"], want["topk_indices"].astype(np.int32),
                        nr.astype(np.float32), ni.astype(np.int32))
    np.testing.assert_allclose(node, rn, atol=3e-5, rtol=0)
    np.testing.assert_allclose(co, rc, atol=3e-5, rtol=0)


def test_sparse_chain_config4_layer(request):
    n, b = 64, 2

    def build(cls):
        torch.manual_seed(0)                                # (the biases keep their default init: seeded, so they can be rebuilt)
        m = cls(dim=512, edge_dim=4, only_sparse_neighbors=True).eval()
        _xavier(m, 3)
        return m
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(b, n, 512, generator=g)
    coors = torch.randn(b, n, 3, generator=g)
    edges = torch.randn(b, n, n, 4, generator=g)
    mask = torch.ones(b, n, dtype=torch.bool)
    i = torch.arange(n)
    adj = (i[:, None] - i[None, :]).abs() <= 1

    def reference(ref):
        rlayer = build(ref.EGNN)
        with torch.no_grad():
            rn, rc = rlayer(feats, coors, edges, mask, adj)
        return dict(node=rn.numpy(), coors=rc.numpy(), state_sha256=state_digest(rlayer))
    want = reference_result(case_key(request), reference)
    layer = build(EGNN)
    check_state(layer, want)
    params = {k: v.numpy() for k, v in layer.state_dict().items()}
    cfg = O.EGNNConfig(dim=512, edge_dim=4, only_sparse_neighbors=True)
    node, co = O.egnn_forward(cfg, params, feats.numpy(), coors.numpy(), edges.numpy(), mask.numpy(), adj.numpy())
    np.testing.assert_allclose(node, want["node"], atol=3e-5, rtol=0)
    np.testing.assert_allclose(co, want["coors"], atol=3e-5, rtol=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_squared_distance_summation_tree_matches_torch_bit_for_bit(dtype):
    """`(rel_coors ** 2).sum(dim=-1)` (egnn_pytorch.py:233) for every coordinate dimension the kernels take: the oracle's restatement of
    ATen's inner-dimension sum (egnn_oracle.inner_sum; the kernels' egnn_sqdist_any follows the same tree) against torch itself."""
    rng = np.random.default_rng(0)
    for c in list(range(1, 41)) + [48, 63, 64, 65, 100, 128, 200]:
        a = rng.standard_normal((2, 24, c)).astype(dtype)
        t = torch.from_numpy(a)
        rel = t[:, :, None, :] - t[:, None, :, :]
        want = (rel ** 2).sum(dim=-1).numpy()
        got_rel, got = O.pairwise(a)
        assert np.array_equal(got_rel, rel.numpy()), c
        assert np.array_equal(got, want), (c, dtype)


@pytest.mark.parametrize("kwargs,cdim", [(dict(dim=32, num_nearest_neighbors=8), 11), (dict(dim=24, num_nearest_neighbors=8, norm_coors=True), 33),
                                         (dict(dim=16), 9)])
def test_layer_with_more_than_eight_coordinates(kwargs, cdim, request):
    def build(cls):
        torch.manual_seed(cdim)
        m = cls(**kwargs).eval()
        _xavier(m, 3)
        return m
    g = torch.Generator().manual_seed(cdim + 1)
    feats, coors = torch.randn(2, 36, kwargs["dim"], generator=g), torch.randn(2, 36, cdim, generator=g)
    mask = torch.arange(36)[None] < torch.tensor([[36], [29]])

    def reference(ref):
        rlayer = build(ref.EGNN)
        with torch.no_grad():
            rn, rc = rlayer(feats, coors, mask=mask)
        return dict(node=rn.numpy(), coors=rc.numpy(), state_sha256=state_digest(rlayer))
    want = reference_result(case_key(request), reference)
    layer = build(EGNN)
    check_state(layer, want)
    want_n, want_c = torch.from_numpy(want["node"]), torch.from_numpy(want["coors"])
    params = {k: v.detach().numpy() for k, v in layer.state_dict().items()}
    got_n, got_c = O.egnn_forward(O.EGNNConfig(**kwargs), params, feats.numpy(), coors.numpy(), mask=mask.numpy())
    np.testing.assert_allclose(got_n, want_n.numpy(), atol=1e-5 * max(1.0, float(want_n.abs().max())), rtol=0)
    np.testing.assert_allclose(got_c, want_c.numpy(), atol=1e-5 * max(1.0, float(want_c.abs().max())), rtol=0)
