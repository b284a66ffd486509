"""Packed batches (`mask=GraphSegments`) through EGNN and EGNN_Network, inference and training, against the reference.

Reference: the reference module in float64 on the PADDED batch (`segments.unpack`) with the prefix mask, its outputs and gradients
gathered back to the real nodes (`segments.pack`) -- recorded on the CPU with EGNN_RECORD_REFERENCE=1 (tests/_reference.py) and stored
under tests/golden/reference/packed_*.npz.  A fixture also carries what had to be derived from the reference's own run, so that both
sides use the same numbers: the `valid_radius` of the radius row (between the median of the selected distances and the next larger
one) and coors_mlp's last bias after the clamp was centred among the coordinate weights (tests/test_gpu_mask_patterns_training.py:
`_centre_clamp`).  The batch holds graphs of 40, 7, 96, 1 and 33 nodes: with K = 8 ... 32 some are smaller than K.

Bars, the project's own: forward tests/_util.ATOL (1e-4); every gradient within 1e-4 of its own scale (max |reference|, asserted > 0),
cotangents random; float64 modules 1e-9 forward and 1e-8 of scale."""
import zlib

import numpy as np
import pytest
import torch

from tests._reference import check_state, reference_result, state_digest
from tests._util import ATOL

pytestmark = pytest.mark.gpu

SIZES = (40, 7, 96, 1, 33)
# id -> (layer kwargs, coordinate dimension, arithmetic class).  After tests/test_gpu_mask_patterns_training.py's table.
ROWS = {
    "pw_k8": (dict(dim=32, num_nearest_neighbors=8), 3, "fast"),                             # wave-per-node edge kernel
    "pw_k32": (dict(dim=64, num_nearest_neighbors=32, norm_feats=True), 3, "fast"),          # one node per wave
    "all_flags": (dict(dim=48, num_nearest_neighbors=24, soft_edges=True, norm_coors=True, m_pool_method="mean",
                       coor_weights_clamp_value=1.5, norm_feats=True, fourier_features=2), 3, "fast"),
    "m32_blocks": (dict(dim=32, num_nearest_neighbors=16, m_dim=32), 3, "fast"),
    "cdim5": (dict(dim=32, num_nearest_neighbors=8, norm_coors=True), 5, "fast"),            # generic tail kernel
    "radius": (dict(dim=32, num_nearest_neighbors=8), 3, "fast"),                            # pair mask = empty slots AND the radius
    "exact_cdim9": (dict(dim=24, num_nearest_neighbors=8), 9, "exact"),                      # plain-fp32 kernels
    "double": (dict(dim=16, num_nearest_neighbors=6, norm_coors=True, fourier_features=1), 3, "double"),   # float64 kernels
}


def _segments(sizes=SIZES, device="cpu"):
    from egnn_pytorch_amd import GraphSegments
    return GraphSegments.from_sizes(sizes, device=device)


def _make_layer(kw, seed, double):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed % (2 ** 31))
    layer = EGNN(**kw)
    with torch.no_grad():
        if kw.get("coor_weights_clamp_value"):           # (xavier weights where a clamp has to fall among the coordinate weights)
            for mod in layer.modules():
                if isinstance(mod, torch.nn.Linear):
                    torch.nn.init.xavier_normal_(mod.weight)
        else:
            for p in layer.parameters():
                p.mul_(40.0)                             # away from the vacuous default init (std 1e-3), as elsewhere
    return layer.double() if double else layer


def _inputs(row, sizes=SIZES):
    kw, cdim, path = ROWS[row]
    seed = zlib.crc32(row.encode())
    g = torch.Generator().manual_seed(seed + 1)
    t, dt = sum(sizes), torch.float64 if path == "double" else torch.float32
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dt)                  # noqa: E731  (float32 values, also for a float64 module)
    scale = min(1.0, 8.0 / kw["num_nearest_neighbors"])                          # (tests/test_gpu_mask_patterns_training.py: `_build`)
    return seed, mk(t, kw["dim"]), mk(t, cdim) * scale, mk(t, kw["dim"]), mk(t, cdim)


def _selected_distances(coors, sizes, k):
    """the squared distances of every node's min(K, n) nearest nodes of its graph, as the reference computes them, sorted"""
    out, lo = [], 0
    for n in sizes:
        x = coors[lo:lo + n].float()
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        out.append(d.topk(min(k, n), dim=-1, largest=False).values.reshape(-1))
        lo += n
    return torch.cat(out).sort().values


def _centred_bias(rl, w, live):
    """coors_mlp's last bias (float32) shifted so that the clamp falls into the widest gap of the live coordinate weights between their
    10 % and 90 % quantiles"""
    ws = w[live].double().sort().values
    lo, hi = ws.numel() // 10, max(ws.numel() // 10 + 1, 9 * ws.numel() // 10)
    gaps = ws[lo + 1:hi + 1] - ws[lo:hi]
    j = int(gaps.argmax())
    assert float(gaps[j]) > 4e-5, "no gap among the coordinate weights wide enough to put the clamp in"
    shift = rl.coor_weights_clamp_value - 0.5 * (ws[lo + j] + ws[lo + j + 1])
    return rl.coors_mlp[3].bias.detach().float() + shift.float()


def _layer_fixture(row, sizes=SIZES):
    """(layer on the CPU with the weights the fixture belongs to, stored arrays, feats, coors, cotangents)"""
    kw, cdim, path = ROWS[row]
    seed, feats, coors, rn, rc = _inputs(row, sizes)
    layer = _make_layer(kw, seed, path == "double")
    seg = _segments(sizes)
    k = kw["num_nearest_neighbors"]

    def reference(ref):
        extra = {}
        rkw = dict(kw)
        if row == "radius":
            d = _selected_distances(coors, sizes, k).unique()
            mid = d.numel() // 2
            rkw["valid_radius"] = extra["valid_radius"] = 0.5 * (float(d[mid]) + float(d[mid + 1]))
        rl = ref.EGNN(**rkw)
        rl.load_state_dict(layer.state_dict())
        rl = rl.double()
        mask = seg.prefix_mask()
        fp, xp = seg.unpack(feats.double()).requires_grad_(True), seg.unpack(coors.double()).requires_grad_(True)
        if kw.get("coor_weights_clamp_value"):
            seen = []
            hook = rl.coors_mlp.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
            with torch.no_grad():
                rl(fp, xp, None, mask)
            hook.remove()
            w = seen[0].squeeze(-1)                                              # (G, N, K): neighbours ascending, the real ones first
            live = mask[:, :, None] & (torch.arange(k)[None, None, :] < torch.tensor(sizes)[:, None, None])
            bias = _centred_bias(rl, w, live)
            with torch.no_grad():
                rl.coors_mlp[3].bias.copy_(bias.double())
            extra["clamp_bias"] = bias.numpy()
        node, co = rl(fp, xp, None, mask)
        params = list(rl.parameters())
        grads = torch.autograd.grad([node, co], [fp, xp] + params, [seg.unpack(rn.double()), seg.unpack(rc.double())])
        out = dict(extra, node=seg.pack(node.detach()).numpy(), coors=seg.pack(co.detach()).numpy(),
                   g_feats=seg.pack(grads[0]).numpy(), g_coors=seg.pack(grads[1]).numpy())
        for i, g in enumerate(grads[2:]):
            out[f"g_param.{i}"] = g.numpy()
        out["state_sha256"] = state_digest(rl if path == "double" else rl.float())
        return out

    stored = reference_result(f"packed_layer_{row}", reference, gpu=True)
    if "clamp_bias" in stored:
        with torch.no_grad():
            layer.coors_mlp[3].bias.copy_(torch.from_numpy(stored["clamp_bias"]).to(layer.coors_mlp[3].bias.dtype))
    if "valid_radius" in stored:
        layer.valid_radius = float(stored["valid_radius"])
    check_state(layer, stored)
    return layer, stored, feats, coors, rn, rc


def _check(row, stored, node, co, grads, names, what):
    f64 = ROWS[row][2] == "double"
    tol_f, tol_g = (1e-9, 1e-8) if f64 else (ATOL, 1e-4)
    for name, got in (("node", node), ("coors", co)):
        assert bool(torch.isfinite(got).all()), (what, name)
        err = float((got.double().cpu() - torch.from_numpy(stored[name])).abs().max())
        print(f"{what}: {name} error {err:.3e} (bar {tol_f:g})")
        assert err <= tol_f, (what, name, err)
    want = [stored["g_feats"], stored["g_coors"]] + [stored[f"g_param.{i}"] for i in range(len(grads) - 2)]
    for name, g, w in zip(names, grads, want):
        w = torch.from_numpy(w)
        scale = float(w.abs().max())
        assert scale > 0, (what, name, "vacuous reference gradient")
        assert bool(torch.isfinite(g).all()), (what, name, "non-finite gradient")
        err = float((g.double().cpu() - w).abs().max())
        print(f"{what}: d/d {name} error / scale {err / scale:.3e} (bar {tol_g:g})")
        assert err <= tol_g * scale, (what, name, err, scale)


def _train(layer, seg, feats, coors, rn, rc):
    f, x = feats.cuda().requires_grad_(True), coors.cuda().requires_grad_(True)
    node, co = layer(f, x, mask=seg)
    assert node.shape == f.shape and co.shape == x.shape
    grads = torch.autograd.grad([node, co], [f, x] + list(layer.parameters()), [rn.cuda(), rc.cuda()])
    return node.detach(), co.detach(), grads


@pytest.mark.parametrize("row", list(ROWS))
def test_packed_layer_matches_the_reference_forward_and_backward(row):
    layer, stored, feats, coors, rn, rc = _layer_fixture(row)
    layer = layer.cuda()
    seg = _segments(device="cuda")
    names = ["feats", "coors"] + [k for k, _ in layer.named_parameters()]
    node, co, grads = _train(layer, seg, feats, coors, rn, rc)
    _check(row, stored, node, co, grads, names, row)
    with torch.no_grad():                                                        # inference: the same forward bars
        node, co = layer(feats.cuda(), coors.cuda(), mask=seg)
    _check(row, stored, node, co, [], [], row + " (no_grad)")


def test_packed_layer_under_exact_arithmetic_matches_the_reference():
    from egnn_pytorch_amd import exact_arithmetic
    layer, stored, feats, coors, rn, rc = _layer_fixture("pw_k8")
    layer = layer.cuda()
    seg = _segments(device="cuda")
    names = ["feats", "coors"] + [k for k, _ in layer.named_parameters()]
    with exact_arithmetic():
        node, co, grads = _train(layer, seg, feats, coors, rn, rc)
    _check("pw_k8", stored, node, co, grads, names, "pw_k8 (exact_arithmetic)")


def test_one_graph_is_the_ordinary_call_bit_for_bit():
    """G = 1, eval mode: the packed call and layer(feats[None], coors[None], mask=ones) -- the same kernels, the same lists"""
    kw, cdim, _ = ROWS["pw_k8"]
    seed, feats, coors, _, _ = _inputs("pw_k8", (40,))
    layer = _make_layer(kw, seed, False).cuda().eval()
    f, x = feats.cuda(), coors.cuda()
    with torch.no_grad():
        node, co = layer(f, x, mask=_segments((40,), "cuda"))
        wn, wc = layer(f[None], x[None], mask=torch.ones(1, 40, dtype=torch.bool, device="cuda"))
    assert torch.equal(node, wn[0]) and torch.equal(co, wc[0])


def test_chunked_call_meets_the_reference_and_cuts_at_graph_boundaries(monkeypatch):
    """the node limit lowered to 64: several calls, each its own EGNNFunction, cut at graph boundaries -- the same bars (not the same
    bits: operand scales are per call)"""
    from egnn_pytorch_amd import EGNN, layer as L
    layer, stored, feats, coors, rn, rc = _layer_fixture("pw_k8")
    layer = layer.cuda()
    seg = _segments(device="cuda")
    pieces = []
    one = EGNN._call_packed_one

    def spy(self, f, x, segments, hint):
        pieces.append(segments.sizes)
        return one(self, f, x, segments, hint)
    monkeypatch.setattr(EGNN, "_call_packed_one", spy)
    monkeypatch.setattr(L, "_PACKED_MAX_NODES", 64)
    names = ["feats", "coors"] + [k for k, _ in layer.named_parameters()]
    node, co, grads = _train(layer, seg, feats, coors, rn, rc)
    assert len(pieces) > 1 and sum(pieces, ()) == SIZES, pieces                  # whole graphs, every one once, in order
    assert all(sum(p) <= 64 or len(p) == 1 for p in pieces), pieces
    _check("pw_k8", stored, node, co, grads, names, "pw_k8 (chunked)")


# ------------------------------------------------------------------------------------------------ EGNN_Network
_NET = dict(depth=3, dim=16, num_tokens=11, num_positions=96, num_nearest_neighbors=8, norm_coors=True)


def test_packed_network_matches_the_reference_with_coor_changes():
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(17)
    net = EGNN_Network(**_NET)
    with torch.no_grad():
        for _, egnn in net.layers:
            for p in egnn.parameters():
                p.mul_(20.0)
    g = torch.Generator().manual_seed(18)
    t = sum(SIZES)
    tok, coors = torch.randint(0, _NET["num_tokens"], (t,), generator=g), torch.randn(t, 3, generator=g)
    seg = _segments()

    def reference(ref):
        rn = ref.EGNN_Network(**_NET)
        rn.load_state_dict(net.state_dict(), strict=True)
        rn = rn.double()
        with torch.no_grad():
            feats, co, changes = rn(seg.unpack(tok), seg.unpack(coors.double()), mask=seg.prefix_mask(), return_coor_changes=True)
        out = dict(feats=seg.pack(feats).numpy(), coors=seg.pack(co).numpy(), state_sha256=state_digest(rn.float()))
        for i, c in enumerate(changes):
            out[f"change.{i}"] = seg.pack(c).numpy()
        return out
    stored = reference_result("packed_network_tokens_pos", reference, gpu=True)
    check_state(net, stored)
    net = net.cuda()
    with torch.no_grad():
        feats, co, changes = net(tok.cuda(), coors.cuda(), mask=seg.to("cuda"), return_coor_changes=True)
    assert feats.shape == (t, _NET["dim"]) and co.shape == (t, 3) and len(changes) == _NET["depth"] + 1
    for name, got in [("feats", feats), ("coors", co)] + [(f"change.{i}", c) for i, c in enumerate(changes)]:
        err = float((got.double().cpu() - torch.from_numpy(stored[name])).abs().max())
        print(f"network: {name} error {err:.3e}")
        assert err <= ATOL, (name, err)


# ------------------------------------------------------------------------------------------------ create_graph=True
def test_force_norm_gradient_matches_the_reference_double_backward():
    """d/d parameters of |dE/d coors|^2 on a .double() layer, against the reference's float64 double backward; the float64 bar of
    tests/test_gpu_second_order.py (1e-9 of the gradient's scale)"""
    from egnn_pytorch_amd import EGNN
    kw = dict(dim=8, num_nearest_neighbors=4)
    sizes = (6, 3, 9, 1)
    torch.manual_seed(5)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(60.0)
    layer = layer.double()
    g = torch.Generator().manual_seed(6)
    t = sum(sizes)
    feats = torch.randn(t, kw["dim"], generator=g, dtype=torch.float64)
    coors = torch.randn(t, 3, generator=g, dtype=torch.float64)
    w = torch.randn(t, kw["dim"], generator=g, dtype=torch.float64)
    seg = _segments(sizes)

    def loss_grads(model, call, x, weight):
        node, _ = call()
        force = torch.autograd.grad((node * weight).sum(), x, create_graph=True)[0]
        return torch.autograd.grad((force ** 2).sum(), list(model.parameters()), allow_unused=True)

    def reference(ref):
        rl = ref.EGNN(**kw)
        rl.load_state_dict(layer.state_dict())
        rl = rl.double()
        fp, xp = seg.unpack(feats), seg.unpack(coors).requires_grad_(True)
        grads = loss_grads(rl, lambda: rl(fp, xp, None, seg.prefix_mask()), xp, seg.unpack(w))
        out = {f"g_param.{i}": (torch.zeros_like(p) if g_ is None else g_).numpy() for i, (p, g_) in enumerate(zip(rl.parameters(), grads))}
        out["state_sha256"] = state_digest(rl)
        return out
    stored = reference_result("packed_layer_force_norm_double", reference, gpu=True)
    check_state(layer, stored)
    layer = layer.cuda()
    x = coors.cuda().requires_grad_(True)
    segd = seg.to("cuda")
    grads = loss_grads(layer, lambda: layer(feats.cuda(), x, mask=segd), x, w.cuda())
    nonzero = 0
    for i, (p, g_) in enumerate(zip(layer.parameters(), grads)):
        want = torch.from_numpy(stored[f"g_param.{i}"])
        got = torch.zeros_like(want) if g_ is None else g_.double().cpu()
        scale = float(want.abs().max())
        nonzero += scale > 0
        err = float((got - want).abs().max())
        print(f"force norm: parameter {i} error {err:.3e} scale {scale:.3e}")
        assert err <= 1e-9 * max(scale, 1e-30), (i, err, scale)
    assert nonzero >= 4


# ------------------------------------------------------------------------------------------------ dropout
def test_training_mode_dropout_runs_and_repeats_under_a_seed():
    kw = dict(ROWS["pw_k8"][0], dropout=0.2)
    seed, feats, coors, rn, rc = _inputs("pw_k8")
    layer = _make_layer(kw, seed, False).cuda().train()
    seg = _segments(device="cuda")
    runs = []
    for _ in range(2):
        torch.manual_seed(99)
        runs.append(_train(layer, seg, feats, coors, rn, rc))
    (n0, c0, g0), (n1, c1, g1) = runs
    assert bool(torch.isfinite(n0).all()) and bool(torch.isfinite(c0).all())
    assert torch.equal(n0, n1) and torch.equal(c0, c1)
    for a in g0 + g1:
        assert bool(torch.isfinite(a).all())
    layer.eval()
    with torch.no_grad():
        ne, _ = layer(feats.cuda(), coors.cuda(), mask=seg)
    assert not torch.equal(ne, n0)                                               # (the masks were on)
