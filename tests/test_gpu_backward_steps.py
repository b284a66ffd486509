"""Steps 2 - 4 of the backward, "ahead of u" (autograd._edge_contract_fused / _edge_contract_blocks, _edge_mlp0_backward, _scalars_to_inputs):
the smallest layers that reach every arm -- the by-source rows as one tile, as row pairs at both ends of 16 < K <= 32 and through the
gather-sum beyond; the dense layer's scatter without a neighbour list; the closed distance form against the scalars' graph with edge
features; two and three blocks of message channels (the second with dropout); chunks of one graph; an edge look-up input; the exact path
in fp32 (17 scalars) and float64 -- in the frame of tests/test_gpu_behind_u_routes.py: each case on the arm it is meant for (the calls of
`_ops.edge_bwd_pass` and what they asked for, whether `_ops.rows_gather_sum` summed the by-source rows), every gradient against the
float64 `_backward_recompute` of a `.double()` copy of the layer over the neighbour list the forward selected: within 1e-4 of each
tensor's maximum in fp32, 1e-9 for a float64 module."""
import copy
import types

import pytest
import torch

from tests.test_gpu_behind_u_routes import B, BASE, scale_parameters

pytestmark = pytest.mark.gpu

N = 37


def passes(row_pairs, blocks=1, chunks=1):
    """the calls of `_ops.edge_bwd_pass` of one backward: (by_dest, row_pairs, block, want_w2, ws_nat is None)"""
    one = [call for blk in range(blocks) for call in ((False, row_pairs, blk, False, False), (True, False, blk, True, True))]
    return one * chunks


# name: (constructor arguments over BASE, options, the backward that runs, the calls of the edge pass, by-source rows through the gather-sum)
CASES = {
    "k8_one_tile": ({}, {}, "native", passes(False), False),
    "k17_row_pairs": (dict(num_nearest_neighbors=17), {}, "native", passes(True), False),
    "k32_row_pairs": (dict(num_nearest_neighbors=32), {}, "native", passes(True), False),
    "k33_gather_sum": (dict(num_nearest_neighbors=33), dict(n=45), "native", passes(False), True),
    "dense_no_list": (dict(num_nearest_neighbors=0), dict(n=20, mask=False), "native", passes(True), False),
    "scalars9_edges": (dict(fourier_features=2, edge_dim=4), dict(edges=True), "native", passes(False), False),
    "m20_two_blocks": (dict(m_dim=20), {}, "native", passes(False, blocks=2), False),
    "m40_three_blocks_dropout": (dict(m_dim=40, dropout=0.1), dict(train=True), "native", passes(False, blocks=3), False),
    "chunks_of_one": ({}, dict(max_graphs=1), "native", passes(False, chunks=B), False),
    "edge_lookup": (dict(edge_dim=4), dict(lookup=True), "native", passes(False), False),
    "exact_scalars17": (dict(fourier_features=8), {}, "exact", [], False),
    "exact_double": ({}, dict(double=True), "exact", [], False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_arm_taken_and_gradients(name, monkeypatch):
    from egnn_pytorch_amd import EGNN, _ops, autograd as A
    from egnn_pytorch_amd.layer import EdgeLookup
    over, opt, path, want_calls, want_gather = CASES[name]
    kw = dict(BASE, **over)
    n = opt.get("n", N)
    dt = torch.float64 if opt.get("double") else torch.float32
    torch.manual_seed(11)
    layer = EGNN(**kw)
    scale_parameters(layer)
    layer = layer.to(device="cuda", dtype=dt).train(bool(opt.get("train")))
    g = torch.Generator().manual_seed(12)
    feats = torch.randn(B, n, kw["dim"], generator=g, dtype=dt).cuda().requires_grad_(True)
    coors = torch.randn(B, n, 3, generator=g, dtype=dt).cuda().requires_grad_(True)
    edges = tok_emb = None
    if opt.get("edges"):
        edges = torch.randn(B, n, n, kw["edge_dim"], generator=g, dtype=dt).cuda().requires_grad_(True)
    if opt.get("lookup"):                                              # (edge tokens behind an embedding: six tokens, width 4)
        tok_emb = torch.randn(6, kw["edge_dim"], generator=g, dtype=dt).cuda().requires_grad_(True)
        edges = EdgeLookup(tok=torch.randint(0, 6, (B, n, n), generator=g).cuda(), tok_emb=tok_emb)
    mask = (torch.arange(n)[None] < torch.tensor([[n], [n - 5], [n // 2 + 3]])).cuda() if opt.get("mask", True) else None
    g_node = torch.randn(B, n, kw["dim"], generator=g, dtype=dt).cuda()
    g_coors = torch.randn(B, n, 3, generator=g, dtype=dt).cuda()

    # plain attribute replacement: the edge passes and the gather-sums recorded, the backward that ran and what it was handed kept
    calls, src_rows, gathered, seen = [], [], [], {}
    recompute, edge_bwd_pass, rows_gather_sum = A._backward_recompute, _ops.edge_bwd_pass, _ops.rows_gather_sum

    def pass_recorded(*a, **k):
        out = edge_bwd_pass(*a, **k)
        calls.append((k["by_dest"], k.get("row_pairs", False), k.get("block", 0), k.get("want_w2", False), k.get("ws_nat") is None))
        if not k["by_dest"]:
            src_rows.append(out["rows"])                               # (kept: its memory is not handed out again during the backward)
        return out

    def gather_recorded(rows, *a, **k):
        gathered.append(any(rows.data_ptr() == r.data_ptr() for r in src_rows))
        return rows_gather_sum(rows, *a, **k)
    monkeypatch.setattr(_ops, "edge_bwd_pass", pass_recorded)
    monkeypatch.setattr(_ops, "rows_gather_sum", gather_recorded)
    for tag in ("native", "exact", "recompute"):
        def kept(ctx, gn, gc, _t=tag, _f=getattr(A, "_backward_" + tag)):
            seen[_t] = (ctx, tuple(ctx.saved_tensors[:6]))
            return _f(ctx, gn, gc)
        monkeypatch.setattr(A, "_backward_" + tag, kept)
    monkeypatch.setattr(A, "_FUSED_MAX_GRAPHS", opt.get("max_graphs", 0))

    params = list(layer.parameters())
    leaves = [feats, coors] + ([edges] if opt.get("edges") else []) + ([tok_emb] if tok_emb is not None else [])
    torch.manual_seed(13)                                              # (the dropout seed is drawn from the CPU generator)
    node, co = layer(feats, coors, edges, mask)
    got = torch.autograd.grad([node, co], leaves + params, [g_node, g_coors], allow_unused=True)
    torch.cuda.synchronize()
    assert list(seen) == [path], (name, list(seen))
    assert calls == want_calls, (name, calls)
    assert any(gathered) == want_gather, (name, gathered)

    # the float64 recompute of a .double() copy over the same neighbour list
    monkeypatch.setattr(_ops, "edge_bwd_pass", edge_bwd_pass)
    monkeypatch.setattr(_ops, "rows_gather_sum", rows_gather_sum)
    ctx, saved = seen[path]
    l64 = copy.deepcopy(layer).double()
    ctx64 = types.SimpleNamespace(layer=l64, saved_tensors=tuple(t.double() if t.is_floating_point() else t for t in saved), flags=ctx.flags,
                                  has_edges=ctx.has_edges, valid_radius=ctx.valid_radius, needs_input_grad=ctx.needs_input_grad,
                                  table_inputs=True, edges_by_k=ctx.edges_by_k, drop=ctx.drop, dead_outputs=(False, False))
    if tok_emb is not None:                                            # (the look-up's tables in float64, their gradients likewise)
        ctx64.lookup, ctx64.table_dtypes, ctx64.csr_pos = ctx.lookup.to(torch.float64), (None, torch.float64, None), None
    want = recompute(ctx64, g_node.double(), g_coors.double())
    want = [want[4], want[5]] + ([want[6]] if opt.get("edges") else []) + ([ctx64.table_grads[0]] if tok_emb is not None else []) + list(want[7:])
    bar = 1e-9 if opt.get("double") else 1e-4
    names = (["feats", "coors"] + (["edges"] if opt.get("edges") else []) + (["tok_emb"] if tok_emb is not None else [])
             + [nm for nm, _ in layer.named_parameters()])
    assert len(names) == len(got) == len(want), name
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
