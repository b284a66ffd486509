"""Every instantiation of the plain fp32 / float64 edge kernels (csrc/edge_exact.hip, csrc/edge_exact_bwd.hip, csrc/edge_hidden.hip)
against the float64 specification of tests/_plain_variants.py, one parametrised case per cell of its table: direct calls of
`_ops.edge_exact`, `_ops.drop_silu_`, `_ops.edge_exact_bwd` + `_ops.edge_exact_node_sums`, `_ops.edge_tail_exact` and `_ops.edge_hidden`
on a few hundred edges.

Every output of every cell is compared with the specification: float64 at 1e-12 max(1, max |ref|), fp32 edge_hidden at 1e-5 of the
tensor's scale, the other fp32 entries at 8 x the error torch fp32 makes on the same specification and inputs + 16 x 2^-24 max |ref|
(`_plain_variants.bar`; never derived from a kernel's output).  Each case prints its error-to-bar ratios.  Beside that, in every cell:
no NaN in a buffer that started as NaN, exact zeros wherever the specification has a structural zero (masked pairs, a node without a
kept edge under mean pooling, self pairs' d/d rel, clamped or masked d/d w, dropped units), the same bits on a second run, the slack
around every output intact (`Guard`: every output and every buffer the binding allocates lies inside a larger buffer of a sentinel
value, at least one row of slack on each side), the dropout cells split by graph bit-equal to the one call, and the refused calls
raising the launcher's code with every output still poisoned."""
import contextlib
import math

import pytest
import torch

from tests import _plain_variants as V

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


class Guard:
    """`_ops.empty` with slack: the tensor handed out is the middle of a larger flat buffer, NaN inside, SENTINEL around it"""

    def __init__(self):
        self.bufs = []

    def empty(self, *shape, dtype, device):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        numel = math.prod(shape)
        pad = (max(shape[-1] if shape else 1, 1) + 15) // 16 * 16               # at least one row, 16 elements keep the alignment
        flat = torch.full((numel + 2 * pad,), SENTINEL if dtype.is_floating_point else 0x55, dtype=dtype, device=device)
        inner = flat[pad:pad + numel]
        inner.fill_(float("nan") if dtype.is_floating_point else 0x7F)
        self.bufs.append((flat, pad, numel))
        return inner.view(shape)

    def assert_slack_intact(self, what):
        for flat, pad, numel in self.bufs:
            fill = SENTINEL if flat.dtype.is_floating_point else 0x55
            assert bool((flat[:pad] == fill).all()) and bool((flat[pad + numel:] == fill).all()), (what, "a write outside an output")

    def assert_nothing_written(self, what):
        for flat, pad, numel in self.bufs:
            if flat.dtype.is_floating_point:
                assert bool(torch.isnan(flat[pad:pad + numel]).all()), (what, "a refused call wrote to an output")


@contextlib.contextmanager
def guarded(guard, bad_inv=False):
    """the binding's own allocations (workspace, node sums, the tail's dict) come out of `guard`; bad_inv: drop_inv_keep = 0.5"""
    from egnn_pytorch_amd import _dropout, _ops
    saved = _ops.empty, _dropout.inv_keep
    _ops.empty = guard.empty
    if bad_inv:
        _dropout.inv_keep = lambda p: 0.5
    try:
        yield
    finally:
        _ops.empty, _dropout.inv_keep = saved


def _up(t, dt):
    if t is None:
        return None
    if t.dtype == torch.bool:
        return t.cuda().contiguous().view(torch.uint8)
    if not t.is_floating_point():
        return t.to(torch.int32).cuda().contiguous()
    return t.to(dt).cuda().contiguous()


def _first_linear_args(a, d, dt, keep):
    """B .. ldws, coors, edges, idx of egnn_edge_exact_args / egnn_edge_exact_bwd_args"""
    p = d.cell.p
    esz = 8 if dt == torch.float64 else 4
    a.B, a.N, a.K, a.m_dim, a.H = d.b, d.n, d.k, p["m"], p["H"]
    a.fourier, a.edge_dim, a.coor_dim, a.edges_by_k = p["fourier"], p["edge_dim"], p["cdim"], int(p["by_k"])
    if p["strided"]:
        proj, w1 = _up(d.node["proj"], dt), _up(d.glob["w1"], dt)
        keep += [proj, w1]
        a.Pi, a.Pj, a.ldp = proj.data_ptr(), proj.data_ptr() + esz * d.hq, 2 * d.hq
        a.Ws, a.ldws = w1.data_ptr() + esz * 2 * d.dim, w1.shape[1]
    else:
        pi, pj, ws = _up(d.node["Pi"], dt), _up(d.node["Pj"], dt), _up(d.glob["Ws"], dt)
        keep += [pi, pj, ws]
        a.Pi, a.Pj, a.ldp, a.Ws, a.ldws = pi.data_ptr(), pj.data_ptr(), p["H"], ws.data_ptr(), d.s
    coors, w2 = _up(d.node["coors"], dt), _up(d.glob["W2"], dt)
    edges = _up(d.edge.get("edges", d.node.get("edges")), dt)
    idx = None if p["no_idx"] else _up(d.edge.get("idx"), dt)
    keep += [coors, w2, edges, idx]
    a.coors, a.W2, a.edges, a.idx = coors.data_ptr(), w2.data_ptr(), _ptr(edges), _ptr(idx)
    return coors, idx


def _ptr(t):
    return None if t is None else t.data_ptr()


def _drop3(d, eid0):
    return None if d.drop is None else (d.drop[0], d.drop[1], eid0)


def run_fwd(d, dt, guard, eid0=0):
    from egnn_pytorch_amd import _abi, _ops
    p, opts = d.cell.p, d.cell.p["opts"]
    m, cd, dev = p["m"], p["cdim"], torch.device("cuda")
    a, keep = _abi.EdgeExactArgs(), []
    coors, _ = _first_linear_args(a, d, dt, keep)
    before = coors.clone()
    a.pool_mean = int("mean" in opts or "mean_mask0" in opts)
    G = {name: _up(t, dt) for name, t in d.glob.items()}
    a.b2 = G["b2"].data_ptr()
    if "gate_w" in G:
        a.gate_w, a.gate_b = G["gate_w"].data_ptr(), G["gate_b"].data_ptr()
    if "W3" in G:
        a.W3, a.b3, a.W4, a.b4 = (G[name].data_ptr() for name in ("W3", "b3", "W4", "b4"))
    if "scale" in G:
        a.coors_scale = G["scale"].data_ptr()
    mask, rank = _up(d.node.get("mask"), dt), _up(d.edge.get("rank"), dt)
    a.mask, a.rank = _ptr(mask), _ptr(rank)
    a.valid_radius = float(getattr(d, "valid_radius", float("inf"))) if rank is not None else 3.0e38
    a.clamp = V.CLAMP if "clamp" in opts else -1.0
    out = {}
    if "no_mi" not in opts:
        out["m_i"] = guard.empty(d.b * d.n, m, dtype=dt, device=dev)
        a.m_i = out["m_i"].data_ptr()
    if "W3" in G:
        out["coors_out"] = guard.empty(d.b * d.n, cd, dtype=dt, device=dev)
        a.coors_out = out["coors_out"].data_ptr()
    if "u_out" in opts:
        out["U_out"] = guard.empty(d.e, m, dtype=dt, device=dev)
        a.U_out = out["U_out"].data_ptr()
    _ops.set_drop(a, d.drop, eid0)
    ws = _ops.edge_exact(a, dev, dt)
    assert ws.numel() == d.e * (m + cd + 1)
    ws = ws.view(d.e, m + cd + 1)
    out.update(ws_m=ws[:, :m], ws_wrel=ws[:, m:m + cd], ws_kept=ws[:, m + cd])
    torch.cuda.synchronize()
    assert torch.equal(coors, before), "the forward wrote to its input coordinates"
    return out


def run_bwd(d, dt, guard, eid0=0):
    from egnn_pytorch_amd import _abi, _ops
    p, dev = d.cell.p, torch.device("cuda")
    a, keep = _abi.EdgeExactBwdArgs(), []
    _, idx = _first_linear_args(a, d, dt, keep)
    gu = _up(d.edge["gU"], dt)
    out = dict(A_T=guard.empty(p["H"], d.e, dtype=dt, device=dev), DZ_T=guard.empty(p["H"], d.e, dtype=dt, device=dev),
               g_scal=guard.empty(d.e, d.s, dtype=dt, device=dev))
    a.gU, a.A_T, a.DZ_T, a.g_scal = gu.data_ptr(), out["A_T"].data_ptr(), out["DZ_T"].data_ptr(), out["g_scal"].data_ptr()
    _ops.set_drop(a, d.drop, eid0)
    _ops.edge_exact_bwd(a, dt)
    dl = _ops.dest_lists(None if idx is None else idx.view(d.b, d.n, d.k), d.b, d.n, d.k, dev)
    out["gPi"], out["gPi_T"], out["gPj"], out["gPj_T"] = _ops.edge_exact_node_sums(out["DZ_T"], d.b * d.n, d.k, dl.order, dl.seg)
    return out


def run_tail(d, dt, guard, eid0=0):
    from egnn_pytorch_amd import _ops
    p, opts = d.cell.p, d.cell.p["opts"]
    G = {name: _up(t, dt) for name, t in d.glob.items()}
    idx = None if p["no_idx"] else _up(d.edge.get("idx"), dt)
    w3 = [G.get(name) for name in ("W3", "b3", "W4", "b4")]
    gate = (G["gate_w"], G["gate_b"]) if "gate_w" in G else None
    return _ops.edge_tail_exact(_up(d.edge["u"], dt), _up(d.node["coors"], dt).view(d.b, d.n, p["cdim"]), idx, _up(d.edge.get("pair_mask"), dt),
                                _up(d.node["g_co"], dt), _up(d.node.get("g_msum"), dt), *w3, G.get("scale"), V.EPS,
                                V.CLAMP if "clamp" in opts else None, gate, d.b, d.n, d.k, drop=d.drop, eid0=eid0)


def run_hidden(d, dt, guard, eid0=0):
    from egnn_pytorch_amd import _ops, autograd as A
    p, dev, entry = d.cell.p, torch.device("cuda"), d.cell.entry
    m, h, e, s = p["m"], p["H"], d.e, d.s
    G = {name: _up(t, dt) for name, t in d.glob.items()}
    N = {name: _up(t, dt) for name, t in d.node.items()}
    Ed = {name: _up(t, dt) for name, t in d.edge.items()}
    idx = None if p["no_idx"] or "idx" not in Ed else Ed["idx"].view(d.b, d.n, d.k)
    a = A._eh_args((d.b, d.n, d.k), 0, d.b, N["Pi"], N["Pj"], Ed["s"], G["Ws"], G["W2"], idx, _drop3(d, eid0))
    new = lambda *sh: guard.empty(*sh, dtype=dt, device=dev)                     # noqa: E731
    if entry == "hfwd":
        out = dict(u=new(e, m))
        a.b2, a.u = G["b2"].data_ptr(), out["u"].data_ptr()
        _ops.edge_hidden("fwd", a, dt)
        return out
    a.gU = Ed["gU"].data_ptr()
    if entry == "hbwd":
        out = dict(A_T=new(h, e), DZ_T=new(h, e), g_s=new(e, s))
        a.A_T, a.DZ_T, a.g_s = (out[name].data_ptr() for name in ("A_T", "DZ_T", "g_s"))
        _ops.edge_hidden("bwd", a, dt)
        return out
    out = dict(g_gU=new(e, m), g_s=new(e, s), DAV_T=new(h, e), R_T=new(h, e), DZ_T=new(h, e))
    a.cPi, a.cPj, a.cs = N["cPi"].data_ptr(), N["cPj"].data_ptr(), Ed["cs"].data_ptr()
    a.cWs, a.cW2, a.cb2 = G["cWs"].data_ptr(), G["cW2"].data_ptr(), G["cb2"].data_ptr()
    a.g_gU, a.g_s, a.DAV_T, a.R_T, a.DZ_T = (out[name].data_ptr() for name in ("g_gU", "g_s", "DAV_T", "R_T", "DZ_T"))
    _ops.edge_hidden("bwd2", a, dt)
    return out


def run_silu(d, dt, guard, row0=0, parts=1):
    """in place on a (rows, cols) view of a (rows, cols + 3) buffer: the three pad columns must keep their sentinel"""
    from egnn_pytorch_amd import _abi, _ops
    z0 = _up(d.glob["Z"], dt)
    rows, cols = z0.shape
    buf = torch.full((rows + 2, cols + 3), SENTINEL, dtype=dt, device=z0.device)     # (a row of slack above and below as well)
    z = buf[1:-1, :cols]
    z.copy_(z0)
    step = (rows + parts - 1) // parts
    try:
        for lo in range(0, rows, step):
            _ops.drop_silu_(z[lo:lo + step], d.drop, row0 + lo)
    except _abi.EGNNHipError:
        torch.cuda.synchronize()
        assert torch.equal(z, z0), "a refused drop_silu wrote to Z"
        raise
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "drop_silu wrote outside its rows"
    assert bool((buf[:, cols:] == SENTINEL).all()), "drop_silu wrote beyond `cols`"
    return dict(Z=z.clone())


RUNNERS = dict(fwd=run_fwd, bwd=run_bwd, sums=run_bwd, tail=run_tail, hfwd=run_hidden, hbwd=run_hidden, hbwd2=run_hidden, silu=run_silu)


def _run(cell, d, guard, **kw):
    with guarded(guard, bad_inv=cell.p["bad_inv"]):
        out = RUNNERS[cell.entry](d, V.torch_dtype(cell.t), guard, **kw)
    torch.cuda.synchronize()
    return out


def _by_graph(cell, d, guard):
    """the same call once per graph with drop_eid0 = g N K (`autograd._chunk_graphs`), the outputs put together again"""
    if cell.entry == "silu":
        return _run(cell, d, guard, parts=2)
    parts = [_run(cell, V.graph_slice(d, g), guard, eid0=g * d.n * d.k) for g in range(d.b)]
    return {name: torch.cat([q[name] for q in parts], dim=1 if name.lower().endswith("_t") else 0) for name in parts[0]}


@pytest.mark.parametrize("cid", [c.id for c in V.RUN])
def test_cell_matches_the_float64_specification(cid):
    cell, d = V.BY_ID[cid], V.prepare(cid)
    ref, aux = V.reference(cid)
    guard = Guard()
    got = _run(cell, d, guard)
    transposes = {name: got.pop(name) for name in ("gPi_T", "gPj_T") if name in got}
    assert set(got) == set(ref), set(got) ^ set(ref)
    guard.assert_slack_intact(cid)
    worst = 0.0
    for name, want in ref.items():
        have = got[name].detach().double().cpu()
        assert have.shape == want.shape, (name, have.shape, want.shape)
        assert not bool(torch.isnan(have).any()), (name, "NaN: an element the kernel did not write")
        err = float((have - want).abs().max())
        bar = V.bar(cid, name)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))    # (bar 0: a tensor that is zero throughout)
        worst = max(worst, ratio)
        print(f"{cid} {name}: err {err:.3e} bar {bar:.3e} ratio {ratio:.3f}")
        assert err <= bar, (name, err, bar)
        zero = want == 0
        assert bool((have[zero] == 0).all()), (name, "a structural zero of the specification is not an exact zero")
    print(f"RATIO {cell.entry} {cell.t} {cid} {worst:.3f}")
    for name, t in transposes.items():                                           # (H, nodes): bit-equal to the (nodes, H) sums
        assert torch.equal(t, got[name[:-2]].t()), name
    if cell.entry == "fwd" and "no_w3" in cell.p["opts"]:                       # no coors_mlp: the coordinate columns are zeros, and
        assert not bool(got["ws_wrel"].any()) and "coors_out" not in got        # `run_fwd` saw the coordinates themselves untouched
    # the same bits on a second run
    guard2 = Guard()
    again = _run(cell, d, guard2)
    for name in got:
        assert torch.equal(got[name], again[name]), (name, "not reproducible")
    # dropout: one call per graph with the row offset = the one call, bit for bit
    if cell.p["drop"] == "split":
        guard3 = Guard()
        split = _by_graph(cell, d, guard3)
        guard3.assert_slack_intact(cid)
        for name in got:
            assert torch.equal(got[name], split[name]), (name, "the call per graph differs from the one call")


@pytest.mark.parametrize("cid", [c.id for c in V.REFUSED])
def test_refusal_raises_the_restated_code_and_writes_nothing(cid):
    from egnn_pytorch_amd import _abi
    cell, d = V.BY_ID[cid], V.prepare(cid)
    guard = Guard()
    with pytest.raises(_abi.EGNNHipError, match=rf"failed with code {cell.expect}:"):
        _run(cell, d, guard)
    torch.cuda.synchronize()
    assert guard.bufs or cell.entry == "silu"                                     # (silu is in place: `run_silu` compares Z itself)
    guard.assert_nothing_written(cid)
    guard.assert_slack_intact(cid)
