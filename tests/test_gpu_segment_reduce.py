"""`GraphSegments.reduce` / `broadcast` / `center` on the MI355X (csrc/segment_reduce.hip).

Every cell of sizes x D x dtype: `sum` equals the numpy restatement of the documented order (tests/_segment_reduce_order.py) element for
element and lies within the standard bound of that order, depth(n, D) u sum|x_i| x 1.01 (u = 2^-24 / 2^-53; `mean` one rounding more),
of the exact sum -- the error is measured exactly, as fsum(x_1, ..., x_n, -got); `max` / `min` equal torch.amax / amin with numpy's
first-occurrence argmax as the winning row, on tied values and with NaN planted; a graph gives the same bits alone, inside the batch and
inside the reversed batch, and twice in a row; sliced, transposed and offset views give the bits of the contiguous call, on the 16-byte
and the scalar load path alike; no output holds a NaN the inputs do not (the allocator is poisoned).  Then the gradients (gradcheck /
gradgradcheck in float64, fp32 against float64 at the forward's bar) and a packed layer into the readout into a loss, against the padded
route, create_graph=True included.

Measured on one MI355X, worst error / bar over the grid (each cell prints its own): sum 0.64 in float32 and 0.63 in float64, mean 0.60
and 0.59, all among the 300 graphs of 1 ... 7 rows; the other size sets stay below 0.46."""
import math

import numpy as np
import pytest
import torch

from tests import _segment_reduce_order as order
from tests._util import ATOL

pytestmark = pytest.mark.gpu

R = order.R
SIZE_SETS = {
    "mixed": (0, 1, 5, 0, 64, 3),
    "chunk_edges": (R - 1, R, R + 1, 2 * R + 1),
    "one_long": (1000,),
    "many_small": tuple(i % 7 + 1 for i in range(300)),
    "empty_ends": (0, 0, 9, R + 2, 0),
}
DS = (1, 3, 4, 5, 64, 130, 257)
DTYPES = (torch.float32, torch.float64)
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
WORST = {}


def _seg(sizes, device="cuda"):
    from egnn_pytorch_amd import GraphSegments
    return GraphSegments.from_sizes(list(sizes), device=device)


def _data(sizes, d, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * len(sizes) + d + seed)
    t = sum(sizes)
    x = torch.randn(t, d, generator=g, dtype=torch.float64) * torch.exp(torch.rand(t, d, generator=g, dtype=torch.float64) * 8 - 4)
    return x.to(dtype)


def _tied(sizes, d, dtype, nan):
    """values from five levels (ties everywhere); `nan`: a NaN in about one element of forty"""
    g = torch.Generator().manual_seed(77 * len(sizes) + d)
    t = sum(sizes)
    levels = torch.tensor([-2.5, -0.0, 0.0, 1.0, 3.75], dtype=dtype)
    x = levels[torch.randint(0, 5, (t, d), generator=g)]
    if nan:
        x = torch.where(torch.rand(t, d, generator=g) < 0.025, torch.full_like(x, math.nan), x)
    return x


def _offsets(sizes):
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    return off


def _winners(x, sizes, is_max):
    """numpy: first-occurrence argmax / argmin (a NaN is the extreme, its first occurrence wins) -> values, rows of the batch"""
    xn = x.numpy()
    vals, rows = [], []
    for a, b in zip(_offsets(sizes), _offsets(sizes)[1:]):
        at = np.argmax(xn[a:b], 0) if is_max else np.argmin(xn[a:b], 0)
        rows.append(at + a)
        vals.append(torch.amax(x[a:b], 0) if is_max else torch.amin(x[a:b], 0))
    return torch.stack(vals), torch.from_numpy(np.stack(rows)).to(torch.int32)


def _same_bits(a, b):
    """equal as bit patterns where both hold numbers, NaN where either holds one"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _extreme(seg, x, op):
    from egnn_pytorch_amd import _ops
    return _ops.segment_reduce(x, seg, op)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_sum_and_mean_follow_the_documented_order_within_its_bound(name, d, dtype):
    sizes = SIZE_SETS[name]
    seg = _seg(sizes)
    x = _data(sizes, d, dtype)
    got = seg.reduce(x.cuda(), "sum")
    mean = seg.reduce(x.cuda(), "mean")
    assert got.shape == mean.shape == (len(sizes), d) and got.dtype == mean.dtype == dtype
    got, mean = got.cpu(), mean.cpu()
    assert not torch.isnan(got).any() and not torch.isnan(mean).any()                       # (poisoned allocator: every element written)
    want = order.batch_sum(x.numpy(), sizes)
    assert np.array_equal(got.numpy(), want), f"sum differs from the documented order in {(got.numpy() != want).sum()} elements"
    assert torch.equal(got, seg.reduce(x.cuda(), "sum").cpu()) and torch.equal(mean, seg.reduce(x.cuda(), "mean").cpu())
    # the bound of that order against the exact sum
    u, xd = UNIT[dtype], x.double()
    worst_s = worst_m = 0.0
    for gi, (a, b) in enumerate(zip(_offsets(sizes), _offsets(sizes)[1:])):
        n = b - a
        if n == 0:
            assert not got[gi].any() and not mean[gi].any()
            continue
        dep = order.depth(n, d)
        cols = xd[a:b].t().tolist()
        for c in range(d):
            mag = math.fsum(abs(v) for v in cols[c])
            err_s = abs(math.fsum(cols[c] + [-float(got[gi, c])]))
            err_m = abs(math.fsum(cols[c] + [-float(mean[gi, c])] * n)) / n
            bar_s, bar_m = dep * u * mag * 1.01, (dep + 1) * u * mag / n * 1.01
            assert err_s <= bar_s and err_m <= bar_m, (gi, c, n, err_s, bar_s, err_m, bar_m)
            worst_s, worst_m = max(worst_s, err_s / bar_s), max(worst_m, err_m / bar_m)
    key = str(dtype)
    WORST[key] = (max(WORST.get(key, (0, 0))[0], worst_s), max(WORST.get(key, (0, 0))[1], worst_m))
    print(f"{name} D={d} {key}: worst error / bar sum {worst_s:.3f} mean {worst_m:.3f}; so far {WORST[key][0]:.3f} {WORST[key][1]:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_max_and_min_values_and_winning_rows(name, d, dtype):
    sizes = SIZE_SETS[name]
    if 0 in sizes:
        with pytest.raises(ValueError, match="empty graph"):
            _seg(sizes).reduce(torch.zeros(sum(sizes), d, dtype=dtype, device="cuda"), "max")
        sizes = tuple(n for n in sizes if n)
    seg = _seg(sizes)
    for x in (_data(sizes, d, dtype), _tied(sizes, d, dtype, False), _tied(sizes, d, dtype, True)):
        for op in ("max", "min"):
            vals, rows = _extreme(seg, x.cuda(), op)
            want_v, want_r = _winners(x, sizes, op == "max")
            assert rows.dtype == torch.int32 and torch.equal(rows.cpu(), want_r), (op, int((rows.cpu() != want_r).sum()))
            assert _same_bits(vals.cpu(), want_v), op
            assert _same_bits(seg.reduce(x.cuda(), op).cpu(), want_v)
            assert bool((torch.isnan(vals.cpu()) == torch.isnan(want_v)).all())
            again = _extreme(seg, x.cuda(), op)
            assert _same_bits(again[0], vals) and torch.equal(again[1], rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_a_graph_gives_the_same_bits_alone_in_the_batch_and_in_the_reversed_batch(name, d, dtype):
    sizes = SIZE_SETS[name]
    off = _offsets(sizes)
    seg, x = _seg(sizes), _data(sizes, d, dtype, seed=1).cuda()
    live = tuple(n for n in sizes if n)
    xt = _tied(live, d, dtype, True).cuda()                                                   # (the same rows: empty graphs hold none)
    rev_sizes = tuple(reversed(sizes))
    rseg = _seg(rev_sizes)
    pieces = [x[a:b] for a, b in zip(off, off[1:])]
    xrev = torch.cat(list(reversed(pieces)))
    singles = {n: _seg((n,)) for n in set(sizes)}
    for op in ("sum", "mean"):
        batch = seg.reduce(x, op)
        alone = torch.cat([singles[b - a].reduce(x[a:b], op) for a, b in zip(off, off[1:])])
        assert torch.equal(batch, alone), op
        assert torch.equal(batch, rseg.reduce(xrev, op).flip(0)), op
    lseg, loff = _seg(live), _offsets(live)
    lrev = _seg(tuple(reversed(live)))
    tpieces = [xt[a:b] for a, b in zip(loff, loff[1:])]
    trev = torch.cat(list(reversed(tpieces)))
    roff = torch.tensor(_offsets(tuple(reversed(live)))[:-1], dtype=torch.int32, device="cuda").flip(0)[:, None]
    base = torch.tensor(loff[:-1], dtype=torch.int32, device="cuda")[:, None]
    for op in ("max", "min"):
        vals, rows = _extreme(lseg, xt, op)
        one = [_extreme(singles[b - a], xt[a:b], op) for a, b in zip(loff, loff[1:])]
        assert _same_bits(vals, torch.cat([v for v, _ in one])) and torch.equal(rows - base, torch.cat([r for _, r in one])), op
        rv, rr = _extreme(lrev, trev, op)
        assert _same_bits(vals, rv.flip(0)) and torch.equal(rows - base, rr.flip(0) - roff), op


def _views(x):
    """x (T, D) on the device -> [(what, a view holding the same values)]"""
    t, d = x.shape
    wide = torch.randn(t, d + 3, dtype=x.dtype, device=x.device)
    wide[:, 1:1 + d] = x
    tall = torch.randn(d + 2, t, dtype=x.dtype, device=x.device)
    tall[1:1 + d] = x.t()
    out = [("column slice", wide[:, 1:1 + d]), ("transposed, then sliced", tall.t()[:, 1:1 + d])]
    for what, elems in (("base offset by 16 bytes", 16 // x.element_size()), ("base offset by one element", 1)):
        buf = torch.randn(t * d + elems, dtype=x.dtype, device=x.device)
        buf[elems:] = x.reshape(-1)
        view = buf[elems:].view(t, d)
        assert view.data_ptr() - buf.data_ptr() == elems * x.element_size() and view.is_contiguous()
        out.append((what, view))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
def test_layouts_give_the_bits_of_the_contiguous_call(d, dtype):
    """D = 4, 64: the contiguous call loads 16 bytes at a time, the column slice and the one-element offset take the scalar loads"""
    sizes = SIZE_SETS["chunk_edges"] + (0, 3)
    seg = _seg(sizes)
    x = _data(sizes, d, dtype, seed=2).cuda()
    assert x.data_ptr() % 16 == 0
    want = {op: seg.reduce(x, op) for op in ("sum", "mean")}
    lseg = _seg(tuple(n for n in sizes if n))
    xt = _tied(lseg.sizes, d, dtype, True).cuda()
    wext = {op: _extreme(lseg, xt, op) for op in ("max", "min")}
    for (what, v), (_, vt) in zip(_views(x), _views(xt)):
        assert torch.equal(v, x)
        for op in ("sum", "mean"):
            assert torch.equal(seg.reduce(v, op), want[op]), (what, op)
        for op in ("max", "min"):
            vals, rows = _extreme(lseg, vt, op)
            assert _same_bits(vals, wext[op][0]) and torch.equal(rows, wext[op][1]), (what, op)


@pytest.mark.parametrize("dtype", DTYPES + (torch.float16, torch.bfloat16), ids=("f32", "f64", "f16", "bf16"))
def test_broadcast_scatter_gather_and_trailing_shapes(dtype):
    from egnn_pytorch_amd import _ops
    sizes = (0, 1, 5, 0, 64, 3, 300)
    seg, cpu = _seg(sizes), _seg(sizes, "cpu")
    g = torch.Generator().manual_seed(9)
    gr = torch.randn(len(sizes), 4, 3, generator=g).to(dtype)
    out = seg.broadcast(gr.cuda())
    assert out.shape == (sum(sizes), 4, 3) and out.dtype == dtype and torch.equal(out.cpu(), cpu.broadcast(gr))
    assert torch.equal(seg.broadcast(gr.cuda()[:, 0, 0]).cpu(), cpu.broadcast(gr[:, 0, 0]))
    x = torch.randn(sum(sizes), 4, 3, generator=g).to(dtype)
    for op in ("sum", "mean"):
        got = seg.reduce(x.cuda(), op)
        assert got.shape == (len(sizes), 4, 3) and got.dtype == dtype and not torch.isnan(got).any()
        torch.testing.assert_close(got.cpu().double(), cpu.reduce(x.double(), op), atol=0.3 if dtype in (torch.float16, torch.bfloat16) else 1e-4, rtol=0)
    cen = seg.center(x.cuda())
    assert cen.shape == x.shape and cen.dtype == dtype
    if dtype in DTYPES:
        live = tuple(n for n in sizes if n)
        lseg, lcpu = _seg(live), _seg(live, "cpu")
        x2 = x.reshape(len(x), -1)
        vals, rows = _ops.segment_reduce(x2.cuda(), lseg, "max")
        gg = torch.randn(len(live), 12, generator=g).to(dtype)
        sc = _ops.segment_scatter_rows(gg.cuda(), rows, lseg)
        want = torch.zeros_like(x2).scatter(0, rows.cpu().long(), gg)
        assert not torch.isnan(sc).any() and torch.equal(sc.cpu(), want)
        assert torch.equal(_ops.segment_gather_rows(x2.cuda(), rows, lseg), vals)
        assert torch.equal(lseg.reduce(x.cuda(), "max").cpu(), lcpu.reduce(x, "max"))


# ------------------------------------------------------------------------------------------------ gradients
def _distinct(t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(t * d, generator=g).double().reshape(t, d) / 7 - 2).cuda().requires_grad_(True)


@pytest.mark.parametrize("op", ("sum", "mean", "max", "min", "broadcast", "center"))
def test_gradcheck_and_gradgradcheck_in_float64(op):
    seg = _seg((5, 1, 6) if op in ("max", "min") else (5, 0, 1, 6))
    if op == "broadcast":
        fn, x = seg.broadcast, _distinct(seg.num_graphs, 3, 1)
    elif op == "center":
        fn, x = seg.center, _distinct(12, 3, 2)
    else:
        fn, x = (lambda t: seg.reduce(t, op)), _distinct(12, 3, 3)
    assert torch.autograd.gradcheck(fn, (x,))
    assert torch.autograd.gradgradcheck(lambda t: fn(t) ** 2, (x,))


@pytest.mark.parametrize("d", (3, 64))
def test_fp32_gradients_against_float64_at_the_forwards_bar(d):
    """loss = sum(w * f(x)): d/dx of sum / max / min / broadcast only moves values (exact); mean multiplies by the rounded 1 / n (two
    roundings of |w| / n); center adds the reduction of the cotangent: (depth + 3) u (|g_t| + sum|g| / n) x 1.01"""
    sizes = (0, 1, 5, 0, 64, 3, R + 1)
    seg, cpu = _seg(sizes), _seg(sizes, "cpu")
    live, lcpu = _seg(tuple(n for n in sizes if n)), _seg(tuple(n for n in sizes if n), "cpu")
    t, g = sum(sizes), torch.Generator().manual_seed(3 + d)
    x = torch.randperm(t * d, generator=g).float().reshape(t, d) / 64 - 3
    wg, wt = torch.randn(len(sizes), d, generator=g), torch.randn(t, d, generator=g)
    u = 2.0 ** -24

    def grad(s, fn, inp, w, dev):
        inp = inp.to(dev).requires_grad_(True)
        (fn(s, inp) * w.to(dev)).sum().backward()
        assert torch.isfinite(inp.grad).all()
        return inp.grad.double().cpu()

    for op in ("sum", "max", "min"):
        s, c, w = (seg, cpu, wg) if op == "sum" else (live, lcpu, wg[:live.num_graphs])
        f = lambda s_, v, op=op: s_.reduce(v, op)
        assert torch.equal(grad(s, f, x, w, "cuda"), grad(c, f, x.double(), w.double(), "cpu")), op
    f = lambda s_, v: s_.broadcast(v)
    gb, wb = grad(seg, f, wg, wt, "cuda"), grad(cpu, f, wg.double(), wt.double(), "cpu")
    mags = cpu.reduce(wt.double().abs(), "sum")
    deps = torch.tensor([order.depth(n, d) for n in sizes], dtype=torch.float64)[:, None]
    assert bool(((gb - wb).abs() <= deps * u * mags * 1.01).all())
    f = lambda s_, v: s_.reduce(v, "mean")
    gm, wm = grad(seg, f, x, wg, "cuda"), grad(cpu, f, x.double(), wg.double(), "cpu")
    assert bool(((gm - wm).abs() <= 2 * u * wm.abs() * 1.01).all())
    f = lambda s_, v: s_.center(v)
    gc, wc = grad(seg, f, x, wt, "cuda"), grad(cpu, f, x.double(), wt.double(), "cpu")
    n_of = torch.tensor(sizes, dtype=torch.float64).clamp(min=1)[:, None]
    bar = cpu.broadcast((deps + 3) * u * mags / n_of) + (cpu.broadcast(deps) + 3) * u * wt.double().abs()
    assert bool(((gc - wc).abs() <= bar * 1.01).all()), float(((gc - wc).abs() / bar).max())


def test_mean_of_an_empty_graph_has_finite_zero_gradients():
    seg = _seg((0, 3, 0))
    x = torch.randn(3, 5, device="cuda", requires_grad=True)
    w = torch.randn(3, 5, device="cuda")
    out = seg.reduce(x, "mean")
    assert not out[0].any() and not out[2].any()
    (out * w).sum().backward()
    assert torch.isfinite(x.grad).all() and torch.equal(x.grad, (w[1] * torch.tensor(1 / 3, device="cuda")).expand(3, 5))
    g = torch.randn(3, 5, device="cuda", requires_grad=True)
    (seg.reduce(seg.broadcast(g), "mean") * w).sum().backward()
    assert torch.isfinite(g.grad).all() and not g.grad[0].any() and not g.grad[2].any() and g.grad[1].any()


# ------------------------------------------------------------------------------------------------ a layer into the readout
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_packed_layer_into_the_readout_matches_the_padded_route(dtype):
    """packed k-NN EGNN -> reduce(node, "mean") -> squared loss -> backward, against the padded call with the prefix mask and a masked
    mean; then once more under create_graph=True with a gradient penalty on coors.  The bars of tests/test_gpu_packed_layers.py."""
    from egnn_pytorch_amd import EGNN
    f64 = dtype == torch.float64
    tol_f, tol_g = (1e-9, 1e-8) if f64 else (ATOL, 1e-4)
    sizes = (7, 1, 12, 5)
    torch.manual_seed(11)
    layer = EGNN(dim=32, num_nearest_neighbors=4)
    layer = (layer.double() if f64 else layer).cuda()
    seg = _seg(sizes)
    g = torch.Generator().manual_seed(12)
    t = sum(sizes)
    feats, coors = torch.randn(t, 32, generator=g).to(dtype).cuda(), torch.randn(t, 3, generator=g).to(dtype).cuda()
    target = torch.randn(len(sizes), 32, generator=g).to(dtype).cuda()
    mask = seg.prefix_mask()
    params = list(layer.parameters())

    def packed(f, x):
        node, co = layer(f, x, mask=seg)
        return seg.reduce(node, "mean"), co

    def padded(f, x):
        node, co = layer(seg.unpack(f), seg.unpack(x), mask=mask)
        m = mask[..., None].to(node.dtype)
        return (node * m).sum(1) / m.sum(1), seg.pack(co)

    def run(route, penalty):
        f, x = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
        pooled, co = route(f, x)
        loss = ((pooled - target) ** 2).sum() + (co ** 2).sum()
        if penalty:
            force = torch.autograd.grad(loss, x, create_graph=True)[0]
            loss = loss + (force ** 2).sum()
        grads = torch.autograd.grad(loss, [f, x] + params, allow_unused=True)
        return pooled.detach(), [torch.zeros_like(p) if g_ is None else g_ for p, g_ in zip([f, x] + params, grads)]

    names = ["feats", "coors"] + [k for k, _ in layer.named_parameters()]
    for penalty in (False, True):
        got, ggrads = run(packed, penalty)
        want, wgrads = run(padded, penalty)
        assert torch.isfinite(got).all() and float((got - want).abs().max()) <= tol_f
        live = 0
        for name, a, b in zip(names, ggrads, wgrads):
            scale, err = float(b.abs().max()), float((a - b).abs().max())
            print(f"readout {dtype} penalty={penalty}: d/d {name} error / scale {err / max(scale, 1e-30):.3e} (bar {tol_g:g})")
            assert torch.isfinite(a).all() and err <= tol_g * max(scale, 1e-30), (name, err, scale)
            live += scale > 0
        assert live >= 6
