"""`GraphSegments.softmax` / `logsumexp` / `attention_pool` on the MI355X (csrc/segment_softmax.hip).

Bit anchors that follow from the documented order: with scores = 0 the pool IS `reduce(values, "mean")`, softmax is
1 / n correctly rounded and logsumexp is log(n); with one score 0 per graph and head and the rest -inf softmax is one-hot and the pool
returns that row of `values`.  A graph gives the same bits alone, inside the batch, inside the reversed batch and twice in a row; sliced,
column-offset and transposed views give the bits of the contiguous call, on the 16-byte and the scalar path alike.  NaN, -inf and empty
graphs behave as torch does on the rows of each graph, and no output holds a NaN its inputs do not explain (the allocator is poisoned).

Accuracy, against float64 torch on the CPU, with bars that are derived, not fitted.  u = 2^-24 / 2^-53, a = max_j |x_j - m| of the
column, depth = tests/_segment_reduce_order.depth, E = 1: the maximum ulp error of expf and exp in the accuracy table of the HIP math API
(ROCm documentation, "HIP math API": expf 1 ULP, exp 1 ULP).  A weight is exp(fl(x - m)) / l: the subtraction moves the argument by at
most u a (relative change a u of the exponential), exp adds E u, l carries the same two for every term plus depth u of its summation,
the division one rounding:
    softmax         |y - w|     <= (depth(n, D) + 2 E + 2 a + 1) u w x 1.01
    attention_pool  |out - ref| <= (depth(n, H Dv) + depth(n, H) + 2 E + 2 a + 2) u sum_i w_i |v_i| x 1.01
    logsumexp       |lse - ref| <= (depth(n, D) + E + a + 2) u x 1.01 + u |ref|
(1.01: second-order terms, as in tests/test_gpu_segment_reduce.py).  One more fp32 cell has scores spanning +-200, where weights
underflow: the same bars plus the smallest normal float32 as an absolute floor (denormal handling is not pinned).

Measured on one MI355X, worst error / bar over the grid (each cell prints its own): softmax 0.48 in float32 and 0.77 in float64,
attention_pool 0.22 and 0.29, logsumexp 0.62 and 0.99.  The float64 logsumexp figure is the reference's own last rounding: at
|lse| ~ 10 ... 17 the kernel's result and torch's float64 one each lie within half an ulp of the exact value (numpy longdouble), on
opposite sides, and the bar grants u |ref| once.  The +-200 cell: softmax 0.46, logsumexp 0.36, attention_pool 0.01."""
import math

import pytest
import torch

from tests import _segment_reduce_order as order
from tests.test_gpu_segment_reduce import DTYPES, SIZE_SETS, UNIT, _offsets, _same_bits, _seg, _views

pytestmark = pytest.mark.gpu

R = order.R
DS = (1, 3, 4, 5, 64, 130)
POOLS = ((1, 1), (1, 3), (3, 5), (4, 16), (2, 65))
E = 1                                                    # ulp: expf / exp, HIP math API accuracy table
TINY = 2.0 ** -126
WORST = {}


def _scores(t, d, dtype, s, seed=0):
    g = torch.Generator().manual_seed(31 * t + d + seed)
    return (torch.randn(t, d, generator=g, dtype=torch.float64) * s).to(dtype)


def _values(t, h, dv, dtype, seed=0):
    g = torch.Generator().manual_seed(17 * t + 5 * h + dv + seed)
    v = torch.randn(t, h, dv, generator=g, dtype=torch.float64) * torch.exp(torch.rand(t, h, dv, generator=g, dtype=torch.float64) * 8 - 4)
    return v.to(dtype)


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return WORST[key]


def _softmax_cell(sizes, x, dtype, floor=0.0):
    """softmax and logsumexp of x (T, D) against float64 torch at the derived bars -> worst error / bar of each"""
    seg, u, d = _seg(sizes), UNIT[dtype], x.shape[1]
    y, lse = seg.softmax(x.cuda()), seg.logsumexp(x.cuda())
    assert y.shape == x.shape and lse.shape == (len(sizes), d) and y.dtype == lse.dtype == dtype
    assert _same_bits(y, seg.softmax(x.cuda())) and _same_bits(lse, seg.logsumexp(x.cuda()))
    y, lse, xd = y.cpu().double(), lse.cpu().double(), x.double()
    assert not torch.isnan(y).any() and not torch.isnan(lse).any()                          # (poisoned allocator: every element written)
    worst_y = worst_l = 0.0
    for gi, (a, b) in enumerate(zip(_offsets(sizes), _offsets(sizes)[1:])):
        n = b - a
        if n == 0:
            assert bool((lse[gi] == -math.inf).all())
            continue
        w, ref = torch.softmax(xd[a:b], 0), torch.logsumexp(xd[a:b], 0)
        spread = (xd[a:b] - xd[a:b].amax(0, keepdim=True)).abs().amax(0)
        dep = order.depth(n, d)
        bar_y = (dep + 2 * E + 2 * spread + 1) * u * w * 1.01 + floor
        bar_l = (dep + E + spread + 2) * u * 1.01 + u * ref.abs()
        ry, rl = ((y[a:b] - w).abs() / bar_y).max().item(), ((lse[gi] - ref).abs() / bar_l).max().item()
        worst_y, worst_l = max(worst_y, ry), max(worst_l, rl)
    return worst_y, worst_l


def _pool_ref(sizes, s, v):
    """float64 torch on the rows of every graph: (ref (G, H, Dv), sum_i w_i |v_i| (G, H, Dv), a (G, H))"""
    sd, vd = s.double(), v.double()
    ref, mag, spread = [], [], []
    for a, b in zip(_offsets(sizes), _offsets(sizes)[1:]):
        if b == a:
            ref.append(torch.zeros(v.shape[1:], dtype=torch.float64))
            mag.append(torch.zeros(v.shape[1:], dtype=torch.float64))
            spread.append(torch.zeros(s.shape[1], dtype=torch.float64))
            continue
        w = torch.softmax(sd[a:b], 0)[..., None]
        ref.append((w * vd[a:b]).sum(0))
        mag.append((w * vd[a:b].abs()).sum(0))
        spread.append((sd[a:b] - sd[a:b].amax(0, keepdim=True)).abs().amax(0))
    return torch.stack(ref), torch.stack(mag), torch.stack(spread)


def _pool_cell(sizes, s, v, dtype, floor=0.0):
    seg, u = _seg(sizes), UNIT[dtype]
    h, dv = v.shape[1:]
    out = seg.attention_pool(s.cuda(), v.cuda())
    assert out.shape == (len(sizes), h, dv) and out.dtype == dtype and _same_bits(out, seg.attention_pool(s.cuda(), v.cuda()))
    out = out.cpu().double()
    assert not torch.isnan(out).any()
    ref, mag, spread = _pool_ref(sizes, s, v)
    worst = 0.0
    for gi, n in enumerate(sizes):
        if n == 0:
            assert not out[gi].any()
            continue
        bar = (order.depth(n, h * dv) + order.depth(n, h) + 2 * E + 2 * spread[gi][:, None] + 2) * u * mag[gi] * 1.01 + floor
        worst = max(worst, ((out[gi] - ref[gi]).abs() / bar).max().item())
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_softmax_and_logsumexp_within_their_derived_bars(name, d, dtype):
    sizes = SIZE_SETS[name]
    for s in (1, 8):
        wy, wl = _softmax_cell(sizes, _scores(sum(sizes), d, dtype, s), dtype)
        print(f"{name} D={d} {dtype} s={s}: worst error / bar softmax {wy:.3f} logsumexp {wl:.3f}; so far "
              f"{_note(('softmax', dtype), wy):.3f} {_note(('lse', dtype), wl):.3f}")
        assert wy <= 1 and wl <= 1, (s, wy, wl)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("h, dv", POOLS)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_attention_pool_within_its_derived_bar(name, h, dv, dtype):
    sizes = SIZE_SETS[name]
    t = sum(sizes)
    for s in (1, 8):
        w = _pool_cell(sizes, _scores(t, h, dtype, s), _values(t, h, dv, dtype), dtype)
        print(f"{name} H={h} Dv={dv} {dtype} s={s}: worst error / bar {w:.3f}; so far {_note(('pool', dtype), w):.3f}")
        assert w <= 1, (s, w)


def test_scores_spanning_400_underflow_within_the_same_bars_and_a_floor():
    """fp32, scores uniform in +-200: most weights of a graph lie below the smallest normal number"""
    sizes = SIZE_SETS["mixed"] + SIZE_SETS["chunk_edges"]
    t, g = sum(sizes), torch.Generator().manual_seed(5)
    for d in (3, 64):
        x = ((torch.rand(t, d, generator=g, dtype=torch.float64) - 0.5) * 400).float()
        wy, wl = _softmax_cell(sizes, x, torch.float32, floor=TINY)
        print(f"+-200 D={d}: worst error / bar softmax {wy:.3f} logsumexp {wl:.3f}")
        assert wy <= 1 and wl <= 1, (d, wy, wl)
    for h, dv in ((3, 5), (4, 16)):
        s = ((torch.rand(t, h, generator=g, dtype=torch.float64) - 0.5) * 400).float()
        w = _pool_cell(sizes, s, _values(t, h, dv, torch.float32), torch.float32, floor=TINY)
        print(f"+-200 H={h} Dv={dv}: worst error / bar {w:.3f}")
        assert w <= 1, (h, dv, w)


# ------------------------------------------------------------------------------------------------ bit anchors
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_zero_scores_give_the_mean_one_over_n_and_log_n(name, dtype):
    sizes = SIZE_SETS[name]
    seg, t, u = _seg(sizes), sum(sizes), UNIT[dtype]
    n_of = torch.tensor(sizes, dtype=torch.float64)
    for h, dv in POOLS:
        v = _values(t, h, dv, dtype, seed=1).cuda()
        out = seg.attention_pool(torch.zeros(t, h, dtype=dtype, device="cuda"), v)
        assert torch.equal(out.reshape(len(sizes), h * dv), seg.reduce(v.reshape(t, h * dv), "mean")), (h, dv)
    for d in DS:
        zero = torch.zeros(t, d, dtype=dtype, device="cuda")
        want = (torch.ones((), dtype=dtype) / n_of.clamp(min=1).to(dtype))[seg.segment_of.long().cpu()]      # 1 / n, correctly rounded
        assert torch.equal(seg.softmax(zero).cpu(), want[:, None].expand(t, d)), d
        lse = seg.logsumexp(zero).cpu().double()
        for gi, n in enumerate(sizes):
            ref = math.log(n) if n else -math.inf
            # m = 0 and l = n are exact: what is left is the device's log (1 ulp in the same table) and its rounding
            assert bool(((lse[gi] - ref).abs() <= 2 * u * abs(ref)).all()) if n else bool((lse[gi] == ref).all()), (d, gi, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_one_finite_score_gives_one_hot_weights_and_that_row_of_values(name, dtype):
    sizes = SIZE_SETS[name]
    seg, t, off = _seg(sizes), sum(sizes), _offsets(sizes)
    g = torch.Generator().manual_seed(len(sizes))
    for h, dv in POOLS:
        pick = torch.stack([a + torch.randint(0, max(b - a, 1), (h,), generator=g) for a, b in zip(off, off[1:])])   # (G, H) rows
        live = torch.tensor(sizes) > 0
        s = torch.full((t, h), -math.inf, dtype=dtype)
        s[pick[live], torch.arange(h)] = 0
        v = _values(t, h, dv, dtype, seed=2)
        y = seg.softmax(s.cuda()).cpu()
        assert torch.equal(y, (s == 0).to(dtype)), (h, dv)
        out = seg.attention_pool(s.cuda(), v.cuda()).cpu()
        want = torch.zeros(len(sizes), h, dv, dtype=dtype)
        want[live] = v[pick[live], torch.arange(h)]
        assert torch.equal(out, want), (h, dv)
        assert torch.equal(seg.logsumexp(s.cuda()).cpu(), torch.where(live[:, None], 0.0, -math.inf).to(dtype).expand(-1, h))


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_a_graph_gives_the_same_bits_alone_in_the_batch_and_in_the_reversed_batch(name, dtype):
    sizes = SIZE_SETS[name]
    off, t = _offsets(sizes), sum(sizes)
    seg, rseg = _seg(sizes), _seg(tuple(reversed(sizes)))
    singles = {n: _seg((n,)) for n in set(sizes)}
    spans = list(zip(off, off[1:]))

    def rev(x):
        return torch.cat([x[a:b] for a, b in reversed(spans)])

    for d in DS:
        x = _scores(t, d, dtype, 3, seed=1).cuda()
        y, lse = seg.softmax(x), seg.logsumexp(x)
        assert torch.equal(y, torch.cat([singles[b - a].softmax(x[a:b]) for a, b in spans])), d
        assert torch.equal(lse, torch.cat([singles[b - a].logsumexp(x[a:b]) for a, b in spans])), d
        assert torch.equal(rev(y), rseg.softmax(rev(x))) and torch.equal(lse, rseg.logsumexp(rev(x)).flip(0)), d
        assert torch.equal(y, seg.softmax(x)) and torch.equal(lse, seg.logsumexp(x)), d
    for h, dv in POOLS:
        s, v = _scores(t, h, dtype, 3, seed=2).cuda(), _values(t, h, dv, dtype, seed=3).cuda()
        out = seg.attention_pool(s, v)
        assert torch.equal(out, torch.cat([singles[b - a].attention_pool(s[a:b], v[a:b]) for a, b in spans])), (h, dv)
        assert torch.equal(out, rseg.attention_pool(rev(s), rev(v)).flip(0)) and torch.equal(out, seg.attention_pool(s, v)), (h, dv)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DS)
def test_softmax_layouts_give_the_bits_of_the_contiguous_call(d, dtype):
    """D = 4, 64: the contiguous call moves 16 bytes at a time, the column slice and the one-element offset take the scalar path"""
    sizes = SIZE_SETS["chunk_edges"] + (0, 3)
    seg = _seg(sizes)
    x = _scores(sum(sizes), d, dtype, 3, seed=4).cuda()
    assert x.data_ptr() % 16 == 0
    y, lse = seg.softmax(x), seg.logsumexp(x)
    for what, v in _views(x):
        assert torch.equal(v, x)
        assert torch.equal(seg.softmax(v), y) and torch.equal(seg.logsumexp(v), lse), what


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("h, dv", POOLS)
def test_pool_layouts_give_the_bits_of_the_contiguous_call(h, dv, dtype):
    """(4, 16): the contiguous values are loaded 16 bytes at a time, their column slice and one-element offset by scalar loads"""
    sizes = SIZE_SETS["chunk_edges"] + (0, 3)
    seg, t = _seg(sizes), sum(sizes)
    s, v = _scores(t, h, dtype, 3, seed=5).cuda(), _values(t, h, dv, dtype, seed=6).cuda()
    out = seg.attention_pool(s, v)
    gr = _values(len(sizes), h, dv, dtype, seed=7).cuda()
    ds, dvv = torch.autograd.grad(seg.attention_pool(s.requires_grad_(True), v.requires_grad_(True)), (s, v), gr)
    s, v = s.detach(), v.detach()
    for (what, sv), (_, vv) in zip(_views(s), _views(v.reshape(t, h * dv))):
        v3 = vv.unflatten(1, (h, dv))
        assert torch.equal(sv, s) and torch.equal(v3, v)
        assert torch.equal(seg.attention_pool(sv, v3), out), what
        sv, v3 = sv.detach().requires_grad_(True), v3.detach().requires_grad_(True)
        got = torch.autograd.grad(seg.attention_pool(sv, v3), (sv, v3), gr)
        assert torch.equal(got[0], ds) and torch.equal(got[1], dvv), what
    if h == 1:                                                                               # the shorthand: scores (T,), values (T, Dv)
        assert torch.equal(seg.attention_pool(s[:, 0], v[:, 0]), out[:, 0])


# ------------------------------------------------------------------------------------------------ NaN, -inf, empty graphs
@pytest.mark.parametrize("dtype", DTYPES + (torch.float16, torch.bfloat16), ids=("f32", "f64", "f16", "bf16"))
def test_nan_and_minus_infinity_stay_in_their_graph_and_column(dtype):
    sizes = (0, 1, 5, 0, 64, 3, R + 2, 0)
    seg, cpu, t, off = _seg(sizes), _seg(sizes, "cpu"), sum(sizes), _offsets(sizes)
    h, dv = 3, 5
    s = _scores(t, h, torch.float64, 2, seed=8).to(dtype)
    s[off[4] + 7, 1] = math.nan                                                              # graph 4 (64 rows), head 1
    s[off[6] + R + 1, 2] = math.nan                                                          # graph 6, in its second chunk, head 2
    s[off[2]:off[3], 0] = -math.inf                                                          # graph 2: head 0 is all -inf
    s[off[4] + 1, 0] = -math.inf                                                             # -inf next to finite scores: weight 0
    v = _values(t, h, dv, torch.float64, seed=9).clamp(-50, 50).to(dtype)
    y, lse, out = seg.softmax(s.cuda()).cpu(), seg.logsumexp(s.cuda()).cpu(), seg.attention_pool(s.cuda(), v.cuda()).cpu()
    assert y.dtype == lse.dtype == out.dtype == dtype
    bad = torch.zeros(len(sizes), h, dtype=torch.bool)
    bad[4, 1] = bad[6, 2] = bad[2, 0] = True
    assert torch.equal(torch.isnan(y), bad[seg.segment_of.long().cpu()])                      # exactly those (graph, column)s, every row
    assert torch.equal(torch.isnan(out), bad[:, :, None].expand(-1, -1, dv))
    want_lse = bad.clone()
    want_lse[2, 0] = False
    assert torch.equal(torch.isnan(lse), want_lse) and lse[2, 0] == -math.inf
    empty = torch.tensor(sizes) == 0
    assert bool((lse[empty] == -math.inf).all()) and not out[empty].any() and y[off[4] + 1, 0] == 0
    # elsewhere: what torch gives on the rows of each graph (the CPU path), at the precision of the dtype
    tol = {torch.float32: 1e-5, torch.float64: 1e-13, torch.float16: 2e-3, torch.bfloat16: 2e-2}[dtype]
    for got, want in ((y, cpu.softmax(s.double())), (lse, cpu.logsumexp(s.double())), (out, cpu.attention_pool(s.double(), v.double()))):
        fin = torch.isfinite(want)
        assert torch.equal(fin, torch.isfinite(got))
        assert bool(((got.double() - want)[fin].abs() <= tol * (1 + want[fin].abs())).all())


# ------------------------------------------------------------------------------------------------ gradients
def _distinct(t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(t * d, generator=g).double().reshape(t, d) / 7 - 2).cuda().requires_grad_(True)


@pytest.mark.parametrize("what", ("softmax", "logsumexp", "attention_pool"))
def test_gradcheck_and_gradgradcheck_in_float64(what):
    seg = _seg((5, 0, 1, 6))
    if what == "attention_pool":
        fn = lambda a, b: seg.attention_pool(a, b.reshape(12, 2, 3))
        inputs = (_distinct(12, 2, 1), _distinct(12, 6, 2))
    else:
        live = torch.tensor(seg.sizes, device="cuda") > 0    # (the empty graph's logsumexp is -inf: no finite difference to take of it)
        fn = seg.softmax if what == "softmax" else (lambda a: seg.logsumexp(a)[live])
        inputs = (_distinct(12, 3, 3),)
    assert torch.autograd.gradcheck(fn, inputs)
    assert torch.autograd.gradgradcheck(lambda *a: fn(*a) ** 2, inputs)


def test_fp32_gradients_against_the_float64_cpu_path():
    """loss = sum(w * f(x)); the bar of the packed-layer tests: error <= 1e-4 max|grad| per tensor, every gradient finite"""
    sizes = (0, 1, 5, 0, 64, 3, R + 1)
    seg, cpu = _seg(sizes), _seg(sizes, "cpu")
    t, live = sum(sizes), torch.tensor(sizes) > 0

    def grads(s_, fn, inputs, w, dev, dt):
        inputs = [i.to(dev, dt).requires_grad_(True) for i in inputs]
        (fn(s_, *inputs) * w.to(dev, dt)).sum().backward()
        assert all(torch.isfinite(i.grad).all() for i in inputs)
        return [i.grad.double().cpu() for i in inputs]

    def check(fn, inputs, w, what):
        got, want = grads(seg, fn, inputs, w, "cuda", torch.float32), grads(cpu, fn, inputs, w, "cpu", torch.float64)
        for a, b in zip(got, want):
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            print(f"{what}: gradient error / max|grad| {err / scale:.3e} (bar 1e-4)")
            assert scale > 0 and err <= 1e-4 * scale, (what, err, scale)

    g = torch.Generator().manual_seed(4)
    for d in (3, 64):
        x = _scores(t, d, torch.float32, 2, seed=9)
        check(lambda s_, v: s_.softmax(v), [x], torch.randn(t, d, generator=g), f"softmax D={d}")
        check(lambda s_, v: s_.logsumexp(v)[live.to(v.device)], [x], torch.randn(int(live.sum()), d, generator=g), f"logsumexp D={d}")
    for h, dv in ((2, 3), (4, 16), (2, 65)):
        s, v = _scores(t, h, torch.float32, 2, seed=10), torch.randn(t, h, dv, generator=g)
        check(lambda s_, a, b: s_.attention_pool(a, b), [s, v], torch.randn(len(sizes), h, dv, generator=g), f"attention_pool H={h} Dv={dv}")


def test_the_pooled_row_of_an_empty_graph_has_zero_gradient():
    seg = _seg((0, 3, 0))
    s = torch.randn(3, 2, device="cuda", requires_grad=True)
    v = torch.randn(3, 2, 4, device="cuda", requires_grad=True)
    out = seg.attention_pool(s, v)
    assert not out[0].any() and not out[2].any()
    w = torch.randn(3, 2, 4, device="cuda")
    (out * w).sum().backward()
    assert torch.isfinite(s.grad).all() and torch.isfinite(v.grad).all() and v.grad.any() and s.grad.any()
    w2 = w.clone()
    w2[0], w2[2] = 7.0, -3.0                                                                 # the empty graphs' cotangent reaches nothing
    s2, v2 = s.detach().requires_grad_(True), v.detach().requires_grad_(True)
    (seg.attention_pool(s2, v2) * w2).sum().backward()
    assert torch.equal(s2.grad, s.grad) and torch.equal(v2.grad, v.grad)


def test_a_batch_without_a_node_is_handled_on_the_host():
    none = _seg((0, 0))
    z = torch.zeros(0, 3, device="cuda")
    assert none.softmax(z).shape == (0, 3) and none.softmax(z).is_cuda
    lse = none.logsumexp(z)
    assert lse.shape == (2, 3) and lse.is_cuda and bool((lse == -math.inf).all())
    out = none.attention_pool(torch.zeros(0, 2, device="cuda"), torch.zeros(0, 2, 4, device="cuda"))
    assert out.shape == (2, 2, 4) and out.is_cuda and not out.any()
