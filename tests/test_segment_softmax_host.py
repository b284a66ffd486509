"""`GraphSegments.softmax` / `logsumexp` / `attention_pool` without a GPU: the CPU path against torch on the rows of every graph (NaN,
-inf and empty graphs included), autograd to second order, the refusals by type and message, and the C entries of
csrc/segment_softmax.hip (declared, bound, exported; `_f64` is `_f32` with double for float; every argument check answers before any
launch, with made-up pointers)."""
import math
import os

import pytest
import torch

from egnn_pytorch_amd import GraphSegments, _abi
from tests import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 5, 0, 64, 3)
ENTRIES = ("egnn_segment_softmax_stats_f32", "egnn_segment_softmax_stats_f64", "egnn_segment_softmax_apply_f32",
           "egnn_segment_softmax_apply_f64", "egnn_segment_pool_f32", "egnn_segment_pool_f64", "egnn_segment_pool_bwd_f32",
           "egnn_segment_pool_bwd_f64")


def _close(a, b):
    """equal to 1e-12 where both hold finite numbers; the same NaN / infinity pattern elsewhere"""
    fin = torch.isfinite(a) & torch.isfinite(b)
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return a.shape == b.shape and a.dtype == b.dtype and bool((same | (fin & ((a - b).abs() <= 1e-12))).all())


def _planted(t, shape, seed):
    """float64 scores: graph 2 (rows 1:6) holds a NaN in column 0 and a -inf next to finite scores in the last column; graph 4 (rows
    6:70) holds a column that is all -inf (the last)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, *shape, generator=g, dtype=torch.float64) * 3
    flat = x.reshape(t, -1)
    flat[3, 0] = math.nan
    flat[2, -1] = -math.inf
    flat[6:70, -1] = -math.inf
    return x


@pytest.mark.parametrize("trailing", ((), (3,), (2, 3)))
def test_cpu_softmax_and_logsumexp_are_torch_on_the_rows_of_every_graph(trailing):
    seg = GraphSegments.from_sizes(list(SIZES))
    x = _planted(seg.num_nodes, trailing, 1)
    y, lse = seg.softmax(x), seg.logsumexp(x)
    assert y.shape == x.shape and lse.shape == (len(SIZES), *trailing) and y.dtype == lse.dtype == torch.float64
    off = seg.host_offsets
    for gi, (a, b) in enumerate(zip(off, off[1:])):
        assert _close(y[a:b], torch.softmax(x[a:b], 0)), gi
        if b > a:
            assert _close(lse[gi], torch.logsumexp(x[a:b], 0)), gi
        else:
            assert bool((lse[gi] == -math.inf).all()), gi
    # the planted values: the NaN poisons its (graph, column) alone; -inf next to finite scores has weight exactly 0; an all -inf column
    y2, l2 = y.reshape(seg.num_nodes, -1), lse.reshape(len(SIZES), -1)
    assert torch.isnan(y2[1:6, 0]).all() and math.isnan(l2[2, 0]) and not torch.isnan(y2[:1]).any() and not torch.isnan(y2[70:]).any()
    if y2.shape[1] > 1:
        assert y2[2, -1] == 0 and not torch.isnan(y2[1:6, 1:]).any()
    assert torch.isnan(y2[6:70, -1]).all() and l2[4, -1] == -math.inf
    assert torch.isnan(l2).nonzero().tolist() == [[2, 0]]


@pytest.mark.parametrize("h, dv, short", ((1, 1, False), (1, 3, True), (3, 5, False), (2, 4, False)))
def test_cpu_attention_pool_is_torch_on_the_rows_of_every_graph(h, dv, short):
    seg = GraphSegments.from_sizes(list(SIZES))
    t = seg.num_nodes
    scores = _planted(t, (h,), 2)
    values = torch.randn(t, h, dv, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    if short:
        scores, values = scores[:, 0], values[:, 0]
    out = seg.attention_pool(scores, values)
    assert out.shape == ((len(SIZES), dv) if short else (len(SIZES), h, dv)) and out.dtype == torch.float64
    off = seg.host_offsets
    for gi, (a, b) in enumerate(zip(off, off[1:])):
        if b > a:
            assert _close(out[gi], (torch.softmax(scores[a:b], 0)[..., None] * values[a:b]).sum(0)), gi
        else:
            assert not out[gi].any(), gi                                                     # an empty graph: a row of zeros
    o3 = out.reshape(len(SIZES), h, dv)
    assert torch.isnan(o3[2, 0]).all() and torch.isnan(o3[4, -1]).all()                      # the NaN's head; the all -inf head
    assert torch.isnan(o3).any(-1).nonzero().tolist() == [[2, 0], [4, h - 1]]


def test_cpu_batches_without_a_node_and_empty_graphs_raise_nothing():
    none = GraphSegments.from_sizes([0, 0])
    assert none.softmax(torch.zeros(0, 3)).shape == (0, 3)
    lse = none.logsumexp(torch.zeros(0, 3))
    assert lse.shape == (2, 3) and bool((lse == -math.inf).all())
    out = none.attention_pool(torch.zeros(0, 2), torch.zeros(0, 2, 4))
    assert out.shape == (2, 2, 4) and not out.any()
    assert none.attention_pool(torch.zeros(0), torch.zeros(0, 4)).shape == (2, 4)
    # the pooled row of an empty graph has zero gradient, the others finite ones
    seg = GraphSegments.from_sizes([0, 3, 0])
    s = torch.randn(3, 2, dtype=torch.float64, requires_grad=True)
    v = torch.randn(3, 2, 4, dtype=torch.float64, requires_grad=True)
    out = seg.attention_pool(s, v)
    assert not out[0].any() and not out[2].any()
    (out * torch.randn(3, 2, 4, dtype=torch.float64)).sum().backward()
    assert torch.isfinite(s.grad).all() and torch.isfinite(v.grad).all() and v.grad.any()


def test_half_precisions_are_computed_in_fp32_and_keep_their_dtype():
    seg = GraphSegments.from_sizes([300, 2])
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.zeros(302, 2, dtype=dtype)
        y, lse = seg.softmax(x), seg.logsumexp(x)
        assert y.dtype == lse.dtype == dtype and float(y[0, 0]) == float(torch.tensor(1 / 300).to(dtype)) and float(y[301, 0]) == 0.5
        assert float(lse[0, 0]) == float(torch.tensor(math.log(300)).to(dtype))
        out = seg.attention_pool(x, torch.ones(302, 2, 3, dtype=dtype))
        assert out.dtype == dtype and bool((out.float() - 1).abs().max() <= 2.0 ** -7)       # (300 bf16 products of 1 / 300 fall short)


def _distinct(t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(t * d, generator=g).double().reshape(t, d) / 7 - 2).requires_grad_(True)


def test_cpu_gradcheck_and_gradgradcheck():
    seg = GraphSegments.from_sizes([5, 0, 1, 6])
    x = _distinct(12, 3, 1)
    live = torch.tensor(seg.sizes) > 0                   # (the empty graph's logsumexp is -inf: no finite difference to take of it)
    for fn in (seg.softmax, lambda t: seg.logsumexp(t)[live]):
        assert torch.autograd.gradcheck(fn, (x,))
        assert torch.autograd.gradgradcheck(lambda t: fn(t) ** 2, (x,))
    s, v = _distinct(12, 2, 2), _distinct(12, 6, 3)
    pool = lambda a, b: seg.attention_pool(a, b.reshape(12, 2, 3))
    assert torch.autograd.gradcheck(pool, (s, v))
    assert torch.autograd.gradgradcheck(lambda a, b: pool(a, b) ** 2, (s, v))


def test_refusals_by_type_and_message():
    seg = GraphSegments.from_sizes([2, 0, 3])
    for fn in (seg.softmax, seg.logsumexp):
        with pytest.raises(TypeError, match="floating-point"):
            fn(torch.ones(5, 3, dtype=torch.int64))
        with pytest.raises(TypeError, match="expected a tensor"):
            fn([1.0] * 5)
        with pytest.raises(ValueError, match=r"expected \(5, \.\.\.\)"):
            fn(torch.randn(6, 3))
        with pytest.raises(ValueError, match="no column"):
            fn(torch.randn(5, 0))
        with pytest.raises(RuntimeError, match="same device"):
            fn(torch.randn(5, 3, device="meta"))
    s, v = torch.randn(5, 2), torch.randn(5, 2, 4)
    with pytest.raises(TypeError, match="expected a tensor"):
        seg.attention_pool(s, None)
    with pytest.raises(TypeError, match="floating-point scores"):
        seg.attention_pool(torch.ones(5, 2, dtype=torch.int32), v)
    with pytest.raises(TypeError, match="floating-point values"):
        seg.attention_pool(s, torch.ones(5, 2, 4, dtype=torch.int64))
    with pytest.raises(TypeError, match="scores are torch.float32, values torch.float64"):
        seg.attention_pool(s, v.double())
    with pytest.raises(ValueError, match=r"scores shape \(6, 2\): expected \(5, H\)"):
        seg.attention_pool(torch.randn(6, 2), v)
    with pytest.raises(ValueError, match=r"scores shape \(5, 2, 1\)"):
        seg.attention_pool(torch.randn(5, 2, 1), v)
    with pytest.raises(ValueError, match=r"values shape \(5, 3, 4\): expected \(5, 2, Dv\)"):
        seg.attention_pool(s, torch.randn(5, 3, 4))
    with pytest.raises(ValueError, match=r"values shape \(5, 2\): expected \(5, 2, Dv\)"):
        seg.attention_pool(s, torch.randn(5, 2))
    with pytest.raises(ValueError, match=r"values shape \(5, 2, 4\): expected \(5, Dv\)"):
        seg.attention_pool(torch.randn(5), v)
    with pytest.raises(ValueError, match=r"values shape \(5, 2, 0\)"):
        seg.attention_pool(s, torch.randn(5, 2, 0))
    with pytest.raises(RuntimeError, match="same device: scores is on meta"):
        seg.attention_pool(s.to("meta"), v.to("meta"))
    with pytest.raises(RuntimeError, match="same device: values is on meta"):
        seg.attention_pool(s, v.to("meta"))


def test_ops_wrappers_refuse_before_any_launch():
    from egnn_pytorch_amd import _ops
    seg = GraphSegments.from_sizes([2, 0, 3])
    s, v, st = torch.randn(5, 2), torch.randn(5, 2, 4), torch.zeros(3, 2)
    with pytest.raises(TypeError, match="float32 or float64"):
        _ops.segment_softmax_stats(s.half(), seg)
    with pytest.raises(ValueError, match=r"expected \(5, D\)"):
        _ops.segment_softmax_stats(torch.randn(4, 2), seg)
    with pytest.raises(ValueError, match="m must be a contiguous"):
        _ops.segment_softmax_apply(s, torch.zeros(3, 3), st, seg)
    with pytest.raises(TypeError, match="expected one dtype"):
        _ops.segment_pool(s, v.double(), st, st, seg)
    with pytest.raises(ValueError, match=r"values shape \(5, 3, 4\)"):
        _ops.segment_pool(s, torch.randn(5, 3, 4), st, st, seg)
    with pytest.raises(ValueError, match="l must be a contiguous"):
        _ops.segment_pool(s, v, st, st.double(), seg)
    with pytest.raises(ValueError, match="g must be a"):
        _ops.segment_pool_bwd(torch.zeros(3, 2, 5), torch.zeros(3, 2, 4), s, v, st, st, seg)
    with pytest.raises(RuntimeError, match="same device"):
        _ops.segment_pool(s, v.to("meta"), st, st, seg)


# ------------------------------------------------------------------ the C entries
def test_entries_are_declared_bound_and_exported():
    prototypes, _, defines = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip.h"))
    lib = _abi.load()
    for sym in ENTRIES:
        assert sym in prototypes and sym in _abi.SIGNATURES and sym in _abi.SYMBOLS and hasattr(lib, sym), sym
    for f32 in ENTRIES[::2]:
        f64 = f32.replace("_f32", "_f64")
        ret, params = prototypes[f32]
        assert prototypes[f64] == (ret, [(ctype.replace("float", "double"), arg) for ctype, arg in params]), f64
        assert _abi.SIGNATURES[f64] == _abi.SIGNATURES[f32]
    assert int(defines["EGNN_ABI_VERSION"]) == _abi.ABI_VERSION == lib.egnn_abi_version() == 44      # additions do not bump it
    from egnn_pytorch_amd import _ops
    assert all(callable(getattr(_ops, f)) for f in ("segment_softmax_stats", "segment_softmax_apply", "segment_pool", "segment_pool_bwd"))
    assert all(callable(getattr(GraphSegments, f)) for f in ("softmax", "logsumexp", "attention_pool"))
    build = open(os.path.join(ROOT, "egnn_pytorch_amd", "csrc", "build.sh")).read()
    assert " segment_softmax " in build and "segment_softmax ]" not in build                          # in the file loop, default flags


@pytest.mark.parametrize("sfx", ("_f32", "_f64"))
def test_argument_checks_answer_before_any_launch(sfx):
    lib = _abi.load()
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    eb = 4 if sfx == "_f32" else 8
    big = lib.egnn_segment_reduce_workspace_bytes(2, 1000, 8, eb)                                      # exactly what (G, T, D) below need

    def stats(x=fake, ld=8, off=fake, crow=fake, cseg=fake, cslot=fake, nch=9, mseg=fake, mslot=fake, nm=1, g=2, t=1000, d=8, m=fake,
              l=fake, w=fake, wb=big):
        return getattr(lib, "egnn_segment_softmax_stats" + sfx)(x, ld, off, crow, cseg, cslot, nch, mseg, mslot, nm, g, t, d, m, l, w, wb, None)

    for name in ("x", "off", "crow", "cseg", "cslot", "m", "l", "mseg", "mslot", "w"):
        assert stats(**{name: None}) == -1, name
    for bad in (dict(g=0), dict(t=0), dict(d=0), dict(g=-1), dict(t=-5), dict(ld=7), dict(nch=1), dict(nm=-1), dict(nm=10), dict(wb=big - 1)):
        assert stats(**bad) == -2, bad
    assert stats(t=1 << 31, wb=1 << 40) == -3
    assert stats(d=65536 * 64, ld=65536 * 64, wb=1 << 40) == -3                                        # more column tiles than a grid holds
    assert stats(w=fake + 4) == -4

    def apply(x=fake, ld=8, m=fake, l=fake, sof=fake, g=2, t=1000, d=8, y=fake):
        return getattr(lib, "egnn_segment_softmax_apply" + sfx)(x, ld, m, l, sof, g, t, d, y, None)

    for name in ("x", "m", "l", "sof", "y"):
        assert apply(**{name: None}) == -1, name
    for bad in (dict(g=0), dict(t=0), dict(d=0), dict(ld=7)):
        assert apply(**bad) == -2, bad
    assert apply(t=1 << 31) == -3

    def pool(s=fake, lds=2, v=fake, ldv=8, m=fake, l=fake, off=fake, crow=fake, cseg=fake, cslot=fake, nch=9, mseg=fake, mslot=fake, nm=1,
             g=2, t=1000, h=2, dv=4, out=fake, w=fake, wb=big):
        return getattr(lib, "egnn_segment_pool" + sfx)(s, lds, v, ldv, m, l, off, crow, cseg, cslot, nch, mseg, mslot, nm, g, t, h, dv, out,
                                                       w, wb, None)

    for name in ("s", "v", "m", "l", "off", "crow", "cseg", "cslot", "out", "mseg", "mslot", "w"):
        assert pool(**{name: None}) == -1, name
    for bad in (dict(g=0), dict(t=0), dict(h=0), dict(dv=0), dict(dv=-1), dict(lds=1), dict(ldv=7), dict(nch=1), dict(nm=-1), dict(nm=10),
                dict(wb=big - 1)):
        assert pool(**bad) == -2, bad
    assert pool(t=1 << 31, wb=1 << 40) == -3
    assert pool(h=1 << 16, dv=1 << 16, lds=1 << 16, ldv=1 << 32, wb=1 << 60) == -3                      # H Dv beyond an int
    assert pool(h=64, dv=65536, lds=64, ldv=1 << 22, wb=1 << 40) == -3                                 # more column tiles than a grid holds
    assert pool(w=fake + 8) == -4

    def bwd(gr=fake, out=fake, s=fake, lds=2, v=fake, ldv=8, m=fake, l=fake, sof=fake, g=2, t=1000, h=2, dv=4, ds=fake, dvv=fake):
        return getattr(lib, "egnn_segment_pool_bwd" + sfx)(gr, out, s, lds, v, ldv, m, l, sof, g, t, h, dv, ds, dvv, None)

    for name in ("gr", "out", "s", "v", "m", "l", "sof", "ds", "dvv"):
        assert bwd(**{name: None}) == -1, name
    for bad in (dict(g=0), dict(t=0), dict(h=0), dict(dv=0), dict(lds=1), dict(ldv=7)):
        assert bwd(**bad) == -2, bad
    assert bwd(t=1 << 31) == -3 and bwd(h=1 << 16, dv=1 << 16, lds=1 << 16, ldv=1 << 32) == -3
