"""`GraphSegments.reduce` / `broadcast` / `center` without a GPU: the semantics on CPU tensors against `unpack` + masked torch reductions
(the tie rule, NaN, +-inf, empty graphs), autograd to second order (gradcheck / gradgradcheck in float64), the refusals by type and
message, the C entries of csrc/segment_reduce.hip (declared, bound, exported; their argument checks answer before any launch, with
made-up pointers), and the numpy restatement of the device's addition order (tests/_segment_reduce_order.py) against itself."""
import math
import os

import numpy as np
import pytest
import torch

from egnn_pytorch_amd import GraphSegments, _abi
from egnn_pytorch_amd import segments as segments_mod
from tests import _cheader
from tests import _segment_reduce_order as order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((0, 1, 5, 0, 64, 3), (9,), (0, 0, 7, 0))
TRAILING = ((), (3,), (4, 3))
OPS = ("sum", "mean", "max", "min")
ENTRIES = ("egnn_segment_reduce_f32", "egnn_segment_reduce_f64", "egnn_segment_broadcast_f32", "egnn_segment_broadcast_f64",
           "egnn_segment_scatter_rows_f32", "egnn_segment_scatter_rows_f64", "egnn_segment_gather_rows_f32",
           "egnn_segment_gather_rows_f64", "egnn_segment_reduce_workspace_bytes", "egnn_segment_reduce_chunk_rows")


def reference(seg, x, op):
    """float64, through the padded layout: (G, ...) of the graphs that hold a node; NaN where a graph holds none"""
    mask = seg.prefix_mask()
    m = mask.reshape(*mask.shape, *([1] * (x.dim() - 1)))
    if op in ("sum", "mean"):
        out = seg.unpack(x.double()).sum(1)
        if op == "mean":
            n = torch.tensor(seg.sizes, dtype=torch.float64).reshape(-1, *([1] * (x.dim() - 1)))
            out = torch.where(n > 0, out / n.clamp(min=1), torch.zeros_like(out))
        return out
    if op == "max":
        return seg.unpack(x.double(), fill=-math.inf).masked_fill(~m, -math.inf).amax(1)
    return seg.unpack(x.double(), fill=math.inf).masked_fill(~m, math.inf).amin(1)


@pytest.mark.parametrize("trailing", TRAILING)
@pytest.mark.parametrize("sizes", SIZES)
def test_cpu_semantics_against_unpack_and_masked_reductions(sizes, trailing):
    seg = GraphSegments.from_sizes(list(sizes))
    g = torch.Generator().manual_seed(len(sizes) * 10 + len(trailing))
    x = torch.randn(seg.num_nodes, *trailing, generator=g, dtype=torch.float64)
    for op in ("sum", "mean"):
        got = seg.reduce(x, op)
        assert got.shape == (seg.num_graphs, *trailing) and got.dtype == x.dtype
        torch.testing.assert_close(got, reference(seg, x, op), atol=1e-13, rtol=0)
    full = GraphSegments.from_sizes([n for n in sizes if n])
    for op in ("max", "min"):
        assert torch.equal(full.reduce(x, op), reference(full, x, op))
        if 0 in sizes:
            with pytest.raises(ValueError, match="empty graph"):
                seg.reduce(x, op)
    bc = seg.broadcast(seg.reduce(x, "sum"))
    assert bc.shape == x.shape
    assert torch.equal(bc, seg.reduce(x, "sum")[seg.segment_of.long()])


def test_cpu_tie_rule_nan_and_infinities():
    seg = GraphSegments.from_sizes([4, 3, 2])
    inf, nan = math.inf, math.nan
    x = torch.tensor([[1., 5.], [7., 5.], [7., -inf], [2., 5.],
                      [nan, inf], [3., inf], [nan, -1.],
                      [-inf, 0.], [-inf, -0.]], dtype=torch.float64)
    mx = seg.reduce(x, "max")
    assert torch.equal(mx[:1], torch.tensor([[7., 5.]], dtype=torch.float64))
    assert math.isnan(mx[1, 0]) and mx[1, 1] == inf and mx[2, 0] == -inf and mx[2, 1] == 0
    rows = seg._winners_host(x, True)
    assert rows.dtype == torch.int32 and rows.tolist() == [[1, 0], [4, 4], [7, 7]]                 # lowest row of a tie; the first NaN
    assert seg._winners_host(x, False).tolist() == [[0, 2], [4, 6], [7, 7]]
    mn = seg.reduce(x, "min")
    assert mn[0].tolist() == [1., -inf] and math.isnan(mn[1, 0]) and mn[1, 1] == -1.
    # the gradient of a tie goes to the lowest row alone
    xg = torch.tensor([[2.], [2.], [1.]], dtype=torch.float64, requires_grad=True)
    GraphSegments.from_sizes([3]).reduce(xg, "max").sum().backward()
    assert xg.grad.reshape(-1).tolist() == [1., 0., 0.]


def test_cpu_mean_of_an_empty_graph_is_zero_with_zero_gradient():
    seg = GraphSegments.from_sizes([0, 2, 0])
    x = torch.tensor([[1., 2.], [3., 6.]], requires_grad=True)
    out = seg.reduce(x, "mean")
    assert out.tolist() == [[0., 0.], [2., 4.]] + [[0., 0.]]
    (out * torch.tensor([[7.], [1.], [9.]])).sum().backward()
    assert torch.equal(x.grad, torch.full((2, 2), 0.5))
    none = GraphSegments.from_sizes([0, 0])
    z = none.reduce(torch.zeros(0, 3), "sum")
    assert z.shape == (2, 3) and not z.any() and none.broadcast(z).shape == (0, 3)


def test_half_precisions_accumulate_in_fp32_and_keep_their_dtype():
    seg = GraphSegments.from_sizes([300, 2])
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.full((302, 2), 1.0, dtype=dtype)
        out = seg.reduce(x, "sum")
        assert out.dtype == dtype and out[:, 0].tolist() == [300., 2.]                         # (a bf16 accumulator stalls at 256)
        assert seg.broadcast(out).dtype == dtype and seg.reduce(x, "max").dtype == dtype


# ------------------------------------------------------------------ autograd, float64
def _distinct(t, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(t * d, generator=g).double().reshape(t, d) / 7 - 2).requires_grad_(True)


@pytest.mark.parametrize("op", OPS)
def test_cpu_gradcheck_and_gradgradcheck_of_reduce(op):
    seg = GraphSegments.from_sizes([5, 1, 6] if op in ("max", "min") else [5, 0, 1, 6])
    x = _distinct(12, 3, 1)
    assert torch.autograd.gradcheck(lambda t: seg.reduce(t, op), (x,))
    assert torch.autograd.gradgradcheck(lambda t: seg.reduce(t, op) ** 2, (x,))


def test_cpu_gradcheck_and_gradgradcheck_of_broadcast_and_center():
    seg = GraphSegments.from_sizes([5, 0, 1, 6])
    g = _distinct(4, 3, 2)
    x = _distinct(12, 3, 3)
    assert torch.autograd.gradcheck(seg.broadcast, (g,))
    assert torch.autograd.gradgradcheck(lambda t: seg.broadcast(t) ** 2, (g,))
    assert torch.autograd.gradcheck(seg.center, (x,))
    assert torch.autograd.gradgradcheck(lambda t: seg.center(t) ** 2, (x,))


def test_identities():
    seg = GraphSegments.from_sizes([0, 1, 5, 0, 64, 3])
    x = torch.randn(seg.num_nodes, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    assert seg.reduce(seg.center(x), "mean").abs().max() < 1e-14
    g = torch.randn(seg.num_graphs, 2, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    back = seg.reduce(seg.broadcast(g), "mean")
    live = torch.tensor(seg.sizes) > 0
    torch.testing.assert_close(back[live], g[live], atol=1e-14, rtol=0)
    assert not back[~live].any()


# ------------------------------------------------------------------ refusals
def test_refusals_by_type_and_message():
    seg = GraphSegments.from_sizes([2, 0, 3])
    x = torch.randn(5, 3)
    with pytest.raises(TypeError, match="floating-point"):
        seg.reduce(torch.ones(5, 3, dtype=torch.int64))
    with pytest.raises(TypeError, match="floating-point"):
        seg.reduce(torch.ones(5, 3, dtype=torch.bool), "max")
    with pytest.raises(TypeError, match="floating-point"):
        seg.broadcast(torch.ones(3, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"expected \(5, \.\.\.\)"):
        seg.reduce(torch.randn(6, 3))
    with pytest.raises(ValueError, match=r"expected \(3, \.\.\.\)"):
        seg.broadcast(torch.randn(5, 3))
    with pytest.raises(ValueError, match="op = 'prod'"):
        seg.reduce(x, "prod")
    with pytest.raises(ValueError, match="graph 1 holds no node"):
        seg.reduce(x, "max")
    with pytest.raises(ValueError, match="empty graph"):
        seg.reduce(x, "min")
    with pytest.raises(ValueError, match="no column"):
        seg.reduce(torch.randn(5, 0))
    with pytest.raises(RuntimeError, match="same device"):
        seg.reduce(torch.randn(5, 3, device="meta"))
    with pytest.raises(RuntimeError, match="same device"):
        seg.broadcast(torch.randn(3, 3, device="meta"))
    with pytest.raises(RuntimeError, match="same device"):
        seg.center(torch.randn(5, 3, device="meta"))


def test_chunk_tables_come_from_the_host_offsets():
    r = segments_mod.SEGMENT_CHUNK_ROWS
    sizes = [0, 1, r, r + 1, 0, 2 * r + 1, 3]
    seg = GraphSegments.from_sizes(sizes)
    tab = seg._reduce_tables()
    assert seg._reduce_tables() is tab                                                        # built once
    off = seg.host_offsets
    want_row, want_seg, want_slot, multi, slot = [], [], [], [], 0
    for g, n in enumerate(sizes):
        parts = order.chunks(n)
        if len(parts) > 1:
            multi.append((g, slot))
        for a, _ in parts:
            want_row.append(off[g] + a)
            want_seg.append(g)
            want_slot.append(slot if len(parts) > 1 else -1)
            slot += len(parts) > 1
    assert tab.chunk_row.tolist() == want_row and tab.chunk_seg.tolist() == want_seg and tab.chunk_slot.tolist() == want_slot
    assert tab.n_chunks == len(want_row) and tab.n_multi == 2
    assert list(zip(tab.multi_seg.tolist(), tab.multi_slot.tolist())) == multi
    assert all(t.dtype == torch.int32 for t in (tab.chunk_row, tab.chunk_seg, tab.chunk_slot, tab.multi_seg, tab.multi_slot))
    small = GraphSegments.from_sizes([3, 0])._reduce_tables()
    assert small.n_multi == 0 and small.multi_seg is None and small.chunk_slot.tolist() == [-1, -1]


# ------------------------------------------------------------------ the C entries
def test_entries_are_declared_bound_and_exported():
    prototypes, _, defines = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip.h"))
    lib = _abi.load()
    for sym in ENTRIES:
        assert sym in prototypes and sym in _abi.SIGNATURES and sym in _abi.SYMBOLS and hasattr(lib, sym), sym
    for f32 in ENTRIES[:8:2]:
        f64 = f32.replace("_f32", "_f64")
        ret, params = prototypes[f32]
        assert prototypes[f64] == (ret, [(ctype.replace("float", "double"), arg) for ctype, arg in params]), f64
        assert _abi.SIGNATURES[f64] == _abi.SIGNATURES[f32]
    assert int(defines["EGNN_ABI_VERSION"]) == _abi.ABI_VERSION == lib.egnn_abi_version() == 44
    assert lib.egnn_segment_reduce_chunk_rows() == segments_mod.SEGMENT_CHUNK_ROWS == order.R
    from egnn_pytorch_amd import _ops
    assert all(callable(getattr(_ops, f)) for f in ("segment_reduce", "segment_broadcast", "segment_scatter_rows", "segment_gather_rows"))
    build = open(os.path.join(ROOT, "egnn_pytorch_amd", "csrc", "build.sh")).read()
    assert " segment_reduce " in build and "segment_reduce ]" not in build                    # in the file loop, default flags


def test_workspace_query_grows_with_the_batch():
    ws = _abi.load().egnn_segment_reduce_workspace_bytes
    for g, t, d in ((1, 1, 1), (3, 100, 7), (173, 66055, 128), (1, 1 << 20, 64), (65536, 262144, 1)):
        for eb in (4, 8):
            assert 0 < ws(g, t, d, eb) <= ws(g + 1, t, d, eb) and ws(g, t, d, eb) <= ws(g, t + 1, d, eb) <= ws(g, t + 128, d, eb)
            assert ws(g, t, d, eb) <= ws(g, t, d + 1, eb)
        assert ws(g, t, d, 4) <= ws(g, t, d, 8)
    assert ws(1, 1 << 20, 64, 4) > ws(1, 1000, 64, 4) and ws(4096, 1 << 20, 64, 4) > ws(1, 1 << 20, 64, 4)
    assert ws(0, 5, 1, 4) == ws(1, 0, 1, 4) == ws(1, 5, 0, 4) == ws(1, 5, 1, 2) == 0
    # the slots cover every chunk of every graph longer than a chunk, whatever the sizes: at most T / R of them, n / R + 1 chunks each
    r = order.R
    for sizes in ((1000,), (r + 1,) * 9 + (3,) * 50, (r,) * 8, (2 * r + 1, 0, 5 * r - 1)):
        t, g = sum(sizes), len(sizes)
        need = sum(len(order.chunks(n)) for n in sizes if n > r)
        assert need <= min(g, t // r) + t // r + 1 and ws(g, t, 1, 4) >= 256


@pytest.mark.parametrize("sfx", ("_f32", "_f64"))
def test_argument_checks_answer_before_any_launch(sfx):
    lib = _abi.load()
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    big = lib.egnn_segment_reduce_workspace_bytes(2, 1000, 8, 4 if sfx == "_f32" else 8)       # exactly what (G, T, D) below need

    def red(x=fake, ld=8, off=fake, crow=fake, cseg=fake, cslot=fake, nch=9, mseg=fake, mslot=fake, nm=1, g=2, t=1000, d=8, op=0, out=fake,
            rows=fake, w=fake, wb=big):
        return getattr(lib, "egnn_segment_reduce" + sfx)(x, ld, off, crow, cseg, cslot, nch, mseg, mslot, nm, g, t, d, op, out, rows, w, wb, None)

    for name in ("x", "off", "crow", "cseg", "cslot", "out", "mseg", "mslot", "w"):
        assert red(**{name: None}) == -1, name
    assert red(rows=None, op=2) == -1 and red(rows=None, op=3) == -1
    for bad in (dict(g=0), dict(t=0), dict(d=0), dict(g=-1), dict(t=-5), dict(ld=7), dict(nch=1), dict(nm=-1), dict(nm=10), dict(wb=big - 1)):
        assert red(**bad) == -2, bad
    assert red(op=4) == -3 and red(op=-1) == -3
    assert red(t=1 << 31, wb=1 << 40) == -3
    assert red(w=fake + 4) == -4

    bc = getattr(lib, "egnn_segment_broadcast" + sfx)
    sc = getattr(lib, "egnn_segment_scatter_rows" + sfx)
    ga = getattr(lib, "egnn_segment_gather_rows" + sfx)
    assert bc(None, fake, 2, 10, 3, fake, None) == bc(fake, None, 2, 10, 3, fake, None) == bc(fake, fake, 2, 10, 3, None, None) == -1
    assert bc(fake, fake, 0, 10, 3, fake, None) == bc(fake, fake, 2, 0, 3, fake, None) == bc(fake, fake, 2, 10, 0, fake, None) == -2
    assert bc(fake, fake, 2, 1 << 31, 3, fake, None) == -3
    assert sc(None, fake, fake, 2, 10, 3, fake, None) == sc(fake, None, fake, 2, 10, 3, fake, None) == -1
    assert sc(fake, fake, None, 2, 10, 3, fake, None) == sc(fake, fake, fake, 2, 10, 3, None, None) == -1
    assert sc(fake, fake, fake, 0, 10, 3, fake, None) == sc(fake, fake, fake, 2, 0, 3, fake, None) == -2
    assert sc(fake, fake, fake, 2, 10, 0, fake, None) == -2 and sc(fake, fake, fake, 2, 1 << 31, 3, fake, None) == -3
    assert ga(None, fake, 2, 10, 3, fake, None) == ga(fake, None, 2, 10, 3, fake, None) == ga(fake, fake, 2, 10, 3, None, None) == -1
    assert ga(fake, fake, 0, 10, 3, fake, None) == ga(fake, fake, 2, 0, 3, fake, None) == ga(fake, fake, 2, 10, 0, fake, None) == -2
    assert ga(fake, fake, 2, 1 << 31, 3, fake, None) == -3


# ------------------------------------------------------------------ the restated order against itself
@pytest.mark.parametrize("n", (0, 1, order.R - 1, order.R, order.R + 1, 2 * order.R + 1, 1000))
def test_restated_chunking_visits_every_row_once(n):
    for d in (1, 3, 4, 5, 64, 130, 257):
        seen = []
        for a, m in order.chunks(n):
            assert 0 <= m <= order.R and (m > 0 or n == 0)
            per = order.strand_rows(m, order.strands(d))
            assert len(per) == order.strands(d) and all(rows == sorted(rows) for rows in per)
            seen += [a + r for rows in per for r in rows]
        assert sorted(seen) == list(range(n))
    assert [order.strands(d) for d in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 130, 257)] == [256, 256, 256, 128, 128, 64, 64, 32, 32, 16, 16, 16, 16]


@pytest.mark.parametrize("n", (1, 5, order.R - 1, order.R + 1, 2 * order.R + 1, 1000))
@pytest.mark.parametrize("d", (1, 3, 5, 64, 130))
def test_restated_sum_meets_its_own_bound_in_float64(n, d):
    rng = np.random.default_rng(n * 1000 + d)
    x = rng.standard_normal((n, d)) * np.exp(rng.uniform(-6, 6, (n, d)))
    got = order.segment_sum(x)
    assert got.dtype == np.float64
    for c in range(d):
        exact = math.fsum(x[:, c].tolist())
        assert abs(got[c] - exact) <= order.depth(n, d) * 2.0 ** -53 * math.fsum(np.abs(x[:, c]).tolist()) * 1.01
    x32 = x.astype(np.float32)
    assert order.segment_sum(x32).dtype == np.float32
    assert np.array_equal(order.batch_sum(np.concatenate([x32, x32]), [n, 0, n]), np.stack([order.segment_sum(x32), np.zeros(d, np.float32)] * 2)[:3])


def test_depth_of_the_restated_order():
    assert order.depth(0, 3) == 0 and order.depth(1, 1) == 8 and order.depth(order.R, 1) == 8            # one row per strand: the tree alone
    assert order.depth(order.R, 64) == 7 + 4 and order.depth(1000, 64) == 7 + 4 + 7 and order.depth(5, 5) == 7
