"""The segmented selection (csrc/knn_segments.hip, `_ops.knn_select_segments`) against the all-pairs selection on the padded batch.

Yardstick: `_ops.knn_select` on the (G, N_max, C) padded batch with the prefix mask, which the existing tests pin bit for bit to the
reference.  For every real node i of graph g (rows [lo, lo + n) of the packed batch):
    slots k <  min(K, n):  idx_packed - lo == idx_padded, and the rank bits are equal;
    slots k >= min(K, n):  idx == i, rank == +inf.
The padded call ranks its padding at 1e5, so it is the per-graph selection only while every squared distance stays below that: asserted
of the inputs.

One batch holds the sizes 0, 1, 2, K - 1, K, K + 1, 63, 64, 65, 257 and 128 / 129.  Every comparison runs twice: on the kernel's own LDS
budget (every segment of these sizes is read from the workgroup's LDS window) and with the window lowered to 128 nodes
(`_ops.KNN_SEGMENTS_LDS_NODES`), where 128 is the largest segment that fits and 129 the smallest that is streamed from memory.

A second batch holds two coincident segments of 200 and 300 nodes: every key of a row is equal, so with K <= 64 more candidates survive
the pruning bound than its list of 128 holds and the row falls back to the radix passes, which then have to resolve the K-th candidate
on the index digits alone -- one digit for 200 nodes, two for 300.

Every comparison also checks the packed lists against the numpy oracle directly (`_check_oracle`)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 8, 32, 48, 64, 65, 128)
SWITCH = 128
INF_BITS = {torch.float32: 0x7F800000, torch.float64: 0x7FF0000000000000}


def _sizes(k):
    return (0, 1, 2, k - 1, k, k + 1, 63, 64, 65, 257, SWITCH, SWITCH + 1)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _batch(sizes, cdim, dtype, geometry, seed=0):
    """(segments, packed coors (T, C), padded coors (G, N_max, C), prefix mask) on the device"""
    from egnn_pytorch_amd import GraphSegments
    seg = GraphSegments.from_sizes(sizes, device="cuda")
    g = torch.Generator().manual_seed(seed)
    t = seg.num_nodes
    if geometry == "random":
        x = torch.randn(t, cdim, generator=g) * 3.0
    elif geometry == "lattice":                          # ties inside a row and across the K boundary
        x = torch.randint(0, 4, (t, cdim), generator=g).float()
    elif geometry == "coincident":                       # every segment is one point of its own: all keys of a row are equal
        x = torch.cat([torch.randn(1, cdim, generator=g).expand(n, cdim) for n in sizes])
    else:                                                # "identical": the segment of 65 nodes is one point, the rest a coarse lattice
        x = torch.randint(0, 3, (t, cdim), generator=g).float()
        at = sizes.index(65)
        x[seg.host_offsets[at]:seg.host_offsets[at + 1]] = 1.5
    x = x.to(dtype).cuda()
    span = x.max(0).values - x.min(0).values             # every squared distance is below the rank of a padded candidate
    assert float((span.double() ** 2).sum()) < 1e5
    return seg, x, seg.unpack(x), seg.prefix_mask()


@functools.lru_cache(maxsize=None)
def _padded(sizes, cdim, dtype, geometry, k):
    from egnn_pytorch_amd import _ops
    _, _, xp, mask = _batch(sizes, cdim, dtype, geometry)
    idx, rank = _ops.knn_select(xp, mask, None, k)
    torch.cuda.synchronize()
    return idx, rank


def _packed(seg, x, k, lds_nodes=None):
    from egnn_pytorch_amd import _ops
    saved = _ops.KNN_SEGMENTS_LDS_NODES
    _ops.KNN_SEGMENTS_LDS_NODES = lds_nodes
    try:
        idx, rank = _ops.knn_select_segments(x, seg, k)
        torch.cuda.synchronize()
    finally:
        _ops.KNN_SEGMENTS_LDS_NODES = saved
    return idx, rank


def _check(seg, k, idx, rank, pidx, prank, what):
    assert idx.shape == rank.shape == (seg.num_nodes, k) and idx.dtype == torch.int32
    off = seg.host_offsets
    for g, n in enumerate(seg.sizes):
        if n == 0:
            continue
        lo, m = off[g], min(k, n)
        assert torch.equal(idx[lo:lo + n, :m] - lo, pidx[g, :n, :m]), (what, "graph", g, "size", n, "indices")
        assert torch.equal(_bits(rank[lo:lo + n, :m]), _bits(prank[g, :n, :m])), (what, "graph", g, "size", n, "rank bits")
        rows = torch.arange(lo, lo + n, device=idx.device, dtype=torch.int32)[:, None].expand(n, k - m)
        assert torch.equal(idx[lo:lo + n, m:], rows), (what, "graph", g, "size", n, "empty slots' indices")
        assert bool((_bits(rank[lo:lo + n, m:]) == INF_BITS[rank.dtype]).all()), (what, "graph", g, "size", n, "empty slots' ranks")


def _check_oracle(seg, x, k, idx, rank, what):
    """The filled slots against the numpy oracle, graph by graph (oracle/egnn_oracle.py: pairwise, build_ranking, topk_smallest with its
    stable sort).  The segmented kernel and the padded yardstick share their arithmetic (csrc/knn_core.h) and would go wrong together, so
    the packed lists are pinned to the oracle on their own."""
    from oracle import egnn_oracle as O
    xc, ic, rc = x.cpu().numpy(), idx.cpu().numpy(), rank.cpu().numpy()
    bits = np.uint32 if rc.dtype == np.float32 else np.uint64
    off = seg.host_offsets
    for g, n in enumerate(seg.sizes):
        if n == 0:
            continue
        lo, m = off[g], min(k, n)
        _, dist = O.pairwise(xc[None, lo:lo + n])
        ranking, _ = O.build_ranking(dist, None, None)
        ref_val, ref_idx = O.topk_smallest(ranking, m)
        np.testing.assert_array_equal(ref_idx[0].astype(np.int32), ic[lo:lo + n, :m] - lo, err_msg=f"{what} graph {g} size {n}")
        np.testing.assert_array_equal(np.ascontiguousarray(ref_val[0]).view(bits), np.ascontiguousarray(rc[lo:lo + n, :m]).view(bits),
                                      err_msg=f"{what} graph {g} size {n}")


def _compare(cdim, dtype, geometry, k, sizes=None):
    sizes = _sizes(k) if sizes is None else sizes
    seg, x, _, _ = _batch(sizes, cdim, dtype, geometry)
    assert k <= seg.num_nodes
    pidx, prank = _padded(sizes, cdim, dtype, geometry, k)
    for lds_nodes in (None, SWITCH):
        idx, rank = _packed(seg, x, k, lds_nodes)
        _check(seg, k, idx, rank, pidx, prank, (geometry, cdim, dtype, k, lds_nodes))
        _check_oracle(seg, x, k, idx, rank, (geometry, cdim, dtype, k, lds_nodes))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype,cdim", [(torch.float32, 3), (torch.float32, 2), (torch.float32, 5), (torch.float32, 9),
                                        (torch.float64, 3), (torch.float64, 9)],
                         ids=["f32_c3", "f32_c2", "f32_c5", "f32_c9", "f64_c3", "f64_c9"])
def test_random_coordinates_match_the_padded_selection(dtype, cdim, k):
    _compare(cdim, dtype, "random", k)


@pytest.mark.parametrize("geometry", ["lattice", "identical"])
@pytest.mark.parametrize("k", (8, 65))
@pytest.mark.parametrize("dtype,cdim", [(torch.float32, 3), (torch.float32, 5), (torch.float32, 9), (torch.float64, 3)],
                         ids=["f32_c3", "f32_c5", "f32_c9", "f64_c3"])
def test_tied_coordinates_match_the_padded_selection(dtype, cdim, k, geometry):
    _compare(cdim, dtype, geometry, k)


COINCIDENT = (200, 300)                                  # survivors of the pruning bound: 200, 300 > 128; index digits: one, two


@pytest.mark.parametrize("k", (8, 33, 64))
@pytest.mark.parametrize("dtype,cdim", [(torch.float32, 3), (torch.float32, 9), (torch.float64, 3)], ids=["f32_c3", "f32_c9", "f64_c3"])
def test_coincident_segments_fall_back_to_the_radix_passes_on_the_index_digits(dtype, cdim, k):
    """K <= 64 and every key of a row equal: the pruning path keeps all n > 128 candidates, which do not fit its list, and the radix
    passes walk every key digit without resolving anything before they reach the index digits.  The padded selection orders ties by
    ascending index, so every list is lo .. lo + K - 1 with rank 0."""
    assert all(n > 128 for n in COINCIDENT) and (COINCIDENT[0] - 1).bit_length() <= 8 < (COINCIDENT[1] - 1).bit_length() and k <= 64
    _compare(cdim, dtype, "coincident", k, sizes=COINCIDENT)
    pidx, prank = _padded(COINCIDENT, cdim, dtype, "coincident", k)
    for g, n in enumerate(COINCIDENT):                   # (the yardstick itself, on this geometry: ties by ascending index)
        assert torch.equal(pidx[g, :n], torch.arange(k, device="cuda", dtype=pidx.dtype).expand(n, k)) and not bool(prank[g, :n].any())


@pytest.mark.parametrize("lds_nodes", (None, SWITCH))
@pytest.mark.parametrize("geometry", ["random", "lattice"])
def test_graphs_in_reversed_order_give_the_same_lists(geometry, lds_nodes):
    """the same graphs packed in the opposite order: every list is the same, re-based to the graph's new first row"""
    from egnn_pytorch_amd import GraphSegments
    k = 32
    sizes = _sizes(k)
    seg, x, _, _ = _batch(sizes, 3, torch.float32, geometry)
    off = seg.host_offsets
    parts = [x[off[g]:off[g + 1]] for g in range(len(sizes))]
    rseg = GraphSegments.from_sizes(tuple(reversed(sizes)), device="cuda")
    idx, rank = _packed(seg, x, k, lds_nodes)
    ridx, rrank = _packed(rseg, torch.cat(parts[::-1]), k, lds_nodes)
    roff = rseg.host_offsets
    for g, n in enumerate(sizes):
        lo, rlo = off[g], roff[len(sizes) - 1 - g]
        assert torch.equal(idx[lo:lo + n] - lo, ridx[rlo:rlo + n] - rlo), (g, n)
        assert torch.equal(_bits(rank[lo:lo + n]), _bits(rrank[rlo:rlo + n])), (g, n)


@pytest.mark.parametrize("lds_nodes", (None, SWITCH))
def test_two_runs_give_equal_bits(lds_nodes):
    k = 48
    seg, x, _, _ = _batch(_sizes(k), 3, torch.float32, "lattice")
    a = _packed(seg, x, k, lds_nodes)
    b = _packed(seg, x, k, lds_nodes)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from egnn_pytorch_amd import GraphSegments, _ops
    seg = GraphSegments.from_sizes((3, 4), device="cuda")
    x = torch.zeros(7, 3, device="cuda")
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        _ops.knn_select_segments(x, seg, 8)                                   # K > T, as torch.topk upstream
    with pytest.raises(ValueError, match="expected \\(7, C\\)"):
        _ops.knn_select_segments(x[:6], seg, 2)
    with pytest.raises(TypeError, match="float32 or float64"):
        _ops.knn_select_segments(x.half(), seg, 2)
    with pytest.raises(RuntimeError, match="same device"):
        _ops.knn_select_segments(x, GraphSegments.from_sizes((3, 4)), 2)
    assert np.array_equal(_ops.knn_select_segments(x, seg, 2)[0].cpu().numpy()[:, 0], np.array([0, 0, 0, 3, 3, 3, 3]))
