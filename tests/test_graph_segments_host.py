"""`GraphSegments` and the host side of packed batches, without a GPU: the constructors against one another, pack / unpack on masks
that are no prefixes (tests/_masks.py) with their gradients, positions / segment_of against numpy, `split`, every refusal of a packed
call by type and message, and the new C entries -- declared, bound, exported, their argument checks answering before any launch."""
import os

import numpy as np
import pytest
import torch

from egnn_pytorch_amd import EGNN, EGNN_Network, GraphSegments, SparseAdjacency, _abi, graphed
from tests import _cheader
from tests._masks import B, PATTERNS, mask_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 5, 0, 64, 3)


# ------------------------------------------------------------------------------------------------ constructors
def test_the_four_constructors_agree():
    a = GraphSegments.from_sizes(SIZES)
    off = np.concatenate(([0], np.cumsum(SIZES)))
    b = GraphSegments.from_offsets(torch.from_numpy(off))
    batch = torch.from_numpy(np.repeat(np.arange(len(SIZES)), SIZES))
    c = GraphSegments.from_batch(batch, num_graphs=len(SIZES))
    mask = torch.arange(max(SIZES))[None, :] < torch.tensor(SIZES)[:, None]
    d = GraphSegments.from_mask(mask)
    e = GraphSegments.from_sizes(torch.tensor(SIZES))
    for s in (a, b, c, d, e):
        assert s.host_offsets == tuple(off.tolist()) and s.sizes == SIZES
        assert s.offsets.dtype == torch.int64 and s.offsets.tolist() == off.tolist()
        assert s.num_graphs == 6 and s.num_nodes == 73 and s.max_size == 64 and s.device == torch.device("cpu")
        assert torch.equal(s.positions, a.positions) and torch.equal(s.segment_of, a.segment_of)
    assert torch.equal(a.prefix_mask(), mask)
    assert a.to("cpu") is a
    assert GraphSegments.from_batch(batch).sizes == SIZES                       # (no trailing empty graph here: G = batch[-1] + 1)
    assert "graphs=6" in repr(a) and "nodes=73" in repr(a)


def test_positions_and_segment_of_against_numpy():
    s = GraphSegments.from_sizes(SIZES)
    assert s.positions.dtype == torch.int64 and s.segment_of.dtype == torch.int32
    assert np.array_equal(s.segment_of.numpy(), np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32))
    assert np.array_equal(s.positions.numpy(), np.concatenate([np.arange(n) for n in SIZES]))


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pack_unpack_round_trip_on_masks_that_are_no_prefixes(pattern):
    n = 12
    mask = torch.from_numpy(mask_pattern(pattern, B, n, 4, np.random.default_rng(3)))
    s = GraphSegments.from_mask(mask)
    assert s.sizes == tuple(mask.sum(-1).tolist())
    x = torch.randn(B, n, 5, generator=torch.Generator().manual_seed(1))
    p = s.pack(x)
    assert p.shape == (s.num_nodes, 5) and torch.equal(p, x[mask])              # graph by graph, slots in order
    u = s.unpack(p, fill=-7.0)
    assert u.shape == x.shape and torch.equal(u[mask], x[mask]) and bool((u[~mask] == -7.0).all())
    assert bool((s.unpack(p)[~mask] == 0).all())
    ids = torch.arange(B * n).view(B, n)                                        # (any trailing shape, any dtype)
    assert torch.equal(s.unpack(s.pack(ids), fill=-1)[mask], ids[mask])


def test_pack_unpack_without_a_mask_use_the_prefix_layout():
    s = GraphSegments.from_sizes((2, 0, 3))
    x = torch.arange(9.0).view(3, 3)
    assert s.pack(x).tolist() == [0.0, 1.0, 6.0, 7.0, 8.0]
    assert s.unpack(s.pack(x), fill=-1.0).tolist() == [[0.0, 1.0, -1.0], [-1.0, -1.0, -1.0], [6.0, 7.0, 8.0]]
    wide = torch.arange(15.0).view(3, 5)                                        # more slots than the largest graph: still the prefix
    assert s.pack(wide).tolist() == [0.0, 1.0, 10.0, 11.0, 12.0]


def test_pack_and_unpack_gradcheck():
    mask = torch.from_numpy(mask_pattern("scattered", B, 6, 4, np.random.default_rng(5)))
    s = GraphSegments.from_mask(mask)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 6, 3, generator=g, dtype=torch.float64, requires_grad=True)
    p = torch.randn(s.num_nodes, 3, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(s.pack, (x,))
    assert torch.autograd.gradcheck(lambda t: s.unpack(t, fill=2.0), (p,))


# ------------------------------------------------------------------------------------------------ split
@pytest.mark.parametrize("sizes,max_nodes", [(SIZES, 6), (SIZES, 64), (SIZES, 73), (SIZES, 1000), ((0, 100, 0, 3, 3, 0), 5),
                                             ((40, 7, 96, 1, 33), 64), ((5,), 2)])
def test_split_cuts_at_boundaries_and_respects_the_limit(sizes, max_nodes):
    s = GraphSegments.from_sizes(sizes)
    pieces = list(s.split(max_nodes))
    assert sum((p.sizes for _, p in pieces), ()) == tuple(sizes)                 # every graph once, in order
    at = 0
    for sl, p in pieces:
        assert sl.start == at and sl.stop - sl.start == p.num_nodes and sl.start in s.host_offsets and sl.stop in s.host_offsets
        assert p.host_offsets[0] == 0 and p.num_nodes > 0
        real = [n for n in p.sizes if n]
        assert p.num_nodes <= max_nodes or len(real) == 1                        # an oversize graph stands alone
        at = sl.stop
    assert at == s.num_nodes
    if max_nodes >= s.num_nodes:
        assert len(pieces) == 1


def test_split_refuses_a_limit_below_one():
    with pytest.raises(ValueError, match="max_nodes"):
        list(GraphSegments.from_sizes((2, 3)).split(0))


# ------------------------------------------------------------------------------------------------ validation
def test_constructors_say_what_was_wrong():
    with pytest.raises(TypeError, match="offsets must be int64"):
        GraphSegments.from_offsets(torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="expected \\(G \\+ 1,\\)"):
        GraphSegments.from_offsets(torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="expected \\(G \\+ 1,\\)"):
        GraphSegments.from_offsets(torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="start at 0"):
        GraphSegments.from_offsets(torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="non-decreasing"):
        GraphSegments.from_offsets(torch.tensor([0, 3, 2]))
    with pytest.raises(TypeError, match="sequence of ints"):
        GraphSegments.from_offsets([0, 1.5])
    with pytest.raises(TypeError, match="sizes must be int64"):
        GraphSegments.from_sizes(torch.tensor([1.0, 2.0]))
    with pytest.raises(TypeError, match="sequence of ints"):
        GraphSegments.from_sizes([1, 2.0])
    with pytest.raises(ValueError, match="non-negative"):
        GraphSegments.from_sizes([1, -2])
    with pytest.raises(ValueError, match="G >= 1"):
        GraphSegments.from_sizes([])
    with pytest.raises(TypeError, match="batch must be an int64 tensor"):
        GraphSegments.from_batch(torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="expected \\(T,\\)"):
        GraphSegments.from_batch(torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="batch must be non-decreasing"):
        GraphSegments.from_batch(torch.tensor([0, 1, 0]))
    with pytest.raises(ValueError, match="negative graph index"):
        GraphSegments.from_batch(torch.tensor([-1, 0]))
    with pytest.raises(ValueError, match="num_graphs = 2"):
        GraphSegments.from_batch(torch.tensor([0, 2]), num_graphs=2)
    with pytest.raises(TypeError, match="mask must be a torch.bool tensor"):
        GraphSegments.from_mask(torch.ones(2, 3))
    with pytest.raises(ValueError, match="expected \\(B, N\\)"):
        GraphSegments.from_mask(torch.ones(3, dtype=torch.bool))
    s = GraphSegments.from_sizes((2, 3))
    with pytest.raises(ValueError, match="expected \\(2, N, ...\\)"):
        s.pack(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="the largest graph 3 nodes"):
        s.pack(torch.zeros(2, 2))
    with pytest.raises(ValueError, match="expected \\(5, ...\\)"):
        s.unpack(torch.zeros(4, 2))
    m = GraphSegments.from_mask(torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="come from a mask of shape \\(2, 3\\)"):
        m.pack(torch.zeros(2, 4))


# ------------------------------------------------------------------------------------------------ refusals of a packed call
def test_packed_calls_refuse_what_is_not_covered_before_any_launch():
    """on CPU tensors: every refusal comes before the device is looked at"""
    s = GraphSegments.from_sizes((3, 4))
    f, c = torch.zeros(7, 8), torch.zeros(7, 3)
    knn = dict(dim=8, num_nearest_neighbors=2)
    with pytest.raises(NotImplementedError, match="packed batch .* with adj_mat"):
        EGNN(**knn)(f, c, mask=s, adj_mat=torch.ones(7, 7, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="packed batch .* with adj_mat"):
        EGNN(**knn)(f, c, mask=s, adj_mat=SparseAdjacency.from_dense(torch.ones(7, 7, dtype=torch.bool)))
    with pytest.raises(NotImplementedError, match="packed batch .* with edges"):
        EGNN(edge_dim=2, **knn)(f, c, edges=torch.zeros(1, 7, 7, 2), mask=s)
    with pytest.raises(NotImplementedError, match="packed batch .* dense layer \\(num_nearest_neighbors = 0\\)"):
        EGNN(dim=8)(f, c, mask=s)
    with pytest.raises(NotImplementedError, match="graphed\\(\\): a GraphSegments"):
        graphed(EGNN(**knn), f, c, mask=s)
    with pytest.raises(NotImplementedError, match="packed batch .* global_linear_attn_every > 0"):
        EGNN_Network(depth=1, global_linear_attn_every=1, **knn)(f, c, mask=s)
    with pytest.raises(NotImplementedError, match="packed batch .* num_adj_degrees"):
        EGNN_Network(depth=1, num_adj_degrees=2, adj_dim=2, **knn)(f, c, mask=s, adj_mat=torch.ones(7, 7, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="packed batch .* with edges"):
        EGNN_Network(depth=1, edge_dim=2, **knn)(f, c, mask=s, edges=torch.zeros(1, 7, 7, 2))
    with pytest.raises(NotImplementedError, match="packed batch .* with adj_mat"):
        EGNN_Network(depth=1, **knn)(f, c, mask=s, adj_mat=torch.ones(7, 7, dtype=torch.bool))
    # shapes, and K against T (a graph below K is legal; K > T is torch.topk's error)
    with pytest.raises(ValueError, match="a packed batch takes \\(T,dim\\) and \\(T,C\\)"):
        EGNN(**knn)(f[None], c[None], mask=s)
    with pytest.raises(ValueError, match="feats holds 6 rows, the segments 7 nodes"):
        EGNN(**knn)(f[:6], c[:6], mask=s)
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        EGNN(dim=8, num_nearest_neighbors=8)(f, c, mask=s)
    with pytest.raises(ValueError, match="a packed batch of 7 nodes takes tokens \\(T,\\)"):
        EGNN_Network(depth=1, num_tokens=5, **knn)(torch.zeros(1, 7, dtype=torch.long), c, mask=s)
    with pytest.raises(AssertionError, match="number of positions 3"):
        EGNN_Network(depth=1, num_tokens=5, num_positions=3, **knn)(torch.zeros(7, dtype=torch.long), c, mask=s)


def test_chunk_pieces_keep_k_rows_each():
    from egnn_pytorch_amd.layer import _packed_pieces
    s = GraphSegments.from_sizes((40, 7, 96, 1, 33, 2))
    for limit, k in ((64, 8), (40, 8), (50, 4), (1000, 8), (16, 8)):
        pieces = _packed_pieces(s, limit, k)
        assert sum((p.sizes for _, p in pieces), ()) == s.sizes
        assert all(p.num_nodes >= k for _, p in pieces)
        assert all(sl.stop - sl.start == p.num_nodes and sl.start in s.host_offsets for sl, p in pieces)
        # within the limit -- except where a graph that leaves no K - 1 rows of room has to take a neighbour of fewer than K rows in
        assert all(p.num_nodes <= limit or max(p.sizes) > limit - (k - 1) for _, p in pieces), (limit, k)


# ------------------------------------------------------------------------------------------------ the C entries
ENTRIES = ("egnn_knn_select_segments_f32", "egnn_knn_select_segments_f64", "egnn_knn_segments_lds_nodes")


def test_new_entries_are_declared_bound_and_exported():
    prototypes, _, defines = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip.h"))
    lib = _abi.load()
    for sym in ENTRIES:
        assert sym in prototypes and sym in _abi.SIGNATURES and sym in _abi.SYMBOLS and hasattr(lib, sym), sym
    f32, f64 = prototypes[ENTRIES[0]], prototypes[ENTRIES[1]]
    assert f64 == (f32[0], [(ctype.replace("float", "double"), arg) for ctype, arg in f32[1]])
    assert _abi.SIGNATURES[ENTRIES[0]] == _abi.SIGNATURES[ENTRIES[1]]
    assert int(defines["EGNN_ABI_VERSION"]) == 44                                # additions do not bump it
    from egnn_pytorch_amd import _ops
    import egnn_pytorch_amd
    assert "GraphSegments" in egnn_pytorch_amd.__all__ and callable(_ops.knn_select_segments)
    build = open(os.path.join(ROOT, "egnn_pytorch_amd", "csrc", "build.sh")).read()
    assert build.count('[ "$f" = knn_segments ] && EXTRA="-ffp-contract=off"') == 2      # the object loop and the scratch re-compile


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_argument_checks_need_no_device(entry):
    """every argument check returns before anything is launched: made-up pointers, no GPU"""
    sel = getattr(_abi.load(), entry)
    fake = 4096                                          # (never dereferenced: every call below is refused first)

    def call(coors=fake, offsets=fake, segment_of=fake, g=3, t=100, k=8, cdim=3, largest=50, idx=fake, rank=fake):
        return sel(coors, offsets, segment_of, g, t, k, cdim, largest, idx, rank, None)

    for name in ("coors", "offsets", "segment_of", "idx", "rank"):               # EGNN_E_NULLPTR
        assert call(**{name: None}) == -1, name
    assert call(g=0) == -2 and call(t=0) == -2 and call(k=0) == -2               # EGNN_E_SHAPE
    assert call(largest=0) == -2 and call(largest=101) == -2
    assert call(cdim=0) == -3 and call(cdim=65) == -3                            # EGNN_E_UNSUPPORTED
    assert call(t=5000, largest=5000, k=1025) == -3
    assert call(k=101) == -5                                                     # EGNN_E_K_GT_N: K against T, torch.topk's error


def test_lds_window_knob_round_trips():
    knob = _abi.load().egnn_knn_segments_lds_nodes
    before = knob(-1)
    assert knob(-1) == before                            # a negative limit changes nothing
    assert knob(128) == before and knob(-1) == 128
    assert knob(0) == 128 and knob(-1) == 0              # 0: the built-in budget again
    knob(before)
