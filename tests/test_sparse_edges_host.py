"""`SparseEdges` on the host (egnn_pytorch_amd/sparse_edges.py): every constructor round-trips through `to_dense()` for float values
and for tokens, a pattern of its own is kept (zero-valued entries included), validation errors, `graphs` and sharding; and the argument
checks of its four entries (csrc/edge_csr.hip, csrc/segment_sum.hip), which return before anything is launched."""
import ctypes

import pytest
import torch

from egnn_pytorch_amd import SparseAdjacency, SparseEdges, _abi, sharding


def _dense(kind, b=3, n=7, d=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(b, n, n, generator=g) < 0.35
    keep[1, 2] = False                                               # an empty row
    keep[:, 4, 4] = True                                             # diagonal entries
    if b > 2:
        keep[2] = False                                              # an empty graph inside the batch
    if kind == "tokens":
        return torch.randint(1, 5, (b, n, n), generator=g) * keep, keep
    return (torch.randn(b, n, n, d, generator=g) + 3.0) * keep[..., None], keep


@pytest.mark.parametrize("kind", ["float", "tokens"])
def test_from_dense_round_trip(kind):
    dense, keep = _dense(kind)
    se = SparseEdges.from_dense(dense)
    assert se.rowptr.dtype == torch.int64 and se.col.dtype == torch.int32 and se.rowptr.shape == (3, 8)
    assert se.col.numel() == int(keep.sum()) == se.values.shape[0]
    assert se.is_tokens == (kind == "tokens") and se.shape == tuple(dense.shape) and se.num_graphs == 3
    back = se.to_dense()
    assert back.dtype == dense.dtype and torch.equal(back, dense)
    SparseEdges(se.rowptr, se.col, se.values, se.n, validate=True)   # what the constructors build passes the validation
    assert torch.equal(se.adjacency().to_dense(), keep)


@pytest.mark.parametrize("kind", ["float", "tokens"])
def test_a_pattern_of_its_own_keeps_entries_whose_value_is_zero(kind):
    dense, keep = _dense(kind)
    g = torch.Generator().manual_seed(11)
    pattern = torch.rand(3, 7, 7, generator=g) < 0.5                 # neither a subset nor a superset of the non-zero pairs
    se = SparseEdges.from_dense(dense, pattern=pattern)
    assert se.col.numel() == int(pattern.sum())
    assert int((pattern & ~keep).sum()) > 0 and int((keep & ~pattern).sum()) > 0
    zero = dense.new_zeros(()) if kind == "tokens" else dense.new_zeros(dense.shape[-1])
    want = torch.where(pattern if kind == "tokens" else pattern[..., None], dense, zero)
    assert torch.equal(se.to_dense(), want)
    held_zero = (se.values == 0) if kind == "tokens" else (se.values == 0).all(-1)
    assert int(held_zero.sum()) == int((pattern & ~keep).sum())     # stored although their value is 0
    with pytest.raises(ValueError):
        SparseEdges.from_dense(dense, pattern=pattern[:, :, :6])


@pytest.mark.parametrize("kind", ["float", "tokens"])
def test_from_edge_index_any_order_and_from_adjacency(kind):
    dense, keep = _dense(kind)
    gi, ri, ci = keep.nonzero(as_tuple=True)
    perm = torch.randperm(gi.numel(), generator=torch.Generator().manual_seed(5))
    vals = dense[gi, ri, ci]
    se = SparseEdges.from_edge_index(torch.stack([ri, ci])[:, perm], vals[perm], 7, graph=gi[perm], num_graphs=3)
    assert torch.equal(se.to_dense(), dense)
    ref = SparseEdges.from_dense(dense)
    assert torch.equal(se.rowptr, ref.rowptr) and torch.equal(se.col, ref.col) and torch.equal(se.values, ref.values)
    # one graph, for B = 1 calls
    one = gi == 0
    s1 = SparseEdges.from_edge_index(torch.stack([ri[one], ci[one]]), vals[one], 7)
    assert s1.num_graphs == 1 and torch.equal(s1.to_dense(), dense[:1])
    # the pattern of a SparseAdjacency, values in the order of its col
    sa = SparseAdjacency.from_dense(keep)
    assert torch.equal(SparseEdges.from_adjacency(sa, ref.values).to_dense(), dense)
    shared = SparseAdjacency.from_dense(keep[0])                     # (one graph's rows: a B = 1 call)
    assert torch.equal(SparseEdges.from_adjacency(shared, vals[one]).to_dense(), dense[:1])
    with pytest.raises(ValueError):
        SparseEdges.from_adjacency(sa, ref.values[:-1])


def test_errors():
    ei = torch.tensor([[0, 1, 0], [1, 2, 1]])
    with pytest.raises(ValueError, match="twice"):
        SparseEdges.from_edge_index(ei, torch.ones(3, 2), 4)
    with pytest.raises(ValueError, match="twice"):                   # the same pair in the same graph only
        SparseEdges.from_edge_index(ei, torch.ones(3, dtype=torch.int64), 4, graph=torch.tensor([1, 0, 1]), num_graphs=2)
    SparseEdges.from_edge_index(ei, torch.ones(3, 2), 4, graph=torch.tensor([0, 0, 1]), num_graphs=2)
    with pytest.raises(ValueError):
        SparseEdges.from_edge_index(ei, torch.ones(2, 2), 4)         # values for two edges, three given
    with pytest.raises(ValueError):
        SparseEdges.from_edge_index(torch.tensor([[0], [4]]), torch.ones(1, 2), 4)
    with pytest.raises(ValueError):
        SparseEdges.from_edge_index(ei[:, :2], torch.ones(2, 2), 4, num_graphs=2)
    rowptr = torch.tensor([[0, 2, 3, 3]])
    col = torch.tensor([0, 2, 1], dtype=torch.int32)
    SparseEdges(rowptr, col, torch.ones(3, 2), 3)
    SparseEdges(rowptr, col, torch.ones(3, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="ascending"):
        SparseEdges(rowptr, torch.tensor([2, 0, 1], dtype=torch.int32), torch.ones(3, 2), 3)      # an unsorted row
    with pytest.raises(ValueError, match="ascending"):
        SparseEdges(rowptr, torch.tensor([2, 2, 1], dtype=torch.int32), torch.ones(3, 2), 3)      # a pair twice
    with pytest.raises(ValueError):
        SparseEdges(rowptr, col, torch.ones(2, 2), 3)                # values do not match col
    with pytest.raises(ValueError):
        SparseEdges(rowptr, col, torch.ones(3), 3)                   # float values are (nnz, d)
    with pytest.raises(ValueError):
        SparseEdges(rowptr, col, torch.ones(3, 1, dtype=torch.int64), 3)
    with pytest.raises(TypeError):
        SparseEdges(rowptr, col, torch.ones(3, dtype=torch.int32), 3)
    with pytest.raises(TypeError):
        SparseEdges(rowptr, col.long(), torch.ones(3, 2), 3)
    with pytest.raises(ValueError):
        SparseEdges(torch.tensor([[0, 2, 3, 4]]), col, torch.ones(3, 2), 3)
    with pytest.raises(ValueError):
        SparseEdges(rowptr, torch.tensor([0, 3, 1], dtype=torch.int32), torch.ones(3, 2), 3)     # a column outside [0, N)
    with pytest.raises(TypeError):
        SparseEdges.from_dense(torch.ones(1, 3, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        SparseEdges.from_dense(torch.ones(1, 3, 4, 2))


def test_values_keep_their_gradient():
    dense, _ = _dense("float")
    se = SparseEdges.from_dense(dense)
    vals = se.values.clone().requires_grad_()
    s2 = SparseEdges(se.rowptr, se.col, vals, se.n)
    assert s2.values is vals and s2.requires_grad
    w = torch.randn(dense.shape, generator=torch.Generator().manual_seed(1))
    (s2.to_dense() * w).sum().backward()
    assert vals.grad.shape == vals.shape
    assert torch.equal(SparseEdges(se.rowptr, se.col, vals.grad, se.n).to_dense(), w * (dense != 0).any(-1, keepdim=True))


def test_graphs_share_col_and_values_and_shard_batch_slices():
    dense, _ = _dense("float", b=5)
    se = SparseEdges.from_dense(dense)
    part = se.graphs(1, 4)
    assert part.num_graphs == 3 and part.col.data_ptr() == se.col.data_ptr() and part.values.data_ptr() == se.values.data_ptr()
    assert part.rowptr.data_ptr() == se.rowptr[1:].data_ptr()       # a slice: the offsets stay absolute
    assert torch.equal(part.to_dense(), dense[1:4])
    assert se.graphs(2, 2).num_graphs == 0
    with pytest.raises(IndexError):
        se.graphs(3, 6)
    feats = torch.zeros(5, 7, 2)
    got = []
    for rank in range(2):
        f, e = sharding.shard_batch(rank, 2, feats, se)
        lo, hi = sharding.shard_bounds(5, rank, 2)
        assert f.shape[0] == hi - lo and isinstance(e, SparseEdges) and e.col.data_ptr() == se.col.data_ptr()
        got.append(e.to_dense())
    assert torch.equal(torch.cat(got), dense)
    assert se.to("cpu") is se and se.device == se.col.device


def test_layer_and_network_refuse_what_a_sparse_edges_cannot_be():
    """the checks that need no device: the host raises before any kernel is reached"""
    from egnn_pytorch_amd import EGNN, EGNN_Network
    dense, _ = _dense("float", b=2, d=4)
    tok, _ = _dense("tokens", b=2)
    with pytest.raises(TypeError):
        EGNN(dim=8, edge_dim=4)(torch.zeros(2, 7, 8), torch.zeros(2, 7, 3), edges=SparseEdges.from_dense(tok))
    net = EGNN_Network(depth=1, dim=8, num_edge_tokens=5, edge_dim=4)
    with pytest.raises(TypeError):
        net(torch.zeros(2, 7, 8), torch.zeros(2, 7, 3), edges=SparseEdges.from_dense(dense))
    with pytest.raises(TypeError):
        EGNN_Network(depth=1, dim=8, edge_dim=4)(torch.zeros(2, 7, 8), torch.zeros(2, 7, 3), edges=SparseEdges.from_dense(tok))


def test_csr_entries_answer_their_argument_checks_before_any_launch():
    lib = _abi.load()
    fake = 4096                                                      # (never dereferenced: every call below is refused first)
    for sfx in ("_f32", "_f64"):
        gather = getattr(lib, "egnn_edge_features_gather_csr" + sfx)

        def call(rowptr=fake, values=fake, tokens=None, emb=None, d1=4, deg=None, deg_emb=None, d2=0, idx=fake, b=1, n=8, k=4,
                 pos=fake, out=fake):
            return gather(rowptr, fake, values, tokens, emb, d1, deg, deg_emb, d2, idx, b, n, k, pos, out, None)

        for name in ("rowptr", "pos", "out"):                        # EGNN_E_NULLPTR
            assert call(**{name: None}) == -1, name
        assert call(values=None, tokens=fake) == -1                  # tokens without their embedding table
        assert call(d2=2) == -1 and call(d2=2, deg=fake) == -1       # a second table without its labels / weights
        assert call(values=None) == -2 and call(tokens=fake, emb=fake) == -2     # EGNN_E_SHAPE: exactly one first table
        assert call(b=0) == -2 and call(n=0) == -2 and call(k=0) == -2 and call(d1=0) == -2 and call(d2=-1) == -2
        assert call(idx=None) == -2                                  # the dense layer has K = N

        grad = getattr(lib, "egnn_edge_features_grad_csr" + sfx)

        def gcall(g=fake, ld=8, pos=fake, tokens=fake, v1=5, d1=4, deg=fake, v2=3, d2=4, idx=fake, b=1, n=8, k=4, g_tok=fake,
                  g_deg=fake, g_val=None, work=None, size=0):
            nw = ctypes.c_int64(size)
            return grad(g, ld, pos, tokens, v1, d1, deg, v2, d2, idx, b, n, k, g_tok, g_deg, g_val, work, ctypes.byref(nw), None), nw.value

        rc, words = gcall()                                          # work == NULL: a size query, nothing is launched
        assert rc == 0 and words == 1 * (5 * 4 + 3 * 4)              # E = 32 edges: one partial of V1 d1 + V2 d2 elements
        assert gcall(pos=None)[0] == -1
        assert gcall(work=fake, size=words, g=None)[0] == -1
        assert gcall(work=fake, size=words - 1)[0] == -2             # a workspace one element short
        assert gcall(ld=7)[0] == -2 and gcall(b=0)[0] == -2 and gcall(idx=None)[0] == -2
        assert gcall(tokens=None)[0] == -2                           # g_tok_emb without tokens
        assert gcall(g_val=fake)[0] == -2                            # g_values belongs to float values, not to tokens
        assert gcall(tokens=None, g_tok=None, g_val=fake)[0] == 0
        assert gcall(d1=2049 if sfx == "_f32" else 1025, ld=4096)[0] == -3       # EGNN_E_UNSUPPORTED, as the dense entries
