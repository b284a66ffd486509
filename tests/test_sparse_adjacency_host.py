"""`SparseAdjacency` on the host (egnn_pytorch_amd/sparse_adj.py): constructors and `to_dense()` round trips, `graphs`, `max_degree`
against the oracle, validation errors, sharding; the argument checks of its entries (CSR selection, csrc/knn_stream.hip; CSR
expansion and slot labels, csrc/adj_csr.hip; gather / gradient by slot, csrc/segment_sum.hip), which return before anything is
launched (header, binding and library on those entries: tests/test_abi_agreement.py); and the expansion's rule restated on CSR rows
in plain Python against the oracle, which pins the XOR relabelling independently of the kernel."""
import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O


def _SA():
    from egnn_pytorch_amd import SparseAdjacency
    return SparseAdjacency


def _graphs():
    """name -> bool adjacency, (N, N) or (B, N, N): directed, with / without self loops, empty rows, empty graph, full rows"""
    g = torch.Generator().manual_seed(7)
    i = torch.arange(9)
    out = {
        "chain": (i[:, None] - i[None, :]).abs() == 1,
        "chain_diag": (i[:, None] - i[None, :]).abs() <= 1,
        "directed": torch.rand(11, 11, generator=g) < 0.25,
        "empty": torch.zeros(5, 5, dtype=torch.bool),
        "full": torch.ones(4, 4, dtype=torch.bool),
        "one_node": torch.ones(1, 1, dtype=torch.bool),
        "batched": torch.rand(3, 7, 7, generator=g) < 0.3,
        "batched_one": torch.rand(1, 6, 6, generator=g) < 0.3,
    }
    out["directed"][3] = False                                       # an empty row in the middle
    out["directed"][:, 5] = False                                    # ... and an empty column
    out["batched"][1] = False                                        # an empty graph inside a batch
    star = torch.zeros(8, 8, dtype=torch.bool)
    star[0, 1:] = True                                               # directed star: one full-ish row, seven empty ones
    out["star_out"] = star
    return out


@pytest.mark.parametrize("name", sorted(_graphs()))
def test_from_dense_round_trip(name):
    adj = _graphs()[name]
    sa = _SA().from_dense(adj)
    n = adj.shape[-1]
    assert sa.n == n and sa.num_graphs == (adj.shape[0] if adj.dim() == 3 else 1)
    assert sa.rowptr.dtype == torch.int64 and sa.col.dtype == torch.int32
    assert sa.rowptr.shape == ((adj.shape[0] if adj.dim() == 3 else 1), n + 1)
    dense = sa.to_dense()
    assert dense.dtype == torch.bool
    assert dense.shape == adj.shape and torch.equal(dense, adj)     # ((1, N, N) stays a batch of one graph)
    assert int(sa.rowptr[-1, -1]) == int(adj.sum()) == sa.col.numel()
    _SA()(sa.rowptr, sa.col, n, validate=True)                       # what the constructors build passes the validation
    assert sa.max_degree() == O.sparse_num_nearest(adj.numpy())


def test_from_edge_index_merges_sorts_and_keeps_direction_and_self_loops():
    SA = _SA()
    ei = torch.tensor([[4, 0, 4, 2, 2, 4, 0, 5], [1, 3, 0, 2, 2, 1, 3, 4]])       # unsorted, (4,1), (2,2), (0,3) duplicated, a self loop
    sa = SA.from_edge_index(ei, 6)
    want = torch.zeros(6, 6, dtype=torch.bool)
    want[ei[0], ei[1]] = True
    assert torch.equal(sa.to_dense(), want)
    assert not torch.equal(want, want.T) and want[2, 2]              # directed as given, the diagonal kept
    assert sa.col.tolist() == [3, 2, 0, 1, 4] and sa.rowptr.tolist() == [[0, 1, 1, 2, 2, 4, 5]]
    assert sa.max_degree() == 2 == O.sparse_num_nearest(want.numpy())
    assert torch.equal(SA.from_dense(want).rowptr, sa.rowptr) and torch.equal(SA.from_dense(want).col, sa.col)
    # no edge at all
    empty = SA.from_edge_index(torch.zeros(2, 0, dtype=torch.int64), 4)
    assert empty.max_degree() == 0 and not empty.to_dense().any() and empty.to_dense().shape == (4, 4)


def test_from_edge_index_batched():
    SA = _SA()
    g = torch.Generator().manual_seed(3)
    b, n, e = 4, 10, 60
    ei = torch.randint(0, n, (2, e), generator=g)
    graph = torch.randint(0, b, (e,), generator=g)
    graph[graph == 2] = 3                                            # graph 2 stays empty
    sa = SA.from_edge_index(ei, n, graph=graph, num_graphs=b)
    want = torch.zeros(b, n, n, dtype=torch.bool)
    want[graph, ei[0], ei[1]] = True
    assert sa.num_graphs == b and not sa.shared and sa.shape == (b, n, n)
    assert torch.equal(sa.to_dense(), want)
    assert sa.max_degree() == O.sparse_num_nearest(want.numpy())
    for lo, hi in ((0, 4), (1, 3), (2, 3), (3, 4), (2, 2)):
        part = sa.graphs(lo, hi)
        assert part.num_graphs == hi - lo and part.col is sa.col
        if hi > lo:
            assert torch.equal(part.to_dense().reshape(hi - lo, n, n), want[lo:hi])
            assert part.max_degree() == O.sparse_num_nearest(want[lo:hi].numpy())
            SA(part.rowptr, part.col, n, validate=True)              # absolute offsets: a slice is a valid object
    shared = SA.from_dense(want[0])
    assert shared.shared and shared.graphs(1, 3) is shared


def test_from_torch_sparse_coo_and_csr():
    SA = _SA()
    g = torch.Generator().manual_seed(11)
    dense = (torch.rand(12, 12, generator=g) < 0.2).float() * torch.randn(12, 12, generator=g)
    want = dense != 0
    for t in (dense.to_sparse(), dense.to_sparse_csr()):
        assert torch.equal(SA.from_torch_sparse(t).to_dense(), want)
    # an uncoalesced COO tensor with a stored zero: the pattern of the non-zero values
    t = torch.sparse_coo_tensor(torch.tensor([[0, 0, 1, 2], [1, 1, 2, 0]]), torch.tensor([1.0, 2.0, 0.0, 5.0]), (3, 3))
    assert SA.from_torch_sparse(t).to_dense().tolist() == [[False, True, False], [False, False, False], [True, False, False]]
    with pytest.raises(ValueError):
        SA.from_torch_sparse(torch.zeros(3, 4).to_sparse())
    with pytest.raises(TypeError):
        SA.from_torch_sparse(torch.zeros(3, 3))


def test_validation_errors():
    SA = _SA()
    rp = torch.tensor([[0, 2, 3, 3]])
    col = torch.tensor([0, 2, 1], dtype=torch.int32)
    assert SA(rp, col, 3).to_dense().tolist() == [[True, False, True], [False, True, False], [False, False, False]]
    assert SA(rp[0], col, 3).num_graphs == 1                         # a 1-D rowptr is one graph
    with pytest.raises(TypeError):
        SA(rp.int(), col, 3)
    with pytest.raises(TypeError):
        SA(rp, col.long(), 3)
    with pytest.raises(ValueError):
        SA(rp, col, 4)                                               # N + 1 offsets
    with pytest.raises(ValueError):
        SA(torch.tensor([[0, 2, 1, 3]]), col, 3)                     # decreasing offsets
    with pytest.raises(ValueError):
        SA(torch.tensor([[0, 2, 3, 4]]), col, 3)                     # past the end of col
    with pytest.raises(ValueError):
        SA(torch.tensor([[-1, 2, 3, 3]]), col, 3)
    with pytest.raises(ValueError):
        SA(rp, torch.tensor([0, 3, 1], dtype=torch.int32), 3)        # column out of range
    with pytest.raises(ValueError):
        SA(rp, torch.tensor([0, -1, 1], dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        SA(rp, torch.tensor([2, 0, 1], dtype=torch.int32), 3)        # descending inside a row
    with pytest.raises(ValueError):
        SA(rp, torch.tensor([1, 1, 1], dtype=torch.int32), 3)        # a duplicate inside a row
    SA(rp, torch.tensor([1, 2, 0], dtype=torch.int32), 3)            # (descending ACROSS rows is fine)
    with pytest.raises(ValueError):
        SA.from_edge_index(torch.tensor([[0], [3]]), 3)
    with pytest.raises(ValueError):
        SA.from_edge_index(torch.tensor([[0], [1]]), 3, graph=torch.tensor([2]), num_graphs=2)
    with pytest.raises(ValueError):
        SA.from_edge_index(torch.tensor([[0], [1]]), 3, num_graphs=2)
    with pytest.raises(TypeError):
        SA.from_dense(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        SA.from_dense(torch.zeros(3, 4, dtype=torch.bool))


def test_shard_batch_slices_a_batched_object_and_replicates_a_shared_one():
    from egnn_pytorch_amd import sharding
    SA = _SA()
    g = torch.Generator().manual_seed(5)
    adj = torch.rand(5, 6, 6, generator=g) < 0.4
    feats = torch.randn(5, 6, 2, generator=g)
    batched, shared = SA.from_dense(adj), SA.from_dense(adj[0])
    for rank in range(2):
        lo, hi = sharding.shard_bounds(5, rank, 2)
        f, a, s = sharding.shard_batch(rank, 2, feats, batched, shared, shared=(shared,))
        assert torch.equal(f, feats[lo:hi]) and s is shared
        assert torch.equal(a.to_dense().reshape(hi - lo, 6, 6), adj[lo:hi])
    with pytest.raises(ValueError):
        sharding.shard_batch(0, 2, feats, SA.from_dense(adj[:3]))
    # a batch of ONE graph stays batched: its image is (1, N, N) and it is sliced, not rejected, like the dense tensor
    one = SA.from_dense(adj[:1])
    assert one.batched and not one.shared and one.shape == (1, 6, 6) and one.to_dense().shape == (1, 6, 6)
    f, a = sharding.shard_batch(0, 1, feats[:1], one)
    assert torch.equal(a.to_dense(), adj[:1])
    assert SA.from_dense(adj[0]).shape == (6, 6) and SA(one.rowptr, one.col, 6).shared         # (raw constructor: G = 1 is shared ...)
    assert SA(one.rowptr, one.col, 6, batched=True).shape == (1, 6, 6)                          # (... unless told otherwise)
    with pytest.raises(ValueError):
        SA(SA.from_dense(adj).rowptr, SA.from_dense(adj).col, 6, batched=False)
    assert one.to(one.device) is one and one.to("cpu") is one


def test_graphed_refuses_the_csr_expansion_before_any_forward():
    """num_adj_degrees > 1 with a SparseAdjacency reads entry counts back per degree: graphed() says so up front (no device needed)."""
    from egnn_pytorch_amd import EGNN_Network, graphed
    sa = _SA().from_dense(_graphs()["chain"])
    net = EGNN_Network(depth=1, dim=8, num_adj_degrees=2, adj_dim=4, only_sparse_neighbors=True)
    with pytest.raises(NotImplementedError, match="cannot be captured"):
        graphed(net, torch.randn(1, 9, 8), torch.randn(1, 9, 3), adj_mat=sa)


@pytest.mark.parametrize("sym", ["egnn_knn_select_csr_f32", "egnn_knn_select_csr_f64"])
def test_csr_argument_checks_need_no_device(sym):
    """Every argument check returns before anything is launched: they run without a GPU."""
    from egnn_pytorch_amd import _abi
    sel = getattr(_abi.load(), sym)
    fake = 4096                                                      # (never dereferenced: every call below is refused first)
    assert sel(None, None, fake, fake, 0, 1, 100, 8, 3, fake, fake, None) == -1
    assert sel(fake, None, None, fake, 0, 1, 100, 8, 3, fake, fake, None) == -1            # rowptr
    assert sel(fake, None, fake, fake, 0, 1, 100, 8, 3, None, fake, None) == -1
    assert sel(fake, None, fake, fake, 0, 1, 100, 8, 3, fake, None, None) == -1
    assert sel(fake, None, fake, fake, 100, 2, 100, 8, 3, fake, fake, None) == -2          # a graph stride other than 0 or N + 1
    assert sel(fake, None, fake, fake, 0, 0, 100, 8, 3, fake, fake, None) == -2
    assert sel(fake, None, fake, fake, 0, 1, 0, 8, 3, fake, fake, None) == -2
    assert sel(fake, None, fake, fake, 0, 1, 100, 0, 3, fake, fake, None) == -2
    assert sel(fake, None, fake, fake, 101, 2, 100, 101, 3, fake, fake, None) == -5        # K > N (torch.topk's error upstream)
    assert sel(fake, None, fake, fake, 0, 1, 100, 8, 0, fake, fake, None) == -3            # coor_dim outside 1 .. 64
    assert sel(fake, None, fake, fake, 0, 1, 100, 8, 65, fake, fake, None) == -3
    assert sel(fake, None, fake, fake, 0, 1, 2000, 1025, 3, fake, fake, None) == -3        # K beyond the kernel's limit
    assert sel(fake, None, fake, fake, 0, 65536, 100, 8, 3, fake, fake, None) == -3


def test_expansion_and_slot_label_argument_checks_need_no_device():
    import ctypes
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    ws = lib.egnn_adj_csr_workspace_bytes
    assert ws(0, 5) == 0 and ws(1, 1) > 0
    for g, n in ((1, 1), (3, 100), (1, 70000), (2, 262144)):
        assert 0 < ws(g, n) <= ws(g + 1, n) and ws(g, n) <= ws(g, n + 1)
    fake, big = 4096, ws(2, 100)
    count, fill = lib.egnn_adj_csr_square_count, lib.egnn_adj_csr_square_fill
    assert count(None, fake, fake, fake, 2, 100, fake, fake, fake, fake, big, 0, None) == -1
    assert count(fake, fake, fake, fake, 2, 100, None, fake, fake, fake, big, 0, None) == -1
    assert count(fake, fake, fake, fake, 2, 100, fake, fake, None, fake, big, 0, None) == -1
    assert count(fake, fake, fake, fake, 2, 100, fake, fake, fake, None, big, 0, None) == -1
    assert count(fake, fake, fake, fake, 0, 100, fake, fake, fake, fake, big, 0, None) == -2
    assert count(fake, fake, fake, fake, 2, 100, fake, fake, fake, fake, big - 1, 0, None) == -2        # a workspace one byte short
    assert count(fake, fake, fake, fake, 2, 100, fake, fake, fake, fake + 4, big, 0, None) == -4        # alignment
    assert count(fake, fake, fake, fake, 65536, 1, fake, fake, fake, fake, ws(65536, 1), 0, None) == -3
    ok = (fake, fake, fake, fake, fake, 2, 100)
    assert fill(*ok, 1, fake, fake, 10, fake, fake, fake, 10, fake, big, 0, None) == -2                  # degree < 2
    assert fill(*ok, 256, fake, fake, 10, fake, fake, fake, 10, fake, big, 0, None) == -3
    assert fill(*ok, 2, fake, fake, 2 ** 31, fake, fake, fake, 10, fake, big, 0, None) == -2             # nnz beyond 2^31 - 1
    assert fill(*ok, 2, fake, fake, 10, fake, fake, fake, 2 ** 31, fake, big, 0, None) == -2
    assert fill(*ok, 2, fake, None, 10, fake, fake, fake, 10, fake, big, 0, None) == -1
    assert fill(*ok, 2, None, fake, 10, fake, fake, fake, 10, fake, big, 0, None) == -1
    slot = lib.egnn_csr_slot_labels_u8
    assert slot(None, fake, fake, 0, fake, 1, 10, 4, fake, None) == -1
    assert slot(fake, fake, fake, 0, fake, 1, 10, 4, None, None) == -1
    assert slot(fake, fake, fake, 10, fake, 1, 10, 4, fake, None) == -2                                  # stride: 0 or N + 1
    assert slot(fake, fake, fake, 0, None, 1, 10, 4, fake, None) == -2                                   # dense layer: K == N
    assert slot(fake, fake, fake, 0, fake, 0, 10, 4, fake, None) == -2
    nw = ctypes.c_int64(0)
    for name in ("egnn_edge_features_grad_slot_f32", "egnn_edge_features_grad_slot_f64"):               # the size query of the dense entries
        ref = ctypes.c_int64(0)
        args = (None, 8, None, 0, 0, fake, 4, 4, fake, 2, 50, 6, None, fake, None, None)
        assert getattr(lib, name)(*args, ctypes.byref(nw), None) == 0
        assert getattr(lib, name.replace("_slot", ""))(*args, ctypes.byref(ref), None) == 0
        assert nw.value == ref.value > 0
    for name in ("egnn_edge_features_gather_slot_f32", "egnn_edge_features_gather_slot_f64"):
        assert getattr(lib, name)(None, None, None, 0, fake, fake, 4, fake, 1, 10, 4, None, None) == -1
        assert getattr(lib, name)(None, None, None, 0, None, fake, 4, fake, 1, 10, 4, fake, None) == -1


# ------------------------------------------------------------------ the expansion's rule, restated on CSR rows in plain Python
def _csr_expand(rows, degrees):
    """rows: list of sorted column lists.  Returns (final rows, labels as a list of {column: label}) by the rule of
    egnn_pytorch.py:414-427 on sets: nxt = pattern(cur . cur), labels[nxt XOR cur] = t -- what csrc/adj_csr.hip computes."""
    cur = [set(r) for r in rows]
    labels = [{c: 1 for c in r} for r in rows]
    for t in range(2, degrees + 1):
        nxt = [set().union(*(cur[j] for j in cur[i])) if cur[i] else set() for i in range(len(cur))]
        for i in range(len(cur)):
            for c in nxt[i] ^ cur[i]:                                # (an entry of cur missing from nxt is relabelled too)
                labels[i][c] = t
        cur = nxt
    return [sorted(r) for r in cur], labels


@pytest.mark.parametrize("degrees", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["chain", "chain_nodiag", "random_asymmetric", "star"])
def test_csr_restatement_of_the_expansion_equals_the_oracle(kind, degrees):
    n = 13
    i = np.arange(n)
    if kind == "chain":
        adj = np.abs(i[:, None] - i[None, :]) <= 1
    elif kind == "chain_nodiag":
        adj = np.abs(i[:, None] - i[None, :]) == 1
    elif kind == "star":
        adj = np.zeros((n, n), dtype=bool)
        adj[0, 1:] = adj[1:, 0] = True
    else:
        adj = np.random.default_rng(2).random((n, n)) < 0.15
    sa = _SA().from_dense(torch.from_numpy(adj))
    rp, col = sa.rowptr[0].tolist(), sa.col.tolist()
    rows, labels = _csr_expand([col[rp[r]:rp[r + 1]] for r in range(n)], degrees)
    ref_lab, ref_adj = O.adjacency_degrees(adj[None], degrees)
    got_adj = np.zeros((n, n), dtype=bool)
    got_lab = np.zeros((n, n), dtype=np.int64)
    for r in range(n):
        got_adj[r, rows[r]] = True
        for c, v in labels[r].items():
            got_lab[r, c] = v
    np.testing.assert_array_equal(got_adj, ref_adj[0])
    np.testing.assert_array_equal(got_lab, ref_lab[0])
    if kind in ("chain_nodiag", "star") and degrees >= 2:
        assert (got_lab[~got_adj] > 0).any()                         # the quirk: labelled pairs that left the adjacency
