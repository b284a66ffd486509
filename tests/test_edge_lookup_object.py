"""layer.EdgeLookup as a Python object, without a GPU: it holds N^2-sized label maps and table copies, so it must be freed by its
reference count the moment a forward or an autograd graph drops it (no reference cycle through its cache of converted copies), and
`to(dtype)` converts from the caller's tensors, not from an already rounded copy."""
import gc
import weakref

import torch


def _lookup(dtype=torch.float32, table_dtype=torch.float64):
    from egnn_pytorch_amd.layer import EdgeLookup
    g = torch.Generator().manual_seed(0)
    b, n = 2, 6
    return EdgeLookup(edges=None, tok=torch.randint(0, 4, (b, n, n), generator=g),
                      tok_emb=torch.randn(4, 3, dtype=table_dtype, generator=g),
                      deg=torch.randint(0, 3, (b, n, n), generator=g).to(torch.uint8),
                      deg_emb=torch.randn(3, 2, dtype=table_dtype, generator=g), dtype=dtype)


def test_edge_lookup_is_freed_by_reference_count():
    was = gc.isenabled()
    gc.disable()
    try:
        lk = _lookup()
        cast = lk.to(torch.float64)                     # (cached on lk)
        part = cast.graphs(0, 1)
        part.to(torch.float32)
        refs = [weakref.ref(o) for o in (lk, cast, part, lk.tok, lk.deg, cast.tok_emb)]
        del lk, cast, part
        assert [r() is None for r in refs] == [True] * len(refs)
    finally:
        if was:
            gc.enable()


def test_to_converts_from_the_callers_tensors_once():
    lk = _lookup(dtype=torch.float32)
    assert lk.tok_emb.dtype == torch.float32 and lk.to(torch.float32) is lk
    up = lk.to(torch.float64)
    assert up is lk.to(torch.float64) and up.dtype == torch.float64
    assert torch.equal(up.tok_emb, lk.live[1]) and torch.equal(up.deg_emb, lk.live[2])       # (not the fp32-rounded values)
    assert not torch.equal(lk.tok_emb.double(), lk.live[1])
    assert up.live is lk.live and up.tok is lk.tok and up.deg is lk.deg
    down = up.to(torch.float32)
    assert torch.equal(down.tok_emb, lk.tok_emb)


def test_graphs_slices_labels_and_dense_edges():
    from egnn_pytorch_amd.layer import EdgeLookup
    edges = torch.randn(3, 4, 4, 2, dtype=torch.float64)
    deg = torch.randint(0, 3, (3, 4, 4)).to(torch.uint8)
    lk = EdgeLookup(edges=edges, deg=deg, deg_emb=torch.randn(3, 2, dtype=torch.float64))
    part = lk.graphs(1, 3)
    assert torch.equal(part.deg, deg[1:3]) and torch.equal(part.edges, edges[1:3].float())
    assert torch.equal(part.to(torch.float64).edges, edges[1:3]) and part.to(torch.float64).deg_emb.dtype == torch.float64
    assert part.width == lk.width == 4
