"""Timing of egnn_edge_features_gather_csr_f32 (csrc/edge_csr.hip) against the dense egnn_edge_features_gather_f32 where the dense
tensor fits, and alone at 262 144 nodes.  Float values, d1 = 4, K = 32; device events around windows of calls,
the variants alternated, median and spread of 9 windows each; one JSON line per shape.

    python3 tools/edge_csr_gather_timing.py [--variant LIB]

--variant: a second library that exports egnn_edge_features_gather_csr_f32 (another build of edge_csr.hip), timed next to the product's
and compared with it bit for bit."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egnn_pytorch_amd import _abi, SparseEdges  # noqa: E402

ENTRY = "egnn_edge_features_gather_csr_f32"


def _ptr(t):
    return None if t is None else t.data_ptr()


def timed(fn, calls, reps=3):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / calls)
    return out


def pattern_edges(b, n, per_row, gen):
    """((2, E), graph): a chain with its diagonal plus random contacts, at most per_row entries per row, the same in every graph"""
    i = torch.arange(n)
    rows, cols = [i, i[:-1], i[1:]], [i, i[1:], i[:-1]]
    extra = max(0, per_row - 3)
    if extra:
        rows.append(i.repeat_interleave(extra))
        cols.append(torch.randint(0, n, (n * extra,), generator=gen))
    key = torch.unique(torch.cat(rows) * n + torch.cat(cols))
    r, c = key // n, key % n
    return torch.stack([r, c]).repeat(1, b), torch.arange(b).repeat_interleave(r.numel())


def local_selection(b, n, k, gen):
    """k distinct neighbours per node among the 2k nearest indices (what the k-NN list of a chain-like molecule looks like)"""
    off = torch.rand(b, n, 2 * k, generator=gen).topk(k, dim=-1).indices - k
    return ((torch.arange(n)[None, :, None] + off) % n).to(torch.int32).contiguous()


def case(lib, var, name, b, n, k, d1, per_row, dense_too, calls):
    gen = torch.Generator().manual_seed(1)
    ei, graph = pattern_edges(b, n, per_row, gen)
    se = SparseEdges.from_edge_index(ei, torch.randn(ei.shape[1], d1, generator=gen), n, graph=graph, num_graphs=b).to("cuda")
    idx = local_selection(b, n, k, gen).to("cuda")
    out, pos = torch.empty(b, n, k, d1, device="cuda"), torch.empty(b, n, k, dtype=torch.int32, device="cuda")
    args = (_ptr(se.rowptr), _ptr(se.col), _ptr(se.values), None, None, d1, None, None, 0, _ptr(idx), b, n, k)
    fns = {"csr": lambda: getattr(lib, ENTRY)(*args, _ptr(pos), _ptr(out), None)}
    assert fns["csr"]() == 0
    if var is not None:
        out2, pos2 = torch.empty_like(out), torch.empty_like(pos)
        fns["csr_variant"] = lambda: getattr(var, ENTRY)(*args, _ptr(pos2), _ptr(out2), None)
        assert fns["csr_variant"]() == 0
        torch.cuda.synchronize()
        assert torch.equal(pos, pos2) and torch.equal(out.view(torch.int32), out2.view(torch.int32)), "the variant differs"
    if dense_too:
        dense, ref = se.to_dense(), torch.empty_like(out)
        fns["dense"] = lambda: lib.egnn_edge_features_gather_f32(_ptr(dense), None, None, d1, None, None, 0, _ptr(idx), b, n, k,
                                                                 _ptr(ref), None)
        assert fns["dense"]() == 0
        torch.cuda.synchronize()
        assert torch.equal(ref.view(torch.int32), out.view(torch.int32)), "the CSR gather differs from the dense one"
    res = {key: [] for key in fns}
    for _ in range(3):                                               # alternate the variants
        for key, fn in fns.items():
            res[key] += timed(fn, calls)
    row = dict(case=name, B=b, N=n, K=k, d1=d1, nnz=int(se.col.numel()), max_row=int((se.rowptr[:, 1:] - se.rowptr[:, :-1]).max()),
               held=round(float((pos >= 0).float().mean()), 4))
    for key, ts in res.items():
        row[key + "_us_median"] = round(statistics.median(ts), 2)
        row[key + "_us_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this timing needs the MI355X")
    lib = _abi.load()
    var = None
    if a.variant:
        var = ctypes.CDLL(a.variant)
        getattr(var, ENTRY).restype, getattr(var, ENTRY).argtypes = _abi.SIGNATURES[ENTRY]
    case(lib, var, "bonds", 16, 1024, 32, 4, 5, True, 300)
    case(lib, var, "rows_of_48", 16, 1024, 32, 4, 48, True, 300)
    case(lib, var, "bonds_262144", 1, 262144, 32, 4, 5, False, 100)
    case(lib, var, "rows_of_48_262144", 1, 262144, 32, 4, 48, False, 100)


if __name__ == "__main__":
    main()
