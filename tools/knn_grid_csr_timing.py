"""Time per graph of the k-NN selection of a call with a SparseAdjacency at C = 3, K = 32, B = 1, unmasked (MI355X; run from the
repository root): the cell-grid entry with CSR rows (egnn_knn_select_grid_csr_f32: build passes, search and fallback launch) beside the
CSR streaming entry (egnn_knn_select_csr_f32, the route such calls took at every N before) on the same inputs in the same process.
N = 65 536, 262 144, 1 048 576; three geometries; four adjacencies (a chain with its diagonal plus sparse contacts, about 3 per row; random
directed, about 6 per row; the chain expanded to 3 degrees; one hub row of N / 4 bonds).  The outputs of the two are asserted equal
before anything is timed.  Device events, 2 warm-up + 5 timed calls per kernel: the grid's median and the streaming kernel's fastest run.
At 1 048 576 nodes one streaming call takes seconds: it runs ONCE there (the call whose outputs are compared), with no warm-up, and that
one time is reported.  One JSON line per (geometry, adjacency, N), then one JSON line with everything.
Usage: knn_grid_csr_timing.py [N ...]"""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import SparseAdjacency, _ops  # noqa: E402
from tools.knn_grid_timing import geometry, timed  # noqa: E402

K = 32
SIZES = (65536, 262144, 1048576)
STREAM_ONCE_N = 1048576            # from here the streaming kernel is timed on its one (compared) call


def chain_contacts(n):
    i = torch.arange(n)
    a = torch.arange(0, n - 40, 97)
    return torch.stack([torch.cat([i, i[:-1], i[1:], a, a + 31]), torch.cat([i, i[1:], i[:-1], a + 31, a])])


def adjacency(name, n):
    g = torch.Generator().manual_seed(n + 1)
    if name == "chain_contacts":
        return SparseAdjacency.from_edge_index(chain_contacts(n), n).to("cuda")
    if name == "random6":
        ei = torch.stack([torch.arange(n).repeat_interleave(6), torch.randint(0, n, (6 * n,), generator=g)])
        return SparseAdjacency.from_edge_index(ei, n).to("cuda")
    if name == "chain_3_degrees":
        return _ops.adj_expand_csr(SparseAdjacency.from_edge_index(chain_contacts(n), n).to("cuda"), 1, 3)[0]
    # one hub: row 0 bonded to N / 4 random nodes (and back), over the chain
    far = torch.randperm(n - 1, generator=g)[:n // 4] + 1
    hub = torch.stack([torch.cat([torch.zeros_like(far), far]), torch.cat([far, torch.zeros_like(far)])])
    return SparseAdjacency.from_edge_index(torch.cat([chain_contacts(n), hub], dim=1), n).to("cuda")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    sizes = tuple(int(a) for a in sys.argv[1:]) or SIZES
    res = {}
    for n in sizes:
        for aname in ("chain_contacts", "random6", "chain_3_degrees", "hub"):
            sa = adjacency(aname, n)
            for gname in ("uniform", "normal", "blobs"):
                c = geometry(gname, n).float().cuda()
                ws = _ops.knn_grid_workspace(1, n, K, c.device)
                out = (torch.empty(1, n, K, dtype=torch.int32, device="cuda"), torch.empty(1, n, K, device="cuda"))
                ref = (torch.empty_like(out[0]), torch.empty_like(out[1]))
                _ops.knn_select_grid(c, None, K, out=out, ws=ws, adj=sa)
                first = once(lambda: _ops.knn_select_csr(c, None, sa, K, out=ref))
                assert torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32)), (gname, aname, n)
                grid = timed(lambda: _ops.knn_select_grid(c, None, K, out=out, ws=ws, adj=sa))
                row = {"nnz_per_row": round(sa.col.numel() / n, 2), "max_degree": sa.max_degree(), "grid_median_ms": grid[2],
                       "grid_max_ms": grid[-1], "same_bits": True}
                if n >= STREAM_ONCE_N:
                    row.update(stream_min_ms=first, stream_calls=1)
                else:
                    stream = timed(lambda: _ops.knn_select_csr(c, None, sa, K, out=ref))
                    row.update(stream_min_ms=stream[0], stream_median_ms=stream[2], stream_calls=5)
                row["grid_wins"] = row["grid_median_ms"] < row["stream_min_ms"]
                res[f"{gname}_{aname}_{n}"] = row
                print(json.dumps({f"{gname}_{aname}_{n}": row}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
