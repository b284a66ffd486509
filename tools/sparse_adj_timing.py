"""A SparseAdjacency (CSR rows) against the dense-adjacency kernels on the same inputs (B = 1; MI355X; run from the repository root) at
N = 4 096, 16 384 and 65 536, on the two graphs of tools/adj_expand_timing.py -- the reference's chain with its diagonal and a random
symmetric graph with about 8 neighbours per row: the neighbour selection with an adjacency (K = 32), the N-degree expansion for
num_adj_degrees 2 and 3 (the CSR figure includes its one host read per degree), one inference forward of
EGNN_Network(depth=2, dim=32, num_nearest_neighbors=16, num_adj_degrees=2, adj_dim=4) and the peak device memory of that forward above
its inputs.  Then the sparse path alone at 262 144 nodes, where the dense map would be 64 GiB.
Device events, 2 warm-up + median of 5 calls, one process; one JSON line per graph.  `quick` runs toy sizes."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import EGNN_Network, SparseAdjacency, _ops  # noqa: E402

QUICK = "quick" in sys.argv[1:]
SIZES = (256, 512) if QUICK else (4096, 16384, 65536)
ALONE = 1024 if QUICK else 262144
K = 32


def edges(kind, n):
    """(2, E) int64 on the device"""
    i = torch.arange(n, device="cuda")
    if kind == "chain":
        return torch.cat([torch.stack([i, i]), torch.stack([i[:-1], i[1:]]), torch.stack([i[1:], i[:-1]])], dim=1)
    g = torch.Generator(device="cuda").manual_seed(n)
    j = torch.randint(0, n, (4 * n,), device="cuda", generator=g)
    r = i.repeat_interleave(4)
    return torch.cat([torch.stack([i, i]), torch.stack([r, j]), torch.stack([j, r])], dim=1)


def t(fn, *args):
    for _ in range(2):
        fn(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(sorted(ts)[2], 4)


def peak_mib(fn, *args):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(*args)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def measure(kind, n, dense):
    res = {"graph": kind, "n": n}
    sa = SparseAdjacency.from_edge_index(edges(kind, n), n)
    g = torch.Generator(device="cuda").manual_seed(1)
    coors = torch.randn(1, n, 3, device="cuda", generator=g) * (n ** (1 / 3))
    tokens = torch.randint(0, 20, (1, n), device="cuda", generator=g)
    torch.manual_seed(0)
    net = EGNN_Network(num_tokens=20, dim=32, depth=2, num_nearest_neighbors=16, num_adj_degrees=2, adj_dim=4).cuda()
    with torch.no_grad():
        for name in ("csr", "dense") if dense else ("csr",):
            adj = sa if name == "csr" else sa.to_dense()
            res[f"select_{name}_ms"] = t(_ops.knn_select, coors, None, adj, K)
            for d in (2, 3):
                expand = _ops.adj_expand_csr if name == "csr" else _ops.adj_expand
                try:
                    res[f"expand_d{d}_{name}_ms"] = t(expand, adj, 1, d)
                except (RuntimeError, torch.OutOfMemoryError) as err:       # (beyond 2^31 - 1 entries / device memory: said, not hidden)
                    res[f"expand_d{d}_{name}_ms"] = f"failed: {type(err).__name__}"
                torch.cuda.empty_cache()
            res[f"network_{name}_ms"] = t(lambda a: net(tokens, coors, adj_mat=a), adj)
            res[f"network_{name}_peak_mib"] = peak_mib(lambda a: net(tokens, coors, adj_mat=a), adj)
            del adj
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


for kind in ("chain", "random"):
    for n in SIZES:
        measure(kind, n, dense=True)
for kind in ("chain", "random"):
    measure(kind, ALONE, dense=False)
