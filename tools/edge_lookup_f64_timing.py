"""One float64 EGNN_Network training step (forward + backward) on edge look-up tables, or on the materialised recipe (MI355X; run from
the repository root):  python tools/edge_lookup_f64_timing.py [lookup | materialised] [quick]
B = 1, N = 4 096 unit-normal nodes, a chain adjacency with fixed contacts and 3 degrees, 6 edge tokens, edge_dim = adj_dim = 8,
depth 2, K = 16, dim 16, the network converted with .double() (tests/test_gpu_edge_lookup_float64.py, the memory test).  "lookup" is
the network itself (the layers read the K selected pairs' embedding rows through egnn_edge_features_gather_f64, the embedding
gradients come from egnn_edge_features_grad_f64); "materialised" builds cat(edge_emb(tokens), adj_emb(labels)) as a dense float64
(1,N,N,16) tensor in torch and calls each EGNN layer with it -- what a float64 network did before it ran on the tables.
Device events, 2 warm-up + median of 5 steps, and the peak device memory of one step above its inputs; one JSON line
(DESIGN.md §4.7).  `quick` runs a toy size."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import EGNN_Network, _ops  # noqa: E402
from egnn_pytorch_amd.layer import _embed_pairs  # noqa: E402

MODE = "materialised" if "materialised" in sys.argv[1:] else "lookup"
N = 512 if "quick" in sys.argv[1:] else 4096


def materialised(net, tokens, coors, adj, edge_tok):
    feats = net.token_emb(tokens)
    adj_mat, deg = _ops.adj_expand(adj, 1, net.num_adj_degrees)
    edges = torch.cat((_embed_pairs(net.edge_emb, edge_tok), _embed_pairs(net.adj_emb, deg.long())), dim=-1)
    for _, egnn in net.layers:
        feats, coors = egnn(feats, coors, edges=edges, adj_mat=adj_mat)
    return feats, coors


def step(fn, coors):
    x = coors.clone().requires_grad_(True)
    h, co = fn(x)
    (h.sum() + co.sum()).backward()


def timed(fn, coors):
    for _ in range(2):
        step(fn, coors)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(fn, coors)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(fn, coors)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return round(sorted(ts)[2], 3), round(peak / 2**30, 3)


torch.manual_seed(0)
net = EGNN_Network(num_tokens=20, num_edge_tokens=6, edge_dim=8, dim=16, depth=2, num_nearest_neighbors=16, num_adj_degrees=3,
                   adj_dim=8).cuda().double()
i = torch.arange(N, device="cuda")
adj = (i[:, None] - i[None, :]).abs() <= 1
a = torch.arange(0, N - 40, 97, device="cuda")
adj[a, a + 31] = True
adj[a + 31, a] = True
tokens = torch.randint(0, 20, (1, N), device="cuda")
coors = torch.randn(1, N, 3, device="cuda", dtype=torch.float64)
edge_tok = torch.randint(0, 6, (1, N, N), device="cuda")
if MODE == "lookup":
    ms, gib = timed(lambda x: net(tokens, x, adj_mat=adj, edges=edge_tok), coors)
else:
    ms, gib = timed(lambda x: materialised(net, tokens, x, adj, edge_tok), coors)
print(json.dumps({"mode": MODE, "dtype": "float64", "n": N, "step_ms": ms, "peak_gib_above_inputs": gib}))
