"""Time per graph of the N-degree adjacency expansion (egnn_adj_expand_u8, B = 1; MI355X; run from the repository root) at
N = 4 096 (the one-word-per-lane kernel), 8 192, 16 384, 40 000 and 65 536 (the any-N kernel), on two graphs -- the reference's chain
with its diagonal and a random symmetric graph with about 8 neighbours per row -- for num_adj_degrees 2 and 3.  Next to it the
reference's recipe restated in torch ((A @ A) > 0 on 0/1 bf16 operands, fp32 accumulation, the XOR labelling; 8.6 GB of operand
at 65 536 nodes).
Device events, 2 warm-up + median of 5 calls; one JSON line.  `quick` runs toy sizes."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _ops  # noqa: E402

QUICK = "quick" in sys.argv[1:]
SIZES = (256, 512) if QUICK else (4096, 8192, 16384, 40000, 65536)


def graph(kind, n):
    i = torch.arange(n, device="cuda")
    if kind == "chain":
        return (i[:, None] - i[None, :]).abs() <= 1
    g = torch.Generator(device="cuda").manual_seed(n)
    j = torch.randint(0, n, (4 * n,), device="cuda", generator=g)
    adj = torch.zeros(n, n, dtype=torch.bool, device="cuda")
    adj[i.repeat_interleave(4), j] = True
    adj |= adj.T.clone()
    adj[i, i] = True
    return adj


def recipe(adj, degrees):
    labels = adj.to(torch.uint8)
    cur = adj
    for d in range(2, degrees + 1):
        a = cur.to(torch.bfloat16)
        nxt = (a @ a) > 0
        labels[nxt != cur] = d
        cur = nxt
    return cur, labels


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


res = {}
for kind in ("chain", "random"):
    for n in SIZES:
        adj = graph(kind, n)
        for d in (2, 3):
            res[f"{kind}_{n}_d{d}_ms"] = t(_ops.adj_expand, adj, 1, d)
            res[f"{kind}_{n}_d{d}_recipe_ms"] = t(recipe, adj, d)
        del adj
        torch.cuda.empty_cache()
print(json.dumps(res))
