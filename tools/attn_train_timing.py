"""One EGNN_Network training step (forward + backward) with a global attention block in front of every layer (MI355X; run from the
repository root): depth 4, dim 256, K = 32, heads 8 x dim_head 64, 4 global tokens, B = 16, N = 1024, fp32.  Two variants in one
process, alternating step by step: "hip" is the network as it is (the blocks on egnn_pytorch_amd/attention.py's autograd Functions:
split-f16 GEMMs and csrc/global_attn_bwd.hip), "aten" is the same network with each block's forward replaced, here, by the plain
module's lines (LayerNorm / Linear / matmul / softmax / GELU under ATen autograd).  "none" bypasses the blocks altogether: a variant's
step minus it is the blocks' share of that step.  Device events, 2 warm-up + median of 5 steps (and the spread: min .. max), and the
peak device memory of one step above its inputs; one JSON line.  `quick` runs a toy size; `trace` runs three
"hip" steps and nothing else, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/attn_train_timing.py trace
"""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import EGNN_Network  # noqa: E402

QUICK = "quick" in sys.argv[1:]
TRACE = "trace" in sys.argv[1:]
B, N, KW = (2, 128, dict(depth=2, dim=32, num_nearest_neighbors=8, global_linear_attn_heads=2, global_linear_attn_dim_head=8)) if QUICK else \
    (16, 1024, dict(depth=4, dim=256, num_nearest_neighbors=32, global_linear_attn_heads=8, global_linear_attn_dim_head=64))


def plain(blk):
    def forward(x, queries, mask=None):
        seq, tok = blk.norm_seq(x), blk.norm_queries(queries)
        induced = blk.attn1(tok, seq, mask=mask)
        x = blk.attn2(seq, induced) + x
        return blk.ff(x) + x, induced + queries
    return forward


def select(net, variant):
    for blk, _ in net.layers:
        blk.__dict__.pop("forward", None)
        if variant == "aten":
            blk.forward = plain(blk)
        elif variant == "none":
            blk.forward = lambda x, queries, mask=None: (x, queries)


def step(net, feats, coors):
    f, c = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
    h, co = net(f, c)
    (h.square().mean() + co.square().mean()).backward()
    net.zero_grad(set_to_none=True)


def timed_step(net, feats, coors):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(net, feats, coors)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak(net, feats, coors):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(net, feats, coors)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


torch.manual_seed(0)
net = EGNN_Network(global_linear_attn_every=1, **KW).cuda()
feats = torch.randn(B, N, KW["dim"], device="cuda")
coors = torch.randn(B, N, 3, device="cuda") * 4
if TRACE:
    for _ in range(3):
        step(net, feats, coors)
    torch.cuda.synchronize()
    sys.exit(0)
variants = ("hip", "aten", "none")
ts = {v: [] for v in variants}
for rep in range(7):                                         # (alternating: clock and cache state are shared by the variants)
    for v in variants:
        select(net, v)
        t = timed_step(net, feats, coors)
        if rep >= 2:
            ts[v].append(t)
res = {"B": B, "N": N, **{k: v for k, v in KW.items()}}
for v in variants:
    select(net, v)
    s = sorted(ts[v])
    res[f"{v}_ms"] = round(s[2], 3)
    res[f"{v}_ms_min_max"] = [round(s[0], 3), round(s[-1], 3)]
    res[f"{v}_peak_mib"] = peak(net, feats, coors)
for v in ("hip", "aten"):
    res[f"{v}_blocks_ms"] = round(res[f"{v}_ms"] - res["none_ms"], 3)
    res[f"{v}_blocks_share"] = round((res[f"{v}_ms"] - res["none_ms"]) / res[f"{v}_ms"], 3)
print(json.dumps(res))
