"""One force-matching training step of an EGNN_Network (MI355X; run from the repository root): depth 4, dim 128, K = 16, B = 32,
N = 256, fp32 -- E = net(feats, coors)[0] . w, F = -dE/d coors with create_graph=True, loss = mean (F - F_ref)^2, loss.backward().
"kernels" is the network itself (`_backward_twice` with the E x H block on csrc/edge_hidden.hip); "aten" is the same `_backward_twice`
with `EdgeHidden` replaced by its torch expression (autograd differentiates the E x H tensors twice).  Device events around the forward,
the create_graph backward and the second backward, 2 warm-up + median of 5 steps, and the peak device memory of one step above its
inputs; one JSON line ("Second order").  `quick` runs a toy size; `kernels` / `aten` runs only that variant (for a kernel
trace: rocprofv3 --kernel-trace --stats -- python tools/force_train_timing.py kernels)."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import EGNN_Network, autograd as A  # noqa: E402

QUICK = "quick" in sys.argv[1:]
B, N = (2, 64) if QUICK else (32, 256)


def step(net, feats, coors, w, f_ref, ev):
    x = coors.clone().requires_grad_(True)
    ev[0].record()
    h, _ = net(feats, x)
    ev[1].record()
    force = -torch.autograd.grad((h * w).sum(), x, create_graph=True)[0]
    ev[2].record()
    ((force - f_ref) ** 2).mean().backward()
    ev[3].record()


def timed(net, feats, coors, w, f_ref):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(2):
        step(net, feats, coors, w, f_ref, ev)
    torch.cuda.synchronize()
    parts = []
    for _ in range(5):
        step(net, feats, coors, w, f_ref, ev)
        torch.cuda.synchronize()
        parts.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
        net.zero_grad(set_to_none=True)
    med = [sorted(p[i] for p in parts)[2] for i in range(3)]
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(net, feats, coors, w, f_ref, ev)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    net.zero_grad(set_to_none=True)
    return [round(t, 3) for t in med] + [round(peak / 2**30, 3)]


torch.manual_seed(0)
net = EGNN_Network(depth=4, dim=128, num_nearest_neighbors=16).cuda()
feats = torch.randn(B, N, 128, device="cuda")
coors = torch.randn(B, N, 3, device="cuda") * 3
w = torch.randn(B, N, 128, device="cuda")
f_ref = torch.randn(B, N, 3, device="cuda")
res = {"B": B, "N": N}
ONLY = [a for a in sys.argv[1:] if a in ("kernels", "aten")]
for name, spec in (("kernels", False), ("aten", True)):
    if ONLY and name not in ONLY:
        continue
    A._EDGE_HIDDEN_SPEC = spec
    fwd, bwd1, bwd2, gib = timed(net, feats, coors, w, f_ref)
    res.update({f"{name}_forward_ms": fwd, f"{name}_create_graph_backward_ms": bwd1, f"{name}_second_backward_ms": bwd2,
                f"{name}_peak_gib": gib})
A._EDGE_HIDDEN_SPEC = False
print(json.dumps(res))
