"""One ragged batch as a PACKED call and as the PADDED call it replaces (MI355X; run from the repository root).

The batch: graph sizes drawn once, log-uniform in 16 ... 2048 from a fixed seed, until T >= 65 536 nodes; dim 128, K = 32, C = 3.
Packed: feats (T, dim), coors (T, 3), mask=GraphSegments.  Padded: (G, N_max, .) with the prefix mask.  Per variant, after 2 warm-up
calls, three device-event windows of back-to-back calls, each about 0.3 s long (time per call: the median window, the fastest, the
slowest): the neighbour selection alone, the whole inference forward, the whole training step (forward + backward of a sum loss);
then the per-kernel times of one more forward under `phase_timer`, and the peak of torch.cuda.max_memory_allocated over a forward and
over a training step, counted from what was allocated before it (inputs and weights).

    python tools/packed_timing.py                    # packed and padded on the library of this tree
    EGNN_HIP_LIB=<parent's libegnn_hip.so> python tools/packed_timing.py --padded-only
                                                     # the same padded call on another build of the library (tools/ab_libs.sh's switch);
                                                     # a library from before this entry existed lacks the segmented selection, which the
                                                     # padded call does not need: its symbols are dropped from the binding first

One JSON line per variant, then one with everything (profiles/packed_batches/ab.txt)."""
import json
import math
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _abi  # noqa: E402

PADDED_ONLY = "--padded-only" in sys.argv
if PADDED_ONLY:
    for name in [n for n in _abi.SIGNATURES if "segments" in n]:
        del _abi.SIGNATURES[name]
    _abi.SYMBOLS = tuple(_abi.SIGNATURES)

from egnn_pytorch_amd import EGNN, GraphSegments, _ops, phase_timer  # noqa: E402

DIM, K, TARGET = 128, 32, 65536


def draw_sizes(seed=0):
    g = torch.Generator().manual_seed(seed)
    sizes = []
    while sum(sizes) < TARGET:
        sizes.append(int(round(math.exp(float(torch.rand(1, generator=g)) * math.log(2048 / 16) + math.log(16)))))
    return tuple(sizes)


def timed(fn, windows=3, warm=2, seconds=0.3):
    """time per call over `windows` device-event windows of back-to-back calls, each about `seconds` long: median, fastest, slowest"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()

    def window(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls
    calls = max(1, min(2000, int(seconds * 1e3 / max(window(1), 1e-3)) + 1))
    per = sorted(window(calls) for _ in range(windows))
    return {"median_ms": per[len(per) // 2], "min_ms": per[0], "max_ms": per[-1], "calls_per_window": calls}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def variant(layer, feats, coors, mask, select):
    def forward():
        with torch.no_grad():
            return layer(feats, coors, mask=mask)

    def step():
        f, x = feats.detach().requires_grad_(True), coors.detach().requires_grad_(True)
        node, co = layer(f, x, mask=mask)
        (node.sum() + co.sum()).backward()
        layer.zero_grad(set_to_none=True)

    row = {"rows": int(feats.numel() // DIM), "input_bytes": feats.numel() * 4 + coors.numel() * 4,
           "selection": timed(select), "forward": timed(forward), "train_step": timed(step),
           "forward_peak_bytes": peak_bytes(forward), "train_step_peak_bytes": peak_bytes(step)}
    with phase_timer() as t:
        forward()
    row["forward_kernels_ms"] = {k: round(sum(v), 4) for k, v in t.summary().items()}
    return row


def main():
    sizes = draw_sizes()
    seg = GraphSegments.from_sizes(sizes, device="cuda")
    g = torch.Generator().manual_seed(1)
    t = seg.num_nodes
    feats, coors = torch.randn(t, DIM, generator=g).cuda(), (torch.randn(t, 3, generator=g) * 3.0).cuda()
    torch.manual_seed(2)
    layer = EGNN(dim=DIM, num_nearest_neighbors=K).cuda()
    res = {"graphs": len(sizes), "nodes": t, "largest": max(sizes), "padded_rows": len(sizes) * max(sizes), "dim": DIM, "K": K,
           "library": _abi.lib_path()}
    fp, xp, pm = seg.unpack(feats), seg.unpack(coors), seg.prefix_mask()
    if not PADDED_ONLY:
        out = (torch.empty(t, K, dtype=torch.int32, device="cuda"), torch.empty(t, K, device="cuda"))
        res["packed"] = variant(layer, feats, coors, seg, lambda: _ops.knn_select_segments(coors, seg, K, out=out))
        print(json.dumps({"packed": res["packed"]}), flush=True)
    pout = (torch.empty(*fp.shape[:2], K, dtype=torch.int32, device="cuda"), torch.empty(*fp.shape[:2], K, device="cuda"))
    res["padded"] = variant(layer, fp, xp, pm, lambda: _ops.knn_select(xp, pm, None, K, out=pout))
    print(json.dumps({"padded": res["padded"]}), flush=True)
    if not PADDED_ONLY:
        with torch.no_grad():                                 # the two calls agree on the real nodes
            a, b = layer(feats, coors, mask=seg), layer(fp, xp, mask=pm)
        res["max_abs_difference"] = [float((a[i] - seg.pack(b[i])).abs().max()) for i in range(2)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
