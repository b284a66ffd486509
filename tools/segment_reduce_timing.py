"""`GraphSegments.reduce(x, "sum")` against the three routes a packed batch had before it (MI355X; run from the repository root).

Shapes: the packed profile batch of tools/packed_timing.py (sizes log-uniform in 16 ... 2048 from seed 0 until T >= 65 536) at D = 128;
one graph of 1 048 576 rows at D = 64; 65 536 graphs of 4 rows at D = 1.  float32.
Routes, forward (rows -> graph rows) and training step (forward + backward of a sum-of-products loss to the rows' gradient):
  reduce        seg.reduce(x, "sum")                                    ordered, no atomics, no padding
  unpack        seg.unpack(x).sum(1)                                    the padded tensor and a dense sum (padding is zero)
  index_add     zeros(G, D).index_add_(0, segment_of, x)               float atomics
  segment_red.  torch.segment_reduce(x, "sum", offsets=...)            ATen's serial walk
A route that runs out of memory or is not implemented for the device reports why instead of a time.  Method: after 3 warm-up calls,
three device-event windows of back-to-back calls, each about 0.3 s long; time per call = the median window (fastest and slowest kept).
Achieved bandwidth = the bytes the reduction must move (T D read + G D written; the backward: G D read + T D written) over that time,
and its share of the 6.3 TB/s a streaming copy achieves on the MI355X.  One JSON line per (shape, route)."""
import json
import math
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import GraphSegments  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def draw_sizes(seed=0, target=65536):
    g = torch.Generator().manual_seed(seed)
    sizes = []
    while sum(sizes) < target:
        sizes.append(int(round(math.exp(float(torch.rand(1, generator=g)) * math.log(2048 / 16) + math.log(16)))))
    return tuple(sizes)


def timed(fn, windows=3, warm=3, seconds=0.3):
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
    calls = max(1, min(5000, int(seconds * 1e3 / max(window(1), 1e-3)) + 1))
    per = sorted(window(calls) for _ in range(windows))
    return dict(ms=per[len(per) // 2], fastest=per[0], slowest=per[-1], calls=calls)


def routes(seg):
    seg_of = seg.segment_of.to(torch.int64)
    lengths = torch.tensor(seg.sizes, device=seg.device)
    return {
        "reduce": lambda x: seg.reduce(x, "sum"),
        "unpack": lambda x: seg.unpack(x).sum(1),
        "index_add": lambda x: torch.zeros(seg.num_graphs, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, seg_of, x),
        "segment_reduce": lambda x: torch.segment_reduce(x, "sum", lengths=lengths, axis=0, unsafe=True),
    }


def main():
    shapes = (("profile", draw_sizes(), 128), ("one_graph", (1 << 20,), 64), ("tiny_graphs", (4,) * 65536, 1))
    for name, sizes, d in shapes:
        seg = GraphSegments.from_sizes(list(sizes), device="cuda")
        t, g = seg.num_nodes, seg.num_graphs
        x = torch.randn(t, d, device="cuda")
        w = torch.randn(g, d, device="cuda")
        want = seg.reduce(x.double(), "sum")
        bytes_fwd = 4 * (t * d + g * d)
        bytes_step = 2 * bytes_fwd
        for route, fn in routes(seg).items():
            row = dict(shape=name, graphs=g, rows=t, max_size=seg.max_size, d=d, route=route, padded_rows=g * seg.max_size)
            try:
                got = fn(x)
                row["max_error_vs_float64"] = float((got.double() - want).abs().max())
                row["repeatable_bits"] = bool(torch.equal(fn(x), got) and torch.equal(fn(x), got))
                fwd = timed(lambda: fn(x))

                def step():
                    xr = x.detach().requires_grad_(True)
                    (fn(xr) * w).sum().backward()
                    return xr.grad
                both = timed(step)
                row.update(forward_ms=fwd["ms"], forward_range=(fwd["fastest"], fwd["slowest"]), step_ms=both["ms"],
                           step_range=(both["fastest"], both["slowest"]),
                           forward_tb_s=bytes_fwd / fwd["ms"] / 1e9, forward_share_of_hbm=bytes_fwd / fwd["ms"] / 1e-3 / HBM_ACHIEVABLE,
                           step_tb_s_of_reduction_bytes=bytes_step / both["ms"] / 1e9)
            except (RuntimeError, NotImplementedError) as exc:
                row["failed"] = str(exc).splitlines()[0][:200]
                if "out of memory" not in str(exc).lower() and "not implemented" not in str(exc).lower() and "support" not in str(exc).lower():
                    print(json.dumps(row), flush=True)
                    raise
            print(json.dumps(row), flush=True)
        del x, w, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("segment_reduce_timing.py measures on the device: no GPU visible")
    main()
