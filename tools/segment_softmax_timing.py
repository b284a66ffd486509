"""`GraphSegments.attention_pool(scores, values)` against the three routes a packed batch had before it (MI355X; run from the repository
root).  The method and the shapes of tools/segment_reduce_timing.py.

Shapes: the packed profile batch of tools/packed_timing.py (sizes log-uniform in 16 ... 2048 from seed 0 until T >= 65 536) at H = 8,
Dv = 64; one graph of 1 048 576 rows at H = 1, Dv = 64; 65 536 graphs of 4 rows at H = Dv = 1.  float32.
Routes, forward and training step (forward + backward of a sum-of-products loss to the gradients of scores and values):
  attention_pool  seg.attention_pool(scores, values)                     ordered, no atomics, no padding, one pass over values
  unpack          seg.unpack, masked_fill(-inf), torch.softmax over the node axis, einsum         the padded tensors
  scatter         scatter_reduce(amax) + exp + index_add_ (the sums) + index_add_ (the pool)       float atomics
  compose         reduce("max"), broadcast, exp, reduce("sum"), broadcast, multiply, reduce("sum") seven launches, (T, H Dv) temporaries
A route that runs out of memory or is not implemented for the device reports why instead of a time.  Method: after 3 warm-up calls,
three device-event windows of back-to-back calls, each about 0.3 s long; time per call = the median window (fastest and slowest kept).
Achieved bandwidth = the bytes the pool must move (T H Dv + 2 T H read, G H Dv written) over the forward's time, and its share of the
6.3 TB/s a streaming copy achieves on the MI355X.  One JSON line per (shape, route)."""
import json
import math
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import GraphSegments  # noqa: E402
from tools.segment_reduce_timing import HBM_ACHIEVABLE, draw_sizes, timed  # noqa: E402


def routes(seg):
    seg_of = seg.segment_of.to(torch.int64)
    mask = seg.prefix_mask()
    g = seg.num_graphs

    def unpack(s, v):
        sp = seg.unpack(s).masked_fill(~mask[..., None], -math.inf)
        return torch.einsum("gnh,gnhd->ghd", torch.softmax(sp, 1), seg.unpack(v))

    def scatter(s, v):
        idx = seg_of[:, None].expand_as(s)
        m = torch.full((g, s.shape[1]), -math.inf, dtype=s.dtype, device=s.device).scatter_reduce(0, idx, s, "amax")
        e = torch.exp(s - m[seg_of])
        l = torch.zeros_like(m).index_add_(0, seg_of, e)
        return torch.zeros(g, *v.shape[1:], dtype=v.dtype, device=v.device).index_add_(0, seg_of, (e / l[seg_of])[..., None] * v)

    def compose(s, v):
        e = torch.exp(s - seg.broadcast(seg.reduce(s, "max")))
        w = e / seg.broadcast(seg.reduce(e, "sum"))
        return seg.reduce(w[..., None] * v, "sum")

    return {"attention_pool": seg.attention_pool, "unpack": unpack, "scatter": scatter, "compose": compose}


def main():
    shapes = (("profile", draw_sizes(), 8, 64), ("one_graph", (1 << 20,), 1, 64), ("tiny_graphs", (4,) * 65536, 1, 1))
    for name, sizes, h, dv in shapes:
        seg = GraphSegments.from_sizes(list(sizes), device="cuda")
        t, g = seg.num_nodes, seg.num_graphs
        s, v = torch.randn(t, h, device="cuda"), torch.randn(t, h, dv, device="cuda")
        w = torch.randn(g, h, dv, device="cuda")
        want = seg.attention_pool(s.double(), v.double())
        bytes_fwd = 4 * (t * h * dv + 2 * t * h + g * h * dv)
        for route, fn in routes(seg).items():
            row = dict(shape=name, graphs=g, rows=t, max_size=seg.max_size, h=h, dv=dv, route=route, padded_rows=g * seg.max_size)
            try:
                got = fn(s, v)
                row["max_error_vs_float64"] = float((got.double() - want).abs().max())
                row["repeatable_bits"] = bool(torch.equal(fn(s, v), got) and torch.equal(fn(s, v), got))
                fwd = timed(lambda: fn(s, v))

                def step():
                    sr, vr = s.detach().requires_grad_(True), v.detach().requires_grad_(True)
                    (fn(sr, vr) * w).sum().backward()
                    return sr.grad, vr.grad
                both = timed(step)
                row.update(forward_ms=fwd["ms"], forward_range=(fwd["fastest"], fwd["slowest"]), step_ms=both["ms"],
                           step_range=(both["fastest"], both["slowest"]),
                           forward_tb_s=bytes_fwd / fwd["ms"] / 1e9, forward_share_of_hbm=bytes_fwd / fwd["ms"] / 1e-3 / HBM_ACHIEVABLE)
            except (RuntimeError, NotImplementedError) as exc:
                row["failed"] = str(exc).splitlines()[0][:200]
                if "out of memory" not in str(exc).lower() and "not implemented" not in str(exc).lower() and "support" not in str(exc).lower():
                    print(json.dumps(row), flush=True)
                    raise
            print(json.dumps(row), flush=True)
        del s, v, w, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("segment_softmax_timing.py measures on the device: no GPU visible")
    main()
