"""Time per call of the all-pairs k-NN selection entries at sizes a user would run (MI355X; run from the repository root): one shape per
kernel family -- the register kernel, the keys-in-LDS row kernel in its four instantiations, the streaming kernel in float32 (C = 3 and C = 5)
and float64.  Normal coordinates from a fixed seed, unmasked, no adjacency.  Device events, 2 warm-up + 5 timed calls per shape
(`--reps N`: another number of timed calls), the median and the fastest.  One JSON line per shape, then one with everything.

    python tools/knn_select_timing.py
    EGNN_HIP_LIB=<another libegnn_hip.so> python tools/knn_select_timing.py      # the same calls on another build of the library

Two builds are compared by alternating such processes (profiles/knn_core/ab.txt)."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _ops  # noqa: E402

# (name, dtype, B, N, C, K): all through `knn_select`, which routes
SHAPES = (
    ("f32_c3_register", torch.float32, 64, 1024, 3, 32),
    ("f32_c3_rows", torch.float32, 1, 16384, 3, 32),
    ("f32_c5_rows", torch.float32, 1, 6000, 5, 24),
    ("f32_c12_rows", torch.float32, 2, 2048, 12, 16),
    ("f64_c3_rows", torch.float64, 4, 4096, 3, 32),
    ("f32_stream", torch.float32, 1, 40000, 3, 32),
    ("f64_stream", torch.float64, 1, 24000, 3, 16),
    ("f32_c5_stream", torch.float32, 1, 36000, 5, 24),
)


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    res = {}
    for name, dtype, b, n, c, k in SHAPES:
        g = torch.Generator().manual_seed(n + c)
        coors = torch.randn(b, n, c, generator=g, dtype=torch.float64).to(dtype).cuda()
        out = (torch.empty(b, n, k, dtype=torch.int32, device="cuda"), torch.empty(b, n, k, dtype=dtype, device="cuda"))
        ts = timed(lambda: _ops.knn_select(coors, None, None, k, out=out), reps=reps)
        res[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "idx_sum": int(out[0].sum(dtype=torch.int64))}
        print(json.dumps({name: res[name]}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
