"""Time per graph of the k-NN selection at C = 3, K = 32, B = 1, unmasked (MI355X; run from the repository root): the cell-grid entry
(egnn_knn_select_grid_f32: build passes, search and fallback launch) beside the streaming entry (egnn_knn_select_stream_f32) on the
same coordinates in the same process, N = 32 768 ... 1 048 576, three geometries.  Device events, 2 warm-up + 5 timed calls per
kernel: the grid's median and the streaming kernel's median and fastest run (the streaming kernel is skipped at the last size, where
one call takes seconds).  The outputs of the two are compared at every size both run.  One JSON line per (geometry, N), then one
JSON line with everything."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _ops  # noqa: E402

K = 32
SIZES = (32768, 65536, 131072, 262144, 1048576)
STREAM_MAX_N = 262144


def geometry(name, n):
    g = torch.Generator().manual_seed(n)
    if name == "uniform":
        return torch.rand(1, n, 3, generator=g)
    if name == "normal":
        return torch.randn(1, n, 3, generator=g)
    # 64 Gaussian blobs of unequal size: weights 1 .. 64, centres uniform in a cube of edge 40, unit spread
    w = torch.arange(1, 65, dtype=torch.float64)
    blob = torch.multinomial(w / w.sum(), n, replacement=True, generator=g)
    centres = torch.rand(64, 3, generator=g) * 40.0
    return (centres[blob] + torch.randn(n, 3, generator=g))[None]


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
    sizes = tuple(int(a) for a in sys.argv[1:]) or SIZES
    res = {}
    for name in ("uniform", "normal", "blobs"):
        for n in sizes:
            c = geometry(name, n).float().cuda()
            ws = _ops.knn_grid_workspace(1, n, K, c.device)
            out = (torch.empty(1, n, K, dtype=torch.int32, device="cuda"), torch.empty(1, n, K, device="cuda"))
            grid = timed(lambda: _ops.knn_select_grid(c, None, K, out=out, ws=ws))
            row = {"grid_median_ms": grid[2], "grid_max_ms": grid[-1]}
            if n <= STREAM_MAX_N:
                ref = (torch.empty_like(out[0]), torch.empty_like(out[1]))
                stream = timed(lambda: _ops.knn_select_stream(c, None, None, K, out=ref))
                row.update(stream_median_ms=stream[2], stream_min_ms=stream[0],
                           same_bits=bool(torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32))))
            res[f"{name}_{n}"] = row
            print(json.dumps({f"{name}_{n}": row}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
