"""A/B of the float64 k-NN selection at C = 3, K = 32, B = 1, unmasked (MI355X; run from the repository root): the cell grid
(`_ops.knn_select_grid` on float64 coordinates: egnn_knn_select_grid_f64 / _grid_csr_f64, build passes, search and fallback launch)
against the route float64 modules took at every size before (`_ops.knn_select` in float64: the streaming kernel, with a SparseAdjacency
its CSR instantiation), on the same coordinates in one process.  N = 70 000, 262 144, 1 048 576; normal and uniform coordinates; without
an adjacency and with a chain SparseAdjacency (the chain with its diagonal plus sparse contacts, about 3 per row).
The outputs of the two routes are asserted bit-equal first; those calls are the warm-up of both.  Then device-synchronised windows of
several calls each (a host clock around the calls and a synchronise), the two routes alternating, WINDOWS windows per route; reported per
route: the per-call time of every window, their median, and the spread (max - min) of the repeated windows.  Where one call of the
all-pairs route takes more than SLOW_CALL_S seconds its windows hold one call each.  One line per case, written as it is measured, to
stdout and to the file named by the first argument (profiles/knn_grid_f64/ab.txt is such a run).
Usage: knn_grid_f64_timing.py OUT.txt [N ...]"""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _ops  # noqa: E402
from tools.knn_grid_csr_timing import adjacency  # noqa: E402
from tools.knn_grid_timing import geometry  # noqa: E402

K = 32
SIZES = (70000, 262144, 1048576)
WINDOWS = 3
GRID_WINDOW_S = 0.5                # the grid: as many calls per window as fit in about this long (at least 5, at most 200)
PARENT_WINDOW_S = 1.0              # the all-pairs route: likewise (at least 1, at most 10)
SLOW_CALL_S = 5.0


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    out_path = sys.argv[1]
    sizes = tuple(int(a) for a in sys.argv[2:]) or SIZES
    lines = ["# float64 k-NN selection, K = 32, B = 1, C = 3, unmasked; ms per call; per route: every window, median, spread = max - min",
             "# geometry adjacency N | grid: windows -> median spread | all-pairs (parent's route): windows -> median spread | "
             "all-pairs / grid | grid faster by more than the all-pairs spread"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    for line in lines[:]:
        print(line, flush=True)
    for n in sizes:
        for aname in ("none", "chain"):
            sa = adjacency("chain_contacts", n) if aname == "chain" else None
            for gname in ("normal", "uniform"):
                c = geometry(gname, n).double().cuda()
                ws = _ops.knn_grid_workspace(1, n, K, c.device, torch.float64)
                out = (torch.empty(1, n, K, dtype=torch.int32, device="cuda"), torch.empty(1, n, K, dtype=torch.float64, device="cuda"))
                ref = (torch.empty_like(out[0]), torch.empty_like(out[1]))
                grid = lambda: _ops.knn_select_grid(c, None, K, out=out, ws=ws, adj=sa)      # noqa: E731
                parent = lambda: _ops.knn_select(c, None, sa, K, out=ref)                    # noqa: E731
                window(grid, 2)
                gfirst = window(grid, 2)
                first = window(parent, 1)
                assert torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int64), ref[1].view(torch.int64)), (gname, aname, n)
                pcalls = 1 if first > SLOW_CALL_S * 1e3 else max(1, min(10, int(PARENT_WINDOW_S * 1e3 / first)))
                gcalls = max(5, min(200, int(GRID_WINDOW_S * 1e3 / gfirst)))
                g, p = [], []
                for _ in range(WINDOWS):
                    g.append(window(grid, gcalls))
                    p.append(window(parent, pcalls))
                gm, pm = statistics.median(g), statistics.median(p)
                gs, ps = max(g) - min(g), max(p) - min(p)
                fmt = lambda v: " ".join(f"{x:.3f}" for x in v)                              # noqa: E731
                emit(f"{gname} {aname} {n} | grid ({gcalls} calls/window): {fmt(g)} -> {gm:.3f} {gs:.3f} | "
                     f"all-pairs ({pcalls} calls/window): {fmt(p)} -> {pm:.3f} {ps:.3f} | {pm / gm:.1f}x | "
                     f"{'yes' if pm - gm > ps else 'no'}")
                del c, ws, out, ref


if __name__ == "__main__":
    main()
