"""Time per graph of the k-NN selection at C = 3, K = 32, B = 1 (MI355X; run from the repository root): the LDS kernel
(egnn_knn_select_f32) at N = 32 768 and the streaming entry (egnn_knn_select_stream_f32) at N = 32 768, 40 000, 65 536.  Device
events, 2 warm-up + median of 5 calls; one JSON line."""
import json
import sys

import torch

sys.path.insert(0, ".")
from egnn_pytorch_amd import _ops  # noqa: E402


def t(fn, n, k=32):
    g = torch.Generator().manual_seed(n)
    c = torch.randn(1, n, 3, generator=g).cuda()
    for _ in range(2):
        fn(c, None, None, k)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(c, None, None, k)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[2]


res = {"lds_32768_ms": t(_ops.knn_select, 32768)}
for n in (32768, 40000, 65536):
    res[f"stream_{n}_ms"] = t(_ops.knn_select_stream, n)
print(json.dumps(res))
