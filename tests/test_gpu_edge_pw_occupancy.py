"""csrc/edge_pw.hip at six workgroups per CU: at most 80 vector registers, no scratch, 26 KB of LDS -- the next round's slot records and
the epilogue's scratch live in the wave's idle gather exchange rows, the epilogue re-reads x_i - x_j from memory.  The results must be
what they were: the wave-per-node kernel against the general kernel (csrc/edge_fused.hip, forced through layer._EDGE_ALGO as in
tests/test_gpu_kernels.py) bit for bit, and against the float64 oracle within bar (a) of tests/test_gpu_edge_variants.py,
1e-4 max(1, max|want| / 256), at the smallest shapes that walk the ring, the record hand-over and the skip paths.  The host test reads
the compiler's resource-usage remarks that csrc/build.sh leaves in csrc/obj/edge_pw.res."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840
WGS = 6

# (id, dim, K, N, B, mask): "ragged" = graph 0 with 37 real nodes (27 padded: whole padded groups), the LAST graph all padding
CASES = [
    ("dim8_one_chunk_half_tail", 8, 32, 64, 2, None),           # Hp = 64: one ring chunk per round; the last step is the half tail step
    ("dim24_n33_waves_past_the_end", 24, 32, 33, 1, None),      # Hp = 128; the last group holds one live wave
    ("dim128_b3", 128, 32, 64, 3, None),
    ("dim64_k64_two_rounds", 64, 64, 96, 1, None),              # the MULTI instantiation: records handed over between a node's rounds
    ("dim512_ring_wraps", 512, 32, 64, 1, None),                # Hp = 2080: 33 chunks, the ring wraps between rounds
    ("dim8_ragged_padded_group_and_graph", 8, 32, 64, 2, "ragged"),
]
_BY_ID = {c[0]: c for c in CASES}
_cache = {}


def _case(cid):
    """layer, inputs and the general kernel's outputs of a case: built once, shared, never modified"""
    if cid in _cache:
        return _cache[cid]
    from egnn_pytorch_amd import EGNN
    _, dim, k, n, b, mk = _BY_ID[cid]
    g = torch.Generator().manual_seed(dim * 1009 + k * 31 + n + b)
    layer = EGNN(dim=dim, num_nearest_neighbors=k)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, generator=g)
    layer = layer.cuda().eval()
    feats = torch.randn(b, n, dim, generator=g).cuda()
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = None
    if mk == "ragged":
        mask = torch.zeros(b, n, dtype=torch.bool)
        mask[0, :37] = True
        mask = mask.cuda()
    with torch.no_grad(), _algo(1):
        ref = layer(feats, coors, mask=mask)
    _cache[cid] = (layer, feats, coors, mask, ref)
    return _cache[cid]


class _algo:
    def __init__(self, algo):
        self.algo = algo

    def __enter__(self):
        from egnn_pytorch_amd import layer as L
        self.old, L._EDGE_ALGO = L._EDGE_ALGO, self.algo

    def __exit__(self, *exc):
        from egnn_pytorch_amd import layer as L
        L._EDGE_ALGO = self.old


def _remarks():
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    res = os.path.join(pkg, "csrc", "obj", "edge_pw.res")
    assert os.path.exists(res), "libegnn_hip.so exists but csrc/obj/edge_pw.res does not: build with csrc/build.sh"
    out, name = {}, None
    for line in open(res):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)", line)
        if m and name:
            out[name][m.group(1)] = m.group(2)
    return out


def test_both_instantiations_fit_six_workgroups_per_cu():
    """Host only; pins the DEFAULT build (csrc/build.sh without -DEGNN_PW_WGS: a library built with the knob at 5 for an A/B goes into
    its own directory, tools/variants.py, and is not what this reads).  Six waves per SIMD need at most 80 of the 512 unified registers (granule 8), AGPRs included; six workgroups need 6 x
    (LDS size rounded up to the allocation granule) <= 163 840 bytes -- asserted for every granule the toolchain has used on this
    family (512, 1280 and 2048 bytes) and against the occupancy the compiler itself derives from registers AND LDS."""
    rem = {k: v for k, v in _remarks().items() if "edge_pw_kernel" in k}
    assert sorted("ILb0E" in k for k in rem) == [False, True] and len(rem) == 2, sorted(rem)
    for name, r in rem.items():
        print(name, r)
        assert int(r["VGPRs"]) + int(r["AGPRs"]) <= 80, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (name, r)
        lds = int(r["LDS Size [bytes/block]"])
        for granule in (512, 1280, 2048):
            assert WGS * (-(-lds // granule) * granule) <= LDS_PER_CU, (name, lds, granule)
        assert int(r["Occupancy [waves/SIMD]"]) == WGS, (name, r)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_wave_per_node_kernel_equals_the_general_one_and_the_oracle(cid):
    from egnn_pytorch_amd import _ops
    from oracle import egnn_oracle as O
    layer, feats, coors, mask, ref = _case(cid)
    _, dim, k, n, b, _mk = _BY_ID[cid]
    with torch.no_grad(), _algo(0), _ops.phase_timer() as pt:
        new = layer(feats, coors, mask=mask)
        again = layer(feats, coors, mask=mask)
    assert "slot_prep" in pt.summary() and "edge_fused" in pt.summary(), sorted(pt.summary())    # (records built: the wave-per-node path)
    for name, a, a2, r in zip(("feats", "coors"), new, again, ref):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, a2), name
        assert torch.equal(a, r), (name, float((a - r).abs().max()))
    cfg = O.EGNNConfig(dim=dim, num_nearest_neighbors=k)
    params = {k_: v.detach().cpu().numpy().astype(np.float64) for k_, v in layer.state_dict().items()}
    want = O.egnn_forward(cfg, params, feats.cpu().numpy().astype(np.float64), coors.cpu().numpy().astype(np.float64), None,
                          None if mask is None else mask.cpu().numpy(), None)
    for name, a, w in zip(("feats", "coors"), new, want):
        tol = 1e-4 * max(1.0, float(np.abs(w).max()) / 256.0)
        err = float(np.abs(a.cpu().numpy().astype(np.float64) - w).max())
        print(f"{cid} {name}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (cid, name, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["dim8_one_chunk_half_tail", "dim8_ragged_padded_group_and_graph"])
def test_u_of_the_forward_under_autograd(cid):
    """U_out written: no round is skipped, every edge's u equals the general kernel's bit for bit (outputs included)"""
    layer, feats, coors, mask, _ = _case(cid)
    res = {}
    for algo in (1, 0):
        with _algo(algo):
            out = layer._forward_hip_checked(feats, coors, None, mask, None, None, want_u=True)
        res[algo] = (out[0], out[1], out[6])
    k = _BY_ID[cid][2]
    assert res[0][2] is not None and res[0][2].shape == (feats.shape[0] * feats.shape[1] * k, 16)
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_two_launches_on_two_streams():
    """the dim-512 case twice at once, on two streams: each bit-identical to a lone launch"""
    from egnn_pytorch_amd import _ops
    layer, feats, coors, mask, _ = _case("dim512_ring_wraps")
    old = _ops.RANGE_CHECK
    _ops.RANGE_CHECK = "off"                                      # (no host read at the end of a forward: the two calls overlap)
    try:
        with torch.no_grad(), _algo(0):
            lone = layer(feats, coors, mask=mask)
            torch.cuda.synchronize()
            main = torch.cuda.current_stream()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = []
            for s in streams:
                s.wait_stream(main)
            for s in streams:
                with torch.cuda.stream(s):
                    outs.append(layer(feats, coors, mask=mask))
            for s in streams:
                main.wait_stream(s)
            torch.cuda.synchronize()
    finally:
        _ops.RANGE_CHECK = old
    for o in outs:
        assert torch.equal(o[0], lone[0]) and torch.equal(o[1], lone[1])
