"""The kernels between the pinned families, cell by cell: the tail backward (csrc/edge_tail.hip: per-lane plain, matrix-core REDUCE,
matrix-core REDUCE with dropout, per-lane REDUCE behind EGNN_TAIL_SCALAR=1), the message pool, and the node-level glue of
csrc/node_ops.hip / csrc/node_mlp_fused.hip (packed images, split_scaled and its column sums, silu_bwd_, unsplit_words_, sum_rows,
node_mlp_fused).  Importable without a GPU: the float64 specifications, the numpy restatements of the bit-exact parts, the cell
tables and `prepare(cell id)`; the host table test (tests/test_glue_variants_table.py) runs every `prepare`, the device test
(tests/test_gpu_glue_variants.py) runs the kernels against it.  `python -m tests._glue_variants --scalar-child` is the one child
process of the per-lane REDUCE kernel (its switch is read once per process).

Bars (`tail_bars`, `bar_f32`): 8 x the error torch fp32 makes on the same specification and inputs + 16 x 2^-24 of the output's scale
(tests/_plain_variants.py), behind split-f16 MFMAs + 2^-20 sum |a| |b| of the products on the path, and never above what the older
test of the same output allows (2e-6 per edge, 2e-5 sums, 3e-5 node_mlp_fused): min(derived, older).  Nothing here looks at a
kernel's output.  The tail cells named `init_*` take coors_mlp, the gate and CoorsNorm.scale as EGNN.__init__ draws them (weights
N(0, 1e-3)) and are held to the same bars on the same four kernels."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

E_NULLPTR, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -4
ATEN_FACTOR, FLOOR = 8.0, 16.0 * 2.0 ** -24
SPLIT = 2.0 ** -20                               # three-term split product: 3 x 2^-22 sum |a| |b|, with a 4/3 margin
EDGE_CAP, SUM_CAP, NMF_CAP = 2e-6, 2e-5, 3e-5    # tests/test_autograd.py, tests/test_gpu_kernels.py
SENTINEL = 12345.0
GUARD = 64
PART = 1192
EPS = 1e-8                                       # CoorsNorm.eps


# ================================================================================================ the tail: cells
_TAIL = dict(b=2, n=8, k=5, dense=False, m=16, mask="none", clamp="mid", norm=True, scale=1.7, dup=True, gate="span", w3=1.5, u="n1",
             drop=None, eid0=0, seed=0, init=False, gm=1.0, gco="randn")
TAIL_MODES = ("plain", "mfma", "scalar")         # kernels a cell without dropout runs on; with dropout: "mfma_drop" only


def _tc(cid, **kw):
    p = dict(_TAIL, **kw)
    return SimpleNamespace(id=cid, p=p, group=cid.split("_")[0])


_ESHAPES = {1: (1, 1, 1, True), 15: (1, 3, 5, False), 16: (1, 4, 4, True), 17: (1, 17, 1, False), 63: (1, 9, 7, False),
            65: (1, 13, 5, False), 255: (3, 17, 5, False), 256: (1, 16, 16, True), 257: (1, 257, 1, False), 769: (1, 769, 1, False)}
TAIL_CELLS = [_tc("base_e80")]
TAIL_CELLS += [_tc(f"eshape_e{e}", b=s[0], n=s[1], k=s[2], dense=s[3], seed=e) for e, s in _ESHAPES.items()]
TAIL_CELLS += [_tc("eshape_e300_dense", b=3, n=10, k=10, dense=True, seed=3), _tc("eshape_e81_dense", b=1, n=9, k=9, dense=True, seed=4)]
TAIL_CELLS += [_tc(f"mdim_m{m}", m=m, seed=10 + m) for m in (1, 7, 13, 16)]
TAIL_CELLS += [_tc(f"mask_{name}", mask=name, seed=20 + i) for i, name in enumerate(("ragged", "scattered", "node", "all"))]
TAIL_CELLS += [_tc("clamp_zero", clamp=0.0, seed=30), _tc("clamp_none", clamp=None, seed=31), _tc("clamp_mid_masked", mask="scattered", b=3, seed=32)]
TAIL_CELLS += [_tc("norm_off", norm=False, seed=40), _tc("norm_scale_small", scale=0.3, seed=41), _tc("norm_nodup", dup=False, scale=-2.5, seed=42)]
TAIL_CELLS += [_tc("gate_none", gate=None, seed=50), _tc("gate_saturated", gate="sat", seed=51)]
TAIL_CELLS += [_tc("w3_zero", w3=0.0, clamp=None, seed=60), _tc("w3_2m8", w3=2.0 ** -8, seed=61), _tc("w3_one", w3=1.0, seed=62),
               _tc("w3_3072", w3=3072.0, seed=63), _tc("w3_1em30", w3=1e-30, clamp=None, seed=64)]
TAIL_CELLS += [_tc("u_n4", u="n4", seed=70), _tc("u_big", u="big", seed=72)]
TAIL_CELLS += [_tc(f"drop_p{int(10 * p)}_eid{eid0}", drop=(p, 12345 + eid0), eid0=eid0, b=4, seed=80 + i)
               for i, (p, eid0) in enumerate(((0.1, 0), (0.5, 0), (0.1, 4096), (0.5, 2 ** 31 + 7)), start=1)]
# the dropout instantiation across the E shapes (dead waves, a ragged last wave, more than one block), a dense list, no CoorsNorm, no gate
TAIL_CELLS += [_tc(f"drop_e{e}", drop=(0.5 if i % 2 else 0.1, 500 + e), eid0=(0, 3 * e, 2 ** 20)[i % 3], b=s[0], n=s[1], k=s[2], dense=s[3], seed=100 + i)
               for i, (e, s) in enumerate(_ESHAPES.items())]
TAIL_CELLS += [_tc("drop_dense_e200", drop=(0.5, 31), eid0=200, b=2, n=10, k=10, dense=True, seed=124),
               _tc("drop_norm_off", drop=(0.1, 32), eid0=80, norm=False, seed=121), _tc("drop_gate_none", drop=(0.5, 33), gate=None, seed=122),
               _tc("drop_mask_ragged_m7", drop=(0.5, 34), eid0=7, m=7, mask="ragged", seed=123)]
TAIL_CELLS += [_tc("combo_dense_mask_m7", b=2, n=9, k=9, dense=True, m=7, mask="ragged", seed=90),
               _tc("combo_drop_mask_sat_m13", drop=(0.5, 77), eid0=160, b=4, m=13, mask="node", gate="sat", u="n4", seed=91),
               _tc("combo_e257_mask_nogate", b=1, n=257, k=1, mask="scattered", gate=None, norm=False, seed=92)]
# the module's own initialisation (`init`): coors_mlp, the gate and CoorsNorm.scale as EGNN.__init__ draws them -- every Linear weight
# N(0, 1e-3), biases U(+-1 / sqrt(fan_in)), scale 1e-2 -- instead of `_tail_params`' scaling.  q = W4 SiLU'(hid) is then ~5e-4 and W3 m
# ~1e-3 against b3 ~0.25: the operands of a training run's first steps.  No clamp (every edge's weight is b4 to seven digits: no value
# separates them), no planted duplicates; gm = 0: g_msum = 0, so that gU is the coordinate branch alone and does not hide behind the
# pooled messages' pass-through, which is six orders above it (one cell keeps g_msum); gco = "coors": g_coors_out = x + randn / 2, the
# cotangent of a quadratic loss.  With a3 the same on every edge to three digits, d/d W4 = a3 sum g_w, and under a zero-mean cotangent
# sum g_w cancels to 1e-3 ... 0.1 of sum |g_w|, draw by draw: below the rounding of ANY fp32 sum of 257 such terms relative to the
# older test's cap (2e-5 of the group's largest |sum|), which `tail_bars` never exceeds.  The cells keep that cap and get a cotangent
# under which the sum is a sum (`_init_conditions`)
_INIT = dict(init=True, clamp=None, dup=False, gate="init", gm=0.0, gco="coors")
TAIL_CELLS += [_tc("init_e80", seed=130, **_INIT), _tc("init_e80_nogate_nonorm", seed=131, **dict(_INIT, gate=None, norm=False)),
               _tc("init_e257_nonorm", b=1, n=257, k=1, seed=132, **dict(_INIT, norm=False)),
               _tc("init_e257_nogate", b=1, n=257, k=1, seed=133, **dict(_INIT, gate=None)),
               _tc("init_e80_pooled", seed=134, **dict(_INIT, gm=1.0)),
               _tc("init_drop_e80", drop=(0.1, 41), eid0=80, seed=135, **_INIT)]
TAIL_BY_ID = {c.id: c for c in TAIL_CELLS}
assert len(TAIL_BY_ID) == len(TAIL_CELLS)


def tail_modes(c):
    return ("mfma_drop",) if c.p["drop"] is not None else TAIL_MODES


def tail_kernel(part, drop_thr, scalar_env):
    """csrc/edge_tail.hip's choice of kernel, restated: the name it launches or the code it refuses with."""
    if drop_thr and (not part or scalar_env):
        return E_UNSUPPORTED
    if part and not scalar_env:
        return "edge_tail_mfma_kernel<true>" if drop_thr else "edge_tail_mfma_kernel<false>"
    return "edge_tail_bwd_kernel<true>" if part else "edge_tail_bwd_kernel<false>"


MODE_KERNEL = {"plain": tail_kernel(False, 0, False), "mfma": tail_kernel(True, 0, False), "mfma_drop": tail_kernel(True, 1, False),
               "scalar": tail_kernel(True, 0, True)}
# every __global__ kernel of csrc/edge_tail.hip, csrc/node_ops.hip and csrc/node_mlp_fused.hip -> the cells that run it (test functions of
# tests/test_gpu_glue_variants.py; absmax_kernel and status_publish_kernel are held by tests/test_gpu_kernels.py / test_status_publish_*.py)
GLUE_KERNELS = {
    "edge_tail_bwd_kernel<false>": "test_tail_cell[*-plain]", "edge_tail_bwd_kernel<true>": "test_tail_per_lane_reduce_kernel_in_a_child_process",
    "edge_tail_mfma_kernel<false>": "test_tail_cell[*-mfma]", "edge_tail_mfma_kernel<true>": "test_tail_cell[*-mfma_drop]",
    "edge_pool_kernel": "test_pool_cell", "node_prep_hl_kernel": "test_node_prep_cell", "split_scaled_kernel": "test_split_scaled_cell",
    "silu_bwd_kernel": "test_silu_bwd_cell", "unsplit_words_kernel": "test_unsplit_words_narrow_and_strided",
    "node_mlp_fused_kernel<2>": "test_node_mlp_fused_cell[32-*]", "node_mlp_fused_kernel<4>": "test_node_mlp_fused_cell[64-*]",
    "node_mlp_fused_kernel<8>": "test_node_mlp_fused_cell[128-*]", "node_mlp_fused_kernel<16>": "test_node_mlp_fused_cell[256-*]",
    "node_mlp_pack_kernel": "test_node_mlp_fused_cell", "absmax_kernel": None, "status_publish_kernel": None}


def nmf_supported(dim, m_dim):
    """egnn_node_mlp_fused_halves > 0, restated"""
    return m_dim == 16 and dim in (32, 64, 128, 256)


def _f32(t):
    return t.to(torch.float32)


def _make_layer(p, m, c, w, dtype):
    from egnn_pytorch_amd import EGNN
    layer = EGNN(dim=4, m_dim=m, norm_coors=p["norm"], soft_edges=p["gate"] is not None, coor_weights_clamp_value=c).to(dtype)
    with torch.no_grad():
        layer.coors_mlp[0].weight.copy_(w["W3"]); layer.coors_mlp[0].bias.copy_(w["b3"])
        layer.coors_mlp[3].weight.copy_(w["W4"][None]); layer.coors_mlp[3].bias.copy_(w["b4"])
        if p["norm"]:
            layer.coors_norm.scale.copy_(w["scale"])
        if p["gate"] is not None:
            layer.edge_gate[0].weight.copy_(w["gate_w"][None]); layer.edge_gate[0].bias.copy_(w["gate_b"])
    return layer


def _init_params(p, m):
    """coors_mlp, the gate and CoorsNorm.scale as the module draws them under the cell's seed (fp32 values)"""
    from egnn_pytorch_amd import EGNN
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7000 + p["seed"])
        layer = EGNN(dim=4, m_dim=m, norm_coors=p["norm"], soft_edges=p["gate"] is not None)
    t = lambda v: v.detach().double()                                             # noqa: E731
    w = dict(W3=t(layer.coors_mlp[0].weight), b3=t(layer.coors_mlp[0].bias), W4=t(layer.coors_mlp[3].weight[0]), b4=t(layer.coors_mlp[3].bias))
    if p["norm"]:
        w["scale"] = t(layer.coors_norm.scale).reshape(1)
    if p["gate"] is not None:
        w["gate_w"], w["gate_b"] = t(layer.edge_gate[0].weight[0]), t(layer.edge_gate[0].bias)
    return w


def _tail_params(p, u, raw):
    """coors_mlp, the gate and CoorsNorm.scale for a cell, every tensor scaled from the float64 forward of the tensors before it"""
    m, e = u.shape[-1], u[..., 0].numel()
    if p["init"]:
        return _init_params(p, m)
    w = {}
    m0 = torch.nn.functional.silu(u)
    mm = m0
    if p["gate"] is not None:
        s = m0 @ raw["gw"]
        span = max(float(s.max() - s.min()), 1e-6) if e > 1 else float(s.abs().max())
        w["gate_w"] = _f32(raw["gw"] * ((80.0 if p["gate"] == "sat" else 10.0) / span)).double()  # pre-activations over [-5, 5] (saturated: [-40, 40])
        s = m0 @ w["gate_w"]
        w["gate_b"] = _f32(-(s.max() + s.min()).reshape(1) / 2).double()          # centred: the gate takes both sides
        mm = m0 * torch.sigmoid(m0 @ w["gate_w"] + w["gate_b"])[..., None]
    w3 = _f32(raw["w3"] * (p["w3"] / float(raw["w3"].abs().max())))
    if p["w3"] > 0:
        w3.view(-1)[int(w3.abs().argmax())] = p["w3"]                            # max |W3| is exactly the cell's value
    w["W3"] = w3.double()
    prod = mm @ w["W3"].t()
    # max |b3| = twice the median |W3 m| (never above max |W3 m|: the product is not bias-dominated).  Scales come from medians and
    # quartiles, not from maxima or moments: a few planted +-90 messages must not set the scale of every other edge -- with b3 and W4 sized
    # by them, the other edges' hidden layer is a constant and their coordinate weight a small difference of large terms, which no fp32
    # evaluation holds to 2e-6 of its scale
    w["b3"] = _f32(raw["b3"] * ((min(2.0 * float(prod.abs().median()), float(prod.abs().max())) if p["w3"] > 1e-20 else 1.0) / float(raw["b3"].abs().max()))).double()
    a3 = torch.nn.functional.silu(prod + w["b3"])
    pre_w = a3 @ raw["w4"]
    flat_w = p["w3"] <= 1e-20 or e == 1                                          # W3 = 0: every edge has the same coordinate weight
    qs = pre_w.reshape(-1).sort().values
    sd = float(pre_w.abs().max()) if flat_w else float(qs[(3 * e) // 4] - qs[e // 4]) / 1.349          # (the quartiles' estimate of the deviation)
    # deviation of w = 1, but max |W4| never below 2^-3 (at max |W3| = 3 * 2^10 the activations are ~1e3 and w ~ 1e2): these cells keep
    # q = W4 SiLU'(hid), an fp16 (hi, lo) operand of the matrix-core kernel, at O(1).  The small end -- W4 ~ 1e-3, q's lo half in fp16's
    # subnormal range unless the kernel scales it -- is the `init` cells'
    w["W4"] = _f32(raw["w4"] * max(1.0 / max(sd, 1e-30), 0.125 / float(raw["w4"].abs().max()))).double()
    srt = (a3 @ w["W4"]).reshape(-1).sort().values
    w["b4"] = torch.tensor([0.3], dtype=torch.float32).double() if flat_w else _f32(-(srt[e // 2 - 1] + srt[e // 2]).reshape(1) / 2).double()
    if p["norm"]:
        w["scale"] = torch.tensor([p["scale"]], dtype=torch.float32).double()
    return w


@functools.lru_cache(maxsize=None)
def prepare(cid):
    """Inputs of a tail cell (fp32 values; every parameter scaled per tensor from the float64 forward of the tensors before it), its
    float64 reference, the torch-fp32 evaluation of the same specification, and the cell conditions asserted on the reference alone."""
    c = TAIL_BY_ID[cid]
    p = c.p
    b, n, k, m, dense = p["b"], p["n"], p["k"], p["m"], p["dense"]
    assert not dense or k == n
    e = b * n * k
    g = torch.Generator().manual_seed(1000 + p["seed"])
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)            # noqa: E731
    coors = rnd(b, n, 3)
    if p["dup"] and n >= 2:
        coors[:, 1] = coors[:, 0]                                                 # coincident points: rn == 0 on a non-self edge
    idx = None
    if not dense:
        idx = torch.randint(0, n, (b, n, k), generator=g)
        if n >= 2:
            idx[:, 0, 0], idx[:, 1, 0] = 1, 0
        if n >= 3:
            idx[:, 2, 0] = 2                                                      # a self pair
    u = rnd(b, n, k, m) * (4.0 if p["u"] == "n4" else 1.0)
    if p["u"] == "big":
        flat = u.view(-1)
        at = torch.randperm(flat.numel(), generator=g)[:8]
        flat[at] = torch.tensor([30.0, -30.0, 90.0, -90.0, 30.0, -30.0, 90.0, -90.0], dtype=torch.float64)
    pm = None
    if p["mask"] != "none":
        if p["mask"] == "ragged":
            node = torch.arange(n)[None] < torch.tensor([n, max(1, n - 3), n // 2 + 1, 2][:b])[:, None]
            j = torch.arange(n)[None, None, :].expand(b, n, n) if dense else idx
            pm = node[:, :, None] & node[torch.arange(b)[:, None, None], j]
        elif p["mask"] == "all":
            pm = torch.zeros(b, n, k, dtype=torch.bool)
        else:
            pm = torch.rand(b, n, k, generator=g) > 0.3
            if p["mask"] == "node":
                pm[:, min(3, n - 1)] = False
    u, coors = _f32(u).double(), _f32(coors).double()
    g_co, g_msum = _f32(rnd(b, n, 3)).double(), _f32(rnd(b, n, m)).double() * p["gm"]
    if p["gco"] == "coors":
        g_co = _f32(coors + 0.5 * g_co).double()
    raw = dict(gw=rnd(m), w3=rnd(4 * m, m), b3=rnd(4 * m), w4=rnd(4 * m))
    w = _tail_params(p, u, raw)
    # ---- coincident non-self edges carry d/d rel = w_c g scale / eps: 1e8 times the rounding error of their coordinate weight.  They get
    # the message of the edge with the largest |w| -- clamped exactly where the cell clamps, least cancellation where it does not -- so
    # that the output's scale is not set by edges whose weight is a difference of large terms; the parameters are scaled again from the result
    j = torch.arange(n)[None, None, :].expand(b, n, n) if dense else idx
    src, dst = torch.arange(e) // k, ((torch.arange(e) // (n * k)) * n + j.reshape(-1))
    flat_co = coors.reshape(-1, 3)
    coinc = ((flat_co[src] - flat_co[dst]).norm(dim=-1) == 0) & (src != dst)
    if bool(coinc.any()) and p["norm"]:
        probe = tail_spec(_make_layer(p, m, None, w, torch.float64), u, coors, idx, pm, g_co, g_msum, p["drop"], p["eid0"])
        cand = probe["w"].reshape(-1).abs().masked_fill(coinc | (src == dst) | (~pm.reshape(-1) if pm is not None else torch.zeros(e, dtype=torch.bool)), -1.0)
        u = u.clone()
        u.view(e, m)[coinc] = u.view(e, m)[int(cand.argmax())].clone()
        w = _tail_params(p, u, raw)
    # ---- the clamp value: from the float64 forward, the midpoint of the two |w| that straddle the median of the unmasked edges
    clamp = p["clamp"]
    drop = p["drop"]
    if clamp == "mid":
        probe = tail_spec(_make_layer(p, m, None, w, torch.float64), u, coors, idx, pm, g_co, g_msum, drop, p["eid0"])
        wl = probe["w"].reshape(-1)[(pm.reshape(-1) if pm is not None else torch.ones(e, dtype=torch.bool))].sort().values
        if wl.numel() >= 8 and float(wl[0]) < 0 < float(wl[-1]):
            # the smaller of the 15 % / 85 % quantiles' magnitudes: at least 15 % of the edges beyond it on either side, then the midpoint
            # between that |w| and the next smaller one (the widest margin there is at that place)
            target = min(abs(float(wl[int(0.15 * wl.numel())])), abs(float(wl[int(0.85 * wl.numel())])))
            aw = wl.abs().sort().values
            at = int((aw < target).sum())
            clamp = float(_f32((aw[max(at - 1, 0)] + aw[at]) / 2))
        elif wl.numel() >= 2:
            aw = wl.abs().sort().values
            clamp = float(_f32((aw[aw.numel() // 2 - 1] + aw[aw.numel() // 2]) / 2))
        else:
            clamp = float(_f32(wl[0].abs() * 2)) if wl.numel() else 0.5
    layer = _make_layer(p, m, clamp, w, torch.float64)
    ref = tail_spec(layer, u, coors, idx, pm, g_co, g_msum, drop, p["eid0"])
    f32 = tail_spec(_make_layer(p, m, clamp, w, torch.float64).float(), u.float(), coors.float(), idx, pm, g_co.float(), g_msum.float(), drop, p["eid0"])
    self_pair = src == dst
    for r in (ref, f32):                                                         # self pairs carry g_rel = 0, as the kernel documents
        r["g_rel"] = r["g_rel"].reshape(e, 3).masked_fill(self_pair[:, None], 0.0)
        r["g_u"] = r["g_u"].reshape(e, m)
    d = SimpleNamespace(cell=c, p=p, b=b, n=n, k=k, m=m, e=e, hid3=4 * m, u=u, coors=coors, idx=idx, pm=pm, g_co=g_co, g_msum=g_msum, w=w,
                        clamp=clamp, drop=drop, eid0=p["eid0"], layer=layer, ref=ref, f32=f32, self_pair=self_pair,
                        coinc=coinc & bool(p["norm"]))
    _tail_conditions(d)
    return d


def tail_spec(layer, u, coors, idx, pm, g_co, g_msum, drop=None, eid0=0):
    """autograd.tail_edge_backward, plus w (the unclamped coordinate weight) and rn; with drop = (p, seed): the test-local extension
    with dropout in coors_mlp (`tail_spec_drop`)."""
    from egnn_pytorch_amd import autograd as A, _dropout
    b, n, k, m = u.shape
    if drop is None:
        r = A.tail_edge_backward(layer, u, coors, idx, pm, g_co, g_msum)
    else:
        rows = torch.arange(b * n * k) + eid0
        keep = _dropout.keep_mask(drop[1], _dropout.SITE_COORS, rows, torch.arange(4 * m), drop[0])
        r = tail_spec_drop(layer, u, coors, idx, pm, g_co, g_msum, keep, _dropout.inv_keep(drop[0]))
        r["keep"] = keep
    lin4 = layer.coors_mlp[3]
    r["w"] = (r["a3"] @ lin4.weight[0] + lin4.bias[0]).detach()
    j = torch.arange(n)[None, None, :].expand(b, n, n) if idx is None else idx
    rel = coors[:, :, None, :] - coors[torch.arange(b)[:, None, None], j]
    r["rel"], r["rn"] = rel.reshape(-1, 3), rel.norm(dim=-1).reshape(-1)
    return {key: (v.detach() if torch.is_tensor(v) else v) for key, v in r.items()}


def tail_spec_drop(layer, u, coors, idx, pair_mask, g_coors_out, g_msum, keep, inv_keep):
    """`autograd.tail_edge_backward` with training-mode dropout behind coors_mlp's first Linear: hid_d = keep ? hid / (1 - p) : 0, the
    SiLU and everything behind it on hid_d, d hid_d / d hid = keep / (1 - p).  keep (E, 4m) bool.  With keep all true and inv_keep 1 it is
    tail_edge_backward term by term; with the hash mask it equals autograd of layer_tail(..., drop=...) (the table test ties both)."""
    b, n, k, m = u.shape
    lin3, lin4 = layer.coors_mlp[0], layer.coors_mlp[3]
    w3, b3, w4, b4 = lin3.weight, lin3.bias, lin4.weight[0], lin4.bias[0]
    sg_u = torch.sigmoid(u)
    m0 = u * sg_u
    gate = layer.edge_gate is not None
    if gate:
        gw, gb = layer.edge_gate[0].weight[0], layer.edge_gate[0].bias[0]
        gt = torch.sigmoid(m0 @ gw + gb)[..., None]
        mm = m0 * gt
    else:
        mm = m0
    keep = keep.view(b, n, k, -1)
    dk = torch.where(keep, torch.full_like(mm[..., :1], inv_keep), torch.zeros_like(mm[..., :1])).expand(keep.shape)
    hid = (mm @ w3.t() + b3) * dk
    sg_h = torch.sigmoid(hid)
    a3 = hid * sg_h
    w = a3 @ w4 + b4
    j = torch.arange(n)[None, None, :].expand(b, n, n) if idx is None else idx
    rel = coors[:, :, None, :] - coors[torch.arange(b)[:, None, None], j]
    g_scale = None
    if layer.norm_coors:
        eps, scale = layer.coors_norm.eps, layer.coors_norm.scale
        rn = rel.norm(dim=-1, keepdim=True)
        den = rn.clamp(min=eps)
        relp = rel / den * scale
    else:
        relp = rel
    wm = w if pair_mask is None else w.masked_fill(~pair_mask, 0.0)
    c = layer.coor_weights_clamp_value
    wc = wm if c is None else wm.clamp(min=-c, max=c)
    g = g_coors_out[:, :, None, :]
    g_wc = (g * relp).sum(dim=-1)
    g_relp = wc[..., None] * g
    g_wm = g_wc if c is None else torch.where((wm >= -c) & (wm <= c), g_wc, torch.zeros_like(g_wc))
    g_w = g_wm if pair_mask is None else g_wm.masked_fill(~pair_mask, 0.0)
    g_hid = g_w[..., None] * w4 * (sg_h * (1 + hid * (1 - sg_h))) * dk
    g_m = g_hid @ w3
    gm_pool = g_msum[:, :, None, :].expand(b, n, k, m)
    g_m = g_m + (gm_pool if pair_mask is None else gm_pool.masked_fill(~pair_mask[..., None], 0.0))
    g_gate = None
    if gate:
        g_s = (g_m * m0).sum(dim=-1, keepdim=True) * gt * (1 - gt)
        g_m = g_m * gt + g_s * gw
        g_gate = g_s.reshape(-1)
    g_u = g_m * (sg_u * (1 + u * (1 - sg_u)))
    if layer.norm_coors:
        dot = (g_relp * rel).sum(dim=-1, keepdim=True)
        g_scale = (dot / den).reshape(-1)
        g_rel = g_relp * (scale / den) - torch.where(rn >= eps, dot * scale / (den * den) * (rel / rn.clamp(min=1e-30)), torch.zeros_like(rel))
    else:
        g_rel = g_relp
    e = b * n * k
    return dict(g_u=g_u, g_rel=g_rel, g_hid=g_hid.reshape(e, -1), a3=a3.reshape(e, -1), g_w=g_w.reshape(e), g_scale=g_scale,
                m=mm.reshape(e, m), m0=m0.reshape(e, m), g_gate=g_gate)


def _tail_conditions(d):
    """The cell conditions, on the float64 reference alone (and the torch-fp32 evaluation for the decision margin)."""
    p, ref, e = d.p, d.ref, d.e
    if p["init"]:
        return _init_conditions(d)
    live = d.pm.reshape(-1) if d.pm is not None else torch.ones(e, dtype=torch.bool)
    wide = int(live.sum()) >= 40                                                 # fractions are asserted where there are edges to count
    w, rn = ref["w"].reshape(-1), ref["rn"]
    # rn in {0} + [1e-3, inf); coincident non-self edges where the cell has duplicated coordinates
    assert bool(((rn == 0) | (rn >= 1e-3)).all()), d.cell.id
    assert bool((rn[d.self_pair] == 0).all())
    if p["dup"] and d.n >= 2:
        assert bool(((rn == 0) & ~d.self_pair).any()), d.cell.id
    else:
        assert bool(((rn == 0) == d.self_pair).all()), d.cell.id
    # the clamp: both signs, unclamped, and the decision margin
    c = d.clamp
    d.margin = None
    if c is not None and bool(live.any()):
        wl = w[live]
        err = float((d.f32["w"].reshape(-1).double() - w).abs().max())
        d.margin = float((wl.abs() - c).abs().min()) / max(err, 1e-300)
        assert d.margin >= 64, (d.cell.id, d.margin)
        if p["clamp"] == "mid" and wide:
            fr = (float((wl > c).float().mean()), float((wl < -c).float().mean()), float((wl.abs() <= c).float().mean()))
            assert fr[0] >= 0.10 and fr[1] >= 0.10 and fr[2] >= 0.30, (d.cell.id, fr)
        if p["clamp"] == 0.0:
            assert bool((wl.abs() > 0).all()) and not bool(ref["g_w"].any()), d.cell.id
    # the gate
    if p["gate"] is not None:
        pre = ref["m0"] @ d.w["gate_w"] + d.w["gate_b"]
        gt = torch.sigmoid(pre)
        if p["gate"] == "sat":
            assert float(pre.abs().max()) > 30, d.cell.id
            if wide:
                assert float(pre.max()) > 30 or float(pre.min()) < -30
        elif wide:
            assert float(gt.min()) <= 0.1 and float(gt.max()) >= 0.9, (d.cell.id, float(gt.min()), float(gt.max()))
    # W3: max |W3| exactly the cell's value; the product is not bias-dominated
    assert float(d.w["W3"].abs().max()) == float(torch.tensor(p["w3"], dtype=torch.float32)), d.cell.id
    if p["w3"] > 1e-20:
        assert float((ref["m"] @ d.w["W3"].t()).abs().max()) >= float(d.w["b3"].abs().max()), d.cell.id
    if p["u"] == "big":
        assert {30.0, -30.0, 90.0, -90.0} <= set(d.u.reshape(-1).tolist())
    if p["mask"] == "all":
        for name in ("g_u", "g_rel", "g_hid", "g_w"):
            assert not bool(ref[name].any()), (d.cell.id, name)
        assert ref["g_scale"] is None or not bool(ref["g_scale"].any())
    elif d.pm is not None:
        assert bool(d.pm.any()) and not bool(d.pm.all())
        assert not bool(ref["g_w"][~live].any()) and not bool(ref["g_u"][~live].any())
        if p["mask"] == "node":
            assert not bool(d.pm[:, min(3, d.n - 1)].any())
    if p["mask"] != "all" and p["clamp"] != 0.0 and p["w3"] != 0.0 and int(live.sum()) >= 4:
        assert float(ref["g_hid"].abs().max()) > 0 and float(ref["g_w"].abs().max()) > 0, d.cell.id      # never 0 == 0
    if d.drop is not None:
        frac = float(ref["keep"].float().mean())
        assert abs(frac - (1 - d.drop[0])) < 0.08, (d.cell.id, frac)
        assert d.eid0 + e <= 2 ** 32 - 1


def _init_conditions(d):
    """The cells at the module's own initialisation, on the reference alone: the weights are the module's draw (std within 30 % of 1e-3;
    the gate's sixteen within 50 %), q = W4 SiLU'(hid) lies where an unscaled fp16 (hi, lo) pair loses its lo half to the subnormals
    (|q| <= 2^-8: lo <= 2^-19, resolved to 2^-24), W3 m is bias-dominated, and nothing compared is 0 == 0."""
    p, ref, w = d.p, d.ref, d.w
    d.margin = None
    assert d.clamp is None and d.pm is None and not bool(d.coinc.any()), d.cell.id
    for name in ("W3", "W4"):
        assert 0.7e-3 <= float(w[name].std()) <= 1.3e-3, (d.cell.id, name, float(w[name].std()))
    if p["gate"] is not None:
        assert 0.5e-3 <= float(w["gate_w"].std()) <= 1.5e-3, (d.cell.id, float(w["gate_w"].std()))
    if p["norm"]:
        assert float(w["scale"]) == float(torch.tensor(1e-2, dtype=torch.float32)), d.cell.id
    ik = 1.0 if d.drop is None else 1.0 / (1.0 - d.drop[0])
    hid = (ref["m"] @ w["W3"].t() + w["b3"]) * ik
    sg = torch.sigmoid(hid)
    q = w["W4"] * (sg * (1 + hid * (1 - sg))) * ik
    assert 0 < float(q.abs().max()) <= 2.0 ** -8, (d.cell.id, float(q.abs().max()))
    assert float((ref["m"] @ w["W3"].t()).abs().max()) < 0.1 * float(w["b3"].abs().max()), d.cell.id
    assert bool(((ref["rn"] == 0) == d.self_pair).all()), d.cell.id
    for name in ("g_u", "g_rel", "g_hid", "g_w"):
        assert float(ref[name].abs().max()) > 0, (d.cell.id, name)
    # d/d W4 and d/d b4 are sums, not cancellations: an fp32 sum of E terms is good to a few 2^-24 sum |g_w| (3e-7 of it over 257 terms
    # taken one after the other), the cap allows 2e-5 |sum g_w|, and 8 x the former has to fit under the latter
    assert float(ref["g_w"].sum().abs()) >= 0.12 * float(ref["g_w"].abs().sum()), (d.cell.id, float(ref["g_w"].sum()), float(ref["g_w"].abs().sum()))
    if p["gm"] == 0.0:
        assert not bool(d.g_msum.any())
        # gU is the coordinate branch alone: g_w W3^T q through the gate and SiLU'(u)
        assert float(ref["g_u"].abs().max()) < 1e-4 * float(ref["g_w"].abs().max()), d.cell.id
    if d.drop is not None:
        frac = float(ref["keep"].float().mean())
        assert abs(frac - (1 - d.drop[0])) < 0.08, (d.cell.id, frac)


def tail_sums(r, m, hid3):
    """the 1192 sums of `part` from a per-edge result (the layout of csrc/edge_tail.hip), and the L1 norms of their terms"""
    out, l1 = torch.zeros(PART, dtype=r["g_u"].dtype), torch.zeros(PART, dtype=torch.float64)
    w3g, w3l = torch.zeros(64, 16, dtype=out.dtype), torch.zeros(64, 16, dtype=torch.float64)
    w3g[:hid3, :m] = r["g_hid"].t() @ r["m"]
    w3l[:hid3, :m] = r["g_hid"].double().abs().t() @ r["m"].double().abs()
    out[:1024], l1[:1024] = w3g.reshape(-1), w3l.reshape(-1)
    out[1024:1024 + hid3], l1[1024:1024 + hid3] = r["g_hid"].sum(0), r["g_hid"].double().abs().sum(0)
    out[1088:1088 + hid3], l1[1088:1088 + hid3] = r["g_w"] @ r["a3"], r["g_w"].double().abs() @ r["a3"].double().abs()
    out[1152:1152 + m], l1[1152:1152 + m] = r["g_u"].sum(0), r["g_u"].double().abs().sum(0)
    if r["g_gate"] is not None:
        out[1168:1168 + m], l1[1168:1168 + m] = r["g_gate"] @ r["m0"], r["g_gate"].double().abs() @ r["m0"].double().abs()
        out[1186], l1[1186] = r["g_gate"].sum(), r["g_gate"].double().abs().sum()
    out[1184], l1[1184] = r["g_w"].sum(), r["g_w"].double().abs().sum()
    if r["g_scale"] is not None:
        out[1185], l1[1185] = r["g_scale"].sum(), r["g_scale"].double().abs().sum()
    return out, l1


def _split_terms(d):
    """What the three-term split-f16 products of the matrix-core tail may add, per output, in float64: hid = W3 m and gm = W3^T q
    (q = W4 SiLU'(hid)) each within 2^-20 sum |a| |b|, carried to g_u through |g_w| |SiLU'| as the specification carries the values."""
    ref, w = d.ref, d.w
    ik = 1.0 if d.drop is None else 1.0 / (1.0 - d.drop[0])
    aw3, aw4 = w["W3"].abs(), w["W4"].abs()
    d_hid = SPLIT * (ref["m"].abs() @ aw3.t()) * ik                               # (E, 4m)
    hid = (ref["m"] @ w["W3"].t() + w["b3"]) * ik
    sg = torch.sigmoid(hid)
    q = w["W4"] * (sg * (1 + hid * (1 - sg))) * ik
    d_q = aw4 * 0.5 * d_hid * ik                                                  # |SiLU''| <= 1/2
    gw_abs = ref["g_w"].abs()[:, None]
    d_ghid = gw_abs * d_q
    d_a3 = 1.1 * d_hid                                                            # |SiLU'| <= 1.1
    d_gm = gw_abs * (d_q @ aw3 + SPLIT * (q.abs() @ aw3))                         # (E, m)
    d_gs = torch.zeros(d.e, dtype=torch.float64)
    if d.p["gate"] is not None:
        d_gs = 0.25 * (d_gm * ref["m0"].abs()).sum(-1)
        d_gm = d_gm + d_gs[:, None] * w["gate_w"].abs()
    d_gu = 1.1 * d_gm
    d_w = (d_a3 * aw4).sum(-1)                                                    # -> g_rel, linear in the unclamped weight
    unit = torch.where(ref["w"].reshape(-1).abs() > 0, ref["g_rel"].abs().amax(-1) / ref["w"].reshape(-1).abs().clamp(min=1e-300), torch.zeros(d.e, dtype=torch.float64))
    d_grel = d_w * unit * (ref["g_w"].abs() > 0)                                  # clamped / masked edges: the weight is a constant
    per_edge = dict(g_u=d_gu, g_rel=d_grel[:, None].expand(d.e, 3), g_hid=d_ghid, a3=d_a3)
    sums = torch.zeros(PART, dtype=torch.float64)
    w3s = torch.zeros(64, 16, dtype=torch.float64)
    w3s[:d.hid3, :d.m] = d_ghid.t() @ ref["m"].abs()
    sums[:1024] = w3s.reshape(-1)
    sums[1024:1024 + d.hid3] = d_ghid.sum(0)
    sums[1088:1088 + d.hid3] = ref["g_w"].abs() @ d_a3
    sums[1152:1152 + d.m] = d_gu.sum(0)
    sums[1168:1168 + d.m] = d_gs @ ref["m0"].abs()
    sums[1186] = d_gs.sum()
    sums[1185] = (d_w * (ref["g_scale"].abs() / ref["w"].reshape(-1).abs().clamp(min=1e-300)) * (ref["g_w"].abs() > 0)).sum() if ref["g_scale"] is not None else 0.0
    return per_edge, sums


def tail_bars(cid, mode):
    """bars of a tail cell: {output name: tensor or float}; 'sums' a (1192,) tensor"""
    d = prepare(cid)
    ref, f32 = d.ref, d.f32
    mfma = mode in ("mfma", "mfma_drop")
    split_e, split_s = _split_terms(d) if mfma else ({}, torch.zeros(PART, dtype=torch.float64))
    bars = {}
    for name in ("g_u", "g_rel", "g_hid", "a3", "g_w", "g_scale", "g_gate"):
        r = ref[name]
        if r is None:
            continue
        if name == "g_rel" and bool(d.coinc.any()):
            # two scales: coincident non-self edges under CoorsNorm carry w_c g scale / eps (1e8 and more), every other edge O(1) -- each
            # group is held to its own largest |reference| and its own torch-fp32 error, so that no edge hides behind another's scale
            bar = torch.zeros(d.e, 1, dtype=torch.float64)
            for grp in (d.coinc, ~d.coinc):
                if not bool(grp.any()):
                    continue
                top = float(r[grp].abs().max())
                aten = float((f32[name][grp].double() - r[grp]).abs().max())
                derived = ATEN_FACTOR * aten + FLOOR * top + (split_e[name][grp][:, :1] if name in split_e else 0.0)
                cap = EDGE_CAP * max(top, 1e-30)
                bar[grp] = torch.clamp(torch.as_tensor(derived, dtype=torch.float64), max=cap).expand(int(grp.sum()), 1)
            bars[name] = bar
            continue
        top = float(r.abs().max()) if r.numel() else 0.0
        aten = float((f32[name].double() - r).abs().max())
        derived = ATEN_FACTOR * aten + FLOOR * top + (split_e[name] if name in split_e else 0.0)
        cap = EDGE_CAP * max(top, 1e-30)
        bars[name] = torch.clamp(derived, max=cap) if torch.is_tensor(derived) else min(derived, cap)
    s64, l1 = tail_sums(ref, d.m, d.hid3)
    s32, _ = tail_sums(f32, d.m, d.hid3)
    derived = ATEN_FACTOR * (s32.double() - s64).abs() + FLOOR * l1 + split_s
    # the older test's scale: max |sum| of the group, for the three scalars also the L1 norm of their terms
    cap = torch.zeros(PART, dtype=torch.float64)
    for lo, hi in ((0, 1024), (1024, 1088), (1088, 1152), (1152, 1168), (1168, 1184)):
        cap[lo:hi] = SUM_CAP * max(float(s64[lo:hi].abs().max()), 1e-30)
    for at in (1184, 1185, 1186):
        cap[at] = SUM_CAP * max(float(s64[at].abs()), float(l1[at]), 1e-30)
    bars["sums"] = torch.minimum(derived, cap)
    bars["sums_ref"] = s64
    return bars


# ================================================================================================ the tail: on the device
def tail_device_inputs(d):
    dev = "cuda"
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()             # noqa: E731
    u16 = torch.zeros(d.e, 16, device=dev); u16[:, :d.m] = f(d.u.reshape(d.e, d.m))
    gm16 = torch.zeros(d.b * d.n, 16, device=dev); gm16[:, :d.m] = f(d.g_msum.reshape(-1, d.m))
    w3p = torch.zeros(64, 16, device=dev); w3p[:d.hid3, :d.m] = f(d.w["W3"])
    b3p = torch.zeros(64, device=dev); b3p[:d.hid3] = f(d.w["b3"])
    w4p = torch.zeros(64, device=dev); w4p[:d.hid3] = f(d.w["W4"])
    t = dict(u=u16, g_msum=gm16, W3=w3p, b3=b3p, W4=w4p, b4=f(d.w["b4"]), coors=f(d.coors.reshape(-1, 3)), g_co=f(d.g_co.reshape(-1, 3)))
    if d.idx is not None:
        t["idx"] = d.idx.reshape(-1).to(device=dev, dtype=torch.int32)
    if d.pm is not None:
        t["pm"] = d.pm.reshape(-1).to(dev).view(torch.uint8)
    if d.p["norm"]:
        t["scale"] = f(d.w["scale"])
    if d.p["gate"] is not None:
        gw16 = torch.zeros(16, device=dev); gw16[:d.m] = f(d.w["gate_w"])
        t["gate_w"], t["gate_b"] = gw16, f(d.w["gate_b"])
    return t


def tail_outputs(e, reduce, want_rel, device="cuda"):
    """every output with GUARD sentinel rows behind row E (`part`: behind its last wave row)"""
    s = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=device)      # noqa: E731
    o = dict(gU=s(e + GUARD, 16), g_rel=s(e + GUARD, 4))
    if reduce:
        o["part"] = s((e + 255) // 256 * 4 + 4, PART)
        o["amax"] = torch.full((1,), 0x7fc00000, dtype=torch.int32, device=device)
    else:
        o.update(g_hid=s(e + GUARD, 64), a3=s(e + GUARD, 64), g_w=s(e + GUARD), g_scale=s(e + GUARD), g_gate=s(e + GUARD))
    if want_rel:
        o.update(rel=s(e + GUARD, 4), dist=s(e + GUARD))
    return o


def tail_args(d, t, o, reduce, drop=None, eid0=0, b=None, edge0=0):
    """the C argument block; b / edge0: a chunk of whole graphs starting at edge `edge0` of the cell's tensors"""
    from egnn_pytorch_amd import _abi, _dropout
    a = _abi.EdgeTailArgs()
    bb = d.b if b is None else b
    a.B, a.N, a.K, a.norm_coors = bb, d.n, d.k, int(d.p["norm"])
    a.clamp = -1.0 if d.clamp is None else float(d.clamp)
    a.eps = EPS if d.p["norm"] else 0.0
    node0 = edge0 // d.k
    ptr = lambda name, off=0: (t[name].data_ptr() + off) if name in t else None   # noqa: E731
    a.u, a.coors = ptr("u", edge0 * 64), ptr("coors", node0 * 12)
    a.idx, a.pair_mask = ptr("idx", edge0 * 4), ptr("pm", edge0)
    a.g_coors_out, a.g_msum = ptr("g_co", node0 * 12), ptr("g_msum", node0 * 64)
    a.W3, a.b3, a.W4, a.b4, a.scale = ptr("W3"), ptr("b3"), ptr("W4"), ptr("b4"), ptr("scale")
    a.gate_w, a.gate_b = ptr("gate_w"), ptr("gate_b")
    a.gU, a.g_rel = o["gU"].data_ptr(), o["g_rel"].data_ptr()
    if reduce:
        a.part, a.amax_gu = o["part"].data_ptr(), o["amax"].data_ptr()
    else:
        a.g_hid, a.a3, a.g_w = o["g_hid"].data_ptr(), o["a3"].data_ptr(), o["g_w"].data_ptr()
        a.g_scale = o["g_scale"].data_ptr() if d.p["norm"] else None
        a.g_gate = o["g_gate"].data_ptr() if d.p["gate"] is not None else None
    if "rel" in o:
        a.rel_out, a.dist_out = o["rel"].data_ptr(), o["dist"].data_ptr()
    if drop is not None:
        a.drop_thr, a.drop_seed, a.drop_inv_keep, a.drop_eid0 = _dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0]), int(eid0)
    return a


def tail_launch(a):
    from ctypes import byref
    from egnn_pytorch_amd import _abi, _ops
    return _abi.load().egnn_edge_tail_bwd_f32(byref(a), _ops._stream())


def tail_run(d, mode, want_rel=True):
    reduce = mode != "plain"
    t = tail_device_inputs(d)
    o = tail_outputs(d.e, reduce, want_rel)
    rc = tail_launch(tail_args(d, t, o, reduce, d.drop, d.eid0))
    assert rc == 0, (d.cell.id, mode, rc)
    torch.cuda.synchronize()
    return t, o


def tail_check(d, mode, o, worst):
    """one run of a cell against the specification and the bars; worst: {kernel: largest error / bar} updated in place"""
    from egnn_pytorch_amd import _ops
    e, m, hid3 = d.e, d.m, d.hid3
    reduce = mode != "plain"
    bars = tail_bars(d.cell.id, mode)
    ref = d.ref
    for name, t in o.items():                                                    # guard rows
        if name == "amax":
            continue
        rows = (e + 255) // 256 * 4 if name == "part" else e
        assert bool((t[rows:] == SENTINEL).all()), (d.cell.id, mode, name, "guard rows written")

    def near(name, got, want, bar):
        err = (got.double().cpu() - want).abs()
        assert bool(torch.isfinite(got).all()), (d.cell.id, mode, name)
        ratio = float((err / torch.as_tensor(bar, dtype=torch.float64).clamp(min=1e-300)).max()) if err.numel() else 0.0
        ok = bool((err <= torch.as_tensor(bar, dtype=torch.float64)).all())
        key = MODE_KERNEL[mode]
        worst[key] = max(worst.get(key, 0.0), ratio if float(err.max() if err.numel() else 0.0) > 0 else 0.0)
        assert ok, (d.cell.id, mode, name, "error / bar", ratio, "error", float(err.max()))

    gu, grel = o["gU"][:e], o["g_rel"][:e]
    near("g_u", gu[:, :m], ref["g_u"], bars["g_u"])
    near("g_rel", grel[:, :3], ref["g_rel"], bars["g_rel"])
    assert not bool(gu[:, m:].any()) and not bool(grel[:, 3].any()), (d.cell.id, mode, "pad channels")
    if "rel" in o:                                                               # the by-products: x_i - x_j exactly, its square within 4 x 2^-24 per edge
        rel32 = (d.coors.float().reshape(-1, 3)[torch.arange(e) // d.k] - d.coors.float().reshape(-1, 3)[_dst(d)])
        assert torch.equal(o["rel"][:e, :3].cpu(), rel32) and not bool(o["rel"][:e, 3].any()), (d.cell.id, mode, "rel")
        dist64 = (rel32.double() ** 2).sum(-1)
        assert bool(((o["dist"][:e].double().cpu() - dist64).abs() <= 4 * 2.0 ** -24 * dist64).all()), (d.cell.id, mode, "dist")
    if not reduce:
        near("g_hid", o["g_hid"][:e, :hid3], ref["g_hid"], bars["g_hid"])
        near("a3", o["a3"][:e, :hid3], ref["a3"], bars["a3"])
        near("g_w", o["g_w"][:e], ref["g_w"], bars["g_w"])
        assert not bool(o["g_hid"][:e, hid3:].any()), (d.cell.id, "pad hidden columns of g_hid")
        if hid3 < 64:                                                            # pad units: W3 row, b3, W4 all zero: a3 = SiLU(0) = 0
            assert not bool(o["a3"][:e, hid3:].any()), (d.cell.id, "pad hidden columns of a3")
        if ref["g_scale"] is not None:
            near("g_scale", o["g_scale"][:e], ref["g_scale"], bars["g_scale"])
        else:
            assert bool((o["g_scale"] == SENTINEL).all())
        if ref["g_gate"] is not None:
            near("g_gate", o["g_gate"][:e], ref["g_gate"], bars["g_gate"])
        else:
            assert bool((o["g_gate"] == SENTINEL).all())
        if d.p["mask"] == "all":
            for name in ("gU", "g_rel", "g_hid", "g_w"):
                assert not bool(o[name][:e].any()), (d.cell.id, name)
        return
    waves = (e + 255) // 256 * 4
    part = o["part"][:waves]
    dead = (e + 63) // 64
    assert not bool(part[dead:].any()), (d.cell.id, mode, "part rows of dead waves")
    sums = _ops.sum_rows(part)
    assert np.array_equal(sums.cpu().numpy(), sum_rows_order(part.cpu().numpy(), 1.0)), (d.cell.id, mode, "sum_rows order")
    near("sums", sums, bars["sums_ref"], bars["sums"])
    w3 = sums[:1024].view(64, 16)
    assert not bool(w3[hid3:].any()) and not bool(w3[:, m:].any()) and not bool(sums[1024 + hid3:1088].any()), (d.cell.id, mode, "pad d/dW3, d/db3")
    assert not bool(sums[1152 + m:1168].any()) and not bool(sums[1168 + m:1184].any()) and not bool(sums[1187:].any()), (d.cell.id, mode, "pad sums")
    assert int(o["amax"][0]) == int(gu.abs().max().view(torch.int32)), (d.cell.id, mode, "amax bits")
    if d.p["mask"] == "all":
        assert not bool(gu.any()) and not bool(grel.any()) and not bool(part.any()) and int(o["amax"][0]) == 0, (d.cell.id, mode, "all masked")


def _dst(d):
    ig = torch.arange(d.e) // d.k
    j = (torch.arange(d.e) % d.k) if d.idx is None else d.idx.reshape(-1)
    return (ig // d.n) * d.n + j


# ================================================================================================ bit-exact restatements (numpy)
def sum_rows_order(part, scale):
    """_ops.sum_rows on egnn_sum_parts_f32: a left-to-right fp32 sum over parts per element; with many rows first the rows p G + g over p
    for each of G groups, then the G group sums; the scale multiplied in last."""
    part = np.asarray(part, dtype=np.float32)
    rows = part.shape[0]
    g = 1
    while g < 256 and rows % (2 * g) == 0 and rows // (2 * g) >= 1:
        g *= 2
    if g > 1 and rows // g > 1:
        part = sum_parts_order(part.reshape(rows // g, -1), 1.0).reshape(g, -1)
    return sum_parts_order(part, scale)


def sum_parts_order(parts, scale):
    parts = np.asarray(parts, dtype=np.float32)
    acc = parts[0].copy()
    for r in range(1, parts.shape[0]):
        acc = (acc + parts[r]).astype(np.float32)
    return (acc * np.float32(scale)).astype(np.float32)


def split_image(x, scale=1.0):
    """hi = fp16(s x), lo = fp16(s x - float32(hi)) of an fp32 array, as numpy float16 arrays (the product s x rounded to fp32 first)"""
    y = (np.asarray(x, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = y.astype(np.float16)
        lo = (y - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo


def padded(a, rows_p, kp):
    out = np.zeros((rows_p, kp), dtype=a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def unpack_full(flat, rows, kp):
    """a packed image decoded WITH its pad rows: (ceil(rows / 32) * 32, kp) numpy float16"""
    from egnn_pytorch_amd._weights import unpack_tiles
    return unpack_tiles(flat.cpu(), rows, kp).numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def colsum_order(x, scale, ld):
    """the column sums of egnn_split_scaled_both_f16 in the kernel's order: scale * x per element, 8-row strands per column, the eight
    strand sums of a 64-row block in order, the blocks by `sum_rows_order`, then x 1 / scale; columns [cols, ld) are zeros."""
    x = np.asarray(x, dtype=np.float32)
    rows, cols = x.shape
    kpt = (rows + 31) // 32 * 32
    rows32 = (rows + 31) // 32 * 32
    nblk = (max(rows32, kpt) + 63) // 64
    y = np.zeros((nblk * 64, ld), dtype=np.float32)
    y[:rows, :cols] = (x * np.float32(scale)).astype(np.float32)
    parts = np.zeros((nblk, ld), dtype=np.float32)
    for blk in range(nblk):
        strands = []
        for q in range(8):
            s = np.zeros(ld, dtype=np.float32)
            for u in range(8):
                s = (s + y[blk * 64 + 8 * q + u]).astype(np.float32)
            strands.append(s)
        t = strands[0]
        for q in range(1, 8):
            t = (t + strands[q]).astype(np.float32)
        parts[blk] = t
    return sum_rows_order(parts, np.float32(1.0) / np.float32(scale)), parts


# ================================================================================================ node-level cells
POOL_CELLS = [dict(id=f"pool_n{n}_k{k}_{'gate' if gate else 'plain'}_{mask}", n=n, k=k, gate=gate, mask=mask)
              for n, k, gate, mask in ((1, 1, False, "none"), (15, 5, True, "scattered"), (16, 32, False, "ragged"), (17, 64, True, "node"),
                                       (33, 5, False, "node"), (33, 1, True, "all"), (16, 5, True, "none"), (17, 32, False, "scattered"),
                                       (1, 64, True, "scattered"), (15, 1, False, "none"))]

PREP_ROWS = (1, 31, 32, 33, 300)
PREP_DIMS = (1, 3, 4, 7, 8, 12, 100, 112, 124, 512)
PREP_CELLS = []
for _i, _dim in enumerate(PREP_DIMS):
    for _ln in (False, True):
        _rows = PREP_ROWS[(_i + int(_ln)) % len(PREP_ROWS)]
        PREP_CELLS.append(dict(id=f"prep_r{_rows}_d{_dim}_{'ln' if _ln else 'id'}_{'mi' if (_i + _ln) % 2 == 0 else 'nomi'}", rows=_rows, dim=_dim,
                               ln=_ln, mi=(_i + _ln) % 2 == 0, raw=_i % 3 == 0, data="randn"))
PREP_CELLS += [dict(id=f"prep_r{r}_d12_ln_mi_raw", rows=r, dim=12, ln=True, mi=True, raw=True, data="randn") for r in PREP_ROWS]
PREP_CELLS += [dict(id="prep_const_rows", rows=33, dim=100, ln=True, mi=True, raw=False, data="const"),
               dict(id="prep_mean1e4", rows=33, dim=112, ln=True, mi=False, raw=True, data="mean1e4"),
               dict(id="prep_gridstride", rows=262144 + 33, dim=4, ln=False, mi=True, raw=False, data="randn"),
               dict(id="prep_gridstride_ln", rows=262144 + 33, dim=4, ln=True, mi=False, raw=False, data="randn")]
SPLIT_ROWS, SPLIT_COLS = (1, 31, 32, 33, 63, 64, 65, 129), (1, 7, 8, 9, 31, 32, 33, 100)
SPLIT_CELLS = [dict(id=f"split_r{r}_c{SPLIT_COLS[(i * 3 + j) % 8]}", rows=r, cols=SPLIT_COLS[(i * 3 + j) % 8], ldx_extra=(0, 3, 4)[(i + j) % 3])
               for i, r in enumerate(SPLIT_ROWS) for j in range(3)]
SILU_COUNTS = (4, 8, 1020, 4100)
SILU_DROP = [dict(rows=r, cols=c, p=p) for (r, c), p in zip(((8, 4), (12, 5), (6, 6), (8, 7), (10, 130), (44, 5), (36, 7), (12, 130)),
                                                            (0.1, 0.5, 0.1, 0.5, 0.1, 0.5, 0.1, 0.5))]
NMF_DIMS, NMF_ROWS = (32, 64, 128, 256), (1, 15, 16, 17, 127, 128, 129)


def pool_case(cell):
    n, k = cell["n"], cell["k"]
    g = torch.Generator().manual_seed(n * 100 + k)
    u = torch.randn(1, n, k, 16, generator=g) * 2
    gate = (torch.randn(16, generator=g) * 0.7, torch.randn(1, generator=g)) if cell["gate"] else None
    pm = None
    if cell["mask"] == "scattered":
        pm = torch.rand(1, n, k, generator=g) > 0.4
    elif cell["mask"] == "ragged":
        pm = (torch.arange(k)[None, :] < torch.randint(0, k + 1, (n, 1), generator=g))[None]
    elif cell["mask"] == "node":
        pm = torch.rand(1, n, k, generator=g) > 0.3
        pm[:, n // 2] = False
    elif cell["mask"] == "all":
        pm = torch.zeros(1, n, k, dtype=torch.bool)

    def spec(dtype):
        mm = torch.nn.functional.silu(u.to(dtype))
        if gate is not None:
            mm = mm * torch.sigmoid(mm @ gate[0].to(dtype) + gate[1].to(dtype))[..., None]
        if pm is not None:
            mm = mm.masked_fill(~pm[..., None], 0.0)
        return mm.sum(dim=2)
    ref = spec(torch.float64)
    top = float(ref.abs().max())
    bar = min(ATEN_FACTOR * float((spec(torch.float32).double() - ref).abs().max()) + FLOOR * top, EDGE_CAP * max(top, 1e-30))
    return u, gate, pm, ref, bar


def prep_case(cell):
    rows, dim = cell["rows"], cell["dim"]
    g = torch.Generator().manual_seed(rows % 1000 + dim)
    x = torch.randn(rows, dim, generator=g) * 3 + 1
    if cell["data"] == "const":
        x[::3] = 2.5                                                              # rows of constants: variance 0, rstd = eps^-1/2
    elif cell["data"] == "mean1e4":
        x = torch.randn(rows, dim, generator=g) + 1e4                             # the two-pass variance
    mi = torch.randn(rows, 16, generator=g) if cell["mi"] else None
    gamma = torch.randn(dim, generator=g) if cell["ln"] else None
    beta = torch.randn(dim, generator=g) if cell["ln"] else None
    return x, mi, gamma, beta


def layer_norm_ref(x, gamma, beta, eps, dtype):
    return torch.nn.functional.layer_norm(x.to(dtype), (x.shape[1],), gamma.to(dtype), beta.to(dtype), eps)


def bar_f32(ref, f32, cap=None):
    top = float(ref.abs().max())
    derived = ATEN_FACTOR * float((f32.double() - ref).abs().max()) + FLOOR * top
    return derived if cap is None else min(derived, cap * max(top, 1e-30))


def silu_spec(z, g, dtype, drop=None, row0=0):
    """float64 autograd of SiLU(dropout(z)) with the hash twin at SITE_NODE: (a, gz)"""
    from egnn_pytorch_amd import _dropout
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        zd = zz
        if drop is not None:
            rows = torch.arange(z.shape[0]) + row0
            zd = _dropout.apply(zz, drop[1], _dropout.SITE_NODE, rows, drop[0])
        a = torch.nn.functional.silu(zd)
        gz = torch.autograd.grad(a, zz, g.to(dtype))[0]
    return a.detach(), gz.detach()


def nmf_case(dim, rows):
    g = torch.Generator().manual_seed(dim * 1000 + rows)
    m = 16
    w5 = torch.randn(2 * dim, dim + m, generator=g) / (dim + m) ** 0.5
    w6 = torch.randn(dim, 2 * dim, generator=g) / (2 * dim) ** 0.5
    b5, b6 = torch.randn(2 * dim, generator=g), torch.randn(dim, generator=g)
    x = torch.randn(rows, dim + m, generator=g)
    res = torch.randn(rows, dim, generator=g)

    def spec(dtype):
        t = lambda v: v.to(dtype)                                                 # noqa: E731
        return torch.nn.functional.silu(t(x) @ t(w5).t() + t(b5)) @ t(w6).t() + t(b6) + t(res)
    ref = spec(torch.float64)
    hid = torch.nn.functional.silu(x.double() @ w5.double().t() + b5.double())
    d_hid = SPLIT * (x.double().abs() @ w5.double().abs().t())
    split = 1.1 * d_hid @ w6.double().abs().t() + SPLIT * (hid.abs() @ w6.double().abs().t())
    top = max(1.0, float(ref.abs().max()))
    derived = ATEN_FACTOR * (spec(torch.float32).double() - ref).abs().max() + FLOOR * top + split
    return SimpleNamespace(w5=w5, w6=w6, b5=b5, b6=b6, x=x, res=res, ref=ref, bar=torch.clamp(derived, max=NMF_CAP * top))


# ================================================================================================ the per-lane REDUCE kernel's child
def scalar_child():
    """EGNN_TAIL_SCALAR=1 in a fresh process: every REDUCE cell on edge_tail_bwd_kernel<true> against the same specification and bars,
    and the launcher's refusal of dropout there."""
    assert os.environ.get("EGNN_TAIL_SCALAR") == "1"
    worst = {}
    ran = 0
    for c in TAIL_CELLS:
        d = prepare(c.id)
        if d.drop is not None:
            t = tail_device_inputs(d)
            o = tail_outputs(d.e, True, False)
            rc = tail_launch(tail_args(d, t, o, True, d.drop, d.eid0))
            torch.cuda.synchronize()
            assert rc == E_UNSUPPORTED, (c.id, rc)
            assert all(bool((v == (0x7fc00000 if name == "amax" else SENTINEL)).all()) for name, v in o.items()), c.id
            continue
        _, o = tail_run(d, "scalar")
        tail_check(d, "scalar", o, worst)
        _, o2 = tail_run(d, "scalar")
        assert all(torch.equal(o[name], o2[name]) for name in o), (c.id, "two runs differ")
        ran += 1
    print(f"scalar child: {ran} cells, worst error / bar {worst}")
    return 0


if __name__ == "__main__":
    if "--scalar-child" in sys.argv:
        sys.exit(scalar_child())
