"""Forward and training at the module's own initialisation (tests/_default_init.py: every Linear weight N(0, 1e-3)) -- the state every
run starts in and stays near for its first tens of optimiser steps, which the other gradient tests leave on purpose.

Reference throughout: float64 autograd of `autograd.layer_given_neighbors` on a `.double()` copy, over the neighbour list the HIP
forward returned (`_float64` of tests/test_gpu_mask_patterns_training.py, whose builders, path pinning and exact checks are used as
they are).  Bars: every gradient within 1e-4 of ITS OWN max |reference| (1e-8 for the float64 row), no absolute term; the forward on
the UPDATES node - feats and coors_out - coors, min(1e-4, 8 x the error torch fp32 makes on that quantity + 16 x 2^-24 max |output|),
the last term being the rounding of the final residual add.  The host conditions of every case: tests/test_default_init_table.py.

Each case prints one `DEFAULT_INIT` line: its worst error / bar (EGNN_TEST_VERBOSE: per tensor, with the torch-fp32 restatement's
error / scale on the same inputs beside it)."""
import contextlib
import copy
import os

import pytest
import torch

from tests import _default_init as D
from tests import test_gpu_mask_patterns_training as M
from tests._util import ATOL

pytestmark = pytest.mark.gpu
VERBOSE = bool(os.environ.get("EGNN_TEST_VERBOSE"))


def _own_scale_errors(c, grads, rgrads):
    out = {}
    for nm, g, r in zip(M._names(c), grads, rgrads):
        if g is None or r is None or not bool(r.any()):
            continue
        out[nm] = float((g.double() - r).abs().max()) / float(r.abs().max())
    return out


def _report(c, what, worst, ref, neigh):
    top = max(worst, key=worst.get)
    print(f"DEFAULT_INIT {what} worst error / bar {worst[top] / D.bar(c):.3f} ({top})", flush=True)
    if VERBOSE:
        f32 = _own_scale_errors(c, D.restated(c, torch.float32, *neigh)[2], ref[2])
        print(f"DEFAULT_INIT {what} error / scale (torch fp32 beside it): "
              + " ".join(f"{k}={v:.1e}({f32.get(k, float('nan')):.1e})" for k, v in worst.items()), flush=True)


def _gradients(c, ref, what, chunks=(0, 2)):
    """the case on its pinned path, whole and in chunks of two graphs, at the bars of tests/test_gpu_mask_patterns_training.py::_compare
    (own scale, structural zeros exact, padded rows exact), with no native backward answered by the recompute"""
    from egnn_pytorch_amd import autograd as A
    reruns = A.backward_reruns
    zeros = D.structural_zeros(c)
    neigh = D.neighbours(c)
    for chunk in chunks:
        got = M._hip(c, chunk)
        worst = M._compare(c, got, ref, f"{what}/chunk{chunk}", structural_zero=zeros)
        _report(c, f"{what}/chunk{chunk}", worst, ref, neigh)
    assert A.backward_reruns == reruns, (what, "a native backward was answered by the ATen recompute")


# ------------------------------------------------------------------------------------------------ 1. gradients at step 0
@pytest.mark.parametrize("row,form", D.CASES, ids=[f"{r}-{f}" for r, f in D.CASES])
def test_gradients_at_step_zero(row, form):
    c = D.build(row, form)
    for mod in c.layer.modules():                                   # the state the host table vouches for
        if isinstance(mod, torch.nn.Linear):
            assert D.STD_RANGE[0] <= float(mod.weight.detach().double().std()) <= D.STD_RANGE[1]
    _gradients(c, M._float64(c), f"{row}/{form}")


# ------------------------------------------------------------------------------------------------ 2. the forward routes
ROUTES = (("c_forward", {}), ("python_launch", dict(_C_FORWARD=False)), ("general_kernel", dict(_EDGE_ALGO=1)))
# the routes give the same bits (tests/test_gpu_offset_limits.py, tests/test_gpu_edge_pw_occupancy.py): fp32 k-NN layers without per-pair features
SAME_BITS = ("pw_k8", "pw_k32", "k48_rounds")


@contextlib.contextmanager
def _switches(**kw):
    from egnn_pytorch_amd import layer as L
    old = {k: getattr(L, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(L, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(L, k, v)


@pytest.mark.parametrize("row", list(M.ROWS))
def test_forward_updates_on_every_route(row):
    """The C forward under no_grad, the Python launch sequence and the general edge kernel (the wave-per-node kernel is what the first
    two run where it covers the shape; a build holds one workgroup count of it).  At this state node_out = feats + ~0.1: the outputs
    themselves pass any bar, the updates do not."""
    c = D.build(row, "both")
    idx, rank, radius = D.neighbours(c)
    ref = D.restated(c, torch.float64, idx, rank, radius)
    f32 = D.restated(c, torch.float32, idx, rank, radius)
    cap = 1e-9 if c.path == "double" else ATOL
    bars = {}
    for i, (name, x) in enumerate((("node - feats", c.feats), ("coors_out - coors", c.coors))):
        want = ref[i] - x.double()
        aten = float(((f32[i].double() - x.double()) - want).abs().max())
        bars[name] = min(cap, 8.0 * aten + 16.0 * 2.0 ** -24 * float(ref[i].abs().max()))
        assert float(want.abs().max()) > 0, (row, name)
    outs = {}
    for route, kw in ROUTES:
        with _switches(**kw), torch.no_grad():
            node, co = c.layer(c.feats, c.coors, c.edges, c.mask, c.adj)
        outs[route] = (node, co)
        assert bool(torch.isfinite(node).all()) and bool(torch.isfinite(co).all()), (row, route)
        assert torch.equal(co[~c.mask], c.coors[~c.mask]), (row, route, "padded nodes moved")
        for i, (name, x) in enumerate((("node - feats", c.feats), ("coors_out - coors", c.coors))):
            got = (node, co)[i].double() - x.double()
            want = ref[i] - x.double()
            err = float((got - want).abs().max())
            print(f"DEFAULT_INIT forward {row}/{route} {name}: error {err:.2e} bar {bars[name]:.2e} (max |update| {float(want.abs().max()):.2e})", flush=True)
            assert err <= bars[name], (row, route, name, err, bars[name])
    if row in SAME_BITS:
        for route in ("python_launch", "general_kernel"):
            assert torch.equal(outs[route][0], outs["c_forward"][0]) and torch.equal(outs[route][1], outs["c_forward"][1]), (row, route)


# ------------------------------------------------------------------------------------------------ 3. small cotangents
@pytest.mark.parametrize("power", [24, 48])
@pytest.mark.parametrize("row", ["pw_k8", "two_tiles_flags", "dense", "exact_cdim9"])
def test_cotangents_of_a_mean_over_a_large_batch(row, power):
    """The cotangents x 2^-24 (a mean over a north-star batch) and x 2^-48 (that squared): the same own-scale bar against float64 at
    that scale; every gradient finite, and non-zero where the reference is."""
    c = D.build(row, "both")
    unit = M._hip(c, 0)[2]
    c.rn, c.rc = c.rn * 2.0 ** -power, c.rc * 2.0 ** -power
    ref = M._float64(c)
    got = M._hip(c, 0)
    worst = M._compare(c, got, ref, f"{row}/2^-{power}")
    for nm, g, r in zip(M._names(c), got[2], ref[2]):
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()) == bool(r.any()), (row, power, nm)
    same = [nm for nm, g, u in zip(M._names(c), got[2], unit) if torch.equal(g, u * 2.0 ** -power)]
    top = max(worst, key=worst.get)
    print(f"DEFAULT_INIT {row}/2^-{power} worst error / bar {worst[top] / D.bar(c):.3f} ({top}); 2^-{power} x the unit-scale bits: "
          f"{len(same)} of {len(unit)} tensors" + ("" if len(same) == len(unit) else f" (not: {[n for n in M._names(c) if n not in same]})"), flush=True)


# ------------------------------------------------------------------------------------------------ 4. the first thirty steps
STEPS = (0, 1, 3, 10, 30)


@pytest.mark.parametrize("row", ["pw_k8", "two_tiles_flags", "dense"])
def test_gradients_along_the_first_adam_steps(row):
    """Teacher-forced: Adam (lr 1e-3) runs on the float64 restatement, on the device, on a masked mean-squared loss over both outputs;
    the inputs are fixed, so is the neighbour list.  At steps 0, 1, 3, 10 and 30 the parameters are cast to fp32 and loaded into the
    HIP layer, and its gradients of that loss are compared with float64 autograd AT THOSE fp32 PARAMETERS, at the own-scale bar.  (The
    cotangent handed to both sides is the loss's derivative at the float64 outputs, cast to fp32.)  A free-running fp32 trajectory
    would diverge from the float64 one through Adam's early sign flips, which says nothing about the kernels."""
    from egnn_pytorch_amd import autograd as A
    c = D.build(row, "both")
    idx, rank, radius = D.neighbours(c)
    i64, r64 = None if idx is None else idx.long(), None if rank is None else rank.double()
    g = torch.Generator().manual_seed(c.seed + 3)
    tn, tc = (torch.randn(c.feats.shape, generator=g).cuda().double(), torch.randn(c.coors.shape, generator=g).cuda().double())
    real = c.mask[..., None].double()
    count = float(c.mask.sum())
    l64 = copy.deepcopy(c.layer).double()
    f64, x64, e64 = c.feats.double(), c.coors.double(), None if c.edges is None else c.edges.double()
    opt = torch.optim.Adam(l64.parameters(), lr=1e-3)
    std0 = float(l64.edge_mlp[0].weight.std())

    def loss_of(layer):
        node, co = A.layer_given_neighbors(layer, f64, x64, e64, c.mask, i64, r64, radius)
        return (((node - tn) ** 2 * real).sum() / (count * node.shape[-1]) + ((co - tc) ** 2 * real).sum() / (count * co.shape[-1])), node, co

    for step in range(STEPS[-1] + 1):
        if step in STEPS:
            state = {k: v.detach().float() for k, v in l64.state_dict().items()}
            c.layer.load_state_dict(state)
            at32 = copy.deepcopy(c.layer).double()                   # float64 arithmetic at the fp32 parameters
            node, co = A.layer_given_neighbors(at32, f64, x64, e64, c.mask, i64, r64, radius)
            c.rn = (2.0 * (node - tn) * real / (count * node.shape[-1])).detach().float()
            c.rc = (2.0 * (co - tc) * real / (count * co.shape[-1])).detach().float()
            _gradients(c, M._float64(c), f"{row}/step{step}", chunks=(0,))
        opt.zero_grad()
        loss_of(l64)[0].backward()
        opt.step()
    std30 = float(l64.edge_mlp[0].weight.std())
    print(f"DEFAULT_INIT {row} std(edge_mlp.0.weight) {std0:.1e} -> {std30:.1e} over {STEPS[-1]} steps", flush=True)
    assert std30 > 3 * std0, (row, std0, std30, "the trajectory did not leave the initial state")
