"""Every template instantiation of the fused edge pass (csrc/edge_fused.hip: 2 coordinate classes x 5 scalar classes x 3 head widths x
3 neighbour-count classes = 90, tests/_edge_variants.py) against float64, in its three modes:

  a. inference (MODE 0)            the float64 oracle, 1e-4 max(1, max|want| / 256) (tests/test_gpu_fuzz.py)
  b. training without dropout      forward under autograd (MODE 1, or MODE 0 writing u) at bar (a); every gradient of the native backward
                                   (csrc/edge_bwd.hip, csrc/edge_tail.hip) against float64 autograd of the restated layer over the same
                                   neighbour list: 2e-4 of the gradient's scale, or four times the fp32 restatement's own distance from
                                   float64 where the sum cancels heavily; None matches None, a zero gradient is exactly zero
  c. training-mode dropout, p 0.2  (MODE 3) forward and gradients against the restatement carrying the same hash masks, the bars of (b)

The backward route is pinned: `_backward_native` runs, `_backward_exact` and `_backward_recompute` raise (`_dropout_native_ok` holds for
every cell of the grid: no class is sent to another backward).  The one cell the wave-per-node kernel covers (csrc/edge_pw.hip) runs (a)
and (b) twice: as dispatched and with the general kernel forced.  Every failure names the cell, the instantiation (CDM, NM, NB, TPI,
HCT), the worst error and its bound; EGNN_EDGE_VARIANTS_OUT=<file> appends one JSON line per cell and mode (profiles/edge_variants)."""
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import _edge_variants as V

pytestmark = pytest.mark.gpu

IDS = [c.id for c in V.CELLS]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _layer(cell, p, dropout=0.0):
    from egnn_pytorch_amd import EGNN
    layer = EGNN(**cell.kw, dropout=dropout)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in p.params.items()}, strict=True)
    return layer.cuda()


def _inputs(p):
    return _dev(p.feats), _dev(p.coors), _dev(p.edges), _dev(p.mask), _dev(p.adj)


def _pw_cell(cell):
    """the wave-per-node kernel runs this cell's inference and autograd forward (egnn_edge_pw_covers, given slot records: a k-NN layer)"""
    from egnn_pytorch_amd import _abi
    kw = cell.kw
    s = 2 * kw["fourier_features"] + 1 + kw["edge_dim"]
    hp = _abi.load().egnn_padded_hidden(2 * (2 * kw["dim"] + s))
    covers = _abi.load().egnn_edge_pw_covers(cell.b, cell.n, cell.k, s, kw["fourier_features"], kw["edge_dim"], kw["m_dim"], cell.cdim, 2 * hp)
    return covers == 1 and cell.source == "knn"


@contextlib.contextmanager
def _edge_algo(algo):
    from egnn_pytorch_amd import layer as L
    old = L._EDGE_ALGO
    L._EDGE_ALGO = algo
    try:
        yield
    finally:
        L._EDGE_ALGO = old


@contextlib.contextmanager
def _native_backward_only(cell):
    """tests/test_gpu_mask_patterns_training.py::_pinned_path: the native backward and no other"""
    from egnn_pytorch_amd import autograd as A
    names = ("_backward_native", "_backward_exact", "_backward_recompute")
    saved = {nm: getattr(A, nm) for nm in names}
    taken = []

    def forbid(nm):
        def raiser(*a, **k):
            raise AssertionError(f"{cell.id} {tuple(cell.inst)}: expected on _backward_native, but {nm} ran")
        return raiser

    def spy(*a, **k):
        taken.append("native")
        return saved["_backward_native"](*a, **k)
    try:
        A._backward_native = spy
        A._backward_exact, A._backward_recompute = forbid("_backward_exact"), forbid("_backward_recompute")
        yield taken
    finally:
        for nm, v in saved.items():
            setattr(A, nm, v)


class _Worst:
    """the worst error-to-bound ratio of one cell and mode; `check` raises with the cell, the instantiation, the error and the bound"""

    def __init__(self, cell, mode):
        self.cell, self.mode, self.ratio, self.what, self.err, self.tol = cell, mode, 0.0, None, 0.0, 0.0
        self.failed = []

    def add(self, what, err, tol):
        assert np.isfinite(err), f"{self.cell.id} {tuple(self.cell.inst)} {self.mode} {what}: non-finite"
        ratio = err / tol
        if ratio > self.ratio or self.what is None:           # (a tie keeps the first: the call as dispatched)
            self.ratio, self.what, self.err, self.tol = ratio, what, err, tol
        if not err <= tol:
            self.failed.append(f"{what}: error {err:.3e} > bound {tol:.3e}")

    def check(self):
        line = dict(cell=self.cell.id, mode=self.mode, inst=list(self.cell.inst), worst_ratio=round(self.ratio, 4), what=self.what,
                    err=float(f"{self.err:.4e}"), bound=float(f"{self.tol:.4e}"))
        print("EDGEVAR " + json.dumps(line), flush=True)
        out = os.environ.get("EGNN_EDGE_VARIANTS_OUT")
        if out:
            with open(out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        assert not self.failed, (f"{self.cell.id} inst (CDM, NM, NB, TPI, HCT) = {tuple(self.cell.inst)} mode {self.mode}: worst {self.what} "
                                 f"error {self.err:.3e} bound {self.tol:.3e}; " + "; ".join(self.failed))


def _forward_bar(worst, tag, got, want):
    """bar (a): 1e-4 max(1, max|want| / 256), for both outputs"""
    for name, g, w in zip(("node", "coors"), got, want):
        w = w if isinstance(w, np.ndarray) else w.detach().cpu().numpy()
        assert np.isfinite(w).all(), (worst.cell.id, name)
        tol = 1e-4 * max(1.0, float(np.abs(w).max()) / 256.0)
        worst.add(f"{tag}{name}", float(np.abs(g.detach().cpu().numpy().astype(np.float64) - w).max()), tol)


def _leaves(args, dtype):
    mk = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)                     # noqa: E731
    return mk(args[0]), mk(args[1]), mk(args[2])


def _restated(layer, args, sel, cot, dtype, drop):
    """(node, coors_out, gradients) of autograd.layer_given_neighbors in `dtype` over the neighbour list `sel` of the HIP forward"""
    from egnn_pytorch_amd import autograd as A
    idx, rank, radius = sel
    mod = copy.deepcopy(layer).to(dtype)
    f, x, e = _leaves(args, dtype)
    with torch.enable_grad():
        node, co = A.layer_given_neighbors(mod, f, x, e, args[3], None if idx is None else idx.long(), None if rank is None else rank.to(dtype),
                                           radius, drop=drop)
        wrt = [t for t in (f, x, e) if t is not None] + list(mod.parameters())
        grads = torch.autograd.grad([node, co], wrt, [cot[0].to(dtype), cot[1].to(dtype)], allow_unused=True)
    return node.detach(), co.detach(), grads


def _training(cell, mode, algos=(0,)):
    from egnn_pytorch_amd import autograd as A
    drop = (V.DROPOUT_P, V.dropout_seed()) if mode == "dropout" else None
    p = V.prepare(cell, drop=drop)
    V.check_preconditions(cell, p)
    layer = _layer(cell, p, dropout=V.DROPOUT_P if drop else 0.0).train()
    assert layer.dropout_active() == (drop is not None)
    if drop is not None:
        assert A._dropout_native_ok(layer), cell.id            # (every class of the grid keeps the native backward under dropout)
    args = _inputs(p)
    g = torch.Generator().manual_seed(cell.seed + 1)
    cot = (torch.randn(cell.b, cell.n, cell.kw["dim"], generator=g).cuda(), torch.randn(cell.b, cell.n, cell.cdim, generator=g).cuda())
    names = ["feats", "coors"] + (["edges"] if args[2] is not None else []) + [k for k, _ in layer.named_parameters()]
    worst = _Worst(cell, mode)
    sel = ref64 = ref32 = None
    for algo in algos:
        tag = "" if algo == 0 else "general kernel forced: "
        f, x, e = _leaves(args, torch.float32)
        with _edge_algo(algo), _native_backward_only(cell) as taken:
            torch.manual_seed(V.TORCH_SEED)                      # (the dropout mode's forward draws `V.dropout_seed()`)
            node, co = layer(f, x, e, args[3], args[4])
            wrt = [t for t in (f, x, e) if t is not None] + list(layer.parameters())
            grads = torch.autograd.grad([node, co], wrt, list(cot), allow_unused=True)
        assert taken, f"{cell.id}: the native backward did not run"
        if sel is None:
            with torch.no_grad():
                sel = layer._forward_hip_checked(args[0], args[1], args[2], args[3], args[4], None, drop_seed=None if drop is None else drop[1])[3:6]
            ref64 = _restated(layer, args, sel, cot, torch.float64, drop)
            ref32 = _restated(layer, args, sel, cot, torch.float32, drop)       # the yardstick for heavily cancelling sums
        # the forward under autograd: against the float64 oracle (no dropout) / the restatement with the same masks (dropout)
        _forward_bar(worst, tag, (node, co), p.want if drop is None else ref64[:2])
        assert len(grads) == len(ref64[2]) == len(names)
        for nm, gg, ww, rr in zip(names, grads, ref64[2], ref32[2]):
            assert (gg is None) == (ww is None), (cell.id, tuple(cell.inst), nm, "None gradient")
            if gg is None:
                continue
            scale = float(ww.abs().max())
            if scale == 0.0:
                assert float(gg.abs().max()) == 0.0, (cell.id, tuple(cell.inst), nm, "a zero gradient is not exactly zero")
                continue
            tol = 2e-4 * scale
            # (CoorsNorm's self pair makes any fp32 autograd of the coordinates carry O(1) noise -- DESIGN.md section 10: no yardstick there)
            if not (nm == "coors" and cell.kw.get("norm_coors")):
                tol = max(tol, 4.0 * float((rr.double() - ww).abs().max()))
            worst.add(f"{tag}d/d {nm}", float((gg.double() - ww).abs().max()), tol)
    worst.check()


@pytest.mark.parametrize("cid", IDS)
def test_inference(cid):
    from egnn_pytorch_amd import _ops
    cell = V.BY_ID[cid]
    p = V.prepare(cell)
    V.check_preconditions(cell, p)                               # on the reference alone; asserted, never skipped
    layer = _layer(cell, p).eval()
    args = _inputs(p)
    worst = _Worst(cell, "inference")
    pw = _pw_cell(cell)
    assert pw == (tuple(cell.inst) == (3, 1, 1, 2, 128)), cid
    for algo in ((0, 1) if pw else (0,)):
        with torch.no_grad(), _edge_algo(algo), _ops.phase_timer() as pt:
            got = layer(*args)
        launched = set(pt.summary())
        assert "edge_fused" in launched and "edge_exact" not in launched, (cid, tuple(cell.inst), launched)
        _forward_bar(worst, "" if algo == 0 else "general kernel forced: ", got, p.want)
    with torch.no_grad():                                        # the same call as a user makes it (the one-call C forward where it covers)
        _forward_bar(worst, "plain call: ", layer(*args), p.want)
    worst.check()


@pytest.mark.parametrize("cid", IDS)
def test_training(cid):
    cell = V.BY_ID[cid]
    _training(cell, "training", algos=(0, 1) if _pw_cell(cell) else (0,))


@pytest.mark.parametrize("cid", IDS)
def test_training_mode_dropout(cid):
    _training(V.BY_ID[cid], "dropout")
