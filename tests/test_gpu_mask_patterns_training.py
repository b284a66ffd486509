"""Training under padding masks that are no prefixes (tests/_masks.py): scattered, padding in front, aligned blocks of four, an empty
graph in the middle of the batch, fewer real nodes than neighbours, interleaved -- on every backward path.

Every other gradient test builds its mask as `arange(n) < len`.  The backward reads the mask geometry in many places (the spatial order
lists padded nodes last, the by-destination entry lists are built over all edges, a padded node's neighbours are the first K nodes
wherever they are), and with a prefix mask those first K nodes are always real.

Reference: float64 autograd of `autograd.layer_given_neighbors` on a `deepcopy(layer).double()`, over the neighbour list the HIP forward
itself returned (tests/test_autograd.py pins that restatement to the reference module's own float64 autograd on exactly these masks).
Cotangents are randn on real rows and exactly zero on padded rows: a loss over real nodes.  Bars: forward 1e-4 (tests/_util.ATOL), every
gradient within 1e-4 of ITS OWN scale (max |reference|, asserted > 0); float64 modules 1e-9 / 1e-8 of scale (tests/test_dropout.py)."""
import contextlib
import copy
import os
import zlib

import numpy as np
import pytest
import torch

from tests._masks import B, PATTERNS, mask_pattern
from tests._util import ATOL

pytestmark = pytest.mark.gpu

# id -> (layer kwargs, n, coordinate dimension, backward path).  The smallest shapes that still take the path named in the comment.
ROWS = {
    "pw_k8": (dict(dim=32, num_nearest_neighbors=8), 40, 3, "native"),                       # wave-per-node edge kernel, four nodes per tile
    "pw_k32": (dict(dim=64, num_nearest_neighbors=32, norm_feats=True), 96, 3, "native"),    # one node per wave
    "two_tiles_flags": (dict(dim=48, num_nearest_neighbors=24, soft_edges=True, norm_coors=True, m_pool_method="mean",
                             coor_weights_clamp_value=1.5, norm_feats=True), 70, 3, "native"),   # second tile padded; gate, CoorsNorm, counts
    "k48_rounds": (dict(dim=24, num_nearest_neighbors=48), 96, 3, "native"),                 # multi-round node groups
    "dense": (dict(dim=32), 20, 3, "native"),                                                # general edge kernel, all pairs
    "scalars5": (dict(dim=32, num_nearest_neighbors=8, edge_dim=3, fourier_features=2, soft_edges=True), 48, 3, "native"),   # d/d s, W_s, edges
    "m32_blocks": (dict(dim=32, num_nearest_neighbors=16, m_dim=32), 40, 3, "native"),       # per-16-channel block passes
    "cdim5": (dict(dim=32, num_nearest_neighbors=8, norm_coors=True), 40, 5, "native"),      # generic tail kernel
    "sparse_adj": (dict(dim=32, edge_dim=4, only_sparse_neighbors=True, norm_coors=True), 40, 3, "native"),   # band adjacency |i - j| <= 2
    "radius": (dict(dim=32, num_nearest_neighbors=8), 40, 3, "native"),                      # pair mask = node masks AND radius (the median)
    "exact_cdim9": (dict(dim=24, num_nearest_neighbors=8, coor_weights_clamp_value=2.0), 30, 9, "exact"),     # egnn_edge_exact_bwd_f32
    "exact_m80": (dict(dim=16, num_nearest_neighbors=6, m_dim=80, soft_edges=True), 24, 3, "exact"),          # blocked plain kernel
    "exact_fourier8": (dict(dim=16, fourier_features=8, edge_dim=2, m_pool_method="mean"), 14, 3, "exact"),   # more than 16 scalars
    "double": (dict(dim=16, num_nearest_neighbors=6, norm_coors=True, fourier_features=1), 20, 3, "double"),  # float64 kernels
    "recompute": (dict(dim=24, num_nearest_neighbors=6), 20, 3, "recompute"),                # autograd._NATIVE = False: ATen recompute
}
BAND = 2


class Case:
    pass


def _neighbour_count(kw):
    """K of a row as tests/_masks.py takes it: None for a dense layer, the band's degree for the adjacency row"""
    if kw.get("only_sparse_neighbors"):
        return 2 * BAND + 1
    return kw.get("num_nearest_neighbors") or None


def _make_layer(kw, seed, path, state=None, device="cuda"):
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed % (2 ** 31))
    layer = EGNN(**kw)
    if state is not None:
        layer.load_state_dict(state)
    else:
        with torch.no_grad():
            if kw.get("coor_weights_clamp_value"):
                # the rows with a clamp: xavier weights (tests/test_autograd.py's baseline-width tests) instead of parameters x 40.  Those
                # leave every Linear dominated by its scaled bias and the coordinate weights within ~1e-2 of one value over all edges:
                # the clamp is then off for every pair, or on for every pair (no gradient behind it), or -- put in between -- within
                # fp32 rounding of thousands of pairs at once, where its derivative jumps.  See `_centre_clamp`.
                for mod in layer.modules():
                    if isinstance(mod, torch.nn.Linear):
                        torch.nn.init.xavier_normal_(mod.weight)
            else:
                for p in layer.parameters():
                    p.mul_(40.0)                               # away from the vacuous default init (std 1e-3), as elsewhere
    if path == "double":
        layer = layer.double()
    return layer.to(device)


def _build(row, pattern, seed, n=None, with_edges=None, dropout=0.0, kw_extra=None, make_layer=None, device="cuda", centre_clamp=True):
    """One case: layer, inputs, mask, cotangents (zero on padded rows).  with_edges: None = as the row says; True / False = the layer
    with / without per-pair edge features (the seeded walk draws it).  make_layer: another layer factory with `_make_layer`'s signature
    (tests/_default_init.py: the module's own initialisation, where no clamp can be centred: centre_clamp=False); device: "cpu" for the host table tests,
    which supply a host forward."""
    make_layer = make_layer or _make_layer
    kw, n0, cdim, path = ROWS[row]
    kw = dict(kw, **(kw_extra or {}))
    if with_edges is True and not kw.get("edge_dim"):
        kw["edge_dim"] = 2
    if with_edges is False:
        kw.pop("edge_dim", None)
    if dropout:
        kw["dropout"] = dropout
    n = n or n0
    c = Case()
    c.row, c.pattern, c.seed, c.n, c.path, c.kw = row, pattern, seed, n, path, kw
    c.k = _neighbour_count(kw)
    dt = torch.float64 if path == "double" else torch.float32
    c.dtype = dt
    c.mask = torch.from_numpy(mask_pattern(pattern, B, n, c.k, np.random.default_rng(seed))).to(device)
    g = torch.Generator().manual_seed(seed + 1)
    dim = kw["dim"]
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dt).to(device)         # noqa: E731  (float32 values, also for a float64 module)
    # coors_out = x_i + sum over K neighbours of w_ij (x_i - x_j), with |w_ij| up to ~7 from coors_mlp's scaled last bias: K |w| |x| has to
    # stay at a few tens for fp32 (ulp(64) = 7.6e-6) to resolve the absolute forward bar of 1e-4 at all -- coordinates of scale 8 / K
    kk = n if c.k is None else c.k
    c.feats, c.coors = mk(B, n, dim), mk(B, n, cdim) * min(1.0, 8.0 / kk)
    c.edges = mk(B, n, n, kw["edge_dim"]) if kw.get("edge_dim") else None
    c.rn, c.rc = mk(B, n, dim) * c.mask[..., None], mk(B, n, cdim) * c.mask[..., None]
    c.adj = None
    if kw.get("only_sparse_neighbors"):
        i = torch.arange(n)
        c.adj = ((i[:, None] - i[None, :]).abs() <= BAND).to(device)
    c.layer = make_layer(kw, seed, path, device=device)
    if kw.get("coor_weights_clamp_value") and centre_clamp:
        _centre_clamp(c)
    if row == "radius":
        # valid_radius = the median distance over the selected pairs that pass the node masks: half of them fall to the radius
        with torch.no_grad():
            idx, rank = c.layer._forward_hip_checked(c.feats, c.coors, c.edges, c.mask, c.adj, None)[3:5]
        bi = torch.arange(B, device=device)[:, None, None]
        live = c.mask[:, :, None] & c.mask[bi, idx.long()]
        radius = float(rank[live].median())
        c.layer = make_layer(dict(kw, valid_radius=radius), seed, path, state=c.layer.state_dict(), device=device)
        c.kw = dict(kw, valid_radius=radius)
    return c


def _centre_clamp(c):
    """Shift coors_mlp's last bias so that the clamp value falls among the coordinate weights of the pairs that pass the masks: into the
    middle of the widest gap between two neighbouring weights between their 10 % and 90 % quantiles.  A good part of the pairs is then
    clamped, whatever the seed, and none sits within rounding of the kink: on which side a pair falls must not depend on fp32 against
    float64 rounding, since the derivative jumps there."""
    from egnn_pytorch_amd import autograd as A
    layer = c.layer
    with torch.no_grad():
        idx, rank, radius, u = layer._forward_hip_checked(c.feats, c.coors, c.edges, c.mask, c.adj, None, want_u=True)[3:7]
        kk = c.n if idx is None else idx.shape[-1]
        mm = torch.nn.functional.silu(u.view(B, c.n, kk, -1)[..., :layer.m_dim])
        if layer.edge_gate is not None:
            mm = mm * layer.edge_gate(mm)
        w = layer.coors_mlp(mm).squeeze(-1)
        pm = A._pair_mask(c.mask, None if idx is None else idx.long(), rank, radius)
        ws = w[pm].double().sort().values
        lo, hi = ws.numel() // 10, max(ws.numel() // 10 + 1, 9 * ws.numel() // 10)
        gaps = ws[lo + 1:hi + 1] - ws[lo:hi]
        j = int(gaps.argmax())
        assert float(gaps[j]) > 4e-5, "no gap among the coordinate weights wide enough to put the clamp in"
        layer.coors_mlp[3].bias += (layer.coor_weights_clamp_value - 0.5 * (ws[lo + j] + ws[lo + j + 1])).float()


def _names(c):
    return ["feats", "coors"] + (["edges"] if c.edges is not None else []) + [k for k, _ in c.layer.named_parameters()]


def _leaves(c, dtype=None):
    mk = lambda t: None if t is None else (t if dtype is None else t.to(dtype)).clone().requires_grad_(True)      # noqa: E731
    return mk(c.feats), mk(c.coors), mk(c.edges)


@contextlib.contextmanager
def _pinned_path(c, chunk):
    """The case's backward path and no other: the two paths it must not take raise.  chunk: graphs per chunk (0 = whole batch) -- each
    path has its own knob for the chunking that very large batches get."""
    from egnn_pytorch_amd import autograd as A
    names = ("_backward_native", "_backward_exact", "_backward_recompute", "_NATIVE", "_FUSED_MAX_GRAPHS", "_EXACT_BWD_BYTES", "_CHUNK_BUDGET_BYTES")
    saved = {nm: getattr(A, nm) for nm in names}
    taken = []
    own = {"native": "_backward_native", "exact": "_backward_exact", "double": "_backward_exact", "recompute": "_backward_recompute"}[c.path]

    def forbid(nm):
        def raiser(*a, **k):
            raise AssertionError(f"{c.row}: expected on {own}, but {nm} ran")
        return raiser

    def spy(*a, **k):
        taken.append(own)
        return saved[own](*a, **k)
    try:
        for nm in names[:3]:
            setattr(A, nm, spy if nm == own else forbid(nm))
        if c.path == "recompute":
            A._NATIVE = False
        if chunk:
            layer = c.layer
            kk = c.n if c.k is None else c.k
            din = 2 * layer.dim + 2 * layer.fourier_features + 1 + layer.edge_dim
            A._FUSED_MAX_GRAPHS = chunk
            A._EXACT_BWD_BYTES = chunk * 2 * c.n * kk * (2 * din) * (8 if c.path == "double" else 4)
            A._CHUNK_BUDGET_BYTES = int(chunk * c.n * kk * (2 * din) * 4.0 * A._BYTES_PER_EDGE_FACTOR)
        yield taken
    finally:
        for nm, v in saved.items():
            setattr(A, nm, v)


def _shape_condition(c):
    layer = c.layer
    s_in = 2 * layer.fourier_features + 1 + layer.edge_dim
    beyond = c.coors.shape[-1] > 8 or layer.m_dim > 64 or s_in > 16
    if c.path == "exact":
        assert beyond and not layer.float64_kernels()
    elif c.path == "double":
        assert layer.float64_kernels()
    else:
        assert not beyond and not layer.float64_kernels()


def _hip(c, chunk, torch_seed=None):
    """(node, coors_out, gradients of feats, coors, [edges,] every parameter) through the drop-in layer on the pinned path"""
    _shape_condition(c)
    f, x, e = _leaves(c)
    with _pinned_path(c, chunk) as taken:
        if torch_seed is not None:
            torch.manual_seed(torch_seed)
        node, co = c.layer(f, x, e, c.mask, c.adj)
        wrt = [t for t in (f, x, e) if t is not None] + list(c.layer.parameters())
        grads = torch.autograd.grad([node, co], wrt, [c.rn, c.rc], allow_unused=True)
    assert taken, f"{c.row}: the expected backward did not run"
    return node.detach(), co.detach(), grads


def _float64(c, drop=None, src=None):
    """float64 autograd of the restated layer over the neighbour list of the HIP forward (of `src`'s inputs, default the case's own)"""
    from egnn_pytorch_amd import autograd as A
    s = src or c
    with torch.no_grad():
        idx, rank, radius = s.layer._forward_hip_checked(s.feats, s.coors, s.edges, s.mask, s.adj, None,
                                                         drop_seed=None if drop is None else drop[1])[3:6]
    l64 = copy.deepcopy(s.layer).double()
    f, x, e = _leaves(s, torch.float64)
    node, co = A.layer_given_neighbors(l64, f, x, e, s.mask, None if idx is None else idx.long(), None if rank is None else rank.double(),
                                       radius, drop=drop)
    wrt = [t for t in (f, x, e) if t is not None] + list(l64.parameters())
    grads = torch.autograd.grad([node, co], wrt, [c.rn.double(), c.rc.double()], allow_unused=True)
    return node.detach(), co.detach(), grads


def _compare(c, got, ref, what, real_rows_only=False, structural_zero=()):
    """The bars of the module docstring + what must hold exactly: finite everywhere, padded rows of d/d feats and d/d coors 0.0, padded
    rows of coors_out the input bits.  Returns {gradient name: error / scale}.  structural_zero: names whose reference gradient is zero
    by the form of the loss (an output with a zero cotangent): there the reference must be exactly zero and the result None or exactly
    zero; every other name keeps the scale > 0 condition."""
    node, co, grads = got
    rnode, rco, rgrads = ref
    f64 = c.path == "double"
    tol_f, tol_g = (1e-9, 1e-8) if f64 else (ATOL, 1e-4)
    pad = ~c.mask
    assert bool(torch.isfinite(node).all()) and bool(torch.isfinite(co).all()), what
    rows = c.mask if real_rows_only else torch.ones_like(c.mask)
    err_n = float((node.double() - rnode)[rows].abs().max())
    err_c = float((co.double() - rco)[rows].abs().max())
    assert torch.equal(co[pad], c.coors[pad]), (what, "padded nodes moved")
    names = _names(c)
    assert len(grads) == len(rgrads) == len(names)
    worst = {}
    for nm, g, r in zip(names, grads, rgrads):
        if nm in structural_zero:
            assert r is None or not bool(r.any()), (what, nm, "the reference gradient is not structurally zero")
            assert g is None or not bool(g.any()), (what, nm, "a gradient where the loss cannot reach")
            continue
        assert (g is None) == (r is None), (what, nm)
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), (what, nm, "non-finite gradient")
        scale = float(r.abs().max())
        assert scale > 0, (what, nm, "the reference gradient vanishes: a vacuous case")
        worst[nm] = float((g.double() - r).abs().max()) / scale
    if os.environ.get("EGNN_TEST_VERBOSE"):
        print(f"MASKPAT {what} fwd={max(err_n, err_c):.2e} " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()), flush=True)
    assert err_n <= tol_f and err_c <= tol_f, (what, err_n, err_c)
    bad = {k: v for k, v in worst.items() if not v <= tol_g}
    assert not bad, (what, bad)
    if bool(pad.any()):
        assert float(grads[0][pad].abs().max()) == 0.0 and float(grads[1][pad].abs().max()) == 0.0, (what, "a padded row received a gradient")
    return worst


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (2 ** 30)


# ------------------------------------------------------------------------------------------------ 3a. every pattern x every path
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("row", list(ROWS))
def test_layer_gradients_on_every_pattern_and_path(row, pattern):
    """Each row of the table on each mask pattern, whole and in chunks of two graphs (chunks start at graph 2; the empty graph of
    `one_graph_empty` sits inside a chunk with a real one), against one float64 reference."""
    c = _build(row, pattern, _seed(row, pattern))
    ref = _float64(c)
    for chunk in (0, 2):
        _compare(c, _hip(c, chunk), ref, f"{row}/{pattern}/chunk{chunk}")


# ------------------------------------------------------------------------------------------------ 3b. what sits in padded rows
FILLS = ("randn", "zeros", "randn_1e3")


def _filled(c, fill):
    """The same case with other contents in the padded rows of feats and coors; real rows keep their bits."""
    d = copy.copy(c)
    if fill == "randn":
        return d
    g = torch.Generator().manual_seed(c.seed + 7)
    pad = ~c.mask[..., None]
    for name in ("feats", "coors"):
        t = getattr(c, name)
        other = torch.zeros_like(t) if fill == "zeros" else 1e3 * torch.randn(t.shape, generator=g).to(t)
        setattr(d, name, torch.where(pad, other, t))
    return d


PADDED_ROWS_1E3_ON_SPLIT_FP16 = (
    "KNOWN GAP: padded rows three orders of magnitude above the real ones, on the split-fp16 (native) paths.  The masks keep them out "
    "of every real row's result, but not out of the RANGE of the kernels: edge_mlp's hidden activation of a pair with a padded end is "
    "computed (then multiplied by gU = 0), and with padded features of 1e3 its SiLU leaves the fp16 x 2^6 range in which "
    "egnn_edge_bwd_pass_f32 carries it for d/d W_2 -- 0 x inf -- so the backward is answered by the plain-fp32 ATen recompute (correct, "
    "several times slower, one RuntimeWarning) instead of the native kernels this test pins; and a chunk's operand scales (absmax over "
    "all rows) cost the real rows ten bits of their split.  Keeping padded rows out of the projection table and of the operand scales "
    "touches the forward GEMMs' scale logic as well: a design change of its own.  Measured figures: DESIGN.md section 10, masks.")
_FILL_CASES = [pytest.param(row, pattern, fill, id=f"{row}-{pattern}-{fill}",
                            marks=[pytest.mark.xfail(strict=True, reason=PADDED_ROWS_1E3_ON_SPLIT_FP16)]
                            if (fill == "randn_1e3" and ROWS[row][3] == "native") else [])
               for row in ("pw_k8", "two_tiles_flags", "dense", "exact_cdim9") for pattern in ("scattered", "leading_padding")
               for fill in FILLS]


@pytest.mark.parametrize("row,pattern,fill", _FILL_CASES)
def test_contents_of_padded_rows_do_not_matter(row, pattern, fill):
    """randn (the baseline above), zeros (pad_sequence: coincident padded nodes at the origin with zero features) and 1e3 x randn (in
    the split-fp16 range, three orders of magnitude above the real rows) in the padded rows: with a zero cotangent there, nothing a
    real row or a parameter receives depends on them -- asserted on the float64 side (each fill's own float64 gradients against the
    baseline's) and, at the bars of the file, for the HIP result against the ONE float64 reference of the baseline.  Catches padded rows
    leaking through the masks, or through an operand scale that a chunk's absmax takes over padded rows too."""
    base = _build(row, pattern, _seed(row, pattern))                 # (the very case of the test above)
    ref = _float64(base)
    c = _filled(base, fill)
    assert torch.equal(c.feats[c.mask], base.feats[base.mask]) and torch.equal(c.coors[c.mask], base.coors[base.mask])
    if fill != "randn":
        own = _float64(c)
        real = c.mask
        for nm, a, r in zip(_names(c), own[2], ref[2]):
            a, r = (a[real], r[real]) if nm in ("feats", "coors") else (a, r)
            assert float((a - r).abs().max()) <= 1e-11 * float(r.abs().max()), (nm, "the float64 reference depends on padded rows")
        assert float((own[0] - ref[0])[real].abs().max()) <= 1e-11 and float((own[1] - ref[1])[real].abs().max()) <= 1e-11
    for chunk in (0, 2):
        _compare(c, _hip(c, chunk), ref, f"{row}/{pattern}/{fill}/chunk{chunk}", real_rows_only=True)


# ------------------------------------------------------------------------------------------------ 3c. dropout, second order, networks
@pytest.mark.parametrize("pattern", ["scattered", "one_graph_empty"])
@pytest.mark.parametrize("row", ["pw_k8", "m32_blocks"])
def test_training_mode_dropout_on_mask_patterns(row, pattern):
    """dropout = 0.2 in training mode, native backward, chunks of two graphs, against the restatement with the masks of that very
    forward: the hash masks' rows are global edge and node ids, which padding in front or in between shifts nowhere."""
    from egnn_pytorch_amd import _dropout, autograd as A
    c = _build(row, pattern, _seed(row, pattern, "drop"), dropout=0.2)
    c.layer.train()
    assert A._dropout_native_ok(c.layer)
    torch.manual_seed(77)
    seed = _dropout.draw_seed()                                      # (what the forward below draws from torch's CPU generator)
    got = _hip(c, 2, torch_seed=77)
    ref = _float64(c, drop=(0.2, seed))
    _compare(c, got, ref, f"dropout/{row}/{pattern}")


@pytest.mark.parametrize("pattern", ["scattered", "one_graph_empty"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float64, 1e-7)], ids=["fp32", "double"])
def test_force_matching_on_mask_patterns(dtype, tol, pattern):
    """create_graph=True (tests/test_second_order.py's force-matching loss) through one layer -- dim 8, k 4, CoorsNorm, n 12 -- against
    the same quantity on the float64 restatement over the HIP forward's neighbour list; the bars of tests/test_gpu_second_order.py (1e-4
    of scale for an fp32 module, 1e-7 in float64 with CoorsNorm)."""
    from egnn_pytorch_amd import EGNN, autograd as A
    from tests.test_second_order import force_matching_grads
    n, dim, k = 12, 8, 4
    seed = _seed("second", pattern)
    torch.manual_seed(seed)
    layer = EGNN(dim=dim, num_nearest_neighbors=k, norm_coors=True)
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(60.0)
    layer = layer.to(dtype).cuda()
    mask = torch.from_numpy(mask_pattern(pattern, B, n, k, np.random.default_rng(seed))).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    feats, coors = torch.randn(B, n, dim, generator=g).to(dtype).cuda(), torch.randn(B, n, 3, generator=g).to(dtype).cuda()

    class Real(torch.nn.Module):                                     # the loss over real nodes: both outputs zeroed on padded rows
        def __init__(self, fn):
            super().__init__()
            self.fn = fn

        def __call__(self):
            node, co = self.fn()
            return node * mask[..., None], co * mask[..., None]

    f, x = feats.clone().requires_grad_(True), coors.clone().requires_grad_(True)
    got = force_matching_grads(layer, Real(lambda: layer(f, x, None, mask)), x, [x, f] + list(layer.parameters()))
    with torch.no_grad():
        idx, rank, radius = layer._forward_hip_checked(feats, coors, None, mask, None, None)[3:6]
    l64 = copy.deepcopy(layer).double()
    f2, x2 = feats.double().requires_grad_(True), coors.double().requires_grad_(True)
    call = lambda: A.layer_given_neighbors(l64, f2, x2, None, mask, idx.long(), rank.double(), radius, edge_hidden=True)     # noqa: E731
    want = force_matching_grads(l64, Real(call), x2, [x2, f2] + list(l64.parameters()))
    names = ["coors", "feats"] + [nm for nm, _ in layer.named_parameters()]
    for nm, a, r in zip(names, got, want):
        assert (a is None) == (r is None), nm
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), nm
        scale = float(r.abs().max())
        assert scale > 0, nm
        err = float((a.double() - r).abs().max())
        if os.environ.get("EGNN_TEST_VERBOSE"):
            print(f"MASKPAT second/{pattern}/{dtype} {nm}={err / scale:.1e}", flush=True)
        assert err <= tol * scale, (nm, err, scale)


_NET = dict(depth=2, dim=16, num_nearest_neighbors=6, num_tokens=11, num_adj_degrees=2, adj_dim=4, num_edge_tokens=5, edge_dim=2,
            global_linear_attn_every=1, global_linear_attn_heads=2, global_linear_attn_dim_head=8, num_global_tokens=2)


def _net_step(fn, params, coors, wn, wc):
    x = coors.clone().requires_grad_(True)
    h, co = fn(x)
    grads = torch.autograd.grad([h, co], [x] + params, [wn.to(h.dtype), wc.to(h.dtype)], allow_unused=True)
    return h.detach(), co.detach(), grads


@pytest.mark.parametrize("pattern", ["scattered", "one_graph_empty"])
def test_network_training_on_mask_patterns(pattern):
    """EGNN_Network -- tokens, adjacency degrees and edge tokens on the look-up-table training path, a global attention block in front of
    every layer -- under a scattered mask and with an empty graph: the fp32 module against its .double() copy (1e-4 of each gradient's
    scale), the .double() module against the materialised float64 recipe (1e-8)."""
    from tests.test_gpu_edge_lookup_training import _chain_adj, _materialised
    from tests.test_gpu_second_order import _net_case
    n = 40
    seed = _seed("net", pattern)
    net = _net_case(_NET, n, seed=seed % 1000).cuda()
    net64 = copy.deepcopy(net).double()
    mask = torch.from_numpy(mask_pattern(pattern, B, n, 6, np.random.default_rng(seed))).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randint(0, 11, (B, n), generator=g).cuda()
    etok = torch.randint(0, 5, (B, n, n), generator=g).cuda()
    coors = torch.randn(B, n, 3, generator=g).cuda()
    adj = _chain_adj(n, seed % 1000)
    wn = torch.randn(B, n, 16, generator=g).cuda() * mask[..., None]
    wc = torch.randn(B, n, 3, generator=g).cuda() * mask[..., None]
    names = ["coors"] + [nm for nm, _ in net.named_parameters()]
    p32, p64 = list(net.parameters()), list(net64.parameters())
    got = _net_step(lambda x: net(tokens, x, adj_mat=adj, edges=etok, mask=mask), p32, coors, wn, wc)
    mid = _net_step(lambda x: net64(tokens, x, adj_mat=adj, edges=etok, mask=mask), p64, coors.double(), wn, wc)
    want = _net_step(lambda x: _materialised(net64, tokens, x, adj, etok, None, mask), p64, coors.double(), wn, wc)
    real = mask
    for what, a, r, tol_f, tol_g in (("fp32 / double", got, mid, ATOL, 1e-4), ("double / materialised", mid, want, 1e-9, 1e-8)):
        assert float((a[0].double() - r[0])[real].abs().max()) <= tol_f and float((a[1].double() - r[1])[real].abs().max()) <= tol_f, what
        assert torch.equal(a[1][~real], coors.to(a[1].dtype)[~real]), (what, "padded nodes moved")
        for nm, ga, gr in zip(names, a[2], r[2]):
            assert (ga is None) == (gr is None), (what, nm)
            if ga is None:
                continue
            assert bool(torch.isfinite(ga).all()), (what, nm)
            scale = float(gr.abs().max())
            assert scale > 0, (what, nm)
            err = float((ga.double() - gr).abs().max()) / scale
            if os.environ.get("EGNN_TEST_VERBOSE"):
                print(f"MASKPAT net/{pattern}/{what} {nm}={err:.1e}", flush=True)
            assert err <= tol_g, (what, nm, err)
        assert float(a[2][0][~real].abs().max()) == 0.0, (what, "a padded node's coordinates received a gradient")


# ------------------------------------------------------------------------------------------------ 3d. a short seeded walk
@pytest.mark.parametrize("i", range(48))
def test_seeded_walk_over_rows_patterns_sizes(i):
    """The gradient counterpart of the forward walk's permuted masks: each case draws a row of the table, a pattern, n within +-8 of
    the row's (not below K + 1), whether per-pair edge features are present, and the chunking; checked as in the first test.  A
    failing case prints its draw: `_build(row, pattern, seed, n=n, with_edges=edges)` and `_hip(c, chunk)` replay it alone."""
    rng = np.random.default_rng(1000 + i)
    row = list(ROWS)[int(rng.integers(len(ROWS)))]
    pattern = PATTERNS[int(rng.integers(len(PATTERNS)))]
    kw, n0 = ROWS[row][:2]
    k = _neighbour_count(kw)
    n = max(n0 + int(rng.integers(-8, 9)), (k or 4) + 1)
    edges = bool(rng.integers(2))
    chunk = (0, 1, 2, 3)[int(rng.integers(4))]
    seed = 5000 + i
    draw = f"walk{i}: row={row} pattern={pattern} n={n} with_edges={edges} chunk={chunk} seed={seed}"
    try:
        c = _build(row, pattern, seed, n=n, with_edges=edges)
        _compare(c, _hip(c, chunk), _float64(c), draw)
    except BaseException:
        print(draw)
        raise
