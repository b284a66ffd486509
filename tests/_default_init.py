"""The module's own initialisation -- every nn.Linear weight N(0, init_eps = 1e-3), biases and norms as torch leaves them -- on every
backward path.  Every other gradient test moves away from that state on purpose (parameters x 40, xavier): with 1e-3 weights the node
output is feats + ~0.1 and an absolute bar passes whatever the edge path does.  Every training run starts there, though, and the
operands the split-f16 kernels were sized for (W4, q = W4 SiLU'(hid), dz, SiLU(z)) are two to three orders smaller.

Importable without a GPU.  The cases are the rows of tests/test_gpu_mask_patterns_training.py::ROWS on the `scattered` mask, built by
that file's own `_build` with a layer factory that does nothing to the parameters after `EGNN(**kw)` under the case's seed, times three
cotangent forms -- randn on both outputs, coordinates only, features only; all zero on padded rows.  The rows with a clamp run WITHOUT
`_centre_clamp`: at this state the coordinate weight of every pair is the same fp32 number (coors_mlp's last bias, about -0.1; the
pairs differ by ~1e-9, below its ulp), so no clamp value separates some pairs from others, let alone by a margin -- the clamp of 1.5 / 2.0
is off for every pair, as it is in a user's first steps, and the kernels' clamp code runs on its pass-through side.  `prepare(row, form)` builds a case on the CPU (neighbour selection of
tests/_cpu_stub.py + the restated layer as the forward), takes its float64 reference and asserts the case conditions on the reference
alone; tests/test_default_init_table.py runs every `prepare`, tests/test_gpu_default_init.py runs the kernels.

Bars: every gradient within 1e-4 of ITS OWN scale (max |reference|), 1e-8 for the float64 row -- the project's bar, no absolute term.
Adam normalises each tensor, and at this state the tensors' scales span ten orders of magnitude."""
import contextlib
import copy
import functools
from types import SimpleNamespace

import torch

from tests import test_gpu_mask_patterns_training as M
from tests._cpu_stub import _select

PATTERN = "scattered"
FORMS = ("both", "coors_only", "feats_only")
CASES = [(row, form) for row in M.ROWS for form in FORMS]
BAR, BAR64 = 1e-4, 1e-8
SENSITIVITY = 5e-4                       # 5 x the bar: what replacing one neighbour per node must move (condition c)
STD_RANGE = (0.7e-3, 1.3e-3)             # init_eps = 1e-3, by the smallest weight's sample count
DENSE_ROWS = tuple(r for r, v in M.ROWS.items() if M._neighbour_count(v[0]) is None)


def default_layer(kw, seed, path, state=None, device="cuda"):
    """`_make_layer` without its rescaling: EGNN(**kw) under the seed, as a user gets it"""
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(seed % (2 ** 31))
    layer = EGNN(**kw)
    if state is not None:
        layer.load_state_dict(state)
    if path == "double":
        layer = layer.double()
    return layer.to(device)


# A row whose draw misses condition (c) gets another draw, never an exemption: the first salt of its seed that meets it.  What misses is
# always d/d edge_mlp.3.bias (once edge_mlp.0.bias) under the form `both`: the feature branch's share of that sum does not depend on the
# selection (`insensitive_by_form`) and, draw by draw, leaves the coordinate branch's share between 1e-5 and 1e-2 of the total.
SALT = {"two_tiles_flags": 1, "k48_rounds": 1, "cdim5": 6, "sparse_adj": 2}


def case_seed(row):
    return M._seed("default_init", row, SALT.get(row, 0))


def insensitive_by_form(c):
    """Exempt from condition (c), with (b) and the bar still holding: under the features-only form d/d of edge_mlp's two biases.  There
    gU = g_m SiLU'(u) with u = b2 + O(1e-3) on every edge, so d/d b2 = sum gU (and d/d b1 behind the same W2) is the same sum over
    whichever neighbours are selected -- measured 1e-6 ... 5e-4 of scale on every row.  The form `both` of the same row holds the two
    tensors at (c): there the coordinate branch reaches them through rel, which does depend on the selection."""
    return ("edge_mlp.0.bias", "edge_mlp.3.bias") if c.form == "feats_only" else ()


def build(row, form, device="cuda"):
    """One case at the default initialisation; the three forms of a row share layer, inputs and mask"""
    c = M._build(row, PATTERN, case_seed(row), make_layer=default_layer, device=device, centre_clamp=False)
    c.form = form
    if form == "coors_only":
        c.rn = torch.zeros_like(c.rn)
    elif form == "feats_only":
        c.rc = torch.zeros_like(c.rc)
    else:
        assert form == "both"
    return c


def structural_zeros(c):
    """parameters no gradient can reach under the case's form: the node branch behind a zero feature cotangent, the coordinate branch
    behind a zero coordinate cotangent"""
    prefixes = {"both": (), "coors_only": ("node_mlp.", "node_norm."), "feats_only": ("coors_mlp.", "coors_norm.")}[c.form]
    return tuple(nm for nm in M._names(c) if nm.startswith(prefixes)) if prefixes else ()


def bar(c):
    return BAR64 if c.path == "double" else BAR


def edge_hidden_out(layer, feats, coors, edges, idx):
    """u (B,N,K,m): the output of edge_mlp's second Linear, restated"""
    from egnn_pytorch_amd import autograd as A
    b, n, dim = feats.shape
    rel, scal = A.edge_scalars(layer, coors, edges, idx)
    if idx is None:
        feats_j = feats[:, None, :, :].expand(b, n, n, dim)
    else:
        feats_j = feats[torch.arange(b, device=feats.device)[:, None, None], idx]
    x = torch.cat((feats[:, :, None, :].expand_as(feats_j), feats_j, scal), dim=-1)
    for mod in list(layer.edge_mlp)[:4]:
        x = mod(x)
    return x, rel


def _host_forward(self, feats, coors, edges, mask, adj_mat, order_hint, want_u=False, drop_seed=None):
    """EGNN._forward_hip_checked's tuple on host tensors: the selection of the reference as tensor ops, the layer restated"""
    from egnn_pytorch_amd import autograd as A
    assert drop_seed is None and not feats.is_cuda
    idx, rank, radius = _select(self, coors, mask, adj_mat)
    with torch.no_grad():
        u, rel = edge_hidden_out(self, feats, coors, edges, idx)
        node, co = A.layer_tail(self, feats, coors, u, rel, mask, idx, rank, radius)
    return node, co, None, None if idx is None else idx.int(), rank, radius, u.reshape(-1, u.shape[-1]) if want_u else None, None


@contextlib.contextmanager
def host_forward():
    """the builders of tests/test_gpu_mask_patterns_training.py read the neighbour list (and, for the clamp, u) from the HIP forward: on
    the host they get `_host_forward` for the time of a `prepare`"""
    from egnn_pytorch_amd import EGNN
    saved = EGNN._forward_hip_checked
    EGNN._forward_hip_checked = _host_forward
    try:
        yield
    finally:
        EGNN._forward_hip_checked = saved


def restated(c, dtype, idx, rank, radius, rn=None, rc=None):
    """(node, coors_out, gradients) of autograd.layer_given_neighbors on a copy of the layer in `dtype` over a given neighbour list"""
    from egnn_pytorch_amd import autograd as A
    layer = copy.deepcopy(c.layer).to(dtype)
    f, x, e = M._leaves(c, dtype)
    node, co = A.layer_given_neighbors(layer, f, x, e, c.mask, None if idx is None else idx.long(), None if rank is None else rank.to(dtype), radius)
    wrt = [t for t in (f, x, e) if t is not None] + list(layer.parameters())
    rn, rc = c.rn if rn is None else rn, c.rc if rc is None else rc
    grads = torch.autograd.grad([node, co], wrt, [rn.to(dtype), rc.to(dtype)], allow_unused=True)
    return node.detach(), co.detach(), grads


def neighbours(c):
    with torch.no_grad():
        return c.layer._forward_hip_checked(c.feats, c.coors, c.edges, c.mask, c.adj, None)[3:6]


def replace_last_live_neighbour(c, idx, rank, radius):
    """The neighbour list with one slot per real node pointing at another real node: the last slot whose pair passes the masks (node
    masks, radius, adjacency -- a slot that fails them carries nothing, and replacing it would test nothing), redirected to the next
    real node of the graph that is neither the node itself nor in its list.  Ranks stay: the pair mask does not move."""
    from egnn_pytorch_amd import autograd as A
    b, n, k = idx.shape
    pm = A._pair_mask(c.mask, idx.long(), rank, radius)
    out = idx.clone()
    moved = 0
    for g in range(b):
        real = c.mask[g].nonzero().flatten().tolist()
        for i in real:
            live = pm[g, i].nonzero().flatten().tolist()
            taken = set(idx[g, i].tolist()) | {i}
            free = [j for j in real if j not in taken]
            if not live or not free:
                continue
            out[g, i, live[-1]] = free[(i + 1) % len(free)]
            moved += 1
    return out, moved


@functools.lru_cache(maxsize=None)
def prepare(row, form):
    """The case on the CPU, its float64 reference and conditions (a)-(c) of the module docstring of tests/test_default_init_table.py"""
    with host_forward():
        c = build(row, form, device="cpu")
        idx, rank, radius = neighbours(c)
        ref = M._float64(c)
        # (a) the module's own draw
        again = default_layer(c.kw, case_seed(row), c.path, device="cpu")
        moved = [nm for (nm, p), (_, q) in zip(c.layer.named_parameters(), again.named_parameters()) if not torch.equal(p, q)]
        assert moved == [], (row, moved)
        for nm, mod in c.layer.named_modules():
            if isinstance(mod, torch.nn.Linear):
                std = float(mod.weight.detach().double().std())
                assert STD_RANGE[0] <= std <= STD_RANGE[1], (row, nm, std)
        # (b) nothing vanishes that the form of the loss reaches
        zeros = structural_zeros(c)
        names = M._names(c)
        scales = {}
        for nm, r in zip(names, ref[2]):
            if nm in zeros:
                assert r is None or not bool(r.any()), (row, form, nm)
                continue
            assert r is not None and bool(torch.isfinite(r).all()), (row, form, nm)
            scales[nm] = float(r.abs().max())
            assert scales[nm] > 0, (row, form, nm, "the reference gradient vanishes")
        # (c) the quantities that tell the edge path: one neighbour per real node replaced
        sens = {}
        if row not in DENSE_ROWS:
            idx2, count = replace_last_live_neighbour(c, idx, rank, radius)
            assert count >= int(c.mask.sum()) // 2, (row, count)
            other = restated(c, torch.float64, idx2, rank, radius)
            if c.kw.get("update_coors", True):
                upd = ref[1] - c.coors.double()
                sens["coors_out - coors"] = float((other[1] - ref[1]).abs().max()) / float(upd.abs().max())
            for nm, r, o in zip(names, ref[2], other[2]):
                if nm in zeros or nm in insensitive_by_form(c) or not nm.startswith(("edge_mlp.", "coors_mlp.")):
                    continue
                if nm.startswith("coors_mlp.") and not c.kw.get("update_coors", True):
                    continue
                sens[nm] = float((o - r).abs().max()) / scales[nm]
            low = {k: v for k, v in sens.items() if not v >= SENSITIVITY}
            assert not low, (row, form, "replacing a neighbour moves these by less than 5 x the bar", low)
    return SimpleNamespace(case=c, ref=ref, idx=idx, rank=rank, radius=radius, scales=scales, sens=sens, zeros=zeros)
