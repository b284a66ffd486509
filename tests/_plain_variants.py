"""One test case per template instantiation of the plain fp32 / float64 edge kernels (csrc/edge_exact.hip, csrc/edge_exact_bwd.hip,
csrc/edge_hidden.hip) -- the table behind tests/test_gpu_plain_variants.py, importable without a GPU.

The three launchers dispatch to 48 kernels:
    fwd    egnn_edge_exact_*            edge_exact_kernel<T, 16 / 32 / 64>, edge_exact_wide_kernel<T> (m_dim > 64), edge_exact_pool_kernel<T>
    silu   egnn_drop_silu_*             drop_silu_kernel<T>
    bwd    egnn_edge_exact_bwd_*        edge_exact_bwd_kernel<T, 16 / 32 / 64 / 0>
    sums   egnn_edge_exact_node_sums_*  edge_exact_node_sums_kernel<T>
    tail   egnn_edge_tail_exact_bwd_*   edge_tail_exact_bwd_kernel<T, 16 / 32 / 64>          (m_dim > 64 refused)
    hfwd   egnn_edge_hidden_fwd_*       edge_hidden_fwd_kernel<float, 16 / 32 / 64 / 0>, <double, 16 / 32 / 0>
    hbwd   egnn_edge_hidden_bwd_*       edge_hidden_bwd_kernel<T, 16 / 32 / 64 / 0>
    hbwd2  egnn_edge_hidden_bwd2_*      edge_hidden_bwd2_kernel<float, 16 / 32 / 0>, <double, 16 / 0>
`dispatch()` restates the launchers (thresholds, LDS bytes, the 64 KiB opt-in, the 160 KiB refusal, the 32-bit dropout rows), `CELLS`
holds one direct call per instantiation (`MAIN`) and the cells beside the grid, `prepare()` builds a cell's operands on the host (rounded
to the cell's type, held in float64), `reference()` evaluates the float64 specification of the entry on them -- written from the
reference's formulas (egnn_pytorch.py:262-333), from `autograd.tail_edge_backward`, `autograd.edge_hidden_*_spec` and torch autograd of
the first Linear -- and `reference(cid, "f")` the same specification in torch fp32, whose error is what the fp32 bars are made of.
A NEW INSTANTIATION NEEDS A NEW CELL: tests/test_plain_variants_table.py compares the table with what the compiler instantiated.

The cells beside the grid (`group`):
    mstep   m_dim = 17, 33, 65: the first head behind every threshold (MAIN sits at 16, 32, 64: every register channel in use)
    lds     the dynamic-LDS opt-in (hipFuncSetAttribute) from both sides, per entry and type
    smax    the largest S an entry admits; smax1: that S + 1, refused with EGNN_E_UNSUPPORTED
    four    fourier = 0, 2, 31          cdim   coordinate dimension 3, 2, 5, 8, 9, 11
    eshape  E = 256 exactly, E = 280 (a second workgroup of 24 threads), E = 40 (one partial wave); m_dim 13 / 7: pad channels
    stride  ldp = 2 hq > H with P_j at offset hq, ldws = Din > S (the tables `_forward_exact` really passes)
    opt     the forward's and the tail's options, one per cell
    drop    dropout (p = 0.25) in one call at drop_eid0 = 0;  split: the same as one call per graph, drop_eid0 = 0 and N K
    refuse  m_dim = 65 on the tail, K != N without idx, drop_inv_keep < 1"""
import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace

# ------------------------------------------------------------------------------------------------ the launchers, restated
E_NULLPTR, E_SHAPE, E_UNSUPPORTED = -1, -2, -3                   # include/egnn_hip.h:34-36 (the codes `_abi.check` reports)
THREADS = 256                                                    # EX_THREADS, XB_THREADS, EH_THREADS
LDS_OPT_IN, LDS_MAX = 64 * 1024, 160 * 1024                      # `run` of the three launchers; their refusal
ESZ = dict(f=4, d=8)
LDS_COLS = dict(fwd=1, bwd=2, hfwd=1, hbwd=2, hbwd2=3)           # columns of S x 256 values: s [, sbar], d/d s
ENTRIES = ("fwd", "silu", "bwd", "sums", "tail", "hfwd", "hbwd", "hbwd2")
EDGE_ENTRIES = ("fwd", "bwd", "tail", "hfwd", "hbwd", "hbwd2")
DROP_ENTRIES = ("fwd", "silu", "bwd", "tail", "hfwd", "hbwd", "hbwd2")
DROP_P = 0.25

Inst = namedtuple("Inst", "kernel T MB")                         # MB = -1: the kernel has no channel parameter


def inst_name(i):
    return f"{i.kernel}<{i.T}{',' + str(i.MB) if i.MB >= 0 else ''}>"


def lds_bytes(entry, t, s):
    return LDS_COLS[entry] * s * THREADS * ESZ[t] if entry in LDS_COLS else 0


def opts_in(entry, t, s):
    """the launch goes through hipFuncSetAttribute(MaxDynamicSharedMemorySize)"""
    return lds_bytes(entry, t, s) > LDS_OPT_IN


def max_s(entry, t):
    return LDS_MAX // (LDS_COLS[entry] * THREADS * ESZ[t])


def _drop_refused(drop, e):
    """drop = None or (inv_keep, first row): the launchers' `drop_thr && (!(inv_keep >= 1) || eid0 < 0 || eid0 + E > 2^32 - 1)`"""
    return drop is not None and (not drop[0] >= 1.0 or drop[1] < 0 or drop[1] + e > 0xFFFFFFFF)


def _by_m(kernel, t, m, steps, last):
    for mb in steps:
        if m <= mb:
            return Inst(kernel, t, mb)
    return last


def dispatch(entry, t, m=16, s=1, fourier=0, e=80, has_idx=True, k_is_n=False, drop=None):
    """The kernels a call launches (a tuple: the forward launches two), or the launcher's refusal code -- the checks in the launcher's
    own order."""
    dense_refused = not has_idx and not k_is_n
    if entry == "fwd":                                           # edge_exact_launch, csrc/edge_exact.hip:325-364
        if m < 1 or m > 1024 or fourier < 0 or fourier > 31:
            return E_UNSUPPORTED
        if lds_bytes(entry, t, s) > LDS_MAX:
            return E_UNSUPPORTED
        if dense_refused or _drop_refused(drop, e):
            return E_SHAPE
        main = _by_m("edge_exact_kernel", t, m, (16, 32, 64), Inst("edge_exact_wide_kernel", t, -1))
        return main, Inst("edge_exact_pool_kernel", t, -1)
    if entry == "silu":                                          # drop_silu_launch, :381-392 (e = rows)
        if drop is not None and (not drop[0] >= 1.0):
            return E_SHAPE
        if drop is not None and (drop[1] < 0 or drop[1] + e > 0xFFFFFFFF):
            return E_SHAPE
        return (Inst("drop_silu_kernel", t, -1),)
    if entry == "bwd":                                           # edge_exact_bwd_launch, csrc/edge_exact_bwd.hip:152-191
        if m < 1 or m > 1024 or fourier < 0 or fourier > 31:
            return E_UNSUPPORTED
        if dense_refused:
            return E_SHAPE
        if lds_bytes(entry, t, s) > LDS_MAX:
            return E_UNSUPPORTED
        if _drop_refused(drop, e):
            return E_SHAPE
        return (_by_m("edge_exact_bwd_kernel", t, m, (16, 32, 64), Inst("edge_exact_bwd_kernel", t, 0)),)
    if entry == "sums":                                          # node_sums_launch, :193-206
        return (Inst("edge_exact_node_sums_kernel", t, -1),)
    if entry == "tail":                                          # edge_tail_exact_launch, :377-409
        if m < 1 or m > 64:
            return E_UNSUPPORTED
        if dense_refused or _drop_refused(drop, e):
            return E_SHAPE
        return (_by_m("edge_tail_exact_bwd_kernel", t, m, (16, 32), Inst("edge_tail_exact_bwd_kernel", t, 64)),)
    assert entry in ("hfwd", "hbwd", "hbwd2")                    # edge_hidden_launch, csrc/edge_hidden.hip:251-307
    if s <= 0 or m <= 0 or dense_refused:
        return E_SHAPE
    if lds_bytes(entry, t, s) > LDS_MAX:
        return E_UNSUPPORTED
    if _drop_refused(drop, e):
        return E_SHAPE
    f64 = t == "d"
    if entry == "hfwd":
        return (_by_m("edge_hidden_fwd_kernel", t, m, (16, 32) if f64 else (16, 32, 64), Inst("edge_hidden_fwd_kernel", t, 0)),)
    if entry == "hbwd":
        return (_by_m("edge_hidden_bwd_kernel", t, m, (16, 32, 64), Inst("edge_hidden_bwd_kernel", t, 0)),)
    return (_by_m("edge_hidden_bwd2_kernel", t, m, (16,) if f64 else (16, 32), Inst("edge_hidden_bwd2_kernel", t, 0)),)


def grid():
    """every instantiation the launchers can reach"""
    out = set()
    for entry in ENTRIES:
        for t in "fd":
            for m in (1, 16, 17, 32, 33, 64, 65, 1024):
                got = dispatch(entry, t, m)
                if not isinstance(got, int):
                    out.update(got)
    return out


# ------------------------------------------------------------------------------------------------ the table
Cell = namedtuple("Cell", "id entry t inst group p expect")
_DEFAULTS = dict(b=2, n=10, k=4, m=16, H=24, fourier=0, edge_dim=0, cdim=3, dense=False, by_k=False, strided=False, opts=(), drop=None,
                 pin=0, bad_inv=False, no_idx=False, rows=37, cols=13)
FWD_OPTS = ("dense", "dense_by_k", "mask", "mask_rank", "mean", "mean_mask0", "gate", "scale", "clamp", "no_w3", "no_mi", "u_out")
TAIL_OPTS = ("pair_mask", "gate", "norm", "clamp", "no_w3", "no_gmsum")
CLAMP = 0.125
EPS = 1e-8


def s_of(p):
    return 2 * p["fourier"] + 1 + p["edge_dim"]


def e_of(p):
    return p["b"] * p["n"] * p["k"]


def expected(entry, t, p):
    """`dispatch` of a cell's own arguments"""
    k_is_n = p["k"] == p["n"]
    has_idx = not (p["dense"] or p["no_idx"])
    drop = None
    if p["drop"] is not None:
        drop = (0.5 if p["bad_inv"] else 4.0 / 3.0, 0)
    if entry == "silu":
        return dispatch(entry, t, e=p["rows"], drop=drop)
    return dispatch(entry, t, p["m"], s_of(p), p["fourier"], e_of(p), has_idx, k_is_n, drop)


def _build_cells():
    cells = []

    def add(entry, t, group, tag, **kw):
        p = dict(_DEFAULTS)
        p.update(kw)
        p["opts"] = tuple(p["opts"])
        if p["dense"]:
            p["k"] = p["n"]
        got = expected(entry, t, p)
        if isinstance(got, int):
            inst, expect = None, got
            cid = f"{entry}_{t}_{group}_{tag}_refused{-got}"
        else:
            inst, expect = got[p["pin"]], None
            cid = f"{inst_name(inst)}_{entry}_{group}_{tag}"
        cells.append(Cell(cid, entry, t, inst, group, p, expect))

    # ---- MAIN: one direct call per instantiation, at the widest head the instantiation takes (every register channel in use)
    for t in "fd":
        for q, m in enumerate((16, 32, 64, 70)):
            add("fwd", t, "main", f"m{m}", m=m, fourier=(0, 2, 0, 1)[q], edge_dim=(0, 3, 1, 2)[q], opts=("u_out", "gate") if q % 2 else ("u_out",))
            add("bwd", t, "main", f"m{m}", m=m if m != 70 else 80, fourier=(0, 2, 0, 1)[q], edge_dim=(0, 3, 1, 2)[q])
            add("hbwd", t, "main", f"m{m}", m=m, edge_dim=(0, 4, 2, 1)[q])
        add("fwd", t, "main", "pool", m=24, opts=("mean", "mask"), pin=1, edge_dim=1)
        add("silu", t, "main", "r37c13", drop="one")
        add("sums", t, "main", "h24", m=16)
        for m in (16, 32, 64):
            add("tail", t, "main", f"m{m}", m=m, opts=("gate",) if m == 32 else ())
        for m in (16, 32, 64, 70) if t == "f" else (16, 32, 40):
            add("hfwd", t, "main", f"m{m}", m=m, edge_dim=m % 5)
        for m in (16, 32, 40) if t == "f" else (16, 24):
            add("hbwd2", t, "main", f"m{m}", m=m, edge_dim=m % 3)
        # ---- the first m_dim behind every threshold: a threshold raised by one leaves this head a channel short
        for entry in EDGE_ENTRIES:
            for m in (17, 33) + ((65,) if entry != "tail" else ()):
                add(entry, t, "mstep", f"m{m}", m=m, H=12, edge_dim=0 if entry == "tail" else 1)
    # ---- the LDS opt-in from both sides, the largest S and that S + 1
    for t in "fd":
        for entry in LDS_COLS:
            lo = LDS_OPT_IN // (LDS_COLS[entry] * THREADS * ESZ[t])
            top = max_s(entry, t)
            for group, s in (("lds", lo), ("lds", lo + 1), ("smax", top), ("smax1", top + 1)):
                add(entry, t, group, f"S{s}", edge_dim=s - 1, H=8, n=6, k=3)
    # ---- fourier, coordinate dimension, E shapes
    for t in "fd":
        for entry in ("fwd", "bwd"):
            for f in (0, 2, 31):
                if 2 * f + 1 <= max_s(entry, t):
                    add(entry, t, "four", f"F{f}", fourier=f, H=12)
        for entry in ("fwd", "bwd", "tail"):
            for c in (3, 2, 5, 8, 9, 11):
                add(entry, t, "cdim", f"C{c}", cdim=c, opts=("scale",) if entry == "fwd" and c in (5, 9) else (("norm",) if entry == "tail" and c in (2, 8) else ()))
        for entry in EDGE_ENTRIES:
            for n, k in ((16, 8), (20, 7), (5, 4)):
                add(entry, t, "eshape", f"E{2 * n * k}", n=n, k=k, H=12, m=7 if entry == "tail" else 13, edge_dim=1 if entry != "tail" else 0)
        # ---- table strides
        for entry in ("fwd", "bwd"):
            add(entry, t, "stride", "H22", strided=True, H=22, fourier=1, edge_dim=2)
        # ---- options
        for o in FWD_OPTS:
            kw = dict(dense=True, n=8) if o.startswith("dense") else {}
            if o == "dense_by_k":
                kw["by_k"] = True
            add("fwd", t, "opt", o, opts=(o,), edge_dim=2 if o.startswith("dense") else 0, **kw)
        for o in TAIL_OPTS:
            add("tail", t, "opt", o, opts=(o,))
        add("tail", t, "opt", "dense", dense=True, n=8)
        # ---- dropout
        for entry in DROP_ENTRIES:
            add(entry, t, "drop", "one", drop="one", edge_dim=0 if entry == "tail" else 1)
            add(entry, t, "drop", "split", drop="split", edge_dim=0 if entry == "tail" else 1)
        # ---- refusals
        add("tail", t, "refuse", "m65", m=65)
        for entry in EDGE_ENTRIES:
            add(entry, t, "refuse", "k_ne_n", no_idx=True)
        for entry in DROP_ENTRIES:
            add(entry, t, "refuse", "inv_keep", drop="one", bad_inv=True)
    return cells


CELLS = _build_cells()
MAIN = [c for c in CELLS if c.group == "main"]
BY_ID = {c.id: c for c in CELLS}
REFUSED = [c for c in CELLS if c.expect is not None]
RUN = [c for c in CELLS if c.expect is None]


# ------------------------------------------------------------------------------------------------ a cell's operands, on the host
def _ceil4(x):
    return (x + 3) // 4 * 4


def torch_dtype(t):
    import torch
    return torch.float32 if t == "f" else torch.float64


def sqdist(rel):
    """(E, C) -> (E,): the squares summed in the kernels' order -- left to right, for 5 .. 7 coordinates s0, s4 .., s1, s2, s3 (the
    restatement of tests/test_float64_property_suite.py::test_knn_select_f64_kernel)"""
    c = rel.shape[-1]
    sq = rel * rel
    order = list(range(c)) if c not in (5, 6, 7) else [0] + list(range(4, c)) + [1, 2, 3]
    d = sq[..., order[0]].clone()
    for i in order[1:]:
        d = d + sq[..., i]
    return d


def edge_ends(idx, b, n, k):
    """(source row, neighbour row) (E,) int64 of every edge in the (B N, .) node tables; idx (E,) or None (dense: j = k)"""
    import torch
    src = torch.arange(b * n).repeat_interleave(k)
    j = torch.arange(k).repeat(b * n) if idx is None else idx.long()
    return src, src // n * n + j


@functools.lru_cache(maxsize=None)
def prepare(cid):
    """The operands of a cell from its id alone (cached: the tests share them and leave them unchanged), every floating-point tensor
    rounded to the cell's type and held in float64.  Four kinds, which is how a call per graph slices them (`graph_slice`):
        .node  (B N, ..) rows      .edge  (E, ..) rows      .glob  weights      plus .src / .dst (E,), .drop = (p, seed) or None"""
    import torch
    c = BY_ID[cid]
    p = c.p
    b, n, k, m, h, cd = p["b"], p["n"], p["k"], p["m"], p["H"], p["cdim"]
    s, e, opts = s_of(p), e_of(p), p["opts"]
    dt = torch_dtype(c.t)
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()) % (2 ** 31))
    rnd = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g, dtype=torch.float64) * scale).to(dt).double()     # noqa: E731
    d = SimpleNamespace(node={}, edge={}, glob={}, cell=c, b=b, n=n, k=k, e=e, s=s)
    d.drop = (DROP_P, 1 + zlib.crc32(cid.encode()) % 100000) if p["drop"] else None
    if c.entry == "silu":
        d.glob["Z"] = rnd(p["rows"], p["cols"], scale=2.0)
        return d
    idx = None
    if not p["dense"]:
        idx = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(b * n)])
        idx[:, 0] = torch.arange(n).repeat(b)                                    # every node has its self pair, as the k-NN lists do
        idx = idx.reshape(-1)
        d.edge["idx"] = idx
    d.src, d.dst = edge_ends(idx, b, n, k)
    if c.entry in ("fwd", "bwd", "sums", "tail"):
        d.node["coors"] = rnd(b * n, cd, scale=0.8)
    if c.entry in ("fwd", "bwd", "sums"):
        dim = 5
        if p["strided"]:                                                         # `_forward_exact`: proj (B N, 2 hq) = [P_i | P_j], W_s inside edge_mlp.0.weight
            hq = _ceil4(h)
            proj = rnd(b * n, 2 * hq, scale=0.5)
            d.node["proj"], d.hq = proj, hq
            w1 = rnd(h, 2 * dim + s, scale=0.4 / s ** 0.5)
            d.glob["w1"], d.dim = w1, dim
            d.pi, d.pj, d.ws = proj[:, :h], proj[:, hq:hq + h], w1[:, 2 * dim:]
        else:
            d.node["Pi"], d.node["Pj"] = rnd(b * n, h, scale=0.5), rnd(b * n, h, scale=0.5)
            d.glob["Ws"] = rnd(h, s, scale=0.4 / s ** 0.5)
            d.pi, d.pj, d.ws = d.node["Pi"], d.node["Pj"], d.glob["Ws"]
        d.glob["W2"] = rnd(m, h, scale=1.0 / h ** 0.5)
        if p["edge_dim"]:
            if p["by_k"]:
                d.edge["edges"] = rnd(e, p["edge_dim"])
            else:
                d.node["edges"] = rnd(b * n, n, p["edge_dim"])                   # (B, N, N, edge_dim)
    if c.entry in ("fwd", "tail"):
        if "gate" in opts:
            d.glob["gate_w"], d.glob["gate_b"] = rnd(m, scale=0.5), rnd(1, scale=0.5)
        if "no_w3" not in opts:
            d.glob["W3"], d.glob["b3"] = rnd(4 * m, m, scale=1.0 / m ** 0.5), rnd(4 * m, scale=0.3)
            d.glob["W4"], d.glob["b4"] = rnd(4 * m, scale=0.6 / (4 * m) ** 0.5), rnd(1, scale=0.1)
        if "scale" in opts or "norm" in opts:
            d.glob["scale"] = rnd(1).abs() + 0.5
    if c.entry == "fwd":
        d.glob["b2"] = rnd(m, scale=0.3)
        if any(o in opts for o in ("mask", "mask_rank", "mean_mask0")):
            mask = torch.rand(b * n, generator=g) > 0.25
            mask[0], mask[2] = True, False                                       # node 2 of graph 0: a query node with no kept edge
            d.node["mask"] = mask
        if "mask_rank" in opts:
            rank = sqdist(d.node["coors"][d.src] - d.node["coors"][d.dst]).to(dt).double()
            vals = rank.unique()
            mid = vals[vals.numel() * 2 // 3 - 1:vals.numel() * 2 // 3 + 1].mean()
            d.edge["rank"], d.valid_radius = rank, float(mid.float())
    if c.entry in ("bwd", "sums"):
        d.edge["gU"] = rnd(e, m)
    if c.entry == "tail":
        d.edge["u"] = rnd(e, m)
        d.node["g_co"] = rnd(b * n, cd)
        if "no_gmsum" not in opts:
            d.node["g_msum"] = rnd(b * n, m)
        if "pair_mask" in opts:
            d.edge["pair_mask"] = torch.rand(e, generator=g) > 0.25
    if c.entry in ("hfwd", "hbwd", "hbwd2"):
        d.node["Pi"], d.node["Pj"] = rnd(b * n, h, scale=0.5), rnd(b * n, h, scale=0.5)
        d.edge["s"] = rnd(e, s)
        d.glob["Ws"], d.glob["W2"], d.glob["b2"] = rnd(h, s, scale=0.4 / s ** 0.5), rnd(m, h, scale=1.0 / h ** 0.5), rnd(m, scale=0.3)
        if c.entry != "hfwd":
            d.edge["gU"] = rnd(e, m)
        if c.entry == "hbwd2":
            d.node["cPi"], d.node["cPj"], d.edge["cs"] = rnd(b * n, h), rnd(b * n, h), rnd(e, s)
            d.glob["cWs"], d.glob["cW2"], d.glob["cb2"] = rnd(h, s), rnd(m, h), rnd(m)
    return d


def graph_slice(d, g):
    """the operands of graph g alone (B = 1): what a chunked backward passes, with drop_eid0 = g N K"""
    out = SimpleNamespace(**vars(d))
    n, nk = d.n, d.n * d.k
    out.node = {name: t[g * n:(g + 1) * n] for name, t in d.node.items()}
    out.edge = {name: t[g * nk:(g + 1) * nk] for name, t in d.edge.items()}
    out.b, out.e = 1, nk
    out.src, out.dst = edge_ends(out.edge.get("idx"), 1, n, d.k)
    if "proj" in out.node:
        h = d.cell.p["H"]
        out.pi, out.pj = out.node["proj"][:, :h], out.node["proj"][:, d.hq:d.hq + h]
    elif "Pi" in out.node:
        out.pi, out.pj = out.node["Pi"], out.node["Pj"]
    return out


# ------------------------------------------------------------------------------------------------ the specification
def _keep(d, site, width, eid0=0, rows=None):
    """(rows, width) bool, and the scale of a kept unit as the kernels hold it (an fp32 number)"""
    import torch
    from egnn_pytorch_amd import _dropout
    rows = d.e if rows is None else rows
    keep = _dropout.keep_mask(d.drop[1], site, torch.arange(rows) + eid0, torch.arange(width), d.drop[0])
    return keep, float(torch.tensor(_dropout.inv_keep(d.drop[0]), dtype=torch.float32))


def _dropped(x, d, site, eid0):
    import torch
    if d.drop is None:
        return x, None
    keep, inv = _keep(d, site, x.shape[1], eid0, x.shape[0])
    return torch.where(keep, x * inv, torch.zeros_like(x)), keep


def _scalars(d, dt):
    """rel (E, C), the squared distance and the per-edge scalars [sin(d / 2^f) .., cos(d / 2^f) .., d, edge features] (:34-41, :270-285)"""
    import torch
    p = d.cell.p
    co = d.node["coors"].to(dt)
    rel = co[d.src] - co[d.dst]
    dist = sqdist(rel)[:, None]
    f = p["fourier"]
    cols = []
    if f:
        x = dist / (2.0 ** torch.arange(f, dtype=dt))
        cols += [x.sin(), x.cos()]
    cols.append(dist)
    if "edges" in d.edge:
        cols.append(d.edge["edges"].to(dt))
    elif "edges" in d.node:
        cols.append(d.node["edges"].to(dt)[d.src, d.dst - d.src // d.n * d.n])
    return rel, torch.cat(cols, dim=1)


def spec_fwd(d, dt, eid0=0):
    """egnn_edge_exact_*: the reference's edge pass (egnn_pytorch.py:262-333) on the operands the kernel takes"""
    import torch
    from egnn_pytorch_amd import _dropout
    F = torch.nn.functional
    p, opts, G = d.cell.p, d.cell.p["opts"], {kk: v.to(dt) for kk, v in d.glob.items()}
    m, k = p["m"], d.k
    rel, scal = _scalars(d, dt)
    z = d.pi.to(dt)[d.src] + d.pj.to(dt)[d.dst] + scal @ d.ws.to(dt).t()
    x, keep_e = _dropped(z, d, _dropout.SITE_EDGE, eid0)
    u = F.silu(x) @ G["W2"].t() + G["b2"]
    mm = F.silu(u)
    if "gate_w" in G:
        mm = mm * torch.sigmoid(mm @ G["gate_w"] + G["gate_b"])[:, None]
    pair = None
    if "mask" in d.node:
        pair = d.node["mask"][d.src] & d.node["mask"][d.dst]
        if "rank" in d.edge:
            pair = pair & (d.edge["rank"].to(dt) <= torch.tensor(d.valid_radius, dtype=dt))
    out = dict(U_out=u)
    aux = dict(keep_e=keep_e, pair=pair)
    if "W3" in G:
        hid, aux["keep_c"] = _dropped(mm @ G["W3"].t() + G["b3"], d, _dropout.SITE_COORS, eid0)
        cw = F.silu(hid) @ G["W4"] + G["b4"]
        relp = rel
        if "scale" in G:
            nrm = rel.norm(dim=-1, keepdim=True)
            aux["norm"] = nrm
            relp = rel / nrm.clamp(min=EPS) * G["scale"]
        if pair is not None:
            cw = cw.masked_fill(~pair, 0.0)
        aux["cw"] = cw
        if "clamp" in opts:
            cw = cw.clamp(min=-CLAMP, max=CLAMP)
        wrel = cw[:, None] * relp
    else:
        wrel = torch.zeros_like(rel)
    if pair is not None:
        mm = mm.masked_fill(~pair[:, None], 0.0)
    kept = torch.ones(d.e, dtype=dt) if pair is None else pair.to(dt)
    out.update(ws_m=mm, ws_wrel=wrel, ws_kept=kept)
    m_i = mm.view(-1, k, m).sum(dim=1)
    if "mean" in opts or "mean_mask0" in opts:
        if pair is not None:
            cnt = kept.view(-1, k).sum(dim=1, keepdim=True)
            m_i = (m_i / cnt.clamp(min=1e-8)).masked_fill(cnt == 0, 0.0)
            aux["cnt"] = cnt
        else:
            m_i = m_i / k
    if "no_mi" not in opts:
        out["m_i"] = m_i
    if "W3" in G:
        out["coors_out"] = d.node["coors"].to(dt) + wrel.view(-1, k, rel.shape[1]).sum(dim=1)
    if "u_out" not in opts:
        del out["U_out"]
    return out, aux


def spec_bwd(d, dt, eid0=0):
    """egnn_edge_exact_bwd_* + egnn_edge_exact_node_sums_*: torch autograd of u = W2 SiLU(drop(P_i[i] + P_j[j] + W_s s)) + b2"""
    import torch
    from egnn_pytorch_amd import _dropout
    with torch.enable_grad():
        _, scal = _scalars(d, dt)
        scal = scal.detach().requires_grad_(True)
        pi, pj = d.pi.to(dt).clone().requires_grad_(True), d.pj.to(dt).clone().requires_grad_(True)
        z = pi[d.src] + pj[d.dst] + scal @ d.ws.to(dt).t()
        z.retain_grad()
        x, keep_e = _dropped(z, d, _dropout.SITE_EDGE, eid0)
        a = torch.nn.functional.silu(x)
        u = a @ d.glob["W2"].to(dt).t()
        (u * d.edge["gU"].to(dt)).sum().backward()
    out = dict(A_T=a.detach().t(), DZ_T=z.grad.t(), g_scal=scal.grad, gPi=pi.grad, gPj=pj.grad)
    return out, dict(keep_e=keep_e)


def _tail_layer(d, dt):
    G = {kk: v.to(dt) for kk, v in d.glob.items()}
    opts = d.cell.p["opts"]
    lin = lambda w, b: SimpleNamespace(weight=w, bias=b)                         # noqa: E731
    return SimpleNamespace(
        coors_mlp=[lin(G["W3"], G["b3"]), None, None, lin(G["W4"][None, :], G["b4"])] if "W3" in G else None,
        edge_gate=[lin(G["gate_w"][None, :], G["gate_b"])] if "gate_w" in G else None,
        norm_coors="scale" in G, coors_norm=SimpleNamespace(eps=EPS, scale=G.get("scale")),
        coor_weights_clamp_value=CLAMP if "clamp" in opts else None), G


def _tail_rel(d, dt):
    co = d.node["coors"].to(dt)
    return co[d.src] - co[d.dst]


def spec_tail_closed(d, dt):
    """`autograd.tail_edge_backward`, the specification of egnn_edge_tail_exact_bwd_* (no dropout; coors_mlp present)"""
    import torch
    from egnn_pytorch_amd import autograd as A
    p = d.cell.p
    b, n, k, m, cd = d.b, d.n, d.k, p["m"], p["cdim"]
    layer, _ = _tail_layer(d, dt)
    idx = d.edge["idx"].view(b, n, k) if "idx" in d.edge else None
    pm = d.edge["pair_mask"].view(b, n, k) if "pair_mask" in d.edge else None
    g_ms = d.node["g_msum"].to(dt) if "g_msum" in d.node else torch.zeros(b * n, m, dtype=dt)
    with torch.no_grad():
        w = A.tail_edge_backward(layer, d.edge["u"].to(dt).view(b, n, k, m), d.node["coors"].to(dt).view(b, n, cd), idx, pm,
                                 d.node["g_co"].to(dt).view(b, n, cd), g_ms.view(b, n, m))
    g_rel = w["g_rel"].reshape(d.e, cd).clone()
    g_rel[d.src == d.dst] = 0.0                   # x_i - x_i: the kernel writes the exact zero its two shares sum to
    out = dict(gU=w["g_u"].reshape(d.e, m), g_rel_t=g_rel.t(), mm_t=w["m"].t(), ghid_t=w["g_hid"].t(), a3_t=w["a3"].t(), g_w=w["g_w"])
    if w["g_scale"] is not None:
        out["g_scale"] = w["g_scale"]
    if w["g_gate"] is not None:
        out.update(m0_t=w["m0"].t(), g_gate=w["g_gate"])
    return out


def spec_tail_autograd(d, dt, eid0=0):
    """The same outputs from torch autograd of the restated chain behind u (second SiLU, gate, coors_mlp with its dropout, CoorsNorm,
    mask, clamp, coordinate update, pooling): what the dropped cells and the cells without coors_mlp are held to."""
    import torch
    from egnn_pytorch_amd import _dropout
    F = torch.nn.functional
    p, opts = d.cell.p, d.cell.p["opts"]
    m = p["m"]
    layer, G = _tail_layer(d, dt)
    pm = d.edge.get("pair_mask")
    aux = {}
    with torch.enable_grad():
        u = d.edge["u"].to(dt).clone().requires_grad_(True)
        rel = _tail_rel(d, dt).requires_grad_(True)
        m0 = F.silu(u)
        mm = m0
        if "gate_w" in G:
            gpre = m0 @ G["gate_w"] + G["gate_b"]
            gpre.retain_grad()
            mm = m0 * torch.sigmoid(gpre)[:, None]
        kept_m = mm if pm is None else mm.masked_fill(~pm[:, None], 0.0)
        loss = 0.0
        if "g_msum" in d.node:
            loss = (d.node["g_msum"].to(dt)[d.src] * kept_m).sum()
        if "W3" in G:
            hpre = mm @ G["W3"].t() + G["b3"]
            hpre.retain_grad()
            hid, aux["keep_c"] = _dropped(hpre, d, _dropout.SITE_COORS, eid0)
            a3 = F.silu(hid)
            w = a3 @ G["W4"] + G["b4"]
            w.retain_grad()
            relp = rel
            if "scale" in G:
                sc = G["scale"].expand(d.e).clone().requires_grad_(True)
                nrm = rel.norm(dim=-1, keepdim=True)
                aux["norm"] = nrm.detach()
                relp = rel / nrm.clamp(min=EPS) * sc[:, None]
            wm = w if pm is None else w.masked_fill(~pm, 0.0)
            aux["cw"] = wm.detach()
            wc = wm.clamp(min=-CLAMP, max=CLAMP) if "clamp" in opts else wm
            loss = loss + (d.node["g_co"].to(dt)[d.src] * (wc[:, None] * relp)).sum()
        if not torch.is_tensor(loss):
            loss = (u * 0.0).sum()
        loss.backward()
    zeros = lambda t: torch.zeros_like(t) if t.grad is None else t.grad          # noqa: E731
    g_rel = zeros(rel).clone()
    g_rel[d.src == d.dst] = 0.0
    out = dict(gU=zeros(u), g_rel_t=g_rel.t(), mm_t=mm.detach().t())
    if "W3" in G:
        out.update(ghid_t=zeros(hpre).t(), a3_t=a3.detach().t(), g_w=zeros(w))
        if "scale" in G:
            out["g_scale"] = zeros(sc)
    if "gate_w" in G:
        out.update(m0_t=m0.detach().t(), g_gate=zeros(gpre))
    return out, aux


def spec_tail(d, dt, eid0=0):
    out, aux = spec_tail_autograd(d, dt, eid0)
    if d.drop is None and "W3" in d.glob:
        out = spec_tail_closed(d, dt)
    return out, aux


def _hidden_args(d, dt, eid0):
    import torch
    idx = d.edge["idx"].view(d.b, d.n, d.k) if "idx" in d.edge else None
    drop = None if d.drop is None else (d.drop[0], d.drop[1], eid0)
    ins = [d.node["Pi"], d.node["Pj"], d.edge["s"], d.glob["Ws"], d.glob["W2"]]
    return [t.to(dt) for t in ins], idx, drop, (d.b, d.n, d.k)


def spec_hidden(d, dt, eid0=0):
    """egnn_edge_hidden_*: u from `autograd.edge_hidden_torch`; the per-edge tables of the two backwards from `autograd._silu_terms`, the
    building block of `edge_hidden_backward_spec` / `edge_hidden_double_backward_spec` (tests/test_plain_variants_table.py contracts
    these tables and compares them with the two specifications' own outputs)."""
    import torch
    from egnn_pytorch_amd import autograd as A
    ins, idx, drop, dims = _hidden_args(d, dt, eid0)
    p_i, p_j, s, w_s, w2 = ins
    entry = d.cell.entry
    aux = dict(keep_e=None if d.drop is None else _keep(d, 0, w_s.shape[0], eid0)[0])
    with torch.no_grad():
        if entry == "hfwd":
            return dict(u=A.edge_hidden_torch(p_i, p_j, s, w_s, w2, d.glob["b2"].to(dt), idx, drop, dims)), aux
        src, dst, dk, a, a1, a2 = A._silu_terms(p_i, p_j, s, w_s, idx, drop, dims)
        g_u = d.edge["gU"].to(dt)
        g_a = g_u @ w2
        dz = dk * a1 * g_a
        if entry == "hbwd":
            return dict(A_T=a.t(), DZ_T=dz.t(), g_s=dz @ w_s), aux
        cpi, cpj, cs = d.node["cPi"].to(dt), d.node["cPj"].to(dt), d.edge["cs"].to(dt)
        cws, cw2, cb2 = d.glob["cWs"].to(dt), d.glob["cW2"].to(dt), d.glob["cb2"].to(dt)
        v = cpi[src] + cpj[dst] + s @ cws.t() + cs @ w_s.t()
        dav = dk * a1 * v
        r = dk * (dk * a2 * g_a * v + a1 * (g_u @ cw2))
        return dict(g_gU=dav @ w2.t() + a @ cw2.t() + cb2, g_s=r @ w_s + dz @ cws, DAV_T=dav.t(), R_T=r.t(), DZ_T=dz.t()), aux


def spec_silu(d, dt, row0=0):
    import torch
    from egnn_pytorch_amd import _dropout
    z = d.glob["Z"].to(dt)
    keep = None
    if d.drop is not None:
        keep, inv = _keep(d, _dropout.SITE_NODE, z.shape[1], row0, z.shape[0])
        z = torch.where(keep, z * inv, torch.zeros_like(z))
    return dict(Z=torch.nn.functional.silu(z)), dict(keep_e=keep)


SPECS = dict(fwd=spec_fwd, bwd=spec_bwd, sums=spec_bwd, tail=spec_tail, hfwd=spec_hidden, hbwd=spec_hidden, hbwd2=spec_hidden,
             silu=spec_silu)


@functools.lru_cache(maxsize=None)
def reference(cid, t="d"):
    """(outputs, aux) of a cell's specification in float64 (t = "d") or in torch fp32 (t = "f": ATen on the same inputs, whose error
    against float64 the fp32 bars are multiples of), outputs returned in float64.  Cached and shared; nobody writes to it."""
    d = prepare(cid)
    out, aux = SPECS[d.cell.entry](d, torch_dtype(t))
    return {name: v.detach().double().contiguous() for name, v in out.items()}, aux


def output_shapes(cid):
    """every tensor a cell's call writes, by its name in `reference`, with the shape the GPU test allocates for it (`ws`: the forward's
    per-edge workspace, which the test reads as ws_m | ws_wrel | ws_kept)"""
    c = BY_ID[cid]
    p = c.p
    e, nodes, m, h, s, cd = e_of(p), p["b"] * p["n"], p["m"], p["H"], s_of(p), p["cdim"]
    opts = p["opts"]
    if c.entry == "silu":
        return dict(Z=(p["rows"], p["cols"]))
    if c.entry == "fwd":
        out = dict(ws=(e, m + cd + 1))
        if "no_mi" not in opts:
            out["m_i"] = (nodes, m)
        if "no_w3" not in opts:
            out["coors_out"] = (nodes, cd)
        if "u_out" in opts:
            out["U_out"] = (e, m)
        return out
    if c.entry in ("bwd", "sums"):
        return dict(A_T=(h, e), DZ_T=(h, e), g_scal=(e, s), gPi=(nodes, h), gPi_T=(h, nodes), gPj=(nodes, h), gPj_T=(h, nodes))
    if c.entry == "tail":
        out = dict(gU=(e, m), g_rel_t=(cd, e), mm_t=(m, e))
        if "no_w3" not in opts:
            out.update(ghid_t=(4 * m, e), a3_t=(4 * m, e), g_w=(e,))
            if "norm" in opts:
                out["g_scale"] = (e,)
        if "gate" in opts:
            out.update(m0_t=(m, e), g_gate=(e,))
        return out
    if c.entry == "hfwd":
        return dict(u=(e, m))
    if c.entry == "hbwd":
        return dict(A_T=(h, e), DZ_T=(h, e), g_s=(e, s))
    return dict(g_gU=(e, m), g_s=(e, s), DAV_T=(h, e), R_T=(h, e), DZ_T=(h, e))


# ------------------------------------------------------------------------------------------------ the bars
HIDDEN_F32_REL = 1e-5                                            # tests/test_gpu_second_order.py::test_kernels_match_specification
F64_REL = 1e-12                                                  # tests/test_float64_property_suite.py
ATEN_FACTOR, FLOOR_ULPS = 8.0, 16.0


def bar(cid, name):
    """The largest |kernel - float64 specification| a tensor of a cell may show.  float64: 1e-12 max(1, max |ref|).  fp32 edge_hidden:
    1e-5 of the tensor's scale.  fp32 elsewhere: 8 x the error torch fp32 makes on the same specification and inputs -- the factor covers
    another summation order over H <= ~200 terms and expf against ATen's SiLU -- plus 16 x 2^-24 max |ref| for the tensors ATen gets
    exactly.  Nothing here looks at a kernel's output."""
    c = BY_ID[cid]
    ref = reference(cid)[0][name]
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if c.t == "d":
        return F64_REL * max(1.0, top)
    if c.entry in ("hfwd", "hbwd", "hbwd2"):
        return HIDDEN_F32_REL * max(top, 1e-30)
    aten = float((reference(cid, "f")[0][name] - ref).abs().max()) if ref.numel() else 0.0
    return ATEN_FACTOR * aten + FLOOR_ULPS * 2.0 ** -24 * top
