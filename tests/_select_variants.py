"""One test case per template instantiation and per run-time route of the neighbour selection kernels (csrc/knn_select.hip,
csrc/knn_rows.hip, csrc/knn_stream.hip, csrc/knn_segments.hip, csrc/knn_grid.hip, sharing csrc/knn_core.h) -- the table behind
tests/test_gpu_select_variants.py, importable without a GPU.  The family's contract is bit equality with the oracle: no bar anywhere.

The launchers dispatch to 50 kernels:
    select    egnn_knn_select_f32 / _f64        knn_select_kernel<CPL 1 .. 64, CDM 3 / 8>, <128, 3>; knn_select_rows_kernel<f, 3 / 8 / 0>,
                                                <d, 0>; beyond 160 KiB of keys (and C <= 8 beyond 32 768 nodes) the streaming kernel
    stream    egnn_knn_select_stream_f32 / _f64 knn_select_stream_kernel<f, 3 / 8 / 0, FL = 0, CSR = 0>, <d, 0, 0, 0>
    csr       egnn_knn_select_csr_f32 / _f64    knn_select_stream_kernel<.., 0, CSR = 1>
    segments  egnn_knn_select_segments_f32/_f64 knn_select_segments_kernel<f, 3 / 8 / 0>, <d, 0>
    grid      egnn_knn_select_grid_f32 / _f64   kg_bbox / kg_setup / kg_count / kg_scan / kg_place_kernel<T>, kg_search_kernel<T, 0>, and
                                                the flagged streaming kernel knn_select_stream_kernel<f, 3, 1, 0> / <d, 0, 1, 0>
    grid_csr  egnn_knn_select_grid_csr_f32/_f64 the same with kg_search_kernel<T, 1> and knn_select_stream_kernel<.., 1, 1>
    maxdeg    egnn_adj_max_degree_u8            adj_max_degree_kernel
`plan()` / `dispatch()` restate the launchers (argument checks in their order, the N / C thresholds, LDS bytes, the 64 KiB opt-in, the
160 KiB hand-over and refusal, R and IBP of the stream, Lp and W of the segments, the grid's own refusals), `route()` restates the
conditions by which a kernel picks a route for a row FROM THE DATA (it chooses inputs and backs coverage claims; the GPU test never
trusts it for correctness), `CELLS` holds one call per instantiation (`MAIN`) and the cells beside the grid, `prepare()` builds a cell's
operands with a seeded numpy generator, `reference()` evaluates the oracle's ranking (oracle.egnn_oracle: the arithmetic of `pairwise`,
`build_ranking`, `topk_smallest`, restated for row subsets and tied to those functions in tests/test_select_variants_table.py) in the
cell's type.  A NEW INSTANTIATION NEEDS A NEW CELL: tests/test_select_variants_table.py compares the table with what the compiler
instantiated.

The cells beside the grid (`group`):
    top       the register kernel at the top of every size class (64 .. 4096, 8192): N % 64 == 0, no pad candidate
    route     one cell per kernel and route, `claims` naming rows that take it (proved on the host from the oracle's keys)
    tie       integer lattice / coincident / collinear nodes: tie groups straddling slot K, lane, thread-slice and wave boundaries
    kclass    K = 1, 32, 33, 64, 65, 128, 129, N, 1024
    cdim      C = 1, 2, 4, 5, 7, 8 on the CDM = 8 instantiations; 9, 16, 33, 64 on the CDM = 0 ones
    adjform   shared / per-graph adjacency, with / without diagonal, isolated row, rows of exactly K - 2, K - 1, K adjacent nodes,
              misaligned rows, CSR shared / per graph / without a column
    underflow three planted pairs of non-adjacent nodes closer than the smallest squared distance float32 can hold
    flagged   the flagged streaming kernel through its own entries with a hand-made flag array: zero-flag rows stay untouched
    refuse    every refusal code once per entry, decided on the host before any launch
`public=True` cells run a second time through `_ops.knn_select`, the public dispatcher, on the same operands.  That is a comparison of
the family's kernels with each other on one input, NOT proof of a hand-over: at these sizes the dispatcher picks the register or rows
kernel, not the stream / grid kernel the cell is named for (it reaches the stream only beyond 32 768 nodes or 160 KiB of keys, where
the table has no cell; tests/test_gpu_large_graphs.py covers that).  The `select` cells run once: there the direct entry IS the public one.
The cells with N = 1 are exempt from "every cell notices at least one deliberate error" (tests/test_select_variants_table.py): with one
candidate per row no error of the selection can change the output."""
import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

# ------------------------------------------------------------------------------------------------ the launchers, restated
E_NULLPTR, E_SHAPE, E_UNSUPPORTED, E_ALIGN, E_K_GT_N = -1, -2, -3, -4, -5        # include/egnn_hip.h:34-38
LDS_OPT_IN, LDS_MAX = 64 * 1024, 160 * 1024
ESZ = dict(f=4, d=8)                                             # bytes of a coordinate, and of its ranking key
KNN_SURVIVORS, KNN_BITS, KNN_WAVES, KNN_ROWS_PER_WG = 128, 16, 4, 32             # knn_select.hip
KR_THREADS, KR_WAVES = 256, 4                                    # knn_rows.hip
KS_RMAX, KS_HSTRIDE = 16, 257                                    # knn_stream.hip
SG_ROWS, SG_WAVES, SG_LDS_BYTES, SG_SURVIVORS = 32, 4, 64 * 1024, 128            # knn_segments.hip
KG_KMAX, KG_PARTS, KG_PW = 128, 64, 16                           # knn_grid.hip
TIE_EPS = 2.0 ** -60                                             # knn_select.hip: KNN_TIE_EPS
ENTRIES = ("select", "stream", "csr", "segments", "grid", "grid_csr", "maxdeg")
ALL_PAIRS = ("select", "stream", "csr", "grid", "grid_csr")      # (B, N, C) coordinates, (B, N, K) outputs

Inst = namedtuple("Inst", "kernel args")                         # args: the template arguments, T as "f" / "d", bools as 0 / 1


def inst_name(i):
    return i.kernel + ("<" + ",".join(str(a) for a in i.args) + ">" if i.args else "")


def up8(x):
    return (x + 7) // 8 * 8


def up256(x):
    return (x + 255) // 256 * 256


def cpl_of(n):
    """keys per lane of the register kernel for N <= 8192"""
    for top, cpl in ((64, 1), (128, 2), (256, 4), (512, 8), (1024, 16), (2048, 32), (4096, 64), (8192, 128)):
        if n <= top:
            return cpl
    raise ValueError(n)


def select_lds(n, k, c):
    """launch_knn_c: the coordinates and mask bytes of Npad nodes, 8-byte aligned, four waves' lists, the duplicate flags"""
    npad = (n + 63) // 64 * 64
    kpad = (k + 1) // 2 * 2 if k > KNN_SURVIVORS else KNN_SURVIVORS
    cbytes = npad * (4 * c + 1)
    return cbytes + 8 - cbytes % 8 + KNN_WAVES * kpad * 8 + 8


def rows_lds(t, n, k):
    return up8(n * ESZ[t]) + k * (ESZ[t] + 4) + 2 * KR_WAVES * 4 + 8


def stream_params(t, n, k, c):
    """(R rows per workgroup, IBP index bits, LDS bytes) of knn_stream_launch"""
    ks = ESZ[t]
    r = KS_RMAX
    while r > 1 and r * k * (ks + 4) > 64 * 1024:
        r >>= 1
    ibits = 1
    while ibits < 31 and (1 << ibits) < n:
        ibits += 1
    ibp = (ibits + 7) // 8 * 8
    head = KS_RMAX * (ks + 4 + 4 * 5) + 4 * 4
    lds = head + ((r * KS_HSTRIDE + 1) & ~1) * 4 + r * k * ks + (r * k + ((r * k) & 1)) * 4 + r * c * ESZ[t]
    return r, ibp, lds


def segments_params(t, k, c, max_segment, lds_nodes=0):
    """(Lp entries of a wave's list, W nodes of the window, LDS bytes) of knn_segments_launch"""
    any_c = t == "d" or c > 8
    lp = (k + 1) & ~1 if k > SG_SURVIVORS else SG_SURVIVORS
    waves = SG_WAVES * up8(lp * (ESZ[t] + 4) + 256 * 4 + (c if any_c else 0) * ESZ[t])
    node = ((c | 1) if any_c else c) * ESZ[t]
    w = (SG_LDS_BYTES - waves - 8) // node if SG_LDS_BYTES > waves + 8 else 0
    w = min(w, SG_ROWS + 2 * max_segment)
    if lds_nodes > 0:
        w = min(w, lds_nodes)
    return lp, w, up8(w * node) + waves


def grid_layout(t, b, n):
    """kg_layout: byte offsets of the row flags and the total"""
    rec = 16 if t == "f" else 32
    cap = n // 4 + 64
    o = up256(b * 64)
    o = up256(o + b * KG_PARTS * KG_PW * 8)
    flag = o
    o = up256(o + b * n)
    o = up256(o + b * n * 4)
    o = up256(o + b * cap * 4)
    o = up256(o + b * (cap + 1) * 4)
    o = up256(o + b * n * rec)
    return SimpleNamespace(flag=flag, total=o)


def _check_args(null, b, n, k, c):
    """knn_core.h::egnn_knn_check_args"""
    if null & {"coors", "idx", "rank"}:
        return E_NULLPTR
    if b <= 0 or n <= 0 or k <= 0:
        return E_SHAPE
    if c < 1 or c > 64:
        return E_UNSUPPORTED
    if k > n:
        return E_K_GT_N
    if k > 1024 or b > 65535:
        return E_UNSUPPORTED
    return 0


def _stream_plan(t, n, k, c, b, null, csr, flagged):
    rc = _check_args(null, b, n, k, c)
    if rc:
        return rc
    if flagged and c != 3:
        return E_UNSUPPORTED
    cdm = 0 if t == "d" or c > 8 else (3 if c == 3 else 8)
    r, ibp, lds = stream_params(t, n, k, c)
    inst = Inst("knn_select_stream_kernel", (t, cdm, int(flagged), int(csr)))
    return SimpleNamespace(insts=(inst,), lds=lds, R=r, IBP=ibp, opt_in=lds > LDS_OPT_IN)


def _rows_plan(t, n, k, c, b, null):
    lds = rows_lds(t, n, k)
    if lds > LDS_MAX:                                            # knn_rows_launch: the keys do not fit, recomputed per pass
        return _stream_plan(t, n, k, c, b, null, False, False)
    cdm = 0 if t == "d" or c > 8 else (3 if c == 3 else 8)
    return SimpleNamespace(insts=(Inst("knn_select_rows_kernel", (t, cdm)),), lds=lds, opt_in=lds > LDS_OPT_IN)


def plan(entry, t, n, k, c, adj=None, flagged=False, b=1, null=(), rp_stride=None, ws_short=0, ws_misalign=0, g=1, max_segment=None,
         lds_nodes=0):
    """What a call does: the refusal code (an int, the checks in the launcher's own order), or the kernels it launches (.insts, a tuple)
    with the launch's LDS bytes and the launcher's derived parameters.  n: N (segments: the T nodes of the packed batch); adj: None,
    "dense" or "csr"; null: the arguments passed as NULL; rp_stride: None = what the adjacency implies."""
    null = set(null)
    if entry == "maxdeg":                                        # egnn_adj_max_degree_u8 (rows = b * n)
        if null & {"adj", "out"}:
            return E_NULLPTR
        if b * n <= 0 or n <= 0:
            return E_SHAPE
        return SimpleNamespace(insts=(Inst("adj_max_degree_kernel", ()),), lds=0, opt_in=False)
    if entry == "select":
        rc = _check_args(null, b, n, k, c)
        if rc:
            return rc
        if t == "d":                                             # egnn_knn_select_f64: knn_rows_launch<double>
            return _rows_plan(t, n, k, c, b, null)
        if c > 8 or n > (8192 if c == 3 else 4096):
            if c <= 8 and n > 32768:
                return _stream_plan(t, n, k, c, b, null, False, False)
            return _rows_plan(t, n, k, c, b, null)
        lds = select_lds(n, k, c)
        if lds > LDS_MAX:
            return E_UNSUPPORTED
        return SimpleNamespace(insts=(Inst("knn_select_kernel", (cpl_of(n), 3 if c == 3 else 8)),), lds=lds, opt_in=lds > LDS_OPT_IN,
                               CPL=cpl_of(n), rows_per_wg=KNN_ROWS_PER_WG if n >= KNN_ROWS_PER_WG else (n + 3) // 4 * 4)
    if entry == "stream":
        return _stream_plan(t, n, k, c, b, null, False, flagged)
    if entry == "csr":                                           # knn_csr
        if "rowptr" in null:
            return E_NULLPTR
        if n > 0 and rp_stride not in (None, 0, n + 1):
            return E_SHAPE
        return _stream_plan(t, n, k, c, b, null, True, flagged)
    if entry == "segments":                                      # knn_segments_launch
        if null & {"offsets", "segment_of"}:
            return E_NULLPTR
        ms = max_segment if max_segment is not None else n
        rc = _check_args(null, 1 if (g > 0 and 0 < ms <= n) else 0, n, k, c)
        if rc:
            return rc
        cdm = 0 if t == "d" or c > 8 else (3 if c == 3 else 8)
        lp, w, lds = segments_params(t, k, c, ms, lds_nodes)
        return SimpleNamespace(insts=(Inst("knn_select_segments_kernel", (t, cdm)),), lds=lds, Lp=lp, W=w, opt_in=False)
    assert entry in ("grid", "grid_csr")                         # kg_select
    csr = entry == "grid_csr"
    if csr and "rowptr" in null:
        return E_NULLPTR
    if null & {"coors", "idx", "rank", "ws"}:
        return E_NULLPTR
    if b <= 0 or n <= 0 or k <= 0 or k > n:
        return E_SHAPE
    if csr and rp_stride not in (None, 0, n + 1):
        return E_SHAPE
    if c != 3 or k > KG_KMAX or b > 65535:
        return E_UNSUPPORTED
    if ws_short > 0:
        return E_SHAPE
    if ws_misalign % 16:
        return E_ALIGN
    build = tuple(Inst(f"kg_{s}_kernel", (t,)) for s in ("bbox", "setup", "count", "scan", "place"))
    tail = _stream_plan(t, n, k, 3, b, null, csr, True)
    assert not isinstance(tail, int)
    return SimpleNamespace(insts=build + (Inst("kg_search_kernel", (t, int(csr))),) + tail.insts, lds=tail.lds, R=tail.R, IBP=tail.IBP,
                           opt_in=tail.opt_in, ws_bytes=grid_layout(t, b, n).total)


def dispatch(entry, t, n, k, c, adj=None, flagged=False, **kw):
    """the `Inst`s a call launches (a tuple: the grid launches seven), or the launcher's refusal code"""
    got = plan(entry, t, n, k, c, adj, flagged, **kw)
    return got if isinstance(got, int) else got.insts


def grid():
    """every instantiation the launchers can reach"""
    out = set()
    for entry in ENTRIES:
        for t in "fd":
            for n in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193):
                for c in (3, 5, 9):
                    got = dispatch(entry, t, n, 1, c)
                    if not isinstance(got, int):
                        out.update(got)
    return out


# ------------------------------------------------------------------------------------------------ the table
Cell = namedtuple("Cell", "id entry t inst group p expect claims")
_DEFAULTS = dict(b=2, n=70, k=8, c=3, mask="prefix", adj=None, band=2, adjopt=(), geom="normal", plant=(), sizes=None, lds_nodes=0,
                 pin=0, raw=None, public=False, flags=None)


def expected(entry, t, p):
    """`plan` of a cell's own arguments"""
    raw = p["raw"] or {}
    n = sum(p["sizes"]) if entry == "segments" else p["n"]
    kw = dict(b=raw.get("b", p["b"]), null=raw.get("null", ()), rp_stride=raw.get("rp_stride"), ws_short=raw.get("ws_short", 0),
              ws_misalign=raw.get("ws_misalign", 0), lds_nodes=p["lds_nodes"])
    if entry == "segments":
        kw.update(g=raw.get("g", len(p["sizes"])), max_segment=raw.get("max_segment", max(max(p["sizes"]), 1)))
        kw["b"] = 1
    adj = None if p["adj"] is None else ("csr" if entry in ("csr", "grid_csr") else "dense")
    return plan(entry, t, raw.get("n", n), raw.get("k", p["k"]), raw.get("c", p["c"]), adj, p["flags"] is not None, **kw)


SEG_SIZES = (5, 3, 200, 40, 1, 300, 3)                            # offsets 0 5 8 208 248 249 549 552: see `route`'s streamed claims
ROUTE_MASK = "route"                                             # graph 0: node 12 masked; graph 1: only nodes 0 .. 4 valid
GRID_N, GRID_OUT = 96, (40, 41, 42, 43, 44)                      # the grid cells: five nodes of graph 0 far away, fewer than K of them


def _build_cells():
    cells = []

    def add(entry, t, group, tag, claims=(), **kw):
        p = dict(_DEFAULTS)
        p.update(kw)
        p["adjopt"], p["plant"] = tuple(p["adjopt"]), tuple(p["plant"])
        if entry in ("csr", "grid_csr") and p["adj"] is None:
            p["adj"] = "band"
        if entry == "segments":
            p["sizes"] = tuple(p["sizes"] or SEG_SIZES)
            p["b"], p["mask"], p["n"] = 1, None, sum(p["sizes"])
        if entry == "maxdeg":
            p["adj"], p["mask"] = p["adj"] or "band", None
        got = expected(entry, t, p)
        if isinstance(got, int):
            inst, expect = None, got
            cid = f"{entry}_{t}_{group}_{tag}_refused{-got}"
        else:
            inst, expect = got.insts[p["pin"]], None
            cid = f"{inst_name(inst)}_{entry}_{group}_{tag}"
        cells.append(Cell(cid, entry, t, inst, group, p, expect, tuple(claims)))

    sizes = ((1, 1), (2, 65), (4, 129), (8, 257), (16, 513), (32, 1025), (64, 2049))
    # ---- MAIN: one call per instantiation, at the SMALLEST N that reaches it (N % 64 == 1: a column of pad candidates), B = 2 with
    # prefix masks of different lengths wherever the entry takes a batch
    for cpl, n in sizes:
        for c in (3, 5):
            add("select", "f", "main", f"n{n}c{c}", n=n, c=c, k=min(n, 8 if cpl % 2 else 12))
    add("select", "f", "main", "n4097c3", n=4097, c=3, k=8)
    add("select", "f", "main", "n8193c3", n=8193, c=3, k=8, b=1)
    add("select", "f", "main", "n4097c5", n=4097, c=5, k=8, b=1)
    add("select", "f", "main", "n70c9", n=70, c=9, k=8)
    add("select", "d", "main", "n70c3", n=70, c=3, k=8)
    for c in (3, 5, 9):
        add("stream", "f", "main", f"n300c{c}", n=300, c=c, k=8, public=True)
        add("csr", "f", "main", f"n300c{c}", n=300, c=c, k=8, public=True)
        add("segments", "f", "main", f"c{c}", c=c, k=8)
    add("stream", "d", "main", "n300c3", n=300, k=8, public=True)
    add("csr", "d", "main", "n300c3", n=300, k=8, public=True)
    add("segments", "d", "main", "c3", k=8)
    grid_claims = (("decided_by_grid", ((0, 0), (0, GRID_N - 1))), ("handed_to_stream", ((0, GRID_OUT[0]), (1, 0), (1, GRID_N - 1))))
    for t in "fd":
        for pin, kern in enumerate(("bbox", "setup", "count", "scan", "place", "search", "flagged")):
            add("grid", t, "main", kern, claims=grid_claims, n=GRID_N, k=8 + pin, mask="grid", geom="outliers", pin=pin, public=True)
            if pin >= 5:
                add("grid_csr", t, "main", kern, claims=grid_claims, n=GRID_N, k=8 + pin, mask="grid", geom="outliers", pin=pin, public=True)
    add("maxdeg", "f", "main", "n70", n=70, band=3, adjopt=("batched",))
    # ---- the register kernel at the top of its size classes: N % 64 == 0, no pad candidate
    for cpl, n in sizes:
        top = 64 * cpl
        for c in (3, 5):
            add("select", "f", "top", f"n{top}c{c}", n=top, c=c, k=min(top, 8))
    add("select", "f", "top", "n8192c3", n=8192, c=3, k=8, b=1)
    # ---- routes.  Wave w of a workgroup walks rows w, w + 4, ..: with node 12 of graph 0 masked, rows 0 / 4 pair, row 8 loses its
    # partner to the mask and takes the single-row code, row 12 returns early; N odd: the last row has no partner.  Graph 1 has five
    # valid nodes: its K-th key is 1e5, every masked candidate survives the pruning bound, and beyond 128 of them the row falls back
    # to the radix descent.
    for n in (61, 301, 2101):
        cpl = cpl_of(n)
        for c in (3, 5):
            pair = c == 3 and cpl <= 16
            one = "pair" if pair else "prune1"
            cl = [(one, ((0, 0), (0, 4))), ("prune1", ((0, 8), (0, n - 4 if pair else 1))), ("masked_row", ((0, 12), (1, 5)))]
            if n > 128:
                cl.append(("survivors_overflow", ((1, 0), (1, 4))))
            add("select", "f", "route", f"n{n}c{c}k8", claims=cl, n=n, c=c, k=8, mask=ROUTE_MASK)
            cl = [("prune2", ((0, 0), (0, 8))), ("masked_row", ((0, 12),))] + ([("survivors_overflow", ((1, 0),))] if n > 128 else [])
            add("select", "f", "route", f"n{n}c{c}k40", claims=cl, n=n, c=c, k=40, mask=ROUTE_MASK)
            if n > 130:
                add("select", "f", "route", f"n{n}c{c}k70", claims=[("k_gt_64", ((0, 0), (1, 0))), ("masked_row", ((0, 12),))], n=n, c=c, k=70,
                    mask=ROUTE_MASK)
                add("select", "f", "route", f"n{n}c{c}k130", claims=[("k_gt_128", ((0, 0), (1, 0))), ("masked_row", ((0, 12),))], n=n, c=c,
                    k=130, mask=ROUTE_MASK)
    # rows the adjacency decides, and the three causes that keep it from deciding (band 2 with the diagonal: four adjacent nodes, K = 4)
    for c in (3, 5):
        cl = [("adj_decided", ((0, 100), (0, 12), (1, 100))), ("adj_refused_degree", ((0, 10), (0, 0))), ("adj_refused_dup", ((0, 50), (0, 200))),
              ("prune1", ((0, 10), (0, 50)))]
        add("select", "f", "route", f"n304c{c}adj", claims=cl, n=304, c=c, k=4, adj="band", adjopt=("special",), mask=ROUTE_MASK, plant=("dupx",))
        for n in (60, 301, 2112):
            # (graph 1's masked rows: self, four adjacent nodes, then everything at 1e5 -- beyond 128 nodes the radix descent)
            cl = [("adj_refused_shape", ((0, 30), (1, 30))), ("prune1", ((0, 30),))] + ([("survivors_overflow", ((1, 30),))] if n > 128 else [])
            add("select", "f", "route", f"n{n}c{c}adj", claims=cl, n=n, c=c, k=8, adj="band", mask=ROUTE_MASK)
    for t, c in (("f", 9), ("d", 3)):
        add("select", t, "route", f"n70c{c}", claims=[("masked_row", ((0, 12), (1, 5))), ("select", ((0, 0), (1, 0)))], n=70, c=c, mask=ROUTE_MASK)
    for entry in ("stream", "csr"):
        for t in "fd":
            cl = [("index_digits", ((0, 0), (0, 3))), ("resolved_in_key_digits", ((1, 5), (1, 100)))]
            if entry == "stream":
                cl.append(("masked_row", ((0, 12),)))
            add(entry, t, "route", "n300", claims=cl, n=300, geom=("coincident", "normal"), mask="one")
    for t in "fd":
        for k, pr in ((8, "prune1"), (40, "prune2")):
            cl = [("take_all+lds", ((0, 0), (0, 248))), (pr + "+lds", ((0, 8), (0, 100))), ("radix+lds", ((0, 249), (0, 251)))]
            add("segments", t, "route", f"k{k}lds", claims=cl, k=k, geom="segtie")
            cl = [("take_all+lds", ((0, 0),)), ("take_all+streamed", ((0, 549), (0, 551))), (pr + "+streamed", ((0, 8), (0, 100))),
                  ("radix+streamed", ((0, 249), (0, 251)))]
            add("segments", t, "route", f"k{k}streamed", claims=cl, k=k, geom="segtie", lds_nodes=64)
    # ---- ties straddling slot K: one size per kernel
    for geom in ("lattice", "coincident", "collinear"):
        add("select", "f", "tie", f"n130_{geom}", n=130, geom=geom)
        add("select", "f", "tie", f"n130c5_{geom}", n=130, c=5, geom=geom)
        add("select", "f", "tie", f"n600c9_{geom}", n=600, c=9, geom=geom)               # per = 3: slices, and waves at 192 / 384 / 576
        add("select", "d", "tie", f"n300_{geom}", n=300, geom=geom)
        add("stream", "f", "tie", f"n300_{geom}", n=300, geom=geom)
        add("csr", "f", "tie", f"n300_{geom}", n=300, geom=geom)
        add("segments", "f", "tie", geom, geom=geom)
        add("grid", "f", "tie", f"n300_{geom}", n=300, geom=geom, pin=5)
    # ---- K classes
    for k in (1, 32, 33, 64, 65, 128, 129, 130):
        add("select", "f", "kclass", f"n130k{k}", n=130, k=k)
        add("stream", "f", "kclass", f"n130k{k}", n=130, k=k)
    for k in (1, 64, 65, 129, 130):
        add("select", "f", "kclass", f"n130c9k{k}", n=130, c=9, k=k)
        add("segments", "f", "kclass", f"k{k}", k=k, sizes=(5, 130, 70))
    add("select", "f", "kclass", "n1024k1024", n=1024, k=1024, mask="prefix")
    add("stream", "f", "kclass", "n1024k1024", n=1024, k=1024, b=1)
    add("stream", "d", "kclass", "n1024k1024", n=1024, k=1024, b=1)
    add("segments", "f", "kclass", "k1024", k=1024, sizes=(1030, 7))
    add("select", "f", "kclass", "n1030c9k1024", n=1030, c=9, k=1024, b=1)
    # ---- coordinate dimensions
    for c in (1, 2, 4, 5, 7, 8):
        add("select", "f", "cdim", f"n100c{c}", n=100, c=c)
        add("select", "f", "cdim", f"n4097c{c}", n=4097, c=c, b=1)
        add("stream", "f", "cdim", f"n200c{c}", n=200, c=c)
        add("segments", "f", "cdim", f"c{c}", c=c, sizes=(5, 130, 70))
    for c in (9, 16, 33, 64):
        for t in "fd":
            add("select", t, "cdim", f"n70c{c}", n=70, c=c)
            add("stream", t, "cdim", f"n70c{c}", n=70, c=c)
            add("segments", t, "cdim", f"c{c}", c=c, sizes=(5, 130, 70))
    for c in (1, 5, 7):
        add("select", "d", "cdim", f"n70c{c}", n=70, c=c)
    # ---- adjacency forms
    for n in (304, 300, 100):                                    # the decided route; N % 16 != 0: rows misaligned for its loads; CPL = 2
        for opts in ((), ("batched",), ("nodiag",), ("batched", "nodiag", "special"), ("special",)):
            add("select", "f", "adjform", f"n{n}_{'_'.join(opts) or 'shared'}", n=n, k=4, adj="band", adjopt=opts)
    add("select", "f", "adjform", "n4097_batched", n=4097, k=4, adj="band", adjopt=("batched", "special"), b=2)
    add("select", "d", "adjform", "n100_batched", n=100, k=4, adj="band", adjopt=("batched", "special"))
    for t in "fd":
        for opts in ((), ("batched",), ("batched", "nodiag", "special"), ("batched", "empty1"), ("empty",)):
            add("csr", t, "adjform", f"n100_{'_'.join(opts) or 'shared'}", n=100, k=4, adj="band", adjopt=opts, public=True)
        add("stream", t, "adjform", "n100_batched", n=100, k=4, adj="band", adjopt=("batched", "special"))
        add("grid_csr", t, "adjform", "n100_empty1", n=100, k=4, adj="band", adjopt=("batched", "empty1"), pin=5)
    # ---- squared distances that underflow to 0.0 between nodes that share no coordinate
    for c in (3, 5):
        for n in (144, 304, 1024, 1040):                          # CPL 4, 8, 16, 32: the decided route
            add("select", "f", "underflow", f"n{n}c{c}", n=n, c=c, k=4, adj="band", mask="under", plant=("under",))
    add("select", "f", "underflow", "n112c3", n=112, k=4, adj="band", mask="under", plant=("under",))      # CPL 2: no shortcut
    add("select", "f", "underflow", "n304c9", n=304, c=9, k=4, adj="band", mask="under", plant=("under",))
    add("stream", "f", "underflow", "n304c3", n=304, k=4, adj="band", mask="under", plant=("under",))
    add("csr", "f", "underflow", "n304c3", n=304, k=4, adj="band", mask="under", plant=("under",))
    # ---- the flagged streaming kernel on its own (egnn_knn_stream_flagged_*: what the grid calls behind kg_search_kernel), with a
    # hand-made flag array: only rows with a non-zero flag are selected and written, every other row is left as it was.  Through the
    # grid a flagged kernel that rewrote the zero-flag rows would go unseen -- the search has written them already, correctly.
    for t in "fd":
        for entry in ("stream", "csr"):
            add(entry, t, "flagged", "n100", n=100, k=8, mask="one", flags="mixed")
            add(entry, t, "flagged", "n700k600", n=700, k=600, b=1, mask="one", flags="mixed")   # R = 8 (float) / 8 (double) rows per workgroup
    # ---- refusals, decided on the host before any launch
    for entry in ALL_PAIRS:
        for t in "fd":
            for tag, raw in (("null_coors", dict(null=("coors",))), ("null_idx", dict(null=("idx",))), ("null_rank", dict(null=("rank",))),
                             ("b0", dict(b=0)), ("k0", dict(k=0)), ("c0", dict(c=0)), ("c65", dict(c=65)), ("k1025", dict(n=1100, k=1025)),
                             ("k_n1", dict(k=71))):
                add(entry, t, "refuse", tag, raw=raw)
    for t in "fd":
        for entry in ("csr", "grid_csr"):
            add(entry, t, "refuse", "null_rowptr", raw=dict(null=("rowptr",)))
            add(entry, t, "refuse", "stride", raw=dict(rp_stride=70))
        for entry in ("grid", "grid_csr"):
            add(entry, t, "refuse", "null_ws", raw=dict(null=("ws",)))
            add(entry, t, "refuse", "c2", raw=dict(c=2))
            add(entry, t, "refuse", "k129", n=200, raw=dict(k=KG_KMAX + 1))
            add(entry, t, "refuse", "ws_short", raw=dict(ws_short=1))
            add(entry, t, "refuse", "ws_misaligned", raw=dict(ws_misalign=8))
        for tag, raw in (("null_coors", dict(null=("coors",))), ("null_offsets", dict(null=("offsets",))), ("null_segment_of", dict(null=("segment_of",))),
                         ("g0", dict(g=0)), ("k0", dict(k=0)), ("maxseg0", dict(max_segment=0)), ("maxseg_gt_t", dict(max_segment=553)),
                         ("c0", dict(c=0)), ("c65", dict(c=65)), ("k_t1", dict(k=553))):
            add("segments", t, "refuse", tag, raw=raw)
        add("segments", t, "refuse", "k1025", sizes=(1030, 7), raw=dict(k=1025))
    # A KNOWN SHORTCOMING, pinned as it is: the register kernel's own 160 KiB refusal, although knn_rows.hip could serve the
    # call (the reference's topk has no such limit).  A fix that hands the call over turns this cell into a run cell.
    add("select", "f", "refuse", "lds_n4096c8k895", raw=dict(n=4096, c=8, k=895, b=1))
    add("maxdeg", "f", "refuse", "null_adj", raw=dict(null=("adj",)))
    add("maxdeg", "f", "refuse", "null_out", raw=dict(null=("out",)))
    add("maxdeg", "f", "refuse", "rows0", raw=dict(b=0))
    return cells


CELLS = _build_cells()
MAIN = [c for c in CELLS if c.group == "main"]
BY_ID = {c.id: c for c in CELLS}
REFUSED = [c for c in CELLS if c.expect is not None]
RUN = [c for c in CELLS if c.expect is None]
FULL_ROWS_N = 2048                                               # cells beyond compare a subset of rows
SUBSET_ROWS = 256


# ------------------------------------------------------------------------------------------------ a cell's operands, on the host
def np_dtype(t):
    return np.float32 if t == "f" else np.float64


def _geometry(kind, rng, n, c, dt):
    if kind == "lattice":                                        # integer lattice: every distance an integer, ties everywhere
        return rng.integers(0, 4, size=(n, c)).astype(dt)
    co = rng.standard_normal((n, c)).astype(dt)
    co[0] *= dt(0.01)                                            # node 0 next to the origin, where admitted pad candidates would sit
    if kind == "coincident":                                     # every third node on one point: a tie group of n / 3 at distance 0 / d
        co[::3] = co[0]
    elif kind == "collinear":                                    # equally spaced on a line: node i ties its two neighbours at every distance
        co = (np.arange(n) % 37)[:, None].astype(dt) * np.ones((1, c), dt) * dt(0.5)
    elif kind == "outliers":                                     # GRID_OUT far from the rest: their K-th neighbour is beyond 1e5
        co[list(GRID_OUT)] += dt(1000.0)
    elif kind != "normal":
        raise ValueError(kind)
    return co


def _mask(kind, b, n, k, rng):
    if kind is None:
        return None
    i = np.arange(n)
    if kind == "prefix":                                         # different lengths: a wrong batch stride shows
        lens = [n - (n // 4 if g % 2 else (n // 8 if b == 1 else 0)) for g in range(b)]
        if b == 1 and n > 1:
            lens = [n - max(1, n // 8)]
        return np.stack([i < ln for ln in lens])
    if kind == ROUTE_MASK:
        m = np.ones((b, n), bool)
        m[0, 12] = False
        m[1:, 5:] = False
        return m
    if kind == "one":                                            # node 12 of graph 0 masked, everything else valid
        m = np.ones((b, n), bool)
        m[0, 12] = False
        return m
    if kind == "grid":                                           # graph 0: the last 16 nodes masked; graph 1: five valid nodes, fewer than K
        m = np.ones((b, n), bool)
        m[0, n - 16:] = False
        m[1:, 5:] = False
        return m
    if kind == "under":                                          # graph 1: the planted node masked, and a few more
        m = np.ones((b, n), bool)
        m[1, [UNDER_J, 40, 41]] = False
        return m
    raise ValueError(kind)


UNDER_I, UNDER_J, UNDER_I3, UNDER_J3 = 100, 5, 90, 7             # the planted pairs of the `underflow` cells


def _adjacency(p, n, b, k):
    i = np.arange(n)
    opts = p["adjopt"]
    eye = np.eye(n, dtype=bool)

    def band(w):
        a = np.abs(i[:, None] - i[None, :]) <= w
        if "nodiag" in opts:
            a &= ~eye
        if "special" in opts and n > 60:
            a[10] = False                                        # an isolated row (its own diagonal cleared too)
            for row, deg in ((20, k - 2), (30, k - 1), (40, k)):  # exactly K - 2, K - 1, K adjacent nodes (the diagonal not counted)
                a[row] = False
                a[row, row + 3:row + 3 + max(deg, 0)] = True
                a[row, row] = "nodiag" not in opts
        return a
    if "empty" in opts:
        return np.zeros((n, n), bool)
    if "batched" in opts:
        a = np.stack([band(p["band"] + g) for g in range(b)])
        if "empty1" in opts:
            a[1:] = False
        return a
    return band(p["band"])


def flag_rows(t, b, n, k, c):
    """(B, N) uint8 row flags of a `flagged` cell, by workgroups of the launcher's R rows: workgroup 0 alternates 1 / 0 (other non-zero
    bytes count as set), workgroup 1 is all zero (it returns at once), workgroups 2 and 3 all set, the rest every third row; node 12 (masked in
    graph 0) is flagged; the graphs differ (graph g is graph 0 shifted by g rows), so a wrong batch stride of the flags shows"""
    r = stream_params(t, n, k, c)[0]
    i = np.arange(n)
    f = np.where(i < r, (i + 1) % 2, np.where(i < 2 * r, 0, np.where(i < 4 * r, 1, (i % 3 == 0)))).astype(np.uint8)
    f[12] = 1 if 12 >= 2 * r or 12 < r else f[12]
    f[f != 0] = np.array([1, 255, 2, 128])[np.flatnonzero(f) % 4]
    return np.stack([np.roll(f, g) for g in range(b)])


def segment_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def prepare(cid):
    """The operands of a cell from its id alone (cached: the tests share them and leave them unchanged): .coors (B, N, C) in the cell's
    type ((T, C) for the segments), .mask (B, N) bool or None, .adj (N, N) / (B, N, N) bool or None, .offsets (G + 1,) int64."""
    c = BY_ID[cid]
    p = c.p
    b, n, k, cd = p["b"], p["n"], p["k"], p["c"]
    dt = np_dtype(c.t)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    d = SimpleNamespace(cell=c, b=b, n=n, k=k, c=cd, t=c.t, mask=None, adj=None, offsets=None)
    geoms = p["geom"] if isinstance(p["geom"], tuple) else (p["geom"],) * b
    if c.entry == "segments":
        d.offsets = segment_offsets(p["sizes"])
        co = rng.standard_normal((n, cd)).astype(dt)
        for lo, hi in zip(d.offsets[:-1], d.offsets[1:]):
            if p["geom"] == "segtie" and hi - lo >= 300:         # every other node of the largest graph on one point: > 128 survivors
                co[lo:hi:2] = co[lo]
            elif p["geom"] not in ("normal", "segtie"):
                co[lo:hi] = _geometry(p["geom"], rng, hi - lo, cd, dt)
            if hi - lo >= 2:
                co[lo + 1] = co[lo]                              # two coincident nodes per graph: a tie in every cell
        d.coors = co
        return d
    d.coors = np.stack([_geometry(geoms[g], rng, n, cd, dt) for g in range(b)])
    if n >= 2 and "under" not in p["plant"]:
        d.coors[:, 1] = d.coors[:, 0]                            # two coincident nodes per graph: a tie in every cell
    if "dupx" in p["plant"]:                                     # nodes 50 and 200 of graph 0 share their FIRST coordinate only
        d.coors[0, 200, 0] = d.coors[0, 50, 0]
    if "under" in p["plant"]:
        # node J = I + 1e-30 in every component (squared distance 3e-60: rounds to 0.0), J not adjacent to I and below I's adjacent
        # nodes; node J3 = I3 + 1e-18 (squared distance 3e-36: a normal number, no tie).  Graph 1 has the same pair with J masked.
        d.coors[:, UNDER_I], d.coors[:, UNDER_J] = dt(1e-30), dt(2e-30)
        d.coors[:, UNDER_I3], d.coors[:, UNDER_J3] = dt(1e-18), dt(2e-18)
    d.mask = _mask(p["mask"], b, n, k, rng)
    d.flags = None
    if p["flags"] is not None:
        d.flags = flag_rows(c.t, b, n, k, cd)
    if p["adj"] is not None:
        d.adj = _adjacency(p, n, b, k)
    return d


def compared_rows(cid):
    """the rows of every graph a cell compares: None = all of them (N <= 2048); beyond, at least 256: rows 0 and N - 1, the first and
    last row of two workgroups, every row a claim names, the rest drawn at random"""
    c = BY_ID[cid]
    n = c.p["n"]
    if c.entry in ("segments", "maxdeg") or n <= FULL_ROWS_N:
        return None
    rows = {0, n - 1, 32, 63, (n - 1) // 32 * 32, (n - 1) // 32 * 32 - 1, UNDER_I, UNDER_J, 10, 20, 30, 40}
    rows |= {r for _, where in c.claims for _, r in where}
    rng = np.random.default_rng(n)
    rows |= set(rng.choice(n, size=SUBSET_ROWS, replace=False).tolist())
    return np.array(sorted(rows))


# ------------------------------------------------------------------------------------------------ the specification
MUTATIONS = ("tie_desc", "pads", "mask0", "adj0", "diag", "ltr", "shortcut")
RANK_MASKED, RANK_SELF, RANK_ADJ = 1e5, -1.0, 0.0                # oracle.egnn_oracle


def _sqdist(rel, ltr=False):
    from oracle import egnn_oracle as O
    sq = rel * rel
    if ltr:
        dist = sq[..., 0].copy()
        for q in range(1, sq.shape[-1]):
            dist = dist + sq[..., q]
        return dist
    return O.inner_sum(sq)


def ranking_rows(d, g, rows, mut=None):
    """The ranking values (len(rows), candidates) of graph g's query rows: oracle.egnn_oracle's `pairwise` and `build_ranking` on a
    subset of rows (egnn_pytorch.py:232-233, 237-256) -- tied to those functions bit for bit in the host test.  mut: one deliberate
    error (`MUTATIONS`), to show on the host that a cell would notice it."""
    co = d.coors[g]
    n, dt = d.n, d.coors.dtype.type
    cand = co
    npad = (n + 63) // 64 * 64 if mut == "pads" else n           # pads: candidates j in [N, Npad) admitted, at the origin, unmasked
    if npad > n:
        cand = np.concatenate([co, np.zeros((npad - n, d.c), co.dtype)])
    rows = np.asarray(rows)
    out = np.empty((len(rows), npad), co.dtype)
    for s in range(0, len(rows), 256):
        rr = rows[s:s + 256]
        dist = _sqdist(co[rr][:, None, :] - cand[None, :, :], ltr=mut == "ltr")
        if d.mask is not None:
            mj = d.mask[0 if mut == "mask0" else g]
            mj = np.concatenate([mj, np.ones(npad - n, bool)])
            dist[~(d.mask[g][rr][:, None] & mj[None, :])] = dt(RANK_MASKED)
        if d.adj is not None:
            a = d.adj if d.adj.ndim == 2 else d.adj[0 if mut == "adj0" else g]
            a = np.concatenate([a[rr], np.zeros((len(rr), npad - n), bool)], axis=1)
            diag = np.arange(npad)[None, :] == rr[:, None]
            dist[diag] = dt(RANK_SELF)
            dist[a if mut == "diag" else (a & ~diag)] = dt(RANK_ADJ)
        out[s:s + 256] = dist
    return out


def topk(ranking, k, desc=False):
    """`topk_smallest`: ascending values, ties by ascending index (desc: the mutation, ties by descending index)"""
    if desc:
        n = ranking.shape[-1]
        idx = n - 1 - np.argsort(ranking[..., ::-1], axis=-1, kind="stable")[..., :k]
    else:
        idx = np.argsort(ranking, axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(ranking, idx, axis=-1), idx


def shortcut_rows(d, g, eps=None):
    """(N,) bool: the rows of graph g the adjacency-decided route of knn_select_kernel decides: eps = None, as the kernel had it (first
    coordinates compared for equality); eps = TIE_EPS, as it has it now"""
    c = d.cell
    out = np.zeros(d.n, bool)
    if c.entry != "select" or c.t != "f" or d.adj is None or d.c > 8 or d.n > 4096:
        return out
    if cpl_of(d.n) not in (4, 8, 16, 32) or d.n % 16:
        return out
    a = (d.adj if d.adj.ndim == 2 else d.adj[g]) & ~np.eye(d.n, dtype=bool)
    x = d.coors[g, :, 0]
    order = np.argsort(x, kind="stable")
    gap = np.diff(x[order])                                      # some OTHER node that close: a neighbour in sorted order is
    close = (gap == 0) if eps is None else ((gap == 0) | (gap < x.dtype.type(eps)))
    near = np.zeros(d.n, bool)
    near[order[:-1]] |= close
    near[order[1:]] |= close
    masked = ~d.mask[g] if d.mask is not None else out
    return (a.sum(axis=1) >= d.k - 1) & (masked | ~near)


@functools.lru_cache(maxsize=4)
def _ranking_of(cid, g, mut):
    d = prepare(cid)
    rows = compared_rows(cid)
    return ranking_rows(d, g, np.arange(d.n) if rows is None else rows, mut)


@functools.lru_cache(maxsize=None)
def reference(cid, mut=None):
    """(idx int32, rank) of a cell -- (B, R, K) over `compared_rows` (all rows: R = N), (T, K) for the segments with the empty slots
    (i, +inf), the maximum degree for maxdeg -- from the oracle's ranking in the cell's type.  Cached and shared; nobody writes to it."""
    d = prepare(cid)
    c, k = d.cell, d.k
    dt = d.coors.dtype.type if c.entry != "maxdeg" else None
    if c.entry == "maxdeg":
        a = d.adj.copy()
        if mut == "diag":
            a &= ~np.eye(d.n, dtype=bool)
        return np.int32(a.reshape(-1, d.n).sum(axis=1).max()), None
    if c.entry == "segments":
        t = d.n
        idx = np.tile(np.arange(t, dtype=np.int32)[:, None], (1, k))
        rank = np.full((t, k), np.inf, d.coors.dtype)
        for lo, hi in zip(d.offsets[:-1], d.offsets[1:]):
            if hi > lo:
                seg = SimpleNamespace(coors=d.coors[None, lo:hi], n=int(hi - lo), c=d.c, mask=None, adj=None)
                val, order = topk(ranking_rows(seg, 0, np.arange(hi - lo), mut if mut == "ltr" else None), min(k, hi - lo), desc=mut == "tie_desc")
                idx[lo:hi, :order.shape[1]] = lo + order
                rank[lo:hi, :order.shape[1]] = val
        return idx, rank
    rows = compared_rows(cid)
    rows = np.arange(d.n) if rows is None else rows
    idx = np.empty((d.b, len(rows), k), np.int32)
    rank = np.empty((d.b, len(rows), k), d.coors.dtype)
    for g in range(d.b):
        val, order = topk(_ranking_of(cid, g, mut if mut in ("pads", "mask0", "adj0", "diag", "ltr") else None), k, desc=mut == "tie_desc")
        if mut == "shortcut":
            decided = shortcut_rows(d, g)
            for q, i in enumerate(rows):
                if decided[i]:
                    a = (d.adj if d.adj.ndim == 2 else d.adj[g])[i].copy()
                    a[i] = False
                    order[q] = np.concatenate([[i], np.flatnonzero(a)[:k - 1]])
                    val[q] = np.concatenate([[dt(RANK_SELF)], np.full(k - 1, dt(RANK_ADJ))])
        idx[g], rank[g] = order, val
    return idx, rank


def mutation_applies(cid, mut):
    """can the mutation change anything the cell's entry computes at all?"""
    c = BY_ID[cid]
    p = c.p
    if c.entry == "maxdeg":
        return mut == "diag"
    if c.entry == "segments":
        return mut == "tie_desc" or (mut == "ltr" and c.t == "f" and p["c"] in (5, 6, 7))
    if mut == "tie_desc":
        return True
    if mut == "pads":
        return p["n"] % 64 != 0
    if mut == "mask0":
        return p["mask"] is not None and p["b"] > 1
    if mut == "adj0":
        return p["adj"] is not None and "batched" in p["adjopt"] and p["b"] > 1
    if mut == "diag":
        return p["adj"] is not None and "nodiag" not in p["adjopt"] and "empty" not in p["adjopt"]
    if mut == "ltr":
        return c.t == "f" and p["c"] in (5, 6, 7)
    return p["adj"] is not None and c.inst.kernel == "knn_select_kernel"       # shortcut: must change the underflow cells ONLY


# ------------------------------------------------------------------------------------------------ the routes, from the data
def rank_key(v):
    """csrc/egnn_common.h::egnn_rank_key: the order-preserving unsigned image of a ranking value"""
    u = np.ascontiguousarray(v).view(np.uint32 if v.dtype == np.float32 else np.uint64)
    top = u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1)
    return np.where(u & top, ~u, u | top)


def prune_survivors(keys, k, count_pads):
    """The pruning path of knn_select_kernel and knn_select_segments_kernel (K <= 64): lane l holds the candidates j % 64 == l; M = the
    K-th smallest of the 64 per-lane minima (K > 32: of the 128 smallest-two-per-lane keys) on the key's leading half of the bits, the
    rest of M set; -> the candidates at or below M."""
    n = len(keys)
    kmax = keys.dtype.type(~keys.dtype.type(0))
    full = np.full((n + 63) // 64 * 64, kmax, keys.dtype)
    full[:n] = keys
    lanes = np.sort(full.reshape(-1, 64), axis=0)
    mins = lanes[0]
    if k > 32:
        mins = np.concatenate([mins, lanes[1] if lanes.shape[0] > 1 else np.full(64, kmax, keys.dtype)])
    shift = keys.dtype.type(4 * keys.itemsize)                   # EGNN_KNN_BITS = 16 of 32; PB = KB / 2
    pre = np.sort(mins >> shift)[k - 1]
    m = (pre << shift) | ((keys.dtype.type(1) << shift) - keys.dtype.type(1))
    return int(((full if count_pads else keys) <= m).sum())


def _select_kernel_routes(d, g):
    """routes of every row of graph g on knn_select_kernel: the workgroups' wave loops replayed (a pair is tried from its FIRST row)"""
    n, k = d.n, d.k
    pl = plan("select", "f", n, k, d.c)
    cpl, rpw, cdm = pl.CPL, pl.rows_per_wg, pl.insts[0].args[1]
    keys = rank_key(ranking_rows(d, g, np.arange(n)))
    mask = d.mask[g] if d.mask is not None else np.ones(n, bool)
    surv = [prune_survivors(keys[i], k, True) if k <= 64 else None for i in range(n)]
    routes = [None] * n
    decided = shortcut_rows(d, g, TIE_EPS)

    def single(i):
        if d.adj is None and not mask[i]:
            return ("masked_row",)
        tags = []
        if d.adj is not None:
            a = (d.adj if d.adj.ndim == 2 else d.adj[g])[i].copy()
            a[i] = False
            if cpl not in (4, 8, 16, 32) or n % 16:
                tags.append("adj_refused_shape")
            elif int(a.sum()) < k - 1:
                tags.append("adj_refused_degree")
            elif not decided[i]:
                tags.append("adj_refused_dup")
            else:
                return ("adj_decided",)
        if k <= 64 and surv[i] <= KNN_SURVIVORS:
            tags.append("prune1" if k <= 32 else "prune2")
        else:
            tags.append("radix")
            tags.append("survivors_overflow" if k <= 64 else "k_gt_64")
            if k > 128:
                tags.append("k_gt_128")
        return tuple(tags)

    for row0 in range(0, n, rpw):
        for w in range(KNN_WAVES):
            r = w
            while r < rpw and row0 + r < n:
                i = row0 + r
                if (cdm == 3 and cpl <= 16 and k <= 32 and d.adj is None and r + KNN_WAVES < rpw and i + KNN_WAVES < n and mask[i]
                        and mask[i + KNN_WAVES] and surv[i] <= 64 and surv[i + KNN_WAVES] <= 64):
                    routes[i] = routes[i + KNN_WAVES] = ("pair",)
                    r += 2 * KNN_WAVES
                    continue
                routes[i] = single(i)
                r += KNN_WAVES
    return routes


def stream_route(keys, k, ibp):
    """knn_select_stream_kernel's radix passes over the digits of (key, index): how many digits until the bin that holds the K-th
    candidate holds exactly what is still missing"""
    kd = keys.itemsize
    j = np.arange(len(keys))
    alive = np.ones(len(keys), bool)
    need, lv = k, 0
    while True:
        dig = ((keys >> keys.dtype.type(8 * (kd - 1 - lv))) & keys.dtype.type(0xff)).astype(np.int64) if lv < kd else (j >> (ibp - 8 * (lv - kd + 1))) & 0xff
        h = np.bincount(dig[alive], minlength=256)
        cum = np.cumsum(h)
        b = int(np.searchsorted(cum, need))
        need -= int(cum[b] - h[b])
        alive &= dig == b
        lv += 1
        if h[b] == need:
            return "resolved_in_key_digits" if lv <= kd else "index_digits"


@functools.lru_cache(maxsize=None)
def _routes_of_graph(cid, g):
    d = prepare(cid)
    c, n, k = d.cell, d.n, d.k
    kern = c.inst.kernel
    if c.entry == "segments":
        pl = expected(c.entry, c.t, c.p)
        out = []
        off = d.offsets
        seg_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
        for i in range(n):
            s = seg_of[i]
            lo, hi = int(off[s]), int(off[s + 1])
            r0 = i // SG_ROWS * SG_ROWS
            rl = min(r0 + SG_ROWS, n) - 1
            wlo = min(int(off[seg_of[r0]]), r0)
            whi = min(int(off[seg_of[rl] + 1]), n, wlo + pl.W)
            src = "lds" if (lo >= wlo and hi <= whi) else "streamed"
            if hi - lo <= k:
                out.append(("take_all+" + src,))
                continue
            seg = SimpleNamespace(coors=d.coors[None, lo:hi], n=hi - lo, c=d.c, mask=None, adj=None)
            keys = rank_key(ranking_rows(seg, 0, np.array([i - lo])))[0]
            if k <= 64 and prune_survivors(keys, k, False) <= SG_SURVIVORS:
                out.append((("prune1+" if k <= 32 else "prune2+") + src,))
            else:
                out.append(("radix+" + src,))
        return out
    if kern == "knn_select_kernel":
        return _select_kernel_routes(d, g)
    mask = d.mask[g] if d.mask is not None else np.ones(n, bool)
    if c.entry in ("grid", "grid_csr"):
        # kg_setup_kernel flags a graph with fewer than K valid nodes (or a non-finite / > 1e18 extent, or an overfull cell: not in
        # this table); kg_search_kernel hands a valid row over when its K-th best ranks at 1e5 or beyond while the graph has masked nodes
        nvalid = int(mask.sum())
        finite = bool(np.isfinite(d.coors[g]).all()) and float(np.ptp(d.coors[g][mask], axis=0).max() if nvalid else 0) <= 1e18
        if nvalid < k or nvalid < 1 or not finite:
            return [("handed_to_stream",)] * n
        kth = topk(ranking_rows(d, g, np.arange(n)), k)[0][:, -1]
        return [("handed_to_stream",) if (mask[i] and kth[i] >= 1e5 and nvalid < n) else ("decided_by_grid",) for i in range(n)]
    keys = rank_key(ranking_rows(d, g, np.arange(n)))
    out = []
    for i in range(n):
        if d.adj is None and not mask[i]:
            out.append(("masked_row",))
        elif kern == "knn_select_rows_kernel":
            out.append(("select",))
        else:
            out.append((stream_route(keys[i], k, stream_params(c.t, n, k, d.c)[1]),))
    return out


def route(cid, g, row):
    """the route tags of row `row` of graph g (segments: g = 0, the row of the packed batch) in the cell's kernel"""
    return _routes_of_graph(cid, g)[row]
