"""tests/_select_variants.py on the host: the table covers the grid of the five selection launchers (csrc/knn_select.hip, knn_rows.hip,
knn_stream.hip, knn_segments.hip, knn_grid.hip) exactly once per instantiation AND equals what the compiler instantiated, the restated
thresholds and LDS formulas hold at their boundary values, every coverage claim of a `route` cell is proved from the oracle's keys,
every cell is decidable and sensitive -- shown on the reference alone, by a set of deliberate errors each of which must change what the
cell compares -- no cell's call can address memory it does not own, and the row-subset restatement of the ranking is the oracle's."""
import os
import re
from collections import Counter

import numpy as np
import pytest

from oracle import egnn_oracle as O
from tests import _select_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = V.Inst
N_INST = 50


def test_the_table_is_exactly_the_instantiation_grid():
    insts = [c.inst for c in V.MAIN]
    assert len(insts) == N_INST and len(set(insts)) == N_INST
    assert set(insts) == V.grid()
    assert len({c.id for c in V.CELLS}) == len(V.CELLS)
    assert Counter(i.kernel for i in insts) == Counter(
        knn_select_kernel=15, knn_select_rows_kernel=4, knn_select_stream_kernel=12, knn_select_segments_kernel=4, kg_bbox_kernel=2,
        kg_setup_kernel=2, kg_count_kernel=2, kg_scan_kernel=2, kg_place_kernel=2, kg_search_kernel=4, adj_max_degree_kernel=1)
    for c in V.CELLS:
        got = V.expected(c.entry, c.t, c.p)
        if c.expect is not None:
            assert got == c.expect and c.inst is None and f"refused{-c.expect}" in c.id, c.id
        else:
            assert c.inst == got.insts[c.p["pin"]] and c.inst in V.grid(), c.id
            assert c.id.startswith(V.inst_name(c.inst) + "_"), c.id                # the collected ids name the instantiation
    assert {c.inst for c in V.RUN} == set(insts)
    # MAIN sits at the smallest N of every size class, `top` at the largest
    main = {c.inst.args: c.p["n"] for c in V.MAIN if c.inst.kernel == "knn_select_kernel"}
    top = {c.inst.args: c.p["n"] for c in V.CELLS if c.group == "top"}
    for cpl in (1, 2, 4, 8, 16, 32, 64):
        for cdm in (3, 8):
            assert main[cpl, cdm] == (1 if cpl == 1 else 32 * cpl + 1) and top[cpl, cdm] == 64 * cpl
    assert main[128, 3] == 4097 and top[128, 3] == 8192
    rows = {c.inst.args: (c.p["n"], c.p["c"]) for c in V.MAIN if c.inst.kernel == "knn_select_rows_kernel"}
    assert rows == {("f", 3): (8193, 3), ("f", 8): (4097, 5), ("f", 0): (70, 9), ("d", 0): (70, 3)}
    assert all(c.p["b"] == 2 for c in V.MAIN if c.entry != "segments" and c.p["n"] < 4097)


def test_the_table_equals_what_the_compiler_instantiated():
    """csrc/build.sh leaves the compiler's resource-usage remarks of every translation unit next to its object; the `Function Name:`
    remarks name the kernels that exist (in an anonymous namespace: _ZN12_GLOBAL__N_1<len><name>I<args>E...).  A new instantiation fails
    here until it has a cell."""
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    compiled = set()
    for unit in ("knn_select", "knn_rows", "knn_stream", "knn_segments", "knn_grid"):
        res = os.path.join(pkg, "csrc", "obj", unit + ".res")
        assert os.path.exists(res), f"libegnn_hip.so exists but csrc/obj/{unit}.res does not: build with csrc/build.sh"
        with open(res) as f:
            names = set(re.findall(r"Function Name: (\S+)", "\n".join(line for line in f if "Function Name:" in line)))
        assert names, unit
        for name in names:
            found = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
            assert found, f"{unit}: a kernel this table cannot name: {name}"
            rest = name[found.end():]
            kernel, rest = rest[:int(found.group(1))], rest[int(found.group(1)):]
            args = ()
            if rest.startswith("I"):
                targs = re.match(r"I((?:Li\d+E|Lb[01]E|[fd])+)E", rest)
                assert targs, f"{unit}: template arguments this table cannot read: {name}"
                args = tuple(a if a in "fd" else int(a[2:-1]) for a in re.findall(r"Li\d+E|Lb[01]E|[fd]", targs.group(1)))
            compiled.add(I(kernel, args))
    print(f"compiled: {len(compiled)} instantiations of the selection kernels")
    table = {c.inst for c in V.MAIN}
    assert compiled == table, dict(without_a_cell=sorted(compiled - table), not_compiled=sorted(table - compiled))
    assert len(compiled) == N_INST


def test_the_dispatch_restatement_at_its_thresholds_and_refusals():
    sel = lambda n, c=3, k=1, t="f": V.dispatch("select", t, n, k, c)[0]          # noqa: E731
    # the size classes from both sides
    for top, cpl in ((64, 1), (128, 2), (256, 4), (512, 8), (1024, 16), (2048, 32), (4096, 64)):
        for c, cdm in ((3, 3), (1, 8), (5, 8), (8, 8)):
            assert sel(top, c) == I("knn_select_kernel", (cpl, cdm))
            assert sel(top + 1, c) == (I("knn_select_kernel", (2 * cpl, cdm)) if (top < 4096 or c == 3) else I("knn_select_rows_kernel", ("f", 8)))
    assert sel(8192) == I("knn_select_kernel", (128, 3)) and sel(8193) == I("knn_select_rows_kernel", ("f", 3))
    assert sel(1, 9) == sel(32768, 9) == I("knn_select_rows_kernel", ("f", 0)) and sel(1, 8).kernel == "knn_select_kernel"
    assert sel(32768, 5) == I("knn_select_rows_kernel", ("f", 8)) and sel(32769, 5) == I("knn_select_stream_kernel", ("f", 8, 0, 0))
    assert sel(32769, 3) == I("knn_select_stream_kernel", ("f", 3, 0, 0))
    assert sel(1, 3, t="d") == sel(20000, 64, t="d") == I("knn_select_rows_kernel", ("d", 0))
    # the 160 KiB hand-over of knn_rows_launch: up8(N key bytes) + K (key + 4) + 40
    assert V.rows_lds("f", 40934, 8) == 163736 + 64 + 40 == V.LDS_MAX and sel(40934, 9, 8) == I("knn_select_rows_kernel", ("f", 0))
    assert V.rows_lds("f", 40935, 8) == 163744 + 104 and sel(40935, 9, 8) == I("knn_select_stream_kernel", ("f", 0, 0, 0))
    assert V.rows_lds("d", 20464, 8) == 163712 + 96 + 40 and sel(20464, 3, 8, "d") == I("knn_select_stream_kernel", ("d", 0, 0, 0))
    assert V.rows_lds("d", 20463, 8) == 163704 + 136 == V.LDS_MAX and sel(20463, 3, 8, "d") == I("knn_select_rows_kernel", ("d", 0))
    opt = lambda *a, **kw: V.plan(*a, **kw).opt_in                                 # noqa: E731
    assert V.rows_lds("f", 16370, 8) == 65584 and opt("select", "f", 16370, 8, 9) and not opt("select", "f", 16350, 8, 9)
    # the register kernel's LDS by hand at three cells, its opt-in and its own refusal
    assert V.select_lds(2048, 3, 3) == 2048 * 13 + 8 + 4 * 128 * 8 + 8 == 30736
    assert V.select_lds(100, 8, 5) == 128 * 21 + 8 + 4096 + 8 == 6800
    assert V.select_lds(130, 130, 3) == 192 * 13 + 8 + 4 * 130 * 8 + 8 == 6672
    assert V.select_lds(4672, 8, 3) == 64848 and not opt("select", "f", 4672, 8, 3)
    assert V.select_lds(4736, 8, 3) == 65680 and opt("select", "f", 4736, 8, 3)
    assert V.select_lds(4096, 894, 8) == 163792 and sel(4096, 8, 894) == I("knn_select_kernel", (64, 8))
    assert V.select_lds(4096, 895, 8) == 163856 and V.dispatch("select", "f", 4096, 895, 8) == V.E_UNSUPPORTED
    # the stream: R rows per workgroup, IBP index bits, LDS
    sp = V.stream_params
    assert sp("f", 300, 8, 3) == (16, 16, 464 + 16448 + 512 + 512 + 192) and sp("f", 256, 8, 3)[1] == 8 and sp("f", 257, 8, 3)[1] == 16
    assert sp("f", 65536, 8, 3)[1] == 16 and sp("f", 65537, 8, 3)[1] == 24 and sp("f", 2, 1, 3)[1] == 8
    assert [sp("f", 2000, k, 3)[0] for k in (512, 513, 1024)] == [16, 8, 8]
    assert [sp("d", 2000, k, 3)[0] for k in (341, 342, 682, 683, 1024)] == [16, 8, 8, 4, 4]
    assert sp("d", 70, 8, 64)[2] == 16 * 32 + 16 + 16448 + 1024 + 512 + 16 * 64 * 8
    assert sp("f", 2000, 378, 3)[2] == 17104 + 128 * 378 == 65488 and not opt("stream", "f", 2000, 378, 3) and opt("stream", "f", 2000, 379, 3)
    for entry, csr in (("stream", 0), ("csr", 1)):
        assert V.dispatch(entry, "f", 300, 8, 3) == (I("knn_select_stream_kernel", ("f", 3, 0, csr)),)
        assert V.dispatch(entry, "f", 300, 8, 8) == (I("knn_select_stream_kernel", ("f", 8, 0, csr)),)
        assert V.dispatch(entry, "f", 300, 8, 9) == (I("knn_select_stream_kernel", ("f", 0, 0, csr)),)
        assert V.dispatch(entry, "d", 300, 8, 3) == (I("knn_select_stream_kernel", ("d", 0, 0, csr)),)
        assert V.dispatch(entry, "f", 300, 8, 3, flagged=True) == (I("knn_select_stream_kernel", ("f", 3, 1, csr)),)
        assert V.dispatch(entry, "f", 300, 8, 5, flagged=True) == V.E_UNSUPPORTED
    # the segments: Lp, W and the LDS bytes
    gp = V.segments_params
    assert gp("f", 8, 3, 300) == (128, 632, 632 * 12 + 8192) and gp("f", 8, 3, 10000) == (128, 4778, 57336 + 8192)
    assert gp("f", 129, 3, 300)[0] == 130 and gp("f", 128, 3, 300)[0] == 128 and gp("f", 8, 3, 300, 64)[1] == 64
    assert gp("d", 8, 3, 10000) == (128, (65536 - 4 * 2584 - 8) // 24, V.up8(((65536 - 4 * 2584 - 8) // 24) * 24) + 4 * 2584)
    assert gp("f", 1024, 9, 10000)[1] == (65536 - 4 * V.up8(1024 * 8 + 1024 + 36) - 8) // 36
    assert all(V.plan("segments", t, 2000, k, c, g=7, max_segment=300).lds <= V.LDS_OPT_IN for t in "fd" for k in (1, 1024) for c in (1, 64))
    # the argument checks, in the launchers' order
    for entry in ("select", "stream", "csr"):
        for t in "fd":
            d = lambda **kw: V.dispatch(entry, t, kw.pop("n", 70), kw.pop("k", 8), kw.pop("c", 3), **kw)     # noqa: E731
            assert d(null=("coors",), b=0) == V.E_NULLPTR and d(b=0, c=0) == V.E_SHAPE and d(k=0, c=65) == V.E_SHAPE
            assert d(c=0, k=71) == V.E_UNSUPPORTED and d(c=65) == V.E_UNSUPPORTED and d(k=71) == V.E_K_GT_N
            assert d(n=1100, k=1025) == V.E_UNSUPPORTED and d(n=1000, k=1025) == V.E_K_GT_N and d(b=65536) == V.E_UNSUPPORTED
            assert not isinstance(d(n=1100, k=1024, b=65535), int)
    assert V.dispatch("csr", "f", 70, 8, 3, null=("rowptr", "coors")) == V.E_NULLPTR
    assert V.dispatch("csr", "f", 70, 8, 3, rp_stride=70, b=0) == V.E_SHAPE and not isinstance(V.dispatch("csr", "f", 70, 8, 3, rp_stride=71), int)
    for entry in ("grid", "grid_csr"):
        for t in "fd":
            d = lambda **kw: V.dispatch(entry, t, kw.pop("n", 200), kw.pop("k", 8), kw.pop("c", 3), **kw)    # noqa: E731
            assert d(null=("ws",), k=0) == V.E_NULLPTR and d(k=201, c=2) == V.E_SHAPE and d(c=2, ws_short=1) == V.E_UNSUPPORTED
            assert d(k=129) == V.E_UNSUPPORTED and d(k=128, ws_short=1, ws_misalign=8) == V.E_SHAPE and d(ws_misalign=8) == V.E_ALIGN
            assert len(d(k=128)) == 7 and d(k=128)[-1].args[2] == 1
    assert V.grid_layout("f", 2, 96).flag == V.grid_layout("d", 2, 96).flag == 256 + V.up256(2 * 64 * 16 * 8)
    assert V.grid_layout("d", 2, 96).total - V.grid_layout("f", 2, 96).total == V.up256(2 * 96 * 32) - V.up256(2 * 96 * 16)
    sg = lambda **kw: V.dispatch("segments", "f", kw.pop("n", 552), kw.pop("k", 8), kw.pop("c", 3), **kw)   # noqa: E731
    assert sg(null=("offsets",), g=0) == V.E_NULLPTR and sg(g=0, c=0) == V.E_SHAPE and sg(max_segment=553) == V.E_SHAPE
    assert sg(k=553) == V.E_K_GT_N and sg(k=1025, n=2000) == V.E_UNSUPPORTED and sg(c=65) == V.E_UNSUPPORTED
    assert V.dispatch("maxdeg", "f", 70, 1, 1, null=("out",)) == V.E_NULLPTR and V.dispatch("maxdeg", "f", 70, 1, 1, b=0) == V.E_SHAPE


def test_the_library_agrees_with_the_restated_grid_workspace():
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    for b, n in ((1, 1), (2, 96), (3, 300), (2, 70000)):
        assert lib.egnn_knn_grid_workspace_bytes(b, n, 8) == V.grid_layout("f", b, n).total
        assert lib.egnn_knn_grid_workspace_bytes_f64(b, n, 8) == V.grid_layout("d", b, n).total
        assert lib.egnn_knn_grid_rowflag_offset_f64(b, n) == V.grid_layout("d", b, n).flag == V.grid_layout("f", b, n).flag


def test_the_cells_beside_the_grid_are_all_there():
    def has(entry, t, group, **kw):
        return any(c.entry == entry and c.t == t and c.group == group and all(c.p[k] == v for k, v in kw.items()) for c in V.CELLS)
    for k in (1, 32, 33, 64, 65, 128, 129, 130):
        assert has("select", "f", "kclass", n=130, k=k, c=3) and has("stream", "f", "kclass", n=130, k=k)
    for entry in ("select", "stream", "segments"):
        assert has(entry, "f", "kclass", k=1024)
    for c in (1, 2, 4, 5, 7, 8):
        assert {cc.inst.args for cc in V.CELLS if cc.group == "cdim" and cc.p["c"] == c and cc.t == "f"} >= {
            (2, 8), ("f", 8), ("f", 8, 0, 0)}, c
    for c in (9, 16, 33, 64):
        for t in "fd":
            assert {cc.inst for cc in V.CELLS if cc.group == "cdim" and cc.p["c"] == c and cc.t == t} == {
                I("knn_select_rows_kernel", (t, 0)), I("knn_select_stream_kernel", (t, 0, 0, 0)), I("knn_select_segments_kernel", (t, 0))}
    for cpl, n in ((1, 61), (8, 301), (64, 2101)):
        for cdm in (3, 8):
            tags = {tag for c in V.CELLS if c.group == "route" and c.inst == I("knn_select_kernel", (cpl, cdm)) for tag, _ in c.claims}
            want = {"prune1", "prune2", "masked_row", "adj_refused_shape"} | ({"pair"} if (cdm == 3 and cpl <= 16) else set())
            if cpl > 1:
                want |= {"survivors_overflow", "k_gt_64", "k_gt_128"}
            if cpl == 8:
                want |= {"adj_decided", "adj_refused_degree", "adj_refused_dup"}
            assert tags >= want, (cpl, cdm, want - tags)
    seg = {tag for c in V.CELLS if c.group == "route" and c.entry == "segments" for tag, _ in c.claims}
    assert seg == {f"{a}+{s}" for a in ("take_all", "prune1", "prune2", "radix") for s in ("lds", "streamed")}
    for kern, entries, tags in (("knn_select_rows_kernel", ("select",), {"masked_row", "select"}),
                                ("knn_select_stream_kernel", ("stream", "csr"), {"masked_row", "index_digits", "resolved_in_key_digits"}),
                                ("kg_search_kernel", ("grid", "grid_csr"), {"decided_by_grid", "handed_to_stream"})):
        assert {tag for c in V.CELLS if c.inst is not None and c.inst.kernel == kern and c.entry in entries for tag, _ in c.claims} == tags
    codes = {(c.entry, c.expect) for c in V.REFUSED}
    for entry in V.ALL_PAIRS:
        assert {(entry, V.E_NULLPTR), (entry, V.E_SHAPE), (entry, V.E_UNSUPPORTED)} <= codes
        assert ((entry, V.E_K_GT_N) in codes) == (not entry.startswith("grid"))
    assert {("grid", V.E_ALIGN), ("grid_csr", V.E_ALIGN), ("segments", V.E_K_GT_N), ("maxdeg", V.E_NULLPTR), ("maxdeg", V.E_SHAPE)} <= codes
    under = [c for c in V.CELLS if c.group == "underflow"]
    assert {c.inst.args for c in under if c.inst.kernel == "knn_select_kernel"} >= {(4, 3), (8, 3), (16, 3), (32, 3), (4, 8), (8, 8), (16, 8), (32, 8)}
    assert {c.inst.kernel for c in under} == {"knn_select_kernel", "knn_select_rows_kernel", "knn_select_stream_kernel"}


def test_every_coverage_claim_is_proved_from_the_oracles_keys():
    n_claims = 0
    for c in V.CELLS:
        if not c.claims:
            continue
        assert c.expect is None, c.id
        rows = V.compared_rows(c.id)
        for tag, where in c.claims:
            assert where, (c.id, tag)
            for g, row in where:
                assert tag in V.route(c.id, g, row), (c.id, tag, g, row, V.route(c.id, g, row))
                assert rows is None or row in rows, (c.id, row)              # ... and the GPU test compares that row
                n_claims += 1
        d = V.prepare(c.id)
        seen = {V.route(c.id, g, r) for g in range(d.b if c.entry != "segments" else 1) for r in range(d.n)}
        # one route for everything would be wrong somewhere -- except where the kernel HAS one route: the register kernel at N <= 128
        # with an adjacency (no early return, K <= 64 and never more than 128 survivors)
        assert len(seen) >= 2 or (c.inst.kernel == "knn_select_kernel" and d.n <= 128 and d.adj is not None), (c.id, seen)
    print(f"{n_claims} claimed rows proved")
    assert n_claims >= 200


def _differs(a, b):
    return any(x is not None and not np.array_equal(x, y) for x, y in zip(a, b))


def test_every_cell_is_decidable_and_sensitive_on_the_reference():
    matrix = Counter()
    flipped_by = Counter()
    per_cell = {}
    for c in V.RUN:
        ref = V.reference(c.id)
        d = V.prepare(c.id)
        if c.entry == "maxdeg":
            assert int(ref[0]) == 2 * c.p["band"] + 3                            # (graph 1's band is one wider; the diagonal counts)
        else:
            idx, rank = ref
            assert idx.dtype == np.int32 and rank.dtype == V.np_dtype(c.t) and not np.isnan(rank).any(), c.id
            # 1. the selection is unique under the (value, index) policy: no two selected composites of a row are equal
            flat = idx.reshape(-1, idx.shape[-1])
            if c.entry == "segments":
                real = np.isfinite(rank.reshape(flat.shape))
                assert all(len(set(r[m])) == int(m.sum()) for r, m in zip(flat, real)), c.id
                sizes = np.repeat(np.diff(d.offsets), np.diff(d.offsets))
                assert np.array_equal(real.sum(axis=1), np.minimum(sizes, d.k)), c.id
            else:
                srt = np.sort(flat, axis=1)
                assert flat.shape[1] == 1 or bool((srt[:, 1:] != srt[:, :-1]).all()), c.id
                assert int(flat.min()) >= 0 and int(flat.max()) < d.n, c.id
            r2 = rank.reshape(flat.shape)
            assert bool((r2[:, 1:] >= r2[:, :-1]).all()), c.id
            # 2. a tie cell has a tie group straddling slot K
            if c.group == "tie":
                straddle = spans = 0
                for g in range(d.b if c.entry != "segments" else 1):
                    if c.entry == "segments":
                        lo, hi = int(d.offsets[2]), int(d.offsets[3])
                        seg = V.SimpleNamespace(coors=d.coors[None, lo:hi], n=hi - lo, c=d.c, mask=None, adj=None)
                        val = V.topk(V.ranking_rows(seg, 0, np.arange(hi - lo)), d.k + 1)[0]
                    else:
                        ranking = V.ranking_rows(d, g, np.arange(d.n))
                        val = V.topk(ranking, d.k + 1)[0]
                        # ... and the members of such a group lie on both sides of the kernel's own boundaries: two lanes and two
                        # key registers (j % 64, j // 64) in the register kernel; two thread slices of per = ceil(N / 256)
                        # candidates and two waves (64 slices) in the rows kernel
                        for i in np.flatnonzero(val[:, d.k - 1] == val[:, d.k]):
                            j = np.flatnonzero(ranking[i] == val[i, d.k - 1])
                            if c.inst.kernel == "knn_select_kernel":
                                spans += len(set(j % 64)) > 1 and len(set(j // 64)) > 1
                            elif c.inst.kernel == "knn_select_rows_kernel":
                                per = (d.n + 255) // 256
                                spans += len(set(j // per)) > 1 and len(set(j // per // 64)) > 1
                    straddle += int((val[:, d.k - 1] == val[:, d.k]).sum())
                assert straddle > 0, c.id
                if c.inst.kernel in ("knn_select_kernel", "knn_select_rows_kernel"):
                    assert spans > 0, c.id
        # 3. every deliberate error that applies to the cell's entry is tried; the cell must notice at least one, and the errors a
        # cell is named for in particular
        hits = []
        for mut in V.MUTATIONS:
            if not V.mutation_applies(c.id, mut):
                continue
            matrix[mut, "applies"] += 1
            if _differs(V.reference(c.id, mut), ref):
                hits.append(mut)
                matrix[mut, "flips"] += 1
                flipped_by[mut] += 1
        per_cell[c.id] = hits
        if c.p["n"] == 1:
            continue                                                             # one candidate per row: nothing to get wrong but the value
        assert hits, f"{c.id}: no mutation of the reference changes what this cell compares"
        if c.group == "underflow" and c.inst.kernel == "knn_select_kernel" and c.inst.args[0] in (4, 8, 16, 32):
            assert "shortcut" in hits, c.id                                      # the cell would have caught the decided route's tie
        else:
            assert "shortcut" not in hits, c.id                                  # everywhere else the decided route is the reference, bit for bit
        if c.group == "tie":
            assert "tie_desc" in hits, c.id
        if c.group == "adjform" and "batched" in c.p["adjopt"]:
            assert "adj0" in hits, c.id
        if c.group == "cdim" and c.t == "f" and c.p["c"] in (5, 7):
            assert "ltr" in hits, c.id
        if c.group == "main" and c.entry in V.ALL_PAIRS and c.p["b"] > 1 and c.p["n"] > 1:
            assert "mask0" in hits, c.id                                         # a wrong batch stride of the mask shows
        if c.group == "main" and c.inst.kernel == "knn_select_kernel" and c.p["n"] > 1:
            assert "pads" in hits, c.id                                          # the column of pad candidates at N % 64 == 1
    print("mutation x cells:  " + "  ".join(f"{m}: flips {matrix[m, 'flips']} of {matrix[m, 'applies']}" for m in V.MUTATIONS))
    print(f"cells: {len(per_cell)}, noticed by the fewest mutations: {min((len(h), cid) for cid, h in per_cell.items())}")
    for mut in V.MUTATIONS:
        assert flipped_by[mut] >= 1, mut
    assert flipped_by["shortcut"] == 8 and matrix["shortcut", "applies"] >= 30   # CPL 4, 8, 16, 32 x CDM 3, 8, of every adjacency cell
    # the underflow cells without the shortcut expect the same thing: the expectation is the family's, not one kernel's
    for c in V.RUN:
        if c.group == "underflow":
            idx, rank = V.reference(c.id)
            k = c.p["k"]
            assert c.p["n"] <= V.FULL_ROWS_N
            assert list(idx[0, V.UNDER_I]) == [V.UNDER_I, V.UNDER_J, V.UNDER_I - 2, V.UNDER_I - 1][:k], c.id      # the lower index takes a slot
            assert list(rank[0, V.UNDER_I]) == [-1.0, 0.0, 0.0, 0.0], c.id
            assert list(idx[1, V.UNDER_I]) == [V.UNDER_I, V.UNDER_I - 2, V.UNDER_I - 1, V.UNDER_I + 1], c.id      # masked: it must not
            assert list(idx[0, V.UNDER_I3]) == [V.UNDER_I3, V.UNDER_I3 - 2, V.UNDER_I3 - 1, V.UNDER_I3 + 1], c.id # 3e-36: a normal number
            d = V.prepare(c.id)
            rel = d.coors[0, V.UNDER_I] - d.coors[0, V.UNDER_J]
            assert bool((rel != 0).all()) and float(V._sqdist(rel)) == 0.0
            rel3 = d.coors[0, V.UNDER_I3] - d.coors[0, V.UNDER_J3]
            assert float(V._sqdist(rel3)) >= float(np.finfo(np.float32).tiny)
            assert abs(float(rel[0])) < V.TIE_EPS                                # what the kernel's pre-pass tests on the first coordinate


def test_no_call_can_address_memory_it_does_not_own():
    """every extent a kernel reads or writes, recomputed from the cell's arguments and compared with what `prepare` allocates (the GPU
    test allocates the outputs from the same numbers, and the grid's workspace from the entry's own *_workspace_bytes)"""
    for c in V.RUN:
        d, p = V.prepare(c.id), c.p
        pl = V.expected(c.entry, c.t, p)
        assert not isinstance(pl, int) and pl.lds <= V.LDS_MAX, c.id
        assert d.coors.dtype == V.np_dtype(c.t) and d.coors.flags["C_CONTIGUOUS"], c.id
        if c.entry == "segments":
            assert d.coors.shape == (sum(p["sizes"]), p["c"]) and d.offsets[0] == 0 and d.offsets[-1] == d.n, c.id
            assert bool((np.diff(d.offsets) >= 0).all()) and len(d.offsets) == len(p["sizes"]) + 1
            assert pl.Lp >= max(p["k"], V.SG_SURVIVORS) and pl.Lp % 2 == 0 and pl.W >= 0
            continue
        assert d.coors.shape == (p["b"], p["n"], p["c"]) and 1 <= p["k"] <= p["n"] and p["k"] <= 1024, c.id
        assert d.mask is None or (d.mask.shape == (p["b"], p["n"]) and d.mask.dtype == bool), c.id
        if d.adj is not None:
            assert d.adj.dtype == bool and d.adj.shape in ((p["n"], p["n"]), (p["b"], p["n"], p["n"])), c.id
        if c.entry in ("csr", "grid_csr"):
            # rowptr as the entries read it: (N + 1) absolute offsets per graph, the last one within the column array
            a = d.adj.reshape(-1, p["n"])
            rowptr = np.concatenate([[0], np.cumsum(a.sum(axis=1))])
            assert rowptr[-1] == int(a.sum()) and len(rowptr) == a.shape[0] + 1 and a.shape[0] in (p["n"], p["b"] * p["n"]), c.id
        if c.entry in ("grid", "grid_csr"):
            assert p["c"] == 3 and p["k"] <= V.KG_KMAX and pl.ws_bytes == V.grid_layout(c.t, p["b"], p["n"]).total, c.id
            assert V.grid_layout(c.t, p["b"], p["n"]).flag + p["b"] * p["n"] <= pl.ws_bytes
        rows = V.compared_rows(c.id)
        if rows is not None:
            assert len(rows) >= V.SUBSET_ROWS and {0, p["n"] - 1} <= set(rows.tolist()) and int(rows.max()) < p["n"], c.id
        assert p["b"] * p["n"] * p["k"] <= 2 * 1024 * 1024 + 1, c.id              # every case stays a handful of small launches
    for c in V.REFUSED:                                                          # a refusal is decided before any launch: nothing to own
        assert isinstance(V.expected(c.entry, c.t, c.p), int), c.id


def test_the_row_subset_restatement_is_the_oracles_ranking():
    """`ranking_rows` + `topk` against oracle.egnn_oracle's pairwise / build_ranking / topk_smallest (which
    tests/test_oracle_vs_reference.py ties to torch bit for bit), on every all-pairs cell of at most 304 nodes; `rank_key` orders as
    the values do"""
    seen = 0
    for c in V.RUN:
        if c.entry not in V.ALL_PAIRS or c.p["n"] > 304:
            continue
        d = V.prepare(c.id)
        _, dist = O.pairwise(d.coors)
        ranking, _ = O.build_ranking(dist, d.mask, d.adj)
        val, idx = O.topk_smallest(ranking, d.k)
        got_idx, got_val = V.reference(c.id)
        assert np.array_equal(idx.astype(np.int32), got_idx), c.id
        assert np.array_equal(val.view(np.uint32 if c.t == "f" else np.uint64), got_val.view(np.uint32 if c.t == "f" else np.uint64)), c.id
        seen += 1
    assert seen >= 100
    for dt in (np.float32, np.float64):
        v = np.array([-1.0, -0.0, 0.0, np.finfo(dt).tiny / 4, 1e-30, 0.5, 1.0, 1e5, np.inf], dt)
        key = V.rank_key(v)
        assert bool((key[1:] > key[:-1]).all())


def test_the_flag_arrays_of_the_flagged_cells_mix_inside_a_workgroup():
    cells = [c for c in V.RUN if c.group == "flagged"]
    assert {c.inst for c in cells} == {i for i in V.grid() if i.kernel == "knn_select_stream_kernel" and i.args[2] == 1}
    for c in cells:
        d = V.prepare(c.id)
        r = V.expected(c.entry, c.t, c.p).R
        assert d.flags.shape == (d.b, d.n) and d.flags.dtype == np.uint8 and r in (8, 16), c.id
        for g in range(d.b):
            f = d.flags[g] != 0
            groups = [f[s:s + r] for s in range(0, d.n, r)]
            assert any(w.any() and not w.all() for w in groups) and any(not w.any() for w in groups) and any(w.all() for w in groups), c.id
            assert len(groups[-1]) < r or d.n % r == 0
        assert d.b == 1 or not np.array_equal(d.flags[0], d.flags[1]), c.id
        assert set(np.unique(d.flags).tolist()) > {0, 1}                         # any non-zero byte is a set flag
    n100 = [V.prepare(c.id) for c in cells if c.p["n"] == 100]
    assert all(d.flags[0, 12] != 0 and not d.mask[0, 12] and d.n % 16 != 0 for d in n100) and len(n100) == 4       # a flagged masked row; a partial workgroup
