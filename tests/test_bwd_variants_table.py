"""tests/_bwd_variants.py on the host: the table covers the dispatcher's grid of csrc/edge_bwd.hip exactly once per instantiation AND equals
what the compiler instantiated, every boundary value, width, slab rule and list shape occurs often enough, no cell's call can address
memory it does not own, and every cell meets the preconditions that make its GPU comparison (tests/test_gpu_bwd_variants.py) decidable,
on the float64 reference alone."""
import os
import re
from collections import Counter

import pytest

from tests import _bwd_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Compiled into the product and launched neither by `autograd._edge_contract_fused` (d/d W_s, d/d s by source, d/d W_2 by destination) nor
# by any test before this table: the ten kernels that write the partial rows only and the two S = 1 kernels that carry everything.  Reachable
# only by a direct call of `_ops.edge_bwd_pass` / egnn_edge_bwd_pass_f32.
DIRECT_ONLY = sorted(
    [V.Instantiation(nm, st, False, False, 8, False, drop, False) for nm, st in V.NM_ST for drop in (False, True)]
    + [V.Instantiation(1, 1, True, True, 8, False, drop, False) for drop in (False, True)])


def _s(c):
    return 2 * c.kw["fourier_features"] + 1 + c.kw["edge_dim"]


def test_the_table_is_exactly_the_instantiation_grid():
    insts = [c.inst for c in V.MAIN]
    assert len(insts) == 42 and len(set(insts)) == 42
    assert set(insts) == V.grid()
    assert len({c.id for c in V.CELLS}) == len(V.CELLS)
    for c in V.CELLS:
        assert _s(c) == c.s
        assert c.inst == V.instantiation(c.s, c.want_w2, c.want_s, c.row_pairs, c.drop is not None, c.by_dest, c.k), c.id
        assert c.inst in V.grid() and V.family(c.inst) == c.fam, c.id
        assert "I" + "-".join(str(int(v)) for v in c.inst) + "_" in c.id           # the collected ids name the instantiation
    assert {c.inst for c in V.CELLS} == set(insts)
    assert Counter(V.family(i) for i in insts) == Counter(w2=10, ss=10, pair=10, none=10, both=2)
    assert {i.CH for i in insts if V.family(i) == "w2"} == {V.CH_W2} and {i.CH for i in insts if V.family(i) != "w2"} == {V.CH_S}
    assert all(i.DSM == (i.SS and i.NM >= 6) for i in insts)


def test_the_dispatch_restatement_at_its_thresholds_and_refusals():
    assert [V.NM_ST[V.s_class(s)] for s in (1, 2, 4, 5, 6, 8, 9, 16)] == [(1, 1), (3, 4), (3, 4), (4, 5), (6, 2), (6, 2), (12, 2), (12, 2)]
    assert V.instantiation(1, 1, 1, 0, 0) == (1, 1, True, True, 8, False, False, False)
    assert V.instantiation(5, 1, 0, 0, 1) == (4, 5, True, False, 6, False, True, False)
    assert V.instantiation(6, 0, 1, 1, 0) == (6, 2, False, True, 8, True, False, True)
    assert V.instantiation(9, 0, 1, 0, 1) == (12, 2, False, True, 8, False, True, True)
    assert [V.instantiation(s, 1, 1, 0, d) for s in (2, 5, 6, 16) for d in (0, 1)] == [V.E_UNSUPPORTED] * 8
    assert V.instantiation(2, 0, 1, 1, 0, by_dest=True) == V.E_SHAPE
    assert V.instantiation(2, 0, 1, 1, 0, k=16) == V.E_SHAPE and V.instantiation(2, 0, 1, 1, 0, k=33) == V.E_SHAPE
    assert V.instantiation(2, 1, 0, 1, 0) == V.E_UNSUPPORTED and V.instantiation(1, 0, 0, 1, 1) == V.E_UNSUPPORTED
    assert V.instantiation(6, 0, 1, 0, 0, has_wsth=False) == V.E_NULLPTR and V.instantiation(5, 0, 1, 0, 0, has_wsth=False).NM == 4
    # the column chunks: fewer than a chunk, exactly one, 9 = 5 + 4 (not 8 + 1), 13 = 5 + 4 + 4 under CH_W2 and 7 + 6 under CH_S
    assert V.chunks(2, 8) == [(0, 2)] and V.chunks(2, 6) == [(0, 2)]
    assert V.chunks(8, 8) == [(0, 8)] and V.chunks(8, 6) == [(0, 4), (4, 4)]
    assert V.chunks(9, 8) == [(0, 5), (5, 4)] and V.chunks(9, 6) == [(0, 5), (5, 4)]
    assert V.chunks(13, 8) == [(0, 7), (7, 6)] and V.chunks(13, 6) == [(0, 5), (5, 4), (9, 4)]
    for steps in range(1, 70):
        for ch in (V.CH_S, V.CH_W2):
            parts = V.chunks(steps, ch)
            assert [p[0] for p in parts] == [sum(q[1] for q in parts[:i]) for i in range(len(parts))]
            assert sum(p[1] for p in parts) == steps and all(1 <= p[1] <= ch for p in parts)
    # the slabs: the product's rule never leaves one empty; 35 slabs are two groups of workgroups per chunk, the second partial
    assert V.slabs(35, 35) == (1, 64, 2) and V.slabs(35, 5) == (7, 32, 1)
    for rounds in range(1, 200):
        for r in V.R_VALUES + (V.ROUNDS_PER_SLAB,):
            n_slabs = V.n_slabs_of(rounds, r)
            assert (n_slabs - 1) * V.slabs(rounds, n_slabs)[0] < rounds
    assert V.lds_bytes(V.Instantiation(12, 2, False, True, 8, False, False, True)) == 110592
    assert V.lds_bytes(V.Instantiation(1, 1, True, False, 6, False, False, False)) == 6 * 2048 + 6 * 512 + 18432


def _compiled(res_text, name):
    return sorted(set(re.findall(name + r"I((?:L[ib]\d+E)+)E", res_text)))


def _args(mangled):
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", mangled))


def test_the_table_equals_what_the_compiler_instantiated():
    """csrc/build.sh leaves the compiler's resource-usage remarks of every translation unit next to its object; the `Function Name:`
    remarks of edge_bwd.hip name the kernels that exist.  A new `launch_v<...>` line fails here until it has a cell."""
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    res = os.path.join(pkg, "csrc", "obj", "edge_bwd.res")
    assert os.path.exists(res), "libegnn_hip.so exists but csrc/obj/edge_bwd.res does not: build with csrc/build.sh"
    with open(res) as f:
        text = "\n".join(line for line in f if "Function Name:" in line)
    kernels = {_args(m) for m in _compiled(text, "edge_bwd_kernel")}
    preps = {_args(m) for m in _compiled(text, "edge_bwd_prep_kernel")}
    print(f"compiled: {len(kernels)} edge_bwd_kernel + {len(preps)} edge_bwd_prep_kernel instantiations")
    table = {tuple(int(v) for v in c.inst) for c in V.MAIN}
    assert kernels == table, dict(without_a_cell=sorted(kernels - table), not_compiled=sorted(table - kernels))
    assert len(kernels) == 42
    assert preps == {(nm,) for nm, _ in V.NM_ST} and len(preps) == 5


def test_reachability_under_the_default_split():
    insts = {c.inst for c in V.MAIN}
    reached = {i for i in insts if V.default_split_reaches(i)}
    assert len(reached) == 30 and sorted(insts - reached) == DIRECT_ONLY and len(DIRECT_ONLY) == 12
    # the product's own calls, restated: by source ws_nat (+ row_pairs where 16 < K <= 32), by destination want_w2 -- with and without dropout
    calls = set()
    for s in (1, 2, 5, 6, 9):
        for drop in (False, True):
            for k in (8, 24, 40):
                calls.add(V.instantiation(s, False, True, 16 < k <= 32, drop, False, k))
                calls.add(V.instantiation(s, True, False, False, drop, True, k))
    assert calls == reached


def test_coverage_counts():
    cells = V.CELLS
    s_count = Counter(c.s for c in cells)
    assert set(s_count) == {1, 2, 4, 5, 6, 8, 9, 16} and all(v >= 3 for v in s_count.values()), s_count
    for s in (4, 5, 6, 8, 9, 16):                                                # realised both ways
        assert {c.kw["fourier_features"] == 0 for c in cells if c.s == s} == {True, False}, s
    fam_drop = {(f, d) for f in V.FAMILIES for d in (False, True)}
    for steps in V.STEPS:
        assert {c.inst.CH for c in cells if c.steps == steps} == {V.CH_S, V.CH_W2}, steps
    with_all = [steps for steps in V.STEPS if {(c.fam, c.drop is not None) for c in cells if c.steps == steps} == fam_drop]
    assert 2 in with_all and len(with_all) >= 2, with_all
    for r in V.R_VALUES:
        assert {c.fam for c in cells if c.r == r} == set(V.FAMILIES), r
    assert {c.k for c in cells if c.fam == "pair"} == set(V.K_PAIR)
    assert {c.k for c in cells if c.fam == "ss" and not c.by_dest} == set(V.K_SRC)
    assert {c.k for c in cells if not c.by_dest} >= set(V.K_SRC) | set(V.K_PAIR)
    by_dest_fams = {c.fam for c in cells if c.by_dest}
    assert by_dest_fams == {"w2", "ss", "none", "both"}
    assert {c.fam for c in cells if c.hub} == by_dest_fams and all(c.by_dest for c in cells if c.hub)
    for fam in by_dest_fams:                                                     # each of them by destination with and without hub
        assert {c.hub for c in cells if c.by_dest and c.fam == fam} == {True, False}, fam
    # every class: d/d W_2 in both roles, d/d W_s in both roles
    for si in range(5):
        in_class = [c for c in cells if V.s_class(c.s) == si]
        assert {c.by_dest for c in in_class if c.fam == "w2"} == {True, False}
        assert {c.by_dest for c in in_class if c.fam == "ss"} == {True, False}
    # dropout: both probabilities, both edge-id offsets, in every family that has more than two dropout cells
    dropped = [c for c in cells if c.drop is not None]
    assert Counter(c.drop[0] for c in dropped)[0.2] * 4 >= len(dropped) - 3 and {c.drop[0] for c in dropped} == {0.5, 0.2}
    assert abs(sum(c.eid0 == 0 for c in dropped) * 2 - len(dropped)) <= 1 and all(c.eid0 in (0, 3 * c.b * c.n * c.k) for c in dropped)
    assert {c.fam for c in dropped if c.drop[0] == 0.2} >= {"w2", "ss", "pair", "none"}
    # pad channels (m_dim 5) under d/d W_2 and under d/d W_s; pad columns everywhere but on a few cells
    assert {c.fam for c in cells if c.m_dim == 5} >= {"w2", "ss", "pair", "none"}
    exact = [c for c in cells if 2 * (2 * c.kw["dim"] + c.s) == 32 * c.steps]
    assert 1 <= len(exact) <= len(cells) // 4, [c.id for c in exact]
    for c in cells:
        h = 2 * (2 * c.kw["dim"] + c.s)
        assert 32 * (c.steps - 1) < h <= 32 * c.steps and c.b == 2 and c.k + 1 <= c.n <= 70
        assert c.n <= 50 or c.extra == "groups"


def test_every_call_is_valid_from_the_table_alone():
    """What the kernel relies on (include/egnn_hip.h, csrc/edge_bwd.hip:863-868): checked on the host lists the GPU test uploads (it
    compares `_ops.dest_lists` with them before the launch)."""
    import torch
    groups = []
    for c in V.CELLS:
        p = V.prepare(c.id)
        e, keys = c.b * c.n * c.k, c.b * c.n
        ent, seg = p.ent, p.seg
        L = ent.numel()
        assert L % 128 == 0 and L >= 128 and ent.dtype == torch.int32, c.id
        assert torch.equal(ent[ent >= 0].sort().values, torch.arange(e, dtype=torch.int32)), c.id          # every edge exactly once
        assert int(seg[0]) == 0 and int(seg[-1]) * 16 <= L < int(seg[-1]) * 16 + 128 and seg.numel() == keys + 1, c.id
        key_of_edge = p.dst if c.by_dest else p.src
        tiles = ent.view(-1, 16)
        for key in range(keys):
            t = tiles[int(seg[key]):int(seg[key + 1])].reshape(-1)
            live = t[t >= 0]
            assert bool((key_of_edge[live.long()] == key).all()) and live.numel() == int((key_of_edge == key).sum()), (c.id, key)
            assert bool((t[:live.numel()] >= 0).all()) and live.numel() > t.numel() - 16, (c.id, key)    # consecutive, padded to whole tiles
        assert bool((tiles[int(seg[-1]):] < 0).all()), c.id
        if c.row_pairs:
            assert not c.by_dest and 16 < c.k <= 32 and L == (keys * 32 + 127) // 128 * 128, c.id
            assert torch.equal(seg, torch.arange(keys + 1) * 2), c.id
        rounds = L // 128
        assert p.rounds == rounds and p.n_slabs == V.n_slabs_of(rounds, c.r)
        per_slab, _, n_groups = V.slabs(rounds, p.n_slabs)
        assert (p.n_slabs - 1) * per_slab < rounds, c.id                          # no empty slab
        assert V.lds_bytes(c.inst) <= 160 * 1024, c.id
        assert int(p.idx.min()) >= 0 and int(p.idx.max()) < c.n
        if c.extra == "groups":
            assert rounds >= 35 and c.r == 1 and n_groups == 2 and p.n_slabs % V.GS != 0, (c.id, rounds)
            groups.append(c.fam)
        else:
            assert n_groups == 1 or (n_groups == 2 and c.r == 1), c.id
    assert sorted(groups) == ["pair", "w2"]
    assert sorted(c.fam for c in V.CELLS if c.extra == "init") == sorted(V.FAMILIES)      # one cell per family at the module's own initialisation


def test_every_cell_meets_its_preconditions_on_the_reference():
    import torch
    for c in V.CELLS:
        p, ref = V.prepare(c.id), V.reference(c.id)
        live = ~p.zero_rows
        assert 0.1 < float(p.zero_rows.float().mean()) < 0.5, c.id
        z, sp = ref["z"][live], ref["sp"][live]
        kept = ref["keep"][live]
        if c.extra == "init":
            # the module's own draw: every weight N(0, 1e-3), z = b1 + O(1e-2) -- SiLU' nearly constant per column, which is the point
            for mod in p.layer.edge_mlp:                                         # (the two Linears this kernel reads)
                if isinstance(mod, torch.nn.Linear):
                    assert 0.7e-3 <= float(mod.weight.detach().std()) <= 1.3e-3, (c.id, float(mod.weight.detach().std()))
            b1 = p.layer.edge_mlp[0].bias.detach().double()
            assert float((ref["z"] - b1).abs().max()) < 0.5 and float(sp[kept].max() - sp[kept].min()) < 0.5, c.id
        else:
            assert float(z.std()) > 0.5, (c.id, float(z.std()))
            assert float(sp[kept].min()) < 0.3 and float(sp[kept].max()) > 0.9, c.id
        if c.drop is not None:
            frac = float(ref["keep"].float().mean())
            lo, hi = (0.3, 0.7) if c.drop[0] == 0.5 else (0.7, 0.9)
            assert lo < frac < hi, (c.id, frac)
        else:
            assert bool(ref["keep"].all())
        tiles_of = p.seg[1:] - p.seg[:-1]
        if c.hub:
            assert int(tiles_of.max()) > 2 and int(tiles_of.min()) == 0, c.id
        # a key with entries whose gU is zero throughout (its per-key sum is an exact zero)
        key = p.dst if c.by_dest else p.src
        n_live = torch.zeros(c.b * c.n).index_add_(0, key, live.float())
        n_all = torch.zeros(c.b * c.n).index_add_(0, key, torch.ones_like(live, dtype=torch.float32))
        if not (c.hub and c.k == 1):
            assert bool(((n_live == 0) & (n_all > 0)).any()), c.id
        for name in V.outputs_of(c):
            r = ref[name]
            assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, (c.id, name)
