"""tests/_gemm_variants.py on the host: the table covers the split-f16 GEMM's grid (csrc/linear_hl.hip: 12 instantiations x 3 output forms)
exactly once per cell, every cell's shape selects the tile configuration it claims and runs both epilogues in one launch, the K-tile
counts around the ring depth all occur -- and the restated block -> tile map is the bijection the kernel's comment claims."""
import itertools
from collections import Counter

import pytest

from tests import _gemm_variants as G


def test_the_table_is_exactly_the_instantiation_grid():
    keys = [(c.cfg, c.act, c.res, c.drop, c.form) for c in G.CELLS]
    assert len(keys) == 36 and len(set(keys)) == 36
    assert len({c.id for c in G.CELLS + G.EXTRA_CELLS}) == len(G.CELLS) + len(G.EXTRA_CELLS)
    insts = set(itertools.product((0, 1), ((0, False, False), (0, True, False), (1, False, False), (1, True, False), (2, False, False),
                                           (1, False, True))))
    assert {(c.cfg, (c.act, c.res, c.drop)) for c in G.CELLS} == insts and len(insts) == 12
    assert set(keys) == {(cfg, *ard, form) for (cfg, ard) in insts for form in G.FORMS}
    assert len(G.INSTANTIATIONS) == 12 and len(set(G.INSTANTIATIONS)) == 12
    for c in G.CELLS:
        assert c.kind == "grid" and not c.extra
        assert not (c.act == 2 and c.res)                      # linear_hl_entry: GELU has no residual form
        assert not c.drop or (c.act == 1 and not c.res)        # launch_hl_cfg: dropout behind SiLU without residual only
    # the three forms of an instantiation share one shape: the GPU test compares them with each other
    for inst in G.INSTANTIATIONS:
        assert len({(c.m, c.n, c.k) for c in G.CELLS if (c.cfg, c.act, c.res, c.drop) == inst}) == 1


def test_every_cell_selects_its_configuration_and_runs_both_epilogues():
    for c in G.CELLS + G.EXTRA_CELLS:
        assert G.select_cfg(c.m, c.n) == c.cfg, c.id
        full, ragged = G.tile_counts(c.m, c.n, c.cfg)
        assert full >= 1 and ragged >= 1, c.id
        assert c.m % G.BM[c.cfg] != 0 and c.n % G.BN != 0, c.id                 # ragged M AND N edges
        if c.kind == "unaligned":
            assert c.n % 4 != 0, c.id
        else:
            assert c.n % 4 == 0, c.id                                           # ldc % 4 == 0: the full tiles are staged
        assert G.kpad(c.k) // G.BK in G.K_TILE_COUNTS, c.id
        if "k_a" in c.extra:
            assert G.kpad(c.extra["k_a"]) > G.kpad(c.k), c.id
        if "split_cols" in c.extra:
            sc = c.extra["split_cols"]
            assert sc % 32 == 0 and sc % 128 != 0 and 0 < sc < c.n and c.form == "f32" and not c.res, c.id
    for cfg in (0, 1):
        assert {G.kpad(c.k) // G.BK for c in G.CELLS if c.cfg == cfg} == set(G.K_TILE_COUNTS)
        # (Kp % 32 == 0: K-tile counts are even) no more K-tiles than the prologue stages, and more than the ring holds
        assert min(G.K_TILE_COUNTS) <= G.STAGES[cfg] - 1 and max(G.K_TILE_COUNTS) > G.STAGES[cfg]
    assert {c.extra["split_cols"] for c in G.EXTRA_CELLS if c.kind == "split_cols" and c.cfg == 0} == {32, 96, 160}
    assert {c.extra["split_cols"] for c in G.EXTRA_CELLS if c.kind == "split_cols" and c.cfg == 1} == {32, 96, 160}
    assert {c.extra["split_cols"] % 64 for c in G.EXTRA_CELLS if c.kind == "split_cols"} == {32}     # inside a wave's 64-column strip
    for kind in ("unaligned", "wide_a", "row_mask"):
        assert {c.cfg for c in G.EXTRA_CELLS if c.kind == kind} == {0, 1}, kind


def test_the_tile_rule_at_its_threshold():
    at, below = [c for c in G.EXTRA_CELLS if c.kind == "threshold"]
    tm, tn = G.tiles(at.m, at.n, 1)
    assert tm * tn == G.BIG_TILES and at.cfg == 1 and G.select_cfg(at.m, at.n) == 1
    tm, tn = G.tiles(below.m, below.n, 1)
    assert tm * tn == G.BIG_TILES - 16 and below.cfg == 0 and G.select_cfg(below.m, below.n) == 0
    ntm, ntn = G.tiles(below.m, below.n, 0)
    assert ntm * ntn == 992 and ntn > 4 and ntm % G.group_m(ntn) != 0           # CFG 0 on many tiles, with a tail group
    assert G.select_cfg(8192, 2048) == 1 and G.select_cfg(8192, 2047) == 1 and G.select_cfg(8192 - 256, 2048) == 0
    assert G.select_cfg(384, 640) == 0 and G.select_cfg(16384, 4160) == 1
    assert G.tiles(1, 1, 0) == (1, 1) and G.tiles(129, 129, 0) == (2, 2) and G.tiles(257, 128, 1) == (2, 1)


def test_group_m_restated():
    assert [G.group_m(ntn) for ntn in (1, 4, 5, 7, 8, 16, 17, 33, 64, 65, 200)] == [8, 8, 16, 16, 16, 8, 8, 4, 2, 2, 2]
    assert G.group_m(33, env=5) == 5 and G.group_m(2, env=1) == 1 and G.group_m(33, env=0) == 4 and G.group_m(33, env=1025) == 4
    assert G.group_m(33, env=1024) == 1024


def _assert_bijection(ntm, ntn, gm):
    seen = [G.tile_of_block(bid, ntm, ntn, gm) for bid in range(ntm * ntn)]
    assert all(0 <= tm < ntm and 0 <= tn < ntn for tm, tn in seen), (ntm, ntn, gm)
    assert len(set(seen)) == ntm * ntn, (ntm, ntn, gm, Counter(seen).most_common(1))


def test_the_tile_map_is_a_bijection():
    """every workgroup index onto its own tile of ntm x ntn: the tile-map cells under every group size the GPU test sets, every shape up
    to 12 x 12 with groups up to 9, and the shapes of the grid and the threshold cells under the dispatcher's own group size"""
    for ntm, ntn in G.TILE_MAP_CELLS:
        for env in G.TILE_MAP_GROUPS:
            _assert_bijection(ntm, ntn, G.group_m(ntn, env))
    for ntm in range(1, 13):
        for ntn in range(1, 13):
            for gm in range(1, 10):
                _assert_bijection(ntm, ntn, gm)
    for c in G.CELLS + G.EXTRA_CELLS:
        ntm, ntn = G.tiles(c.m, c.n, c.cfg)
        _assert_bijection(ntm, ntn, G.group_m(ntn))


def test_the_tile_map_cells_have_tail_groups_beyond_four_n_tiles():
    assert set(G.TILE_MAP_CELLS) == {(1, 1), (3, 1), (5, 3), (7, 5), (9, 5), (11, 7)} and G.TILE_MAP_GROUPS == (None, 1, 3, 5)
    hit = 0
    for ntm, ntn in G.TILE_MAP_CELLS:
        m, n = G.tile_map_shape(ntm, ntn)
        assert G.tiles(m, n, 0) == (ntm, ntn) and G.select_cfg(m, n) == 0 and n % 4 == 0
        for env in G.TILE_MAP_GROUPS:
            gm = G.group_m(ntn, env)
            hit += ntn > 4 and ntm % gm != 0 and (ntm * ntn) % 8 != 0
    assert hit >= 6                                            # a tail group with nblk % 8 != 0 and more than four N-tiles
    # the map's grouping: the first `gm * ntn` indices of XCD 0's run cover gm M-tiles x all N-tiles, M fastest
    assert [G.tile_of_block(8 * i, 16, 8, 2) for i in range(4)] == [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_split_k_cells():
    assert {c.k_splits for c in G.SPLITK_CELLS} >= {3, 5, 7}
    for c in G.SPLITK_CELLS:
        parts = G.splitk_parts(c.r, c.k_splits)
        assert parts is not None and len(parts) == c.k_splits and min(parts) >= 1 and sum(parts) == G.kpad(c.r) // G.BK, c.id
        assert G.select_cfg(c.m, c.n) == 0
    for ks in (3, 5, 7):
        parts = [G.splitk_parts(c.r, c.k_splits) for c in G.SPLITK_CELLS if c.k_splits == ks][0]
        assert parts[-1] < parts[0], ks                        # a shorter last part
    assert any(set(G.splitk_parts(c.r, c.k_splits)) == {1} for c in G.SPLITK_CELLS)
    assert any((c.m * c.n) % 4 != 0 for c in G.SPLITK_CELLS)
    e = G.SPLITK_EMPTY_PART
    assert G.splitk_parts(e.r, e.k_splits) is None


@pytest.mark.parametrize("swap", [False, True])
def test_a_map_with_the_tile_roles_swapped_is_no_bijection(swap):
    """the check above can fail: the same map with tile_m and tile_n exchanged leaves ntm x ntn on every shape that is not square"""
    ntm, ntn, gm = 7, 5, 3
    seen = [G.tile_of_block(bid, ntm, ntn, gm) for bid in range(ntm * ntn)]
    if swap:
        seen = [(tn, tm) for tm, tn in seen]
    inside = all(0 <= tm < ntm and 0 <= tn < ntn for tm, tn in seen)
    assert inside == (not swap)
