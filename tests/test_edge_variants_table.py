"""tests/_edge_variants.py on the host: the table covers the dispatcher's grid of csrc/edge_fused.hip exactly once per instantiation, every
boundary value of the classes often enough, every option with every accumulator-tile count and every P_i variant -- and every cell
meets the preconditions that make its GPU comparison (tests/test_gpu_edge_variants.py) decidable, on the float64 oracle alone."""
import itertools
from collections import Counter

import pytest

from tests import _edge_variants as V


def test_the_table_is_exactly_the_instantiation_grid():
    insts = [c.inst for c in V.CELLS]
    assert len(insts) == 90 and len(set(insts)) == 90
    assert len({c.id for c in V.CELLS}) == 90
    grid = set(itertools.product((3, 8), V.NM_OF_CLASS, (1, 2, 4), (2, 1, 0)))
    assert {i[:4] for i in insts} == grid
    for c in V.CELLS:
        s = 2 * c.kw["fourier_features"] + 1 + c.kw["edge_dim"]
        assert c.inst == V.instantiation(c.cdim, s, c.kw["m_dim"], c.k), c.id
        assert (c.inst.CDM == 3) == (c.cdim == 3)
        assert not V.wide_shape(c.kw, c.cdim), c.id                              # (would run on the plain-fp32 kernels)
    # the staging chunk follows from the other four: HC (256) only for one scalar and one tile off the five-workgroup kernel
    assert Counter(i.HCT for i in insts) == Counter({64: 66, 128: 19, 256: 5})
    assert [i for i in insts if i.HCT == 128 and i.NM == 1 and i.NB == 1] == [V.Instantiation(3, 1, 1, 2, 128)]


def test_the_dispatch_restatement_at_its_thresholds():
    assert [V.edge_mfmas(s) for s in (1, 2, 4, 5, 6, 8, 9, 16)] == [1, 3, 3, 4, 6, 6, 12, 12]
    assert V.instantiation(3, 1, 16, 32) == (3, 1, 1, 2, 128) and V.instantiation(5, 1, 16, 32) == (8, 1, 1, 2, 256)
    assert V.instantiation(3, 1, 17, 32) == (3, 1, 2, 2, 128) and V.instantiation(3, 1, 33, 31) == (3, 1, 4, 1, 64)
    assert V.instantiation(3, 4, 32, 6) == (3, 3, 2, 1, 64) and V.instantiation(3, 5, 16, 5) == (3, 4, 1, 0, 128)
    # launch_edge's groups: one round of 128 slots (4 waves x 2 tiles x 16 edges), the whole-rounds rule, the clamps to 64 nodes and to N
    assert V.SLOTS_PER_ROUND == 128
    assert [V.group_size(k, 1000) for k in (1, 5, 6, 24, 31, 32, 33, 48, 64, 128, 160)] == [64, 25, 21, 16, 4, 4, 3, 8, 2, 1, 1]
    assert V.group_size(6, 9) == 9


def test_every_boundary_value_occurs_in_at_least_three_cells():
    cells = V.CELLS
    s_count = Counter(2 * c.kw["fourier_features"] + 1 + c.kw["edge_dim"] for c in cells)
    assert all(s_count[s] >= 3 for s in (1, 2, 4, 5, 6, 8, 9, 16)) and set(s_count) == {1, 2, 4, 5, 6, 8, 9, 16}
    m_count = Counter(c.kw["m_dim"] for c in cells)
    assert all(m_count[m] >= 3 for m in (1, 16, 17, 32, 33, 64)) and len(m_count) == 6
    k_count = Counter(c.k for c in cells if c.source != "dense")
    assert all(k_count[k] >= 3 for k in (32, 64, 128, 160, 6, 24, 31, 33, 48, 1, 5)), k_count
    dense = Counter(c.n for c in cells if c.source == "dense")
    assert all(dense[n] >= 3 for n in (32, 64, 7, 33, 3, 5)), dense
    sparse = Counter(c.k for c in cells if c.source == "sparse")
    assert all(sparse[k] >= 3 for k in (6, 24, 31, 1, 5)), sparse
    cd = Counter(c.cdim for c in cells)
    assert cd[3] == 45 and all(cd[d] == 9 for d in V.OTHER_CDIMS)
    assert Counter(c.kw["dim"] for c in cells) == Counter({8: 46, 40: 44})
    # each S beyond 2 is realised both ways: mostly edge_dim, mostly fourier_features
    for s in (4, 5, 6, 8, 9, 16):
        ways = {c.kw["fourier_features"] == 0 for c in cells if 2 * c.kw["fourier_features"] + 1 + c.kw["edge_dim"] == s}
        assert ways == {True, False}, s


def test_sizes_and_group_geometry():
    small = 0
    for c in V.CELLS:
        g = V.group_size(c.k, c.n)
        assert c.b == (1 if c.k == 160 else 2)
        if c.source == "dense":
            assert c.n == c.k
            continue
        assert c.k + 1 <= c.n <= c.k + 9, c.id
        full = V.group_size(c.k, 10 ** 6)
        assert (full == 1) == (c.k >= 128), c.id
        assert full == 1 or c.n < full or c.n % g != 0, c.id                     # a ragged last workgroup (or one workgroup: G clamped to N)
        small += c.n < V.group_size(c.k, 10 ** 6)
    assert small >= 4
    masks = Counter(c.mask for c in V.CELLS)
    assert masks["ragged"] >= 45 - 3 and masks["scattered"] >= 20 and masks["none"] >= 20, masks


def test_each_option_occurs_with_every_tile_count_and_every_pi_variant():
    for opt in V.OPTIONS + ("ragged", "scattered"):
        have = [c for c in V.CELLS if opt in c.options or c.mask == opt]
        assert {c.inst.NB for c in have} == {1, 2, 4}, opt
        assert {c.inst.TPI for c in have} == {0, 1, 2}, opt
        assert {c.inst.CDM for c in have} == {3, 8}, opt
    for c in V.CELLS:
        assert c.kw.get("update_feats", True) or c.kw.get("update_coors", True)


@pytest.mark.parametrize("mode", ["plain", "dropout"])
def test_every_cell_meets_its_preconditions_on_the_oracle(mode):
    """No tie decides a neighbour (the K-th and (K+1)-th ranking value of every valid row more than 1e-4 apart), no selected pair on
    the radius, no live coordinate weight on the clamp's kink (with and without the dropout mode's masks) -- and the float64 outputs
    stay within the range where the forward bar 1e-4 max(1, max|want| / 256) is absolute."""
    import numpy as np
    drop = (V.DROPOUT_P, V.dropout_seed()) if mode == "dropout" else None
    for c in V.CELLS:
        if drop is not None and "clamp" not in c.options:
            continue                                                             # (only the clamp's centring depends on the masks)
        p = V.prepare(c, drop=drop)
        V.check_preconditions(c, p)
        if p.want is not None:
            assert all(np.isfinite(w).all() and np.abs(w).max() < 256.0 for w in p.want), c.id
