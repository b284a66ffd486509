"""One test case per template instantiation and output form of the split-f16 GEMM (csrc/linear_hl.hip) -- the table behind
tests/test_gpu_gemm_variants.py, importable without a GPU.

`linear_hl_entry` -> `launch_hl` -> `launch_hl_cfg` picks `linear_hl_kernel<CFG, ACT, HAS_RES, DROP>` from the shape (CFG: the 256 x 128
tile when there are at least 512 of them, else 128 x 128), the activation (0 none, 1 SiLU, 2 exact GELU), the residual and training-mode
dropout (SiLU without residual only): 2 x 6 = 12 kernels, each with two epilogues (full tiles staged through LDS; ragged tiles and calls
with ldc % 4 != 0 per element) and three output forms (fp32 C, packed (hi, lo) images, both).  `select_cfg`, `group_m` and `tile_of_block`
restate the dispatch and the block -> tile map of `linear_hl_body`; `CELLS` is the grid (12 x 3 = 36 cells, every shape with interior full
tiles AND ragged M and N edges, so that one launch runs both epilogues); `EXTRA_CELLS`, `TILE_MAP_CELLS` and `SPLITK_CELLS` hold the
cases beside the grid.  A NEW INSTANTIATION NEEDS A NEW CELL: tests/test_gemm_variants_table.py fails when grid and table disagree."""
from collections import namedtuple

# ------------------------------------------------------------------------------------------------ the dispatcher, restated
BK = 16                                   # K-tile (csrc/linear_hl.hip: BK)
BN = 128                                  # both configurations
BM = {0: 128, 1: 256}                     # Cfg<0>, Cfg<1>
STAGES = {0: 4, 1: 3}
BIG_TILES = 512                           # launch_hl: at least this many 256 x 128 tiles -> CFG 1
GROUP_M_DEFAULT = 8                       # EGNN_HL_GROUP_M of the build

INSTANTIATIONS = tuple((cfg, act, res, drop) for cfg in (0, 1)
                       for act, res, drop in ((0, False, False), (0, True, False), (1, False, False), (1, True, False), (2, False, False),
                                              (1, False, True)))
FORMS = ("f32", "hl", "both")             # fp32 C only | packed (hi, lo) only (out_f32=False, out_hl=True) | both
K_TILE_COUNTS = (2, 4, 6, 34)             # Kp / 16: fewer than, equal to and more than STAGES - 1 K-tiles, and a long loop


def kpad(k):
    return (k + 31) // 32 * 32


def tiles(m, n, cfg):
    """(ntm, ntn) of launch_hl_cfg<CFG>"""
    return (m + BM[cfg] - 1) // BM[cfg], (n + BN - 1) // BN


def select_cfg(m, n):
    """launch_hl's tile rule (the W image of `_weights.split_f16` always covers whole 128-row tiles, the rule's other condition)"""
    tm, tn = tiles(m, n, 1)
    return 1 if tm * tn >= BIG_TILES else 0


def group_m(ntn, env=None):
    """hl_group_m: M-tiles per group of the block -> tile map; env = the value of EGNN_HL_GROUP_M (an int) or None"""
    if env is not None and 1 <= int(env) <= 1024:
        return int(env)
    if ntn <= 4:
        return GROUP_M_DEFAULT
    g = (128 + ntn // 2) // ntn
    return 2 if g < 2 else (16 if g > 16 else g)


def tile_of_block(bid, ntm, ntn, gm):
    """(tile_m, tile_n) of workgroup `bid` -- linear_hl_body's map: consecutive indices of one XCD (bid & 7) are consecutive tiles, the
    tiles run through groups of `gm` M-tiles x all N-tiles, M fastest; the last group may hold fewer M-tiles"""
    nblk = ntm * ntn
    q, rr = nblk >> 3, nblk & 7
    xcd = bid & 7
    v = (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + (bid >> 3)
    width = gm * ntn
    gid = v // width
    first_m = gid * gm
    gsz = min(ntm - first_m, gm)
    tile_m = first_m + (v % width) % gsz
    tile_n = (v % width) // gsz
    return tile_m, tile_n


def tile_counts(m, n, cfg):
    """(full tiles, ragged tiles) of a launch: a tile is staged iff it lies inside the matrix (and ldc % 4 == 0)"""
    ntm, ntn = tiles(m, n, cfg)
    full = (m // BM[cfg]) * (n // BN)
    return full, ntm * ntn - full


# ------------------------------------------------------------------------------------------------ the grid
# k: the contraction length; extra: dict of split_cols / k_a (columns of the A image, wider than k) / row_mask
Cell = namedtuple("Cell", "id kind cfg act res drop form m n k extra")

SHAPE = {0: (3 * 128 + 5, 5 * 128 + 4),          # 4 x 6 tiles of 128 x 128: 15 full, 9 ragged
         1: (8192 + 5, 2048 + 4)}                # 33 x 17 tiles of 256 x 128 (561 >= 512): 512 full, 49 ragged
K_OF_TILES = {2: 29, 4: 50, 6: 89, 34: 530}      # Kp / 16 -> K (none a multiple of 32: every A image has pad columns)
DROP_P, DROP_SEED = 0.2, 12345


def _name(cfg, act, res, drop):
    return f"cfg{cfg}-act{act}{'-res' if res else ''}{'-drop' if drop else ''}"


def _grid():
    cells = []
    for i, (cfg, act, res, drop) in enumerate(INSTANTIATIONS):
        m, n = SHAPE[cfg]
        k = K_OF_TILES[K_TILE_COUNTS[(i % 6) % 4]]
        for form in FORMS:
            cells.append(Cell(f"{_name(cfg, act, res, drop)}-{form}-{m}x{n}x{k}", "grid", cfg, act, res, drop, form, m, n, k, {}))
    return cells


def _extras():
    cells = []

    def add(kind, cfg, act, res, form, m, n, k, **extra):
        tag = "-".join(f"{a}{b}" for a, b in extra.items())
        cells.append(Cell(f"{kind}-{_name(cfg, act, res, False)}-{form}-{m}x{n}x{k}" + (f"-{tag}" if tag else ""), kind, cfg, act, res, False,
                          form, m, n, k, extra))
    # exactly 512 large tiles, and 31 x 16 = 496 of them: CFG 0 on 62 x 16 tiles (a tail group of 6 M-tiles behind groups of 8)
    add("threshold", 1, 1, True, "both", 32 * 256 - 3, 16 * 128 - 4, 50)
    add("threshold", 0, 1, True, "both", 31 * 256 - 3, 16 * 128 - 4, 50)
    for cfg in (0, 1):
        m, n = SHAPE[cfg]
        add("unaligned", cfg, 1, True, "both", m, n - 2, 50)                     # ldc % 4 == 2: the whole launch per element
        for sc in (32, 96, 160):                                                 # inside a 128-column tile, inside a wave's 64-column strip
            add("split_cols", cfg, 0, False, "f32", m, n, 50, split_cols=sc)
        add("wide_a", cfg, 0, False, "both", m, n, 29, k_a=89)                   # Kp_a = 96 > Kp = 32
        add("row_mask", cfg, 0, False, "f32", m, n, 29, k_a=89, row_mask=1)
    return cells


CELLS = _grid()
EXTRA_CELLS = _extras()
BY_ID = {c.id: c for c in CELLS + EXTRA_CELLS}

# the block -> tile map on CFG 0 (K = 32): (ntm, ntn), each run with EGNN_HL_GROUP_M unset and set to 1, 3 and 5.  (7, 5), (9, 5) and
# (11, 7) have more than four N-tiles, a tail group under the default group size (16: one short group) and under 3 and 5, and
# nblk % 8 != 0.
TILE_MAP_CELLS = ((1, 1), (3, 1), (5, 3), (7, 5), (9, 5), (11, 7))
TILE_MAP_GROUPS = (None, 1, 3, 5)
TILE_MAP_K = 32


def tile_map_shape(ntm, ntn):
    return 128 * ntm - 5, 128 * ntn - 4


# split-K (egnn_linear_hl_splitk_f32 through _ops.grad_tn): g (R, M)^T @ x (R, N), the contraction over R in `k_splits` parts of
# ceil(nkt / k_splits) K-tiles, nkt = kpad(R) / 16
SplitK = namedtuple("SplitK", "id r m n k_splits")
SPLITK_CELLS = (SplitK("ks3-nkt8", 128, 161, 140, 3),             # parts of 3, 3, 2 K-tiles
                SplitK("ks5-nkt14", 219, 161, 140, 5),            # 3, 3, 3, 3, 2
                SplitK("ks7-nkt20", 317, 161, 140, 7),            # 3 x 6, 2
                SplitK("one-tile-parts", 50, 161, 140, 4),        # nkt = 4: every part owns one K-tile (the prologue stages dummies only)
                SplitK("odd-count", 128, 33, 7, 3))               # m n % 4 != 0: the parts are summed by torch
SPLITK_EMPTY_PART = SplitK("ks5-nkt12", 192, 161, 140, 5)         # ceil(12 / 5) = 3, 4 x 3 = 12: the fifth part would be empty -> EGNN_E_SHAPE


def splitk_parts(r, k_splits):
    """K-tiles per part, or None where egnn_linear_hl_splitk_f32 refuses (a part without a K-tile)"""
    nkt = kpad(r) // BK
    per = (nkt + k_splits - 1) // k_splits
    if per * (k_splits - 1) >= nkt:
        return None
    return [min(per, nkt - p * per) for p in range(k_splits)]
