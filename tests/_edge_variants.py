"""One test case per template instantiation of the fused edge pass (csrc/edge_fused.hip) -- the table behind
tests/test_gpu_edge_variants.py, importable without a GPU.

The dispatcher picks `edge_kernel<NM, HCT, TPI, NB, MODE>` of one of two translation units (CDM = 3 / 8) from four properties of a
call: the coordinate dimension, the number of per-edge scalars S = 2 fourier + 1 + edge_dim, m_dim and K.  2 x 5 x 3 x 3 = 90
instantiations per MODE (0 inference, 1 / 0 + U_out the forward under autograd, 3 training-mode dropout), each with its own register
allocation, LDS carve-up and group geometry; the native backward (csrc/edge_bwd.hip) is keyed by the same axes.  `instantiation()`
restates the dispatch, `CELLS` holds one fixed case per cell, `prepare()` builds a cell's parameters, inputs and float64 oracle result
on the host.  A NEW INSTANTIATION NEEDS A NEW CELL: tests/test_edge_variants_table.py fails when the grid and the table disagree.

The representatives are not drawn, they follow a rule (the boundary values of every class, alternating with the other axes' indices):
    S        1 | 2, 4 | 5 | 6, 8 | 9, 16, each realised mostly through edge_dim and mostly through fourier_features
    m_dim    1, 16 | 17, 32 | 33, 64
    K        K % 32 == 0: k-NN 32, 64, 128, 160 and the dense path with N = 32, 64
             6 <= K otherwise: k-NN 6, 24, 31, 33, 48; dense N = 7, 33; only_sparse_neighbors with a band of maximum degree 6, 24, 31
             K < 6: k-NN 1, 5; dense N = 3, 5; only_sparse_neighbors with maximum degree 1, 5
    cdim     3 against 1, 2, 4, 5, 8 in rotation
    dim      8 (Hp = 64: less than one staging chunk) and 40 (Hp = 192: a full chunk and a partial one), alternating
    n        K + 1 ... K + 9 and no multiple of the group size G of `group_size()`, so that the last workgroup is ragged (K = 128 and
             K = 160 have G = 1: a node spans one round and more; the dense path has n = K); K <= 6: n < G, one workgroup with G
             clamped to N; b = 2, K = 160: b = 1
    options  soft_edges, norm_coors, mean pooling, clamp, a finite radius, update_feats=False, update_coors=False in rotation, two per
             cell; a ragged mask on half of the cells, a scattered one on a quarter
K = 1 selects the node itself in every cell, k-NN as well as adjacency (distance 0, or the reference's rank -1, comes first): x_i - x_j
= 0 there, so the coordinate branch and coors_mlp's gradients of those TPI = 0 instantiations see only zeros (the adjacency cells keep
node_mlp for that reason); the K = 5 and dense N = 3, 5 cells of the same class exercise them with real differences.
Weights are the oracle's seeded xavier parameters with the factors of tests/test_gpu_fuzz.py (outputs of order one to ten)."""
import zlib
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------------------ the dispatcher, restated
EDGE_HC, EDGE_HC5, GMAX = 256, 128, 64                           # csrc/edge_fused.hip:59, :151, :118
SLOTS_PER_ROUND = (256 // 64) * (2 * 16)                         # EDGE_WAVES * SLOTS_PER_WAVE = 4 waves x 2 tiles x 16 edges = 128 (:86-93)
S_CLASSES = ((1,), (2, 4), (5,), (6, 8), (9, 16))                # egnn_edge_mfmas, csrc/edge_fused.hip:1196
NM_OF_CLASS = (1, 3, 4, 6, 12)
M_CLASSES = ((1, 16), (17, 32), (33, 64))                        # dispatch_tpi, csrc/edge_fused.hip:1181-1184
OTHER_CDIMS = (1, 2, 4, 5, 8)

Instantiation = namedtuple("Instantiation", "CDM NM NB TPI HCT")


def edge_mfmas(s):
    """egnn_edge_mfmas (csrc/edge_fused.hip:1196)"""
    return 1 if s <= 1 else (3 if s <= 4 else (4 if s <= 5 else (6 if s <= 8 else 12)))


def _edge_min_blocks(cdm, nm, tpi, nb):
    """edge_min_blocks (csrc/edge_fused.hip:132-141) with the build's defaults (EGNN_EDGE_T0_BLOCKS 4, EGNN_EDGE_MINW 5)"""
    if nb >= 4:
        return 1
    if nb == 2:
        return 1 if nm > 4 else 2
    if nm >= 12:
        return 1
    if nm > 4:
        return 2
    if nm > 1:
        return 3 if (cdm == 3 and tpi == 2) else (4 if (cdm == 3 and tpi == 0) else 2)
    if cdm == 3 and tpi == 2:
        return 5
    return 4 if (cdm == 3 and tpi >= 1) else 3


def instantiation(cdim, s, m_dim, k):
    """(CDM, NM, NB, TPI, HCT) of the kernel egnn_edge_fused_f32 launches for a call -- EGNN_EDGE_ENTRY's chain over S
    (csrc/edge_fused.hip:1271-1276), dispatch_tpi over m_dim (:1161-1189), dispatch_tpi_nb over K (:1149-1157), the translation unit by
    the coordinate dimension (:1221-1226)."""
    assert 1 <= cdim <= 8 and 1 <= s <= 16 and 1 <= m_dim <= 64 and k >= 1
    cdm = 3 if cdim == 3 else 8
    nm = edge_mfmas(s)
    hct = {1: EDGE_HC, 3: 128, 4: 128, 6: 64, 12: 64}[nm]                        # :1271-1276
    nb = 1 if m_dim <= 16 else (2 if m_dim <= 32 else 4)
    if nb == 2:
        hct = max(hct // 2, 64)                                                  # :1183
    elif nb == 4:
        hct = 64                                                                 # :1184
    tpi = 2 if k % 32 == 0 else (1 if k >= 6 else 0)                             # :1154-1156
    if tpi == 2 and nm == 1 and nb == 1 and _edge_min_blocks(cdm, nm, 2, nb) >= 5:
        hct = EDGE_HC5                                                           # :1154, the five-workgroup kernel
    return Instantiation(cdm, nm, nb, tpi, hct)


def group_size(k, n):
    """nodes per workgroup, launch_edge (csrc/edge_fused.hip:1120-1133) for the small batches of this table (the two-rounds rule of
    :1126 needs B N / 2 G >= 4096)"""
    g = max(1, min(SLOTS_PER_ROUND // k, GMAX))
    if k < SLOTS_PER_ROUND and (g * k) % SLOTS_PER_ROUND != 0:
        for g2 in range(g + 1, 17):                                              # the whole-rounds rule (K = 48: 8 nodes = 3 rounds)
            if (g2 * k) % SLOTS_PER_ROUND == 0:
                g = g2
                break
    return min(g, n)


def wide_shape(kw, cdim):
    """layer.py's `wide_shape` rule (EGNN._forward_hip_impl) for graphs of ordinary size: such a call runs on the plain-fp32 kernels"""
    return 2 * kw.get("fourier_features", 0) + 1 + kw.get("edge_dim", 0) > 16 or cdim > 8 or kw.get("m_dim", 16) > 64


# ------------------------------------------------------------------------------------------------ the table
K_VARIANTS = {
    2: (("knn", 32), ("knn", 64), ("dense", 32), ("knn", 128), ("dense", 64), ("knn", 160)),
    1: (("knn", 6), ("sparse", 24), ("knn", 31), ("dense", 7), ("knn", 48), ("sparse", 6), ("knn", 24), ("dense", 33), ("sparse", 31),
        ("knn", 33)),
    0: (("knn", 1), ("dense", 5), ("sparse", 5), ("knn", 5), ("dense", 3), ("sparse", 1)),
}
OPTIONS = ("soft_edges", "norm_coors", "pool_mean", "clamp", "radius", "no_feats", "no_coors")
MASK_KINDS = ("ragged", "none", "ragged", "scattered")
DROPOUT_P = 0.2
TORCH_SEED = 77                       # torch.manual_seed(TORCH_SEED) in front of a training-mode forward: it draws `dropout_seed()`

Cell = namedtuple("Cell", "id kw b n cdim k source mask options inst seed")

# cells whose first seed misses a precondition of `prepare` (ranking gap, radius or clamp margin): the next seed that meets them
SEED_BUMP = {"c3-S1f0e0-m17-knn64-d40-n69": 1, "c3-S1f0e0-m32-sparse24-d8-n29": 1, "c3-S5f0e4-m17-knn128-d8-n132": 2,
             "c1-S2f0e1-m16-sparse31-d40-n33": 3, "c8-S8f0e7-m1-sparse5-d40-n8": 1}


def _option_kw(opt, cdim):
    return {"soft_edges": dict(soft_edges=True), "norm_coors": dict(norm_coors=True), "pool_mean": dict(m_pool_method="mean"),
            "clamp": dict(coor_weights_clamp_value=0.25), "radius": dict(valid_radius=2.0 * cdim),     # (E |x_i - x_j|^2 = 2 cdim)
            "no_feats": dict(update_feats=False), "no_coors": dict(update_coors=False)}[opt]


def _build_cells():
    cells, q = [], 0
    for ci in range(2):
        for si in range(5):
            for mi in range(3):
                for ti, tpi in enumerate((2, 1, 0)):
                    s_vals, m_vals = S_CLASSES[si], M_CLASSES[mi]
                    s = s_vals[(ci + mi + ti) % 2 % len(s_vals)]
                    m_dim = m_vals[(ci + si + ti) % 2]
                    if ((mi + ti) // 2 + ci) % 2:                               # mostly fourier_features
                        fourier, edge_dim = (s - 1) // 2, (s - 1) % 2
                    else:                                                       # mostly edge_dim
                        fourier, edge_dim = 0, s - 1
                    cdim = 3 if ci == 0 else OTHER_CDIMS[(si * 9 + mi * 3 + ti) % 5]
                    variants = K_VARIANTS[tpi]
                    r = ci * 15 + si * 3 + mi
                    source, k = variants[(r + r // 3) % 6 if len(variants) == 6 else r % len(variants)]
                    dim = (8, 40)[(q // 2) % 2]
                    kw = dict(dim=dim, m_dim=m_dim, fourier_features=fourier, edge_dim=edge_dim)
                    if source == "knn":
                        kw["num_nearest_neighbors"] = k
                    elif source == "sparse":
                        kw["only_sparse_neighbors"] = True
                    opts = [OPTIONS[q % 7], OPTIONS[(q % 7 + 1 + (q // 7) % 5) % 7]]
                    if set(opts) == {"no_feats", "no_coors"}:                   # (the layer needs one of its two updates)
                        opts = opts[:1]
                    if source == "sparse" and k == 1 and "no_feats" in opts:
                        # (the only neighbour is the node itself, x_i - x_i = 0: without node_mlp the cell would compute nothing)
                        opts = [o for o in opts if o != "no_feats"] + (["no_coors"] if "no_coors" not in opts else [])
                    for o in opts:
                        kw.update(_option_kw(o, cdim))
                    if source == "dense":
                        n = k
                    else:
                        n = k + 1 + q % 9
                        g = group_size(k, 10 ** 6)                              # (n < G: one workgroup, G clamped to N)
                        for _ in range(9):
                            if g == 1 or n < g or n % g != 0:
                                break
                            n = n + 1 if n < k + 9 else k + 1
                    b = 1 if k == 160 else 2
                    inst = instantiation(cdim, s, m_dim, k)
                    assert inst == (3 if ci == 0 else 8, NM_OF_CLASS[si], (1, 2, 4)[mi], tpi, inst.HCT)
                    cid = f"c{cdim}-S{s}f{fourier}e{edge_dim}-m{m_dim}-{source}{k}-d{dim}-n{n}"
                    seed = zlib.crc32(cid.encode()) % (2 ** 30) + SEED_BUMP.get(cid, 0)
                    cells.append(Cell(cid, kw, b, n, cdim, k, source, MASK_KINDS[(q + q // 4) % 4], tuple(opts), inst, seed))
                    q += 1
    return cells


CELLS = _build_cells()
BY_ID = {c.id: c for c in CELLS}


# ------------------------------------------------------------------------------------------------ a cell's data, on the host
def adjacency(cell):
    """only_sparse_neighbors: the band |i - j| <= w WITH its diagonal (the reference counts the diagonal into K and ranks the node itself
    first, then its neighbours at rank 0: K = 2 w + 1 entries, no tie at the K-th place); an even K: one more bond between node w and
    node 2 w + 1, whose rows alone reach the maximum degree.  K = 1 is w = 0: every node its own and only neighbour."""
    if cell.source != "sparse":
        return None
    n, k = cell.n, cell.k
    w = (k - 1) // 2
    i = np.arange(n)
    adj = np.abs(i[:, None] - i[None, :]) <= w
    if k % 2 == 0:
        adj[w, 2 * w + 1] = adj[2 * w + 1, w] = True
    assert int(adj.sum(-1).max()) == k
    return adj


def node_mask(cell, rng):
    if cell.mask == "none":
        return None
    b, n, k = cell.b, cell.n, cell.k
    # k-NN: at least K real nodes per graph (with fewer, the K-th and the (K+1)-th ranking value of a row are both the padding constant)
    lo = {"knn": max(k, n - 6), "dense": max(2, n // 2), "sparse": max(1, n - 4)}[cell.source]
    lens = rng.integers(lo, n + 1, size=b)
    lens[-1] = min(lens[-1], max(lo, n - 1))                                     # (at least one graph is padded where n > lo)
    mask = np.arange(n)[None, :] < lens[:, None]
    if cell.mask == "scattered":
        mask = np.stack([rng.permutation(row) for row in mask])
    return mask


def dropout_seed():
    """the mask seed a training-mode forward draws from torch's CPU generator right after torch.manual_seed(TORCH_SEED)"""
    import torch
    from egnn_pytorch_amd import _dropout
    torch.manual_seed(TORCH_SEED)
    return _dropout.draw_seed()


class Prepared:
    pass


def _cpu_layer(kw, params, dropout=0.0):
    import torch
    from egnn_pytorch_amd import EGNN
    layer = EGNN(**kw, dropout=dropout)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return layer.eval()


def _centre_clamp(cell, p, drop):
    """Shift coors_mlp's last bias so that the clamp value falls into the widest gap among the coordinate weights of the live pairs,
    leaving out a tail of one pair in fifty (at most 32 pairs) at either end.  Some pairs are then clamped and some are not, and none
    sits within rounding of the kink, where the derivative jumps and fp32 against float64 rounding would decide a gradient.
    The weights come from the float64 restatement on the host (`autograd.layer_given_neighbors`, with the hash masks of `drop`); a
    forward hook on coors_mlp's last Linear reads them, which relies on the restatement calling that module on host tensors.
    This is set-up of the case, made on the reference side before anything is compared: the shifted bias is a parameter of the
    layer under test and of the reference alike, and no bar changes.
    Returns the distance of the nearest live weight to +- the clamp value after the shift."""
    import torch
    from egnn_pytorch_amd import autograd as A
    c = float(cell.kw["coor_weights_clamp_value"])
    t64 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).double()            # noqa: E731
    mask = None if p.mask is None else torch.from_numpy(p.mask)
    idx = None if p.idx is None else torch.from_numpy(p.idx).long()
    rank = t64(p.rank)
    margin = None
    for _ in range(2):                                                           # (second pass: the margin after the shift)
        layer = _cpu_layer(cell.kw, p.params, DROPOUT_P if drop else 0.0).double()
        seen = []
        hook = layer.coors_mlp[3].register_forward_hook(lambda mod, args, out: seen.append(out.detach()))
        with torch.no_grad():
            A.layer_given_neighbors(layer, t64(p.feats), t64(p.coors), t64(p.edges), mask, idx, rank, p.radius, drop=drop)
        hook.remove()
        w = seen[-1].squeeze(-1)
        pm = A._pair_mask(mask, idx, rank, p.radius)
        ws = (w if pm is None else w[pm]).reshape(-1).sort().values
        if margin is not None or ws.numel() < 4:
            return float(torch.minimum((ws - c).abs(), (ws + c).abs()).min()) if ws.numel() else 1.0
        lo = min(ws.numel() // 50, 32)                                          # (a tail of one pair in fifty, at most 32 pairs)
        hi = max(lo + 1, ws.numel() - 1 - lo)
        gaps = ws[lo + 1:hi + 1] - ws[lo:hi]
        j = int(gaps.argmax())
        p.params["coors_mlp.3.bias"] = (p.params["coors_mlp.3.bias"].astype(np.float64)
                                        + (c - 0.5 * float(ws[lo + j] + ws[lo + j + 1]))).astype(np.float32)
        margin = 0.0


def prepare(cell, drop=None):
    """Parameters, inputs and the float64 oracle's view of a cell, from its seed alone.  drop = (p, seed): the data of the dropout mode
    (the clamp is centred under those hash masks; no oracle output -- the reference of that mode is the restatement with the masks).
        .params (float32 arrays, reference state_dict keys)  .feats .coors .edges .mask .adj (numpy; None where absent)
        .idx .rank  the float64 oracle's neighbour list (None: dense)      .radius  the radius the pair mask applies
        .want       (node, coors) of the float64 oracle (drop is None)
        .rank_gap   the smallest (K+1)-th minus K-th ranking value over the valid rows (inf: dense, or n == K)
        .radius_margin / .clamp_margin  distance of the nearest selected ranking value to the radius / live weight to the clamp"""
    from oracle import egnn_oracle as O
    kw, b, n, cdim, k = cell.kw, cell.b, cell.n, cell.cdim, cell.k
    p = Prepared()
    cfg = O.EGNNConfig(**kw)
    p.cfg = cfg
    params = O.random_params(cfg, seed=cell.seed)
    # wide neighbourhoods sum many messages: outputs of order one to ten (tests/test_gpu_fuzz.py:50-54)
    if "coors_mlp.3.weight" in params:
        params["coors_mlp.3.weight"] = params["coors_mlp.3.weight"] * np.float32(min(1.0, 8.0 / k))
    params["edge_mlp.3.weight"] = params["edge_mlp.3.weight"] * np.float32(min(1.0, 4.0 / np.sqrt(k)))
    p.params = params
    rng = np.random.default_rng(cell.seed)
    p.feats = rng.standard_normal((b, n, kw["dim"])).astype(np.float32)
    p.coors = rng.standard_normal((b, n, cdim)).astype(np.float32)
    p.edges = rng.standard_normal((b, n, n, kw["edge_dim"])).astype(np.float32) if kw["edge_dim"] else None
    p.mask = node_mask(cell, rng)
    p.adj = adjacency(cell)
    # ---- the neighbour list and its margins, float64
    p.idx = p.rank = None
    p.rank_gap = p.radius_margin = float("inf")
    p.radius = kw.get("valid_radius", float("inf"))
    if cell.source != "dense":
        ranking, _ = O.build_ranking(O.pairwise(p.coors.astype(np.float64))[1], p.mask, p.adj)
        if cell.source == "sparse":
            assert O.sparse_num_nearest(p.adj) == k
            p.radius = 0.0
        p.rank, p.idx = O.topk_smallest(ranking, k)
        rows = np.ones((b, n), dtype=bool) if p.mask is None else p.mask
        if n > k:
            vals = np.sort(ranking, axis=-1)
            p.rank_gap = float((vals[..., k] - vals[..., k - 1])[rows].min())
        if cell.source == "knn" and np.isfinite(p.radius) and p.mask is not None:
            p.radius_margin = float(np.abs(p.rank[rows] - p.radius).min())
    p.clamp_margin = float("inf")
    if "coor_weights_clamp_value" in kw and kw.get("update_coors", True):
        p.clamp_margin = _centre_clamp(cell, p, drop)
    p.want = None
    if drop is None:
        f64 = lambda a: None if a is None else a.astype(np.float64)                                        # noqa: E731
        p.want = O.egnn_forward(cfg, {name: v.astype(np.float64) for name, v in params.items()}, f64(p.feats), f64(p.coors), f64(p.edges),
                                p.mask, p.adj)
    return p


def check_preconditions(cell, p):
    """On the reference alone: no tie decides a neighbour (`min_rank_gap` of tests/test_gpu_attention_training.py), no selected pair
    sits on the radius, no live coordinate weight on the clamp's kink."""
    assert p.rank_gap > 1e-4, (cell.id, "ranking gap", p.rank_gap)
    assert p.radius_margin > 1e-4, (cell.id, "radius margin", p.radius_margin)
    assert p.clamp_margin > 2e-5, (cell.id, "clamp margin", p.clamp_margin)
