"""Tied and degenerate geometries on the MI355X: integer lattices, duplicated and coincident nodes, collinear nodes, -0.0 components.

Integer (and half-integer) coordinates give squared distances that are exact in fp32 and float64 whatever the summation order, so the
numpy oracle (oracle/egnn_oracle.py: pairwise / inner_sum, build_ranking, topk_smallest with a stable argsort) is an unambiguous
reference under the tie policy of SURVEY.md §8c(5) -- ascending value, ties by ascending index -- and the comparison is bit for bit:

1. the four selection kernels (the register kernel with its pair path / two-smallest-keys pruning / hand-over to the radix descent,
   the workgroup-per-row kernel in its four instantiations, the streaming kernel), alone and with an adjacency, against the oracle;
2. the Morton order and the destination lists on these inputs;
3. layers and a network, forward, against the oracle (neighbour lists bit for bit, outputs at the parity bar, the launch paths bit
   identical to each other);
4. layers, backward and under create_graph=True, against float64 autograd of the restated layer over the kernel's own neighbour list.

Every selection case asserts from the oracle alone that it really contains ties at the K boundary (`_assert_ties`)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O
from tests._util import ATOL
from tests.test_gpu_large_graphs import _sampled_topk
from tests.test_second_order import force_matching_grads

pytestmark = pytest.mark.gpu

VERBOSE = bool(os.environ.get("EGNN_TEST_VERBOSE"))


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()        # (a copy: the cached geometries are read-only)


# ------------------------------------------------------------------------------------------------ geometries
def lattice(side, c=3):
    """all integer points of {0..side-1}^c, (side^c, c)"""
    return np.stack(np.meshgrid(*([np.arange(side)] * c), indexing="ij"), axis=-1).reshape(-1, c).astype(np.float64)


def hypercube9():
    """the 512 points of {0,1}^9: squared distance = Hamming distance, shells of 1, 9, 36, 84, ..."""
    return lattice(2, 9)


def dups(m, r, rng):
    """m random integer points of [-3, 3]^3, each repeated r times"""
    return np.repeat(rng.integers(-3, 4, size=(m, 3)).astype(np.float64), r, axis=0)


def point(n):
    return np.full((n, 3), 1.5)


def line(n):
    """0..N-1 on x (the shuffle of `_batch` makes it a permutation), y = z = 0"""
    return np.concatenate([np.arange(n, dtype=np.float64)[:, None], np.zeros((n, 2))], axis=1)


def negzero(side, rng):
    """a lattice in which half of the zero components are -0.0"""
    p = lattice(side)
    zeros = np.argwhere(p == 0)
    pick = zeros[rng.permutation(len(zeros))[: len(zeros) // 2]]
    p[pick[:, 0], pick[:, 1]] = -0.0
    assert np.signbit(p).sum() == len(zeros) // 2
    return p


def _with_repeats(p, count):
    """p followed by copies of its first `count` points"""
    return np.concatenate([p, p[:count]], axis=0)


def _batch(graphs, rng, dtype=np.float32, same_order=False):
    """(B, N, C): every graph's node order shuffled (fixed seed: `rng`); same_order: one permutation for all graphs"""
    n = graphs[0].shape[0]
    perm = rng.permutation(n)
    out = []
    for g in graphs:
        assert g.shape[0] == n
        out.append(g[perm if same_order else rng.permutation(n)])
    return np.stack(out).astype(dtype)


def _ragged(n, valid1):
    """graph 0 unmasked, graph 1 with `valid1` real nodes"""
    return np.arange(n)[None, :] < np.array([[n], [valid1]])


@functools.lru_cache(maxsize=None)
def _geometry(name, dtype="float32"):
    """(coors (B, N, C), mask (B, N)) of a named case, computed once and read-only; B = 2 (graph 0 unmasked, graph 1 ragged) unless the
    graph is large."""
    coors, mask = _build_geometry(name, dtype)
    coors.setflags(write=False)
    mask.setflags(write=False)
    return coors, mask


def _build_geometry(name, dtype):
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dt = np.dtype(dtype).type
    if name == "lattice8":
        # graph 0 the plain lattice, graph 1 scaled by 0.5 and shifted by a negative integer (coordinates of both signs)
        return _batch([lattice(8), 0.5 * lattice(8) - 2.0], rng, dt), _ragged(512, 400)
    if name == "lattice10":
        return _batch([0.5 * lattice(10) - 3.0, lattice(10)], rng, dt), _ragged(1000, 777)
    if name == "dups150x40":
        return _batch([dups(150, 40, rng)], rng, dt), (np.arange(6000) < 5800)[None]
    if name == "dups16x4":
        return _batch([dups(16, 4, rng), dups(16, 4, rng)], rng, dt), _ragged(64, 50)
    if name.startswith("point"):
        n = int(name[5:])
        return _batch([point(n), point(n)], rng, dt), _ragged(n, n - n // 4)
    if name == "line300_30valid":
        # fewer valid nodes than K = 40 in every row: the ties at 1e5 straddle K and are picked in index order
        return _batch([line(300), line(300)], rng, dt), np.broadcast_to(np.arange(300) < 30, (2, 300)).copy()
    if name.startswith("line"):
        n = int(name[4:])
        return _batch([line(n), line(n)], rng, dt), _ragged(n, n - n // 4)
    if name == "negzero125":
        return _batch([negzero(5, rng), negzero(5, rng)], rng, dt), _ragged(125, 100)
    if name == "lattice5_plus3":
        p = _with_repeats(lattice(5), 3)
        return _batch([p, p - 2.0], rng, dt), _ragged(128, 40)
    if name == "lattice32_2d":
        return _batch([lattice(32, 2), 0.5 * lattice(32, 2) - 7.0], rng, dt), _ragged(1024, 800)
    if name == "lattice4_5d":
        return _batch([lattice(4, 5), lattice(4, 5) - 1.0], rng, dt), _ragged(1024, 800)
    if name == "hypercube9":
        return _batch([hypercube9(), hypercube9()], rng, dt), _ragged(512, 400)
    if name == "lattice64_2d_plus4":
        return _batch([_with_repeats(lattice(64, 2), 4)], rng, dt), (np.arange(4100) < 4000)[None]
    if name == "lattice20_plus200":
        return _batch([_with_repeats(lattice(20), 200)], rng, dt), (np.arange(8200) < 8000)[None]
    if name == "lattice4":
        return _batch([lattice(4), lattice(4) - 2.0], rng, dt), _ragged(64, 50)
    raise KeyError(name)


MAX_COLUMNS = 129        # ranked candidates kept per row: every K below is <= 128, plus the (K + 1)-th for the tie condition


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype="float32"):
    """The oracle's ranking + stable top-k of a named geometry, computed once: the first min(N, 129) ranked candidates of every row
    (a stable sort's first K columns are the stable top-K for every K).  Read-only."""
    coors, mask = _geometry(name, dtype)
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, None)
    val, idx = O.topk_smallest(ranking, min(coors.shape[1], MAX_COLUMNS))
    val.setflags(write=False)
    idx.setflags(write=False)
    return val, idx


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_ties(val_sorted, k, what):
    """At least half of the checked rows -- and of the unmasked graph 0's -- have the K-th and the (K + 1)-th ranking value equal (from
    the oracle alone)."""
    tied = val_sorted[..., k - 1] == val_sorted[..., k]
    share = float(tied.mean())
    share0 = float(tied[0].mean()) if tied.ndim == 2 else share        # (graph 0 is unmasked: no rows of 1e5 alone)
    if VERBOSE:
        print(f"{what}: share of rows with a tie at K = {k}: {share:.2f} (graph 0: {share0:.2f})")
    assert share >= 0.5 and share0 >= 0.5, (what, k, share, share0)


def _assert_selection(ref_val, ref_idx, rank, idx, what):
    """indices and the bit patterns of the ranking values equal the oracle's; a mismatch reports the first differing row"""
    k = ref_idx.shape[-1]
    assert idx.shape == ref_idx.shape and rank.shape == ref_val.shape, (what, idx.shape, ref_idx.shape)
    ri, gi = ref_idx.reshape(-1, k).astype(np.int64), idx.reshape(-1, k).astype(np.int64)
    rv, gv = ref_val.reshape(-1, k), rank.reshape(-1, k)
    bad = np.flatnonzero((ri != gi).any(axis=1) | (_bits(rv) != _bits(gv)).any(axis=1))
    if bad.size:
        r = int(bad[0])
        col = int(np.flatnonzero((ri[r] != gi[r]) | (_bits(rv[r]) != _bits(gv[r])))[0])
        raise AssertionError(f"{what}: {bad.size} of {ri.shape[0]} rows differ; first: flat row {r}, column {col}, tied value "
                             f"{rv[r, col]!r}\n oracle idx {ri[r].tolist()}\n kernel idx {gi[r].tolist()}\n oracle rank {rv[r].tolist()}\n"
                             f" kernel rank {gv[r].tolist()}")
    np.testing.assert_array_equal(_bits(ref_val), _bits(rank))
    np.testing.assert_array_equal(ref_idx.astype(np.int32), idx)


def _no_tie_condition(name, k, n):
    """The cases the tie condition does not apply to: K = N (no (K + 1)-th candidate); K = 1 on a lattice (the self pair alone);
    K = 5 on a line, where the shells {0}, {+-1}, {+-2} are complete at K = 5 -- 0, 1, 1, 4, 4 | 9 -- so no tie can straddle it
    (the even K of `line300` below do tie)."""
    return k == n or (name.startswith("lattice") and k == 1) or (name.startswith("line") and k == 5)


def _check_selection(entry, name, k, dtype="float32"):
    from egnn_pytorch_amd import _ops
    coors, mask = _geometry(name, dtype)
    val, idx_sorted = _oracle(name, dtype)
    n = coors.shape[1]
    if not _no_tie_condition(name, k, n):
        _assert_ties(val, k, f"{name} K={k}")
    idx, rank = getattr(_ops, entry)(_dev(coors), _dev(mask), None, k)
    _assert_selection(val[..., :k], idx_sorted[..., :k], rank.cpu().numpy(), idx.cpu().numpy(), f"{entry} {name} K={k}")


# ------------------------------------------------------------------------------------------------ 1. selection, bit for bit
REGISTER_C3 = [
    ("lattice8", 7, "pair_path"), ("lattice8", 32, "pair_path"),                       # ties straddle K on the two-rows-per-wave path
    ("lattice10", 33, "lmin2_pruning"), ("lattice10", 64, "lmin2_pruning"),            # pruning on the two smallest keys per lane
    ("lattice10", 65, "radix_descent"), ("lattice10", 100, "radix_descent"),
    ("lattice8", 1, "self_pair_only"),
    ("dups150x40", 16, "survivor_handover"), ("dups150x40", 64, "survivor_handover"),  # far more than 128 survivors inside K <= 64
    ("dups16x4", 1, "lower_duplicate_wins"), ("dups16x4", 64, "k_equals_n"),
    ("point128", 8, "all_keys_equal"), ("point128", 64, "all_keys_equal"), ("point128", 128, "all_keys_equal"),
    ("line300", 5, "collinear"), ("line300", 6, "collinear"), ("line300", 40, "collinear"),
    ("negzero125", 8, "minus_zero"),
    ("lattice5_plus3", 64, "masked_ties_fill_the_row"),                                # graph 1: 40 valid nodes, 1e5 ties fill the row
]


@pytest.mark.parametrize("name,k,reaches", REGISTER_C3, ids=[f"knn_select_kernel_c3-{n}-k{k}-{r}" for n, k, r in REGISTER_C3])
def test_register_kernel_3d_against_the_oracle(name, k, reaches):
    _check_selection("knn_select", name, k)


@pytest.mark.parametrize("name", ["lattice32_2d", "lattice4_5d"], ids=lambda n: f"knn_select_kernel_c8-{n}-k24")
def test_register_kernel_other_dimensions_against_the_oracle(name):
    _check_selection("knn_select", name, 24)


ANY_KERNEL = [("hypercube9", 16, "float32"), ("hypercube9", 32, "float32"), ("hypercube9", 64, "float32"),
              ("lattice8", 7, "float64"), ("lattice8", 33, "float64"), ("dups16x4", 7, "float64"), ("dups16x4", 33, "float64"),
              ("line300_30valid", 40, "float64")]


@pytest.mark.parametrize("name,k,dtype", ANY_KERNEL, ids=[f"knn_select_any_kernel-{n}-k{k}-{d}" for n, k, d in ANY_KERNEL])
def test_any_kernel_against_the_oracle(name, k, dtype):
    """csrc/knn_rows.hip, the instantiations that read through pointers: more than 8 coordinates in float32 (K = 16, 32, 64 end inside
    a Hamming shell: 10, 46 and 130 would end on one), and float64 coordinates (the last case: 30 valid nodes, K = 40)."""
    _check_selection("knn_select", name, k, dtype)


@functools.lru_cache(maxsize=None)
def _sampled_rows(name):
    coors, mask = _geometry(name)
    n = coors.shape[1]
    valid = int(mask[0].sum())
    rng = np.random.default_rng(n)
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), [0, n - 1, valid - 1, valid]]))
    val, idx = _sampled_topk(coors, mask, None, rows, MAX_COLUMNS)
    val.setflags(write=False)
    idx.setflags(write=False)
    return rows, val, idx


LARGE = [("lattice64_2d_plus4", 24), ("lattice64_2d_plus4", 100), ("lattice20_plus200", 32), ("lattice20_plus200", 100)]


@pytest.mark.parametrize("name,k", LARGE, ids=[f"knn_select_large_kernel-{n}-k{k}" for n, k in LARGE])
def test_workgroup_per_row_kernel_against_the_oracle_on_sampled_rows(name, k):
    """N = 4100 in 2-D (beyond the 4096 of C != 3) and N = 8200 in 3-D (beyond 8192): 96 sampled rows plus rows 0, N - 1, the last
    valid row and the first padded row."""
    from egnn_pytorch_amd import _ops
    coors, mask = _geometry(name)
    rows, val, idx_sorted = _sampled_rows(name)
    assert len(rows) >= 96
    _assert_ties(val, k, f"{name} K={k}")
    idx, rank = _ops.knn_select(_dev(coors), _dev(mask), None, k)
    _assert_selection(val[:, :k], idx_sorted[:, :k], rank.cpu().numpy()[0, rows], idx.cpu().numpy()[0, rows],
                      f"knn_select {name} K={k} (rows {rows.tolist()})")


STREAM = [(n, k) for n in ("lattice10", "dups150x40", "point128", "hypercube9") for k in (16, 100)]


@pytest.mark.parametrize("name,k", STREAM, ids=[f"knn_select_stream-{n}-k{k}" for n, k in STREAM])
def test_streaming_kernel_against_the_oracle(name, k):
    """the streaming kernel against the ORACLE (tests/test_gpu_large_graphs.py compares it with the pinned kernels only)"""
    _check_selection("knn_select_stream", name, k)


def _lattice_bonds(coors):
    """(..., N, N) bool: nearest-neighbour bonds of lattice points (squared distance = the squared spacing), no diagonal"""
    d = ((coors[..., :, None, :] - coors[..., None, :, :]) ** 2).sum(-1)
    spacing = np.where(d > 0, d, np.inf).min(axis=(-1, -2), keepdims=True)
    return d == spacing


ADJ = [(form, diag, k) for form in ("NN", "BNN") for diag in (True, False) for k in (5, 9)]


@pytest.mark.parametrize("form,diag,k", ADJ, ids=[f"knn_select_kernel_adj-lattice8-{f}-{'diag' if d else 'nodiag'}-k{k}" for f, d, k in ADJ])
def test_register_kernel_with_lattice_bonds_against_the_oracle(form, diag, k):
    """Nearest-neighbour bonds of lattice(8) as adj_mat: rows have 3 to 6 bonds, so K = 5 is decided by the adjacency in the interior
    and by distance at faces and corners, K = 9 by distance everywhere.  Every row shares its first coordinate with another node, so
    none may be copied straight from the adjacency row (csrc/knn_select.hip: a non-adjacent node at distance 0 would tie)."""
    from egnn_pytorch_amd import _ops
    rng = np.random.default_rng(88 + k)
    graphs = [lattice(8), 0.5 * lattice(8) - 2.0]
    coors = _batch(graphs, rng, np.float32, same_order=(form == "NN"))
    mask = _ragged(512, 400)
    adj = _lattice_bonds(coors.astype(np.float64))
    deg = adj.sum(-1)
    assert deg.min() == 3 and deg.max() == 6
    if form == "NN":
        assert np.array_equal(adj[0], adj[1])
        adj = adj[0]
    if diag:
        adj = adj | np.eye(512, dtype=bool)
    _, dist = O.pairwise(coors)
    ranking, _ = O.build_ranking(dist, mask, adj)
    ref_val, ref_idx = O.topk_smallest(ranking, k)
    for entry in ("knn_select", "knn_select_stream"):
        idx, rank = getattr(_ops, entry)(_dev(coors), _dev(mask), _dev(adj), k)
        _assert_selection(ref_val, ref_idx, rank.cpu().numpy(), idx.cpu().numpy(), f"{entry} lattice8 bonds {form} diag={diag} K={k}")


# ------------------------------------------------------------------------------------------------ 2. spatial order, destination lists
def _layer(kw, seed, dtype=np.float32):
    """(cfg, params, module on the device in eval mode) with the oracle's seeded xavier-scale weights"""
    from egnn_pytorch_amd import EGNN
    cfg = O.EGNNConfig(**kw)
    params = O.random_params(cfg, seed=seed, dtype=dtype)
    net = EGNN(**kw)
    if dtype == np.float64:
        net = net.double()
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return cfg, params, net.cuda().eval()


@pytest.mark.parametrize("name", ["lattice8", "point128", "line300", "dups16x4"])
def test_spatial_order_on_coinciding_morton_keys(name, monkeypatch):
    """Many equal Morton keys: the order and its masked form are still permutations, padded nodes last, and a layer's outputs do not
    depend on the order, bit for bit."""
    from egnn_pytorch_amd import _ops, layer as L
    coors, mask = _geometry(name)
    b, n, _ = coors.shape
    cd, md = _dev(coors), _dev(mask)
    plain = _ops.spatial_order(cd).cpu().numpy()
    masked = _ops.spatial_order(cd, mask8=_ops._u8(md)).cpu().numpy()
    assert plain.shape == (b, n) and masked.shape == (b, n)
    for g in range(b):
        assert np.array_equal(np.sort(plain[g]), np.arange(n)), (name, g)
        assert np.array_equal(np.sort(masked[g]), np.arange(n)), (name, g)
        real = mask[g][masked[g]]
        nreal = int(mask[g].sum())
        assert real[:nreal].all() and not real[nreal:].any(), (name, g)
    _, _, net = _layer(dict(dim=32, num_nearest_neighbors=8), seed=3)
    feats = _dev(np.random.default_rng(n).standard_normal((b, n, 32)).astype(np.float32))
    with torch.no_grad():
        monkeypatch.setattr(L, "_SPATIAL_ORDER", True)
        n1, c1 = net(feats, cd, mask=md)
        monkeypatch.setattr(L, "_SPATIAL_ORDER", False)
        n0, c0 = net(feats, cd, mask=md)
    assert torch.equal(n0, n1) and torch.equal(c0, c1)


def test_dest_lists_when_every_row_selects_the_same_nodes():
    """Coincident nodes: every row of the index tensor is [0..31], in-degree 1024 for 32 nodes and 0 for the rest -- the full form of
    test_dest_lists_equal_a_stable_sort."""
    from egnn_pytorch_amd import _ops, autograd as A
    b, n, k = 2, 1024, 32
    idx, rank = _ops.knn_select(_dev(np.full((b, n, 3), 1.5, np.float32)), None, None, k)
    assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device="cuda").expand(b, n, k))
    assert bool((rank == 0).all())
    dest = (idx.long() + (torch.arange(b, device="cuda") * n)[:, None, None]).reshape(-1)
    dl = _ops.dest_lists(idx, b, n, k, "cuda")
    dl2 = _ops.dest_lists(idx, b, n, k, "cuda")
    dest_sorted, by_dest = torch.sort(dest, stable=True)
    seg = torch.searchsorted(dest_sorted, torch.arange(b * n + 1, device="cuda"))
    deg = seg.diff().view(b, n)
    assert bool((deg[:, :k] == n).all()) and bool((deg[:, k:] == 0).all())
    assert torch.equal(dl.seg, seg)
    assert torch.equal(dl.order, by_dest)
    ent, tile_seg = A.entry_list(by_dest, dest_sorted, b * n)
    assert torch.equal(dl.tile_seg, tile_seg) and torch.equal(dl.ent, ent)
    assert torch.equal(dl.ent, dl2.ent) and torch.equal(dl.order, dl2.order)


# ------------------------------------------------------------------------------------------------ 3. layers, forward
LAYER_GEOMETRIES = ["lattice4", "dups16x4", "point64", "line64"]
LAYER_CONFIGS = [
    ("plain", dict(dim=32, num_nearest_neighbors=8), np.float32),
    ("norm_coors_soft_edges", dict(dim=32, num_nearest_neighbors=8, norm_coors=True, soft_edges=True), np.float32),
    # (on a lattice the pairs at squared distance 2 sit exactly on the radius: the reference keeps `<=`, egnn_pytorch.py:260)
    ("fourier_radius_mean", dict(dim=32, num_nearest_neighbors=8, fourier_features=2, valid_radius=2.0, m_pool_method="mean"), np.float32),
    ("dense_norm_coors", dict(dim=32, norm_coors=True), np.float32),
    ("double", dict(dim=32, num_nearest_neighbors=8), np.float64),
]
LAYER_CASES = [(g, c) for g in LAYER_GEOMETRIES for c in LAYER_CONFIGS]
LAYER_IDS = [f"{g}-{c[0]}" for g, c in LAYER_CASES]


def _layer_inputs(geometry, dtype):
    coors, mask = _geometry(geometry, np.dtype(dtype).name)
    b, n, _ = coors.shape
    assert n == 64 and b == 2
    import zlib
    feats = np.random.default_rng(zlib.crc32(geometry.encode()) + 1).standard_normal((b, n, 32)).astype(dtype)
    return feats, coors, mask


@pytest.mark.parametrize("geometry,config", LAYER_CASES, ids=LAYER_IDS)
def test_layer_forward_against_the_oracle(geometry, config):
    from egnn_pytorch_amd import _ops, layer as L
    cname, kw, dtype = config
    feats, coors, mask = _layer_inputs(geometry, dtype)
    cfg, params, net = _layer(kw, seed=17, dtype=dtype)
    ref_node, ref_co, ref_rank, ref_idx = O.egnn_forward(cfg, params, feats, coors, None, mask, None, return_neighbors=True)
    fd, cd, md = _dev(feats), _dev(coors), _dev(mask)
    with torch.no_grad():
        checked = net._forward_hip_checked(fd, cd, None, md, None, None)
        idx, rank, radius = checked[3:6]
        # the neighbour list, bit for bit
        if ref_idx is None:
            assert idx is None and rank is None
        else:
            assert radius == kw.get("valid_radius", float("inf"))
            _assert_selection(ref_rank, ref_idx, rank.cpu().numpy(), idx.cpu().numpy(), f"layer {geometry} {cname}")
        # the module, twice
        calls = []
        orig = L.EGNN._forward_c
        L.EGNN._forward_c = lambda self, *a: calls.append(1) or orig(self, *a)
        try:
            node, co = net(fd, cd, None, md)
            node2, co2 = net(fd, cd, None, md)
        finally:
            L.EGNN._forward_c = orig
        if dtype == np.float32:
            assert L._C_FORWARD and calls, "the module's inference forward did not take the one-call path"
            launches = net._forward_hip(fd, cd, None, md, None)[:2]                 # the Python launch sequence
            one_call = _ops.forward_c(net, fd, cd, None, md, None)                  # the C host packer's blob, one C call
            torch.cuda.synchronize()
            assert torch.equal(one_call[0], node) and torch.equal(one_call[1], co)
        else:
            assert not calls and node.dtype == torch.float64
            launches = checked[:2]
        assert torch.equal(launches[0], node) and torch.equal(launches[1], co)
        assert torch.equal(node2, node) and torch.equal(co2, co)                    # a repeat: the same bits
        assert torch.equal(checked[0], node) and torch.equal(checked[1], co)
    for got, ref, what in ((node, ref_node, "node"), (co, ref_co, "coors")):
        got = got.cpu().numpy()
        scale = float(np.abs(ref).max())
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        if VERBOSE:
            print(f"{geometry} {cname} {what}: |out| <= {scale:.3g}, error {err:.3g}")
        assert np.isfinite(got).all()
        atol = ATOL * max(1.0, scale) if dtype == np.float32 else 1e-10 * scale
        np.testing.assert_allclose(got, ref, atol=atol, rtol=0, err_msg=f"{geometry} {cname} {what}")


def test_network_on_lattice_bonds_against_the_oracle():
    """EGNN_Network(num_adj_degrees=2, only_sparse_neighbors=True) with the lattice's nearest-neighbour bonds as adj_mat."""
    from egnn_pytorch_amd import EGNN_Network
    depth = 2
    kw = dict(depth=depth, dim=32, num_adj_degrees=2, adj_dim=2, only_sparse_neighbors=True)
    cfg = O.EGNNConfig(dim=32, edge_dim=2, only_sparse_neighbors=True, norm_feats=True)
    rng = np.random.default_rng(29)
    params = {"adj_emb.weight": rng.standard_normal((3, 2)).astype(np.float32)}
    for layer in range(depth):
        pl = O.random_params(cfg, seed=200 + layer, prefix=f"layers.{layer}.1.")
        pl[f"layers.{layer}.1.coors_mlp.3.weight"] *= np.float32(0.1)     # (stacked xavier-scale layers: keep the activations O(10),
        pl[f"layers.{layer}.1.node_mlp.3.weight"] *= np.float32(0.3)      #  as tests/test_gpu_parity.py::test_network_c3_vs_oracle does)
        pl[f"layers.{layer}.1.edge_mlp.3.weight"] *= np.float32(0.3)
        params.update(pl)
    coors, mask = _geometry("lattice4")
    b, n, _ = coors.shape
    adj = _lattice_bonds(coors.astype(np.float64))                        # (B, N, N): every graph has its own node order
    feats = rng.standard_normal((b, n, 32)).astype(np.float32)
    ref_node, ref_co = O.egnn_network_forward(depth, cfg, params, feats, coors, adj_mat=adj, mask=mask, num_adj_degrees=2)
    net = EGNN_Network(**kw)
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.cuda().eval()
    with torch.no_grad():
        node, co = net(_dev(feats), _dev(coors), adj_mat=_dev(adj), mask=_dev(mask))
        node2, co2 = net(_dev(feats), _dev(coors), adj_mat=_dev(adj), mask=_dev(mask))
    assert torch.equal(node, node2) and torch.equal(co, co2)
    for got, ref in ((node, ref_node), (co, ref_co)):
        np.testing.assert_allclose(got.cpu().numpy(), ref, atol=ATOL * max(1.0, float(np.abs(ref).max())), rtol=0)


# ------------------------------------------------------------------------------------------------ 4. layers, backward
# The one case whose native backward leaves the range of egnn_edge_bwd_pass_f32 (d/d W_2 holds SiLU(z) as fp16 x 2^6, up to 1023): the
# dense layer on the line, where real pairs reach |x_i - x_j|^2 = 3969 and SiLU(z) ~ 1200.  Its backward is answered by the plain-fp32
# re-run (autograd._w2_in_range_or_recomputed); every other case here must stay on the HIP backward.
RERUN_CASES = {("line64", "dense_norm_coors")}


@pytest.fixture
def backward_reruns():
    """call the returned function with the number of native backwards the test expects to have been re-run in plain fp32"""
    from egnn_pytorch_amd import autograd as A
    before = A.backward_reruns

    def check(expected):
        assert A.backward_reruns - before == expected, (A.backward_reruns - before, expected)
    return check


def _grad_names(net):
    return ["feats", "coors"] + [n for n, _ in net.named_parameters()]


def _restated_grads(net, feats, coors, mask, idx, rank, radius, loss_of, dtype, device):
    """gradients of `loss_of(node, coors_out)` through autograd.layer_given_neighbors over the given neighbour list, in `dtype`"""
    from egnn_pytorch_amd import autograd as A
    mod = copy.deepcopy(net).to(device=device, dtype=dtype)
    f = feats.detach().to(device=device, dtype=dtype).requires_grad_(True)
    c = coors.detach().to(device=device, dtype=dtype).requires_grad_(True)
    mv = lambda t: None if t is None else t.to(device)                  # noqa: E731
    with torch.enable_grad():
        node, co = A.layer_given_neighbors(mod, f, c, None, mv(mask), None if idx is None else mv(idx).long(),
                                           None if rank is None else mv(rank).to(dtype), radius)
        return torch.autograd.grad(loss_of(node, co), [f, c] + list(mod.parameters()), allow_unused=True)


@pytest.mark.parametrize("geometry,config", LAYER_CASES, ids=LAYER_IDS)
def test_layer_backward_against_float64_autograd(geometry, config, backward_reruns):
    """Every gradient within 1e-4 of its own scale of float64 autograd of the restated layer over the kernel's own neighbour list.
    d/d coors with norm_coors=True is the exception: x / clamp(|x|, 1e-8) of coincident pairs (the self pair, duplicated nodes) leaves
    cancellation noise in ANY fp32 autograd (tests/test_autograd.py), so its bar is the error of the fp32 CPU restatement on the same
    inputs, e_ref, with the margin of tests/test_gpu_parity.py: e_hip <= max(4 e_ref, 1e-4 scale)."""
    cname, kw, dtype = config
    feats, coors, mask = _layer_inputs(geometry, dtype)
    _, _, net = _layer(kw, seed=17, dtype=dtype)
    net.train()                                                          # (no dropout: train() only arms autograd-style use)
    fd, cd, md = _dev(feats), _dev(coors), _dev(mask)
    g = torch.Generator().manual_seed(6)
    rn = torch.randn(feats.shape, generator=g, dtype=torch.float64)
    rc = torch.randn(coors.shape, generator=g, dtype=torch.float64)
    loss_of = lambda node, co: (node * rn.to(node)).sum() + (co * rc.to(co)).sum()      # noqa: E731
    f, c = fd.clone().requires_grad_(True), cd.clone().requires_grad_(True)
    with torch.enable_grad():
        node, co = net(f, c, None, md)
        got = torch.autograd.grad(loss_of(node, co), [f, c] + list(net.parameters()), allow_unused=True)
    backward_reruns(1 if (geometry, cname) in RERUN_CASES else 0)
    with torch.no_grad():
        idx, rank, radius = net._forward_hip_checked(fd, cd, None, md, None, None)[3:6]
    want = _restated_grads(net, fd, cd, md, idx, rank, radius, loss_of, torch.float64, "cuda")
    names = _grad_names(net)
    assert len(got) == len(want) == len(names)
    rel = 1e-4 if dtype == np.float32 else 1e-8
    for name, a, r in zip(names, got, want):
        assert (a is None) == (r is None), name
        if a is None:
            continue
        assert torch.isfinite(a).all(), name
        scale = float(r.abs().max())
        e_hip = float((a.double() - r).abs().max())
        if name == "coors" and kw.get("norm_coors"):
            ref32 = _restated_grads(net, fd, cd, md, idx, rank, radius, loss_of, torch.float32, "cpu")[1]
            e_ref = float((ref32.double() - r.cpu()).abs().max())
            if VERBOSE:
                print(f"{geometry} {cname} d/d coors: scale {scale:.3g}, fp32 restatement vs float64 {e_ref:.3g}, HIP vs float64 {e_hip:.3g}")
            assert e_hip <= max(4.0 * e_ref, 1e-4 * scale), (geometry, cname, name, scale, e_ref, e_hip)
        else:
            if VERBOSE:
                print(f"{geometry} {cname} d/d {name}: scale {scale:.3g}, HIP vs float64 {e_hip:.3g}")
            assert e_hip <= rel * scale, (geometry, cname, name, scale, e_hip)       # (a reference of exactly 0: exactly 0)


@pytest.mark.parametrize("geometry", LAYER_GEOMETRIES)
def test_layer_force_matching_against_float64_autograd(geometry, backward_reruns):
    """create_graph=True: one force-matching loss (tests/test_second_order.py::force_matching_grads) through the layer, every gradient
    within 1e-4 of its own scale of the same loss through the float64 restatement over the kernel's own neighbour list."""
    from egnn_pytorch_amd import autograd as A
    kw = dict(dim=32, num_nearest_neighbors=8)
    feats, coors, mask = _layer_inputs(geometry, np.float32)
    _, _, net = _layer(kw, seed=17)
    net.train()
    fd, cd, md = _dev(feats), _dev(coors), _dev(mask)
    f, c = fd.clone().requires_grad_(True), cd.clone().requires_grad_(True)
    with torch.enable_grad():
        got = force_matching_grads(net, lambda: net(f, c, None, md), c, [c, f] + list(net.parameters()))
    with torch.no_grad():
        idx, rank, radius = net._forward_hip_checked(fd, cd, None, md, None, None)[3:6]
    n64 = copy.deepcopy(net).double()
    f2, c2 = fd.double().requires_grad_(True), cd.double().requires_grad_(True)
    with torch.enable_grad():
        want = force_matching_grads(n64, lambda: A.layer_given_neighbors(n64, f2, c2, None, md, idx.long(), rank.double(), radius),
                                    c2, [c2, f2] + list(n64.parameters()))
    names = ["coors", "feats"] + [n for n, _ in net.named_parameters()]
    for name, a, r in zip(names, got, want):
        assert (a is None) == (r is None), name
        if a is None:
            continue
        assert torch.isfinite(a).all(), name
        scale = float(r.abs().max())
        err = float((a.double() - r).abs().max())
        if VERBOSE:
            print(f"{geometry} force matching d/d {name}: scale {scale:.3g}, HIP vs float64 {err:.3g}")
        assert err <= 1e-4 * scale, (geometry, name, scale, err)                    # (a reference of exactly 0: exactly 0)
    backward_reruns(0)
