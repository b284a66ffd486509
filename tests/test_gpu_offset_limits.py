"""Forward and training at the sizes where a kernel's tables pass 2^31 elements, 2^31 bytes and 2^32 bytes (DESIGN.md section 6 lists
the boundaries and which case crosses each).

Oracle: graphs never interact, and far-apart clusters of one graph never interact either, so a huge call is checked against THE SAME
LAYER ON SMALL PARTS -- batch slices of 64 graphs, or single clusters of 4096 nodes -- which test_gpu_parity.py, test_autograd.py and
test_gpu_large_graphs.py pin to the reference and to float64.  Nothing runs at the full sizes but the code under test.

Inputs: Xavier-scale weights (the default 1e-3 init makes a wrong row invisible), ragged masks, features generated on the device.
Bars (all the project's own): batch slices of an inference call bit-equal (tests/test_gpu_rccl.py); clusters alone against the big graph
rtol = atol = 1e-5 (tests/test_gpu_large_graphs.py -- not torch.equal: a graph beyond 4 GB runs on the plain-fp32 kernels, its clusters
alone on the split-fp16 ones); gradients 1e-4 of each gradient's own scale with max |reference| > 0, parameter gradients against the
float64 sum of the parts' gradients; float64 modules 1e-9 forward / 1e-8 of scale (tests/test_gpu_mask_patterns_training.py).

Every case computes its table sizes from the shape (egnn_padded_hidden, ldp = 2 Hp), asserts that the boundary it is named for is
crossed, that the compared rows lie on both sides of it and include the table's last row, and that the layer moves the compared rows
by far more than the bar.  Every case keeps torch.cuda.max_memory_allocated() under 24 GB and may skip only with less than 32 GB free.
E = B N K >= 2^31 needs more than 50 GB of index tensors and stays out of scope."""
import contextlib
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GB = 1 << 30
CL = 4096                        # nodes per cluster
I31, I32 = 1 << 31, 1 << 32


# ------------------------------------------------------------------ helpers
@contextlib.contextmanager
def _budget(what):
    """the conditions every case runs under: 32 GB free or skip, peak allocation below 24 GB, everything freed afterwards"""
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 32 * GB:
        pytest.skip(f"{free / GB:.1f} GB free on the device; these shapes want 32 GB")
    torch.cuda.reset_peak_memory_stats()
    try:
        with _switches(_warn_rerun=_no_rerun):
            yield
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"OFFSET-LIMITS {what}: peak {peak / GB:.2f} GB", flush=True)
        assert peak < 24 * GB, (what, peak / GB)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


def _no_rerun(err):
    """No case may be answered by the automatic plain-fp32 re-run (layer.py::_warn_rerun is called when one starts): rows read through a
    wrapped offset can trip the range status by accident, and the re-run then hides them -- but only while the status is read
    synchronously (not with EGNN_RANGE_CHECK=off / deferred, not under graph capture)."""
    raise AssertionError(f"the call was answered by the plain-fp32 re-run, not by the path under test: {err}")


def _widths(dim, edge_dim=0, fourier=0):
    """(H, Hp, ldp) of the split-fp16 path's projection table: rows of ldp = 2 Hp floats"""
    from egnn_pytorch_amd import _abi
    h = 2 * (2 * fourier + 2 * dim + edge_dim + 1)
    hp = _abi.load().egnn_padded_hidden(h)
    return h, hp, 2 * hp


def _exact_ld(dim, edge_dim=0, fourier=0):
    """row length of the plain kernels' projection table (layer.py::_forward_exact: 2 hq, hq = H rounded up to 4)"""
    h = 2 * (2 * fourier + 2 * dim + edge_dim + 1)
    return 2 * ((h + 3) // 4 * 4)


def _layer(seed, **kw):
    from egnn_pytorch_amd import EGNN
    g = torch.Generator().manual_seed(seed)
    layer = EGNN(**kw)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, generator=g)
    return layer.cuda().eval()


def _batch(b, n, dim, k, seed, dtype=torch.float32):
    """device-generated features and coordinates, a ragged mask (every graph keeps >= max(K, N / 2) nodes; the last graph is full, so
    that the table's last row is a real node)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    feats = torch.randn(b, n, dim, device="cuda", generator=g, dtype=dtype)
    coors = torch.randn(b, n, 3, device="cuda", generator=g, dtype=dtype)
    lens = torch.randint(max(k, n // 2), n + 1, (b, 1), device="cuda", generator=g)
    lens[-1] = n
    mask = torch.arange(n, device="cuda")[None] < lens
    return feats, coors, mask


def _cluster_graph(n_clusters, dim, k, seed, dtype=torch.float32, real_nodes=None):
    """one graph of unit-normal clusters of 4096 nodes on a 5 x 4 x 4 grid of spacing 40 (squared distances across clusters > ~900, all
    < 1e5), each with a ragged tail of padding (>= 3 K real nodes); the first and the last cluster are full"""
    assert n_clusters <= 80
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in range(5) for y in range(4) for z in range(4)], dtype=np.float64)[:n_clusters] * 40.0
    coors = np.concatenate([rng.standard_normal((CL, 3)) + grid[c] for c in range(n_clusters)])[None]
    real = CL - rng.integers(0, CL - 3 * k, size=n_clusters)
    real[0] = real[-1] = CL
    for c, count in (real_nodes or {}).items():                           # {cluster: its number of real nodes}
        real[c] = count
    mask = np.concatenate([np.arange(CL) < real[c] for c in range(n_clusters)])[None]
    g = torch.Generator(device="cuda").manual_seed(seed)
    feats = torch.randn(1, n_clusters * CL, dim, device="cuda", generator=g, dtype=dtype)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    return feats, torch.from_numpy(coors.astype(np_dtype)).cuda(), torch.from_numpy(mask).cuda()


def _cluster_of_byte(byte, row_bytes):
    return byte // row_bytes // CL


def _covers_both_sides(ranges, boundary_row, last_row):
    """the compared row ranges hold a row below the boundary, a row at or above it, and the table's last row"""
    assert any(lo < boundary_row for lo, hi in ranges), (ranges, boundary_row)
    assert any(hi > boundary_row for lo, hi in ranges), (ranges, boundary_row)
    assert any(lo <= last_row < hi for lo, hi in ranges), (ranges, last_row)


def _moved(out, inp, floor):
    """the layer changes the compared rows by far more than the bar: a comparison of untouched rows would pass vacuously"""
    d = float((out - inp).abs().max())
    assert d > floor, (d, floor)


def _compare_batch_slices(layer, feats, coors, mask, big, slices, what, edges=None, atol=None):
    """the big call's rows of graphs [lo, hi) against the same layer on those graphs alone: bit-equal, or within `atol` (float64)"""
    for lo, hi in slices:
        with torch.no_grad():
            kw = {} if edges is None else {"edges": edges[lo:hi]}
            node, co = layer(feats[lo:hi], coors[lo:hi], mask=mask[lo:hi], **kw)
        for name, got, ref in (("feats", big[0][lo:hi], node), ("coors", big[1][lo:hi], co)):
            assert bool(torch.isfinite(ref).all()), (what, name, lo, "non-finite reference")
            if atol is None:
                assert torch.equal(got, ref), (what, name, (lo, hi), float((got - ref).abs().max()))
            else:
                err = float((got - ref).abs().max())
                assert err <= atol, (what, name, (lo, hi), err)
        _moved(node, feats[lo:hi], 1e-2)
        del node, co


def _compare_clusters(layer, feats, coors, mask, big, clusters, what, real_only=False):
    """(real_only -- NaN padding: the feature rows of real nodes; a padded node's output row is whatever its input row gives)"""
    for c in clusters:
        s = slice(c * CL, (c + 1) * CL)
        real = mask[0, s] if real_only else torch.ones_like(mask[0, s])
        with torch.no_grad():
            node, co = layer(feats[:, s], coors[:, s], mask=mask[:, s])
        assert bool(torch.isfinite(node[0, real]).all()) and bool(torch.isfinite(co).all()), (what, c)
        _moved(node[0, real], feats[0, s][real], 1e-2)                   # (the bar is 1e-5)
        torch.testing.assert_close(big[0][0, s][real], node[0, real], rtol=1e-5, atol=1e-5,
                                   msg=lambda m: f"{what}, cluster {c}, feats: {m}")
        torch.testing.assert_close(big[1][:, s], co, rtol=1e-5, atol=1e-5, msg=lambda m: f"{what}, cluster {c}, coors: {m}")
        del node, co


@contextlib.contextmanager
def _switches(**kw):
    from egnn_pytorch_amd import layer as L
    old = {k: getattr(L, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(L, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(L, k, v)


# ------------------------------------------------------------------ a. a batch whose P table passes 2^31 elements
def test_a_batch_table_beyond_2_31_elements_equals_its_slices():
    """B = 520 graphs of 1024 nodes, K = 32, dim = 512 (BASELINE.json's c5 global batch is 512 of them): 532 480 table rows of 4160 floats
    -- more than 2^31 ELEMENTS, 8.9 GB -- behind the projection GEMM's epilogue, the edge pass's per-graph bases, the node images.  The
    one-call C forward, the Python launch sequence and the general edge kernel, each against all slices of 64 graphs (and the
    remainder of 8) of the default path: bit-equal."""
    b, n, k, dim = 520, 1024, 32, 512
    _, _, ldp = _widths(dim)
    assert b * n * ldp > I31, "the table does not pass 2^31 elements"
    slices = [(lo, min(b, lo + 64)) for lo in range(0, b, 64)]
    _covers_both_sides([(lo * n, hi * n) for lo, hi in slices], I31 // ldp, b * n - 1)
    with _budget("a"):
        _run_a(b, n, k, dim, slices)


def _run_a(b, n, k, dim, slices):
    from egnn_pytorch_amd import layer as L
    layer = _layer(101, dim=dim, num_nearest_neighbors=k)
    feats, coors, mask = _batch(b, n, dim, k, 102)
    assert L._C_FORWARD and L._default_policy()
    with torch.no_grad():                                               # the reference once: the default path on the slices
        parts = [layer(feats[lo:hi], coors[lo:hi], mask=mask[lo:hi]) for lo, hi in slices]
    ref = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    del parts
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[1]).all())
    _moved(ref[0], feats, 1e-2)
    bad = []
    for what, kw in (("c_forward", {}), ("python_launch", dict(_C_FORWARD=False)), ("general_kernel", dict(_EDGE_ALGO=1))):
        with _switches(**kw), torch.no_grad():
            big = layer(feats, coors, mask=mask)
        for name, got, want in (("feats", big[0], ref[0]), ("coors", big[1], ref[1])):
            if not torch.equal(got, want):
                rows = (got != want).flatten(2).any(-1).flatten().nonzero().flatten()
                bad.append((what, name, int(rows.numel()), int(rows[0]), int(rows[-1]), float((got - want).abs().max())))
        del big
    assert not bad, bad                                                  # (path, output, rows that differ, first, last, max |diff|)


# ------------------------------------------------------------------ b, c. one graph beyond 2^32 / 2^31 bytes
@pytest.mark.parametrize("range_check", ["sync", "off"])
def test_b_single_graph_beyond_2_32_bytes_equals_its_clusters(range_check):
    """One graph of 66 clusters (270 336 nodes, cell-grid selection), K = 32, dim = 512: its rows of the projection table take more than
    2^32 bytes, which no 32-bit byte offset of the fused edge kernels reaches -- the layer has to answer on a path that addresses it
    (the plain-fp32 kernels: egnn_edge_fused_covers).  Clusters 0, the two around byte 2^31, the two around byte 2^32 and the last,
    each against the layer on that cluster alone, at rtol = atol = 1e-5.  With the range status read synchronously and not at all:
    before egnn_edge_fused_covers the general kernel ran this graph on wrapped offsets, and only the range status -- tripped by the
    garbage -- had the call re-run on the plain kernels."""
    from egnn_pytorch_amd import _ops
    n_clusters, k, dim = 66, 32, 512
    row_bytes = _widths(dim)[2] * 4
    n = n_clusters * CL
    assert n * row_bytes > I32, "the graph's table does not pass 2^32 bytes"
    c31, c32 = _cluster_of_byte(I31, row_bytes), _cluster_of_byte(I32, row_bytes)
    assert n_clusters == c32 + 3, "not the smallest such graph: the boundary's cluster, the one after it, and a last one"
    clusters = sorted({0, c31, c31 + 1, c32, c32 + 1, n_clusters - 1})
    assert clusters[-1] == n_clusters - 1 and c32 + 1 <= n_clusters - 1
    ranges = [(c * CL, (c + 1) * CL) for c in clusters]
    _covers_both_sides(ranges, I32 // row_bytes, n - 1)
    _covers_both_sides(ranges, I31 // row_bytes, n - 1)
    old = _ops.RANGE_CHECK
    try:
        _ops.RANGE_CHECK = range_check
        with _budget(f"b/{range_check}"):
            _run_clusters(n_clusters, k, dim, clusters, 201, f"b/{range_check}", [{}])
    finally:
        _ops.RANGE_CHECK = old


@pytest.mark.parametrize("algo", [0, 1])
def test_c_single_graph_between_2_31_and_2_32_bytes_equals_its_clusters(algo):
    """As (b) with 40 clusters (163 840 nodes, 2.7 GB of table rows): per-lane byte offsets with the top bit set, on the wave-per-node
    kernel (algo 0) and the general one (algo 1).  Clusters 0, the two around byte 2^31 and the last."""
    from egnn_pytorch_amd import _abi
    n_clusters, k, dim = 40, 32, 512
    ldp = _widths(dim)[2]
    row_bytes = ldp * 4
    n = n_clusters * CL
    assert I31 < n * row_bytes <= 0xffffffff
    lib = _abi.load()
    assert lib.egnn_edge_fused_covers(n, k, ldp) == 1
    assert lib.egnn_edge_pw_covers(1, n, k, 1, 0, 0, 16, 3, ldp) == 1    # algo 0 really is the wave-per-node kernel
    c31 = _cluster_of_byte(I31, row_bytes)
    clusters = sorted({0, c31, c31 + 1, n_clusters - 1})
    _covers_both_sides([(c * CL, (c + 1) * CL) for c in clusters], I31 // row_bytes, n - 1)
    with _budget(f"c/algo{algo}"):
        _run_clusters(n_clusters, k, dim, clusters, 301, f"c/algo{algo}", [dict(_EDGE_ALGO=algo)])


def test_c_tiles_of_several_nodes_beyond_2_31_bytes_keep_padding_out():
    """As (c) with K = 16: a 16-slot tile of the general kernel carries the P_i rows of up to four nodes and reads "no such row" at
    byte offset 0x80000000 -- a real row once the graph's table passes 2^31 bytes, and whatever a padded node holds there (NaN here, which
    tests/test_gpu_parity.py::test_nan_padding_behind_the_mask_is_harmless allows) would reach the tile's valid edges.
    egnn_edge_fused_covers hands such a graph to the plain kernels.  Real rows of clusters 0, the two around byte 2^31 and the last, against
    the clusters alone (NaN-padded as well)."""
    from egnn_pytorch_amd import _abi
    n_clusters, k, dim = 40, 16, 512
    ldp = _widths(dim)[2]
    row_bytes = ldp * 4
    n = n_clusters * CL
    assert I31 < n * row_bytes <= 0xffffffff
    assert _abi.load().egnn_edge_fused_covers(n, k, ldp) == 0 and _abi.load().egnn_edge_fused_covers(CL, k, ldp) == 1
    c31 = _cluster_of_byte(I31, row_bytes)
    clusters = sorted({0, c31, c31 + 1, n_clusters - 1})
    _covers_both_sides([(c * CL, (c + 1) * CL) for c in clusters], I31 // row_bytes, n - 1)
    with _budget("c/k16"):
        _run_clusters(n_clusters, k, dim, clusters, 311, "c/k16", [{}], nan_padding=True)


def _run_clusters(n_clusters, k, dim, clusters, seed, what, switch_sets, nan_padding=False):
    from egnn_pytorch_amd import layer as L
    layer = _layer(seed, dim=dim, num_nearest_neighbors=k)
    row31 = I31 // (_widths(dim)[2] * 4)                                  # the row at byte offset 2^31 of the graph's table
    feats, coors, mask = _cluster_graph(n_clusters, dim, k, seed + 1, real_nodes={row31 // CL: max(3 * k, row31 % CL // 2)} if nan_padding else None)
    assert feats.shape[1] >= L._KNN_GRID_MIN_N                            # (the cell grid selects the neighbours)
    if nan_padding:
        assert not bool(mask[0, row31]), "the row at byte 2^31 is not a padded one"
        feats[~mask] = float("nan")
    for kw in switch_sets:
        with _switches(**kw), torch.no_grad():
            big = layer(feats, coors, mask=mask)
        assert bool(torch.isfinite(big[0][mask]).all()) and bool(torch.isfinite(big[1]).all()), what
        _compare_clusters(layer, feats, coors, mask, big, clusters, what, real_only=nan_padding)   # (the clusters alone: the default path)
        del big


# ------------------------------------------------------------------ d. slot records beyond 2^32 bytes
def test_d_slot_records_beyond_2_32_bytes_equal_their_slices():
    """B = 8200 graphs of 1024 nodes, K = 32, dim = 8: the per-slot records take B N K 16 > 2^32 bytes (the wave-per-node kernel declines:
    the general kernel reads them), idx and rank pass 2^28 entries, the batch's P table passes 2^32 bytes.  The first 64 graphs, the 64
    below record byte 2^32, the graphs from there on and the last 64: bit-equal."""
    from egnn_pytorch_amd import _abi
    b, n, k, dim = 8200, 1024, 32, 8
    _, _, ldp = _widths(dim)
    rec_graph = n * k * 16
    assert b * rec_graph > I32 and (b - 8) * rec_graph <= I32, "not the smallest batch (in steps of 8) beyond 2^32 bytes of records"
    assert b * n * k > 1 << 28 and b * n * k < I31
    assert b * n * ldp * 4 > I32
    assert _abi.load().egnn_edge_pw_covers(b, n, k, 1, 0, 0, 16, 3, ldp) == 0
    assert _abi.load().egnn_edge_pw_covers(64, n, k, 1, 0, 0, 16, 3, ldp) == 1   # (the slices run the wave-per-node kernel: same bits)
    g0 = I32 // rec_graph                                                 # the graph whose records start at byte 2^32
    slices = [(0, 64), (g0 - 64, g0), (g0, b), (b - 64, b)]
    assert 64 < g0 < b
    _covers_both_sides([(lo * n, hi * n) for lo, hi in slices], g0 * n, b * n - 1)
    _covers_both_sides([(lo * n, hi * n) for lo, hi in slices], I32 // (ldp * 4), b * n - 1)
    with _budget("d"):
        _run_batch(b, n, k, dim, slices, 401, "d")


def _run_batch(b, n, k, dim, slices, seed, what, layer_kw=None, ctx=contextlib.nullcontext, dtype=torch.float32, atol=None,
               edge_dim=0, check=None):
    kw = dict(dim=dim, num_nearest_neighbors=k) if k else dict(dim=dim)
    kw.update(layer_kw or {})
    layer = _layer(seed, **kw)
    if dtype == torch.float64:
        layer = layer.double()
    feats, coors, mask = _batch(b, n, dim, k or 1, seed + 1, dtype)
    edges = None
    if edge_dim:
        edges = torch.randn(b, n, n, edge_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 2))
    if check is not None:
        check(layer, b, n)
    with ctx(), torch.no_grad():
        big = layer(feats, coors, mask=mask) if edges is None else layer(feats, coors, edges=edges, mask=mask)
        assert bool(torch.isfinite(big[0]).all()) and bool(torch.isfinite(big[1]).all()), what
        _compare_batch_slices(layer, feats, coors, mask, big, slices, what, edges=edges, atol=atol)


# ------------------------------------------------------------------ e. dense layers beyond 2^32 bytes of table
@pytest.mark.parametrize("kernel", ["general", "dense_pw"])
def test_e_dense_layer_table_beyond_2_32_bytes_equals_its_slices(kernel):
    """Dense all-pairs layers at dim = 512 whose batch P table passes 2^32 bytes.  general: B = 1040, N = 256 (the general kernel: the
    wave-per-node kernel takes dense batches only up to 2^28 bytes of records, layer.py::_dense_pw).  dense_pw: N = 32, where that bound
    leaves room -- the smallest B (in steps of 8) beyond 2^32 bytes -- on the wave-per-node kernel.  First, middle and last slices of 64."""
    dim = 512
    ldp = _widths(dim)[2]
    if kernel == "general":
        b, n = 1040, 256
    else:
        n = 32
        b = (I32 // (n * ldp * 4) + 8) // 8 * 8
    assert b * n * ldp * 4 > I32
    at = min(b - 64, I32 // (n * ldp * 4) - 32)                            # a slice that holds byte 2^32
    slices = [(0, 64), (b // 2 - 32, b // 2 + 32), (at, at + 64), (b - 64, b)]
    _covers_both_sides([(lo * n, hi * n) for lo, hi in slices], I32 // (ldp * 4), b * n - 1)

    def check(layer, b_, n_):
        from egnn_pytorch_amd import layer as L
        assert layer._dense_pw(b_, n_, 3) == (kernel == "dense_pw")
        assert kernel == "dense_pw" or (not L._DENSE_PW and not layer._dense_pw(64, n_, 3))

    # (general: the slices of 64 would take the wave-per-node kernel, which sums a node's eight rounds of K = 256 in another order than
    # the general kernel -- both calls on the general kernel; dense_pw: one round per node, the same bits on either kernel)
    with _budget(f"e/{kernel}"), _switches(**({"_DENSE_PW": False} if kernel == "general" else {})):
        _run_batch(b, n, 0, dim, slices, 501, f"e/{kernel}", check=check)


# ------------------------------------------------------------------ f. dense float edges beyond 2^31 elements
def test_f_dense_edge_features_beyond_2_31_elements_equal_their_slices():
    """B = 140, N = 1024, K = 8, dim = 16, edge_dim = 15 with a dense float (B, N, N, 15) `edges`: 2.2 G elements, read at the selected
    pairs.  All slices of 64 (and the remainder): bit-equal."""
    b, n, k, dim, ed = 140, 1024, 8, 16, 15
    assert b * n * n * ed > I31 and (b - 4) * n * n * ed <= I31
    slices = [(lo, min(b, lo + 64)) for lo in range(0, b, 64)]
    g0 = I31 // (n * n * ed)
    _covers_both_sides(slices, g0, b - 1)
    with _budget("f"):
        _run_batch(b, n, k, dim, slices, 601, "f", layer_kw=dict(edge_dim=ed), edge_dim=ed)


# ------------------------------------------------------------------ g. the plain-fp32 and float64 kernels beyond 2^32 bytes
@pytest.mark.parametrize("mode", ["exact", "double"])
def test_g_plain_kernels_table_beyond_2_32_bytes_equals_its_slices(mode):
    """exact_arithmetic() and a .double() module at the smallest B x 1024, K = 32, dim = 512 that puts THEIR projection table (rows of
    2 hq elements, layer.py::_forward_exact; float64 halves the row count) past 2^32 bytes.  All slices of 64: bit-equal in plain fp32,
    float64 at its forward bar of 1e-9."""
    from egnn_pytorch_amd import exact_arithmetic
    n, k, dim = 1024, 32, 512
    esz = 8 if mode == "double" else 4
    row_bytes = _exact_ld(dim) * esz
    b = I32 // (n * row_bytes) + 1
    assert b * n * row_bytes > I32 and (b - 1) * n * row_bytes <= I32
    slices = [(lo, min(b, lo + 64)) for lo in range(0, b, 64)]
    _covers_both_sides([(lo * n, hi * n) for lo, hi in slices], I32 // row_bytes, b * n - 1)
    with _budget(f"g/{mode}"):
        if mode == "exact":
            _run_batch(b, n, k, dim, slices, 701, "g/exact", ctx=exact_arithmetic)
        else:
            _run_batch(b, n, k, dim, slices, 702, "g/double", dtype=torch.float64, atol=1e-9)


# ------------------------------------------------------------------ training
def _grads(layer, feats, coors, mask, wn, wc, s, batch_dim):
    """(d/d feats, d/d coors, {parameter: gradient}, node_out) of sum(node * wn) + sum(coors_out * wc) over the part `s` of dimension
    `batch_dim` (0: graphs, 1: nodes of the one graph)"""
    cut = (lambda t: t[s]) if batch_dim == 0 else (lambda t: t[:, s])
    layer.zero_grad(set_to_none=True)
    f = cut(feats).clone().requires_grad_(True)
    x = cut(coors).clone().requires_grad_(True)
    node, co = layer(f, x, mask=cut(mask))
    ((node * cut(wn)).sum() + (co * cut(wc)).sum()).backward()
    pg = {name: p.grad.detach().clone() for name, p in layer.named_parameters() if p.grad is not None}
    layer.zero_grad(set_to_none=True)
    return f.grad, x.grad, pg, node.detach()


def _check_training(layer, feats, coors, mask, parts, compare, batch_dim, what, tol, seed):
    """the whole call's gradients against the parts': input gradients on the parts in `compare`, parameter gradients against the float64
    sum over ALL parts; each within `tol` of its own scale"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    wn = torch.randn(feats.shape, device="cuda", generator=g, dtype=feats.dtype) * mask[..., None]
    wc = torch.randn(coors.shape, device="cuda", generator=g, dtype=coors.dtype) * mask[..., None]
    whole = slice(0, feats.shape[batch_dim])
    gf, gc, gp, node = _grads(layer, feats, coors, mask, wn, wc, whole, batch_dim)
    assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gc).all()) and bool(torch.isfinite(node).all()), what
    _moved(node, feats, 1e-2)
    cut = (lambda t, s: t[s]) if batch_dim == 0 else (lambda t, s: t[:, s])
    psum, worst = None, {}
    for s in parts:
        f1, c1, p1, node1 = _grads(layer, feats, coors, mask, wn, wc, s, batch_dim)
        psum = {nm: v.double() for nm, v in p1.items()} if psum is None else {nm: psum[nm] + p1[nm].double() for nm in p1}
        if s in compare:
            for nm, got, ref in (("feats", cut(gf, s), f1), ("coors", cut(gc, s), c1)):
                scale = float(ref.abs().max())
                assert scale > 0, (what, nm, s, "the reference gradient vanishes")
                worst[f"{nm}[{s.start}:{s.stop}]"] = float((got.double() - ref.double()).abs().max()) / scale
        del f1, c1, p1, node1
    assert gp.keys() == psum.keys()
    for nm in gp:
        scale = float(psum[nm].abs().max())
        assert scale > 0, (what, nm, "the reference gradient vanishes")
        assert bool(torch.isfinite(gp[nm]).all()), (what, nm)
        worst[nm] = float((gp[nm].double() - psum[nm]).abs().max()) / scale
    print(f"OFFSET-LIMITS {what}: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()), flush=True)
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (what, bad)


def test_h_training_chunks_by_the_size_formula():
    """Training, B = 160, N = 1024, K = 32, dim = 512, fp32: the backward splits the batch by `_fused_graphs_per_chunk` alone (no
    `_FUSED_MAX_GRAPHS`) -- into chunks whose P table and partial rows sit just below 2^31 bytes.  Against parts of 64 / 64 / 32 graphs, so
    that no part boundary coincides with a chunk boundary."""
    from egnn_pytorch_amd import autograd as A
    b, n, k, dim = 160, 1024, 32, 512
    hp = _widths(dim)[1]
    assert A._FUSED_MAX_GRAPHS == 0
    step = A._fused_graphs_per_chunk(b, n, k, hp)
    assert 0 < step < b and step not in (64, 128), step                   # really chunked, and not at a part boundary
    assert b * n * 2 * hp * 4 > I31                                       # the whole batch's table would not fit one call
    parts = [slice(0, 64), slice(64, 128), slice(128, 160)]
    with _budget("h"):
        layer = _layer(801, dim=dim, num_nearest_neighbors=k)
        feats, coors, mask = _batch(b, n, dim, k, 802)
        _check_training(layer, feats, coors, mask, parts, parts, 0, "h", 1e-4, 803)
        del layer, feats, coors, mask


def _largest_trainable_clusters(k, hp):
    from egnn_pytorch_amd import autograd as A
    c = 1
    while A._fused_graphs_per_chunk(1, (c + 1) * CL, k, hp) == 1:
        c += 1
    return c


def test_i_single_graph_beyond_the_fused_backward_raises_before_any_launch():
    """Training one graph of 34 clusters (139 264 nodes), K = 32, dim = 512: its projection table alone passes the fused backward's 2^31
    bytes, and no chunk of graphs can hold it.  The call raises FusedBackwardLimit -- naming the limit and the shape -- from the forward,
    before anything is launched (nothing is allocated); the same call under no_grad answers.  (README section Scope and DESIGN.md
    section 9 item 7 state the limit in nodes.)"""
    from egnn_pytorch_amd import autograd as A
    n_clusters, k, dim = 34, 32, 512
    hp = _widths(dim)[1]
    n = n_clusters * CL
    assert n * 2 * hp * 4 > I31
    assert A._fused_graphs_per_chunk(1, n, k, hp) == 0
    with _budget("i"):
        layer = _layer(901, dim=dim, num_nearest_neighbors=k)
        feats, coors, mask = _cluster_graph(n_clusters, dim, k, 902)
        with torch.no_grad():                                             # (whatever a first call allocates once: packed weights, status words)
            layer(feats[:, :CL], coors[:, :CL], mask=mask[:, :CL])
        feats.requires_grad_(True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with pytest.raises(A.FusedBackwardLimit) as err:
            layer(feats, coors, mask=mask)
        assert torch.cuda.max_memory_allocated() == before, "something was allocated (and launched) before the limit was named"
        msg = str(err.value)
        assert str(n) in msg and "2^31" in msg and f"K = {k}" in msg, msg
        with torch.no_grad():
            node, co = layer(feats, coors, mask=mask)
        assert bool(torch.isfinite(node).all()) and bool(torch.isfinite(co).all())
        del layer, feats, coors, mask, node, co


def test_i_largest_single_graph_the_fused_backward_takes_trains_like_its_clusters():
    """The largest one-graph call `_fused_graphs_per_chunk` admits at K = 32, dim = 512 (whole clusters: its partial rows end within a
    cluster's worth of 2^31 bytes, signed offsets at the top of their range).  Input gradients on clusters 0, the middle and the last,
    parameter gradients against the float64 sum over ALL clusters."""
    k, dim = 32, 512
    hp = _widths(dim)[1]
    n_clusters = _largest_trainable_clusters(k, hp)
    n = n_clusters * CL
    rows_bytes = (n * k // 16 + n) * hp * 4
    assert rows_bytes < I31 <= ((n + CL) * k // 16 + n + CL + 8) * hp * 4, "not the largest graph below the partial rows' limit"
    assert rows_bytes > I31 - I31 // 8                                     # ... and close to it
    parts = [slice(c * CL, (c + 1) * CL) for c in range(n_clusters)]
    compare = [parts[0], parts[n_clusters // 2], parts[-1]]
    with _budget("i/fits"):
        layer = _layer(911, dim=dim, num_nearest_neighbors=k)
        feats, coors, mask = _cluster_graph(n_clusters, dim, k, 912)
        _check_training(layer, feats, coors, mask, parts, compare, 1, "i/fits", 1e-4, 913)
        del layer, feats, coors, mask


@pytest.mark.parametrize("mode", ["exact", "double"])
def test_j_plain_backward_tables_beyond_2_32_bytes_train_like_their_clusters(mode):
    """exact_arithmetic() training on one graph of 6 clusters, and a .double() module on 3 (K = 32, dim = 512): one graph's (H, E) tables
    of the plain backward (egnn_edge_exact_bwd_*, egnn_edge_exact_node_sums_*, egnn_edge_hidden_*) pass its 2 GB budget and 2^32 bytes
    each.  Every cluster compared: fp32 at 1e-4 of scale, float64 at 1e-8."""
    from egnn_pytorch_amd import exact_arithmetic
    k, dim = 32, 512
    n_clusters, esz, tol = (6, 4, 1e-4) if mode == "exact" else (3, 8, 1e-8)
    h = _widths(dim)[0]
    e = n_clusters * CL * k
    from egnn_pytorch_amd import autograd as A
    assert h * e * esz > I32                                              # each (H, E) table of the one graph beyond 2^32 bytes ...
    assert 2 * h * e * esz > A._EXACT_BWD_BYTES                           # ... and the pair beyond `_backward_exact`'s budget per chunk
    parts = [slice(c * CL, (c + 1) * CL) for c in range(n_clusters)]
    with _budget(f"j/{mode}"):
        layer = _layer(1001, dim=dim, num_nearest_neighbors=k)
        dtype = torch.float32
        if mode == "double":
            layer, dtype = layer.double(), torch.float64
        feats, coors, mask = _cluster_graph(n_clusters, dim, k, 1002, dtype)
        with (exact_arithmetic() if mode == "exact" else contextlib.nullcontext()):
            _check_training(layer, feats, coors, mask, parts, parts, 1, f"j/{mode}", tol, 1003)
        del layer, feats, coors, mask
