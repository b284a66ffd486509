"""Every template instantiation of the split-f16 GEMM (csrc/linear_hl.hip: 2 tile configurations x 6 epilogue variants = 12 kernels,
tests/_gemm_variants.py) in its three output forms, against float64 of the same fp32 operands:

  a. the grid (36 cells)     every shape has interior full tiles (epilogue staged through LDS) and ragged M and N edges (per element):
                             fp32 C within 3e-5 of float64 (the bound of tests/test_gpu_kernels.py::test_linear_hl_lds_dma at these
                             operand scales), the packed (hi, lo) output = C to the split bounds (rtol 3e-7, atol 3.1e-8) with exactly
                             zero pad columns, the packed-only and the fp32-only call the same bits as the call with both outputs;
                             dropout: dropped positions exactly zero, kept ones against the reference carrying the same hash mask
  b. both epilogues          per instantiation one shape of whole tiles (all staged) and the same call one column narrower (ldc % 4 != 0:
                             all per element): bit-equal on every shared element, fp32 and packed
  c. beside the grid         the tile rule's threshold (512 large tiles, and 496), ldc % 4 != 0 on ragged shapes, split_cols ending
                             inside a tile, the wide-A form with and without a row mask, the range status from either epilogue
  d. the block -> tile map   six tile counts under four group sizes (EGNN_HL_GROUP_M): float64, and the bits of the default group size
  e. split-K                 3, 5 and 7 parts with a shorter last one, one K-tile per part, a count that is no multiple of four; a
                             part without a K-tile is refused before any launch

Every failure names the cell and its instantiation; each cell prints one `GEMMVAR {...}` line with its worst error.
Worst measured (MI355X), per output form: fp32 C against float64 6.0e-6 (fp32 only and both; grid), 3.6e-6 beside the grid, 4.7e-6 on
the whole-tile shapes of (b), 2.2e-6 on the tile-map cells; packed (hi, lo) against C (packed only and both) 9.5e-7 absolute, 0.96 of
the split bounds; split-K 0.055 of its bound.  No cell needed its operands scaled down."""
import functools
import json

import pytest
import torch

from tests import _gemm_variants as G

pytestmark = pytest.mark.gpu

ATOL = 3e-5                                   # fp32 C against float64 (test_linear_hl_lds_dma)
SPLIT_RTOL, SPLIT_ATOL = 3e-7, 3.1e-8         # hi + lo against the fp32 value (22-bit split; lo below ~1e-3 is an fp16 subnormal)
GRID_IDS = [c.id for c in G.CELLS]
EXTRA_IDS = [c.id for c in G.EXTRA_CELLS]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


class _Ops:
    pass


def _operands(m, n, k, res, seed, k_a=None):
    """as test_linear_hl_lds_dma builds them: a ~ 2 N(0, 1) with every 7th column x 1e-3, w ~ N(0, 1) / sqrt(k), random bias and
    residual -- neither symmetric nor tile aligned.  Pre-activations have a standard deviation of about 2.1: over the 250 000 and more
    outputs of a cell they span beyond +-8, both tails of the GELU."""
    from egnn_pytorch_amd import _ops, _weights
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = _Ops()
    o.a = torch.randn(m, k_a or k, generator=g, device="cuda") * 2
    o.a[:, ::7] *= 1e-3
    o.w = torch.randn(n, k, generator=g, device="cuda") / k ** 0.5
    o.bias = torch.randn(n, generator=g, device="cuda")
    o.r = torch.randn(m, n, generator=g, device="cuda") if res else None
    o.ahl = _ops.split_f16(o.a)
    o.ws = _weights.split_f16(o.w)
    o.k = k
    return o


def _reference(o, act, drop=False, n=None):
    """float64 of the same fp32 operands; dropout between the bias and the SiLU (egnn_pytorch.py:196-201) with the kernels' hash mask"""
    from egnn_pytorch_amd import _dropout
    n = o.w.shape[0] if n is None else n
    z = o.a[:, :o.k].double() @ o.w[:n].double().t() + o.bias[:n].double()
    pre = z
    keep = None
    if drop:
        dev = z.device
        keep = _dropout.keep_mask(G.DROP_SEED, _dropout.SITE_NODE, torch.arange(z.shape[0], device=dev), torch.arange(n, device=dev), G.DROP_P)
        z = torch.where(keep, z * _dropout.inv_keep(G.DROP_P), torch.zeros_like(z))
    if act == 1:
        z = z * torch.sigmoid(z)
    elif act == 2:
        z = 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    if o.r is not None:
        z = z + o.r[:, :n].double()
    return z, pre, keep


def _call(cell, o, form, n=None, **kw):
    from egnn_pytorch_amd import _ops
    n = cell.n if n is None else n
    r = None if o.r is None else (o.r if n == o.r.shape[1] else o.r[:, :n].contiguous())
    out = _ops.linear_hl(o.ahl, o.ws, n, o.bias[:n], r, act=cell.act, out_f32=form in ("f32", "both"), out_hl=form in ("hl", "both"),
                         drop=(G.DROP_P, G.DROP_SEED) if cell.drop else None, **kw)
    if form == "both":
        return out
    return (out, None) if form == "f32" else (None, out)


def _inst(cell):
    return f"{cell.id} (CFG, ACT, RES, DROP) = {(cell.cfg, cell.act, cell.res, cell.drop)}"


def _report(cell, what, **figures):
    print("GEMMVAR " + json.dumps(dict(cell=cell.id, what=what, **{k: float(f"{v:.4e}") for k, v in figures.items()})), flush=True)


def _check_f32(cell, c, ref, what="C"):
    assert torch.isfinite(c).all(), _inst(cell)
    err = float((c.double() - ref).abs().max())
    _report(cell, what, err=err, bound=ATOL)
    assert err <= ATOL, f"{_inst(cell)}: {what} error {err:.3e} > {ATOL:.1e}"
    return err


def _check_packed(cell, hl, c):
    """PackedHL.dense() against the fp32 C of the same call / of the call with both outputs; pad columns exactly zero"""
    m, n = c.shape
    back = hl.dense()
    assert back.shape[0] == m and hl.kp == G.kpad(n), _inst(cell)
    diff = (back[:, :n].double() - c.double()).abs()
    ratio = float((diff / (SPLIT_ATOL + SPLIT_RTOL * c.double().abs())).max())
    _report(cell, "packed", abs_err=float(diff.max()), ratio=ratio)
    assert ratio <= 1.0, f"{_inst(cell)}: hi + lo is {ratio:.3f} of the split bounds away from the fp32 value"
    if hl.kp > n:
        assert float(back[:, n:].abs().max()) == 0.0, f"{_inst(cell)}: pad columns of the packed output are not zero"


def _images(hl):
    from egnn_pytorch_amd._weights import unpack_tiles
    return unpack_tiles(hl.hi, hl.rows, hl.kp)[:hl.rows], unpack_tiles(hl.lo, hl.rows, hl.kp)[:hl.rows]


def _seed(cell):
    return 1000 * cell.cfg + 100 * cell.act + 10 * cell.res + cell.drop + cell.k


@functools.lru_cache(maxsize=1)
def _both(inst):
    """operands, float64 reference and the call with both outputs of an instantiation's grid shape, shared by its three cells"""
    cell = [c for c in G.CELLS if (c.cfg, c.act, c.res, c.drop) == inst and c.form == "both"][0]
    o = _operands(cell.m, cell.n, cell.k, cell.res, _seed(cell))
    o.ref, o.pre, o.keep = _reference(o, cell.act, cell.drop)
    o.c, o.hl = _call(cell, o, "both")
    return o


# ------------------------------------------------------------------------------------------------ a. the grid
@pytest.mark.parametrize("cid", GRID_IDS)
def test_grid(cid):
    cell = G.BY_ID[cid]
    o = _both((cell.cfg, cell.act, cell.res, cell.drop))
    if cell.act == 2:                                            # on the reference alone: both GELU tails are exercised
        assert float(o.pre.min()) < -8.0 and float(o.pre.max()) > 8.0, _inst(cell)
    if cell.form == "both":
        _check_f32(cell, o.c, o.ref)
        _check_packed(cell, o.hl, o.c)
        if cell.drop:
            dropped = ~o.keep
            assert 0.15 < float(dropped.double().mean()) < 0.25
            assert float(o.c[dropped].abs().max()) == 0.0, f"{_inst(cell)}: a dropped position is not exactly zero"
            hi, lo = _images(o.hl)
            assert float(hi[:, :cell.n][dropped].abs().max()) == 0.0 and float(lo[:, :cell.n][dropped].abs().max()) == 0.0
            # kept positions: SiLU(inv_keep x the no-dropout pre-activation)
            z = o.pre * (1.0 / (1.0 - G.DROP_P))
            kept = float((o.c.double() - z * torch.sigmoid(z)).abs()[o.keep].max())
            assert kept <= ATOL, f"{_inst(cell)}: kept positions {kept:.3e}"
        return
    c, hl = _call(cell, o, cell.form)
    if cell.form == "f32":
        assert hl is None
        _check_f32(cell, c, o.ref)
        assert torch.equal(c, o.c), f"{_inst(cell)}: the fp32-only call differs from the call with both outputs"
    else:
        assert c is None
        _check_packed(cell, hl, o.c)
        assert torch.equal(hl.hi, o.hl.hi) and torch.equal(hl.lo, o.hl.lo), \
            f"{_inst(cell)}: the packed-only call and the call with both outputs give different (hi, lo) images"


# ------------------------------------------------------------------------------------------------ b. both epilogues, the same bits
@pytest.mark.parametrize("inst", G.INSTANTIATIONS, ids=[G._name(*i) for i in G.INSTANTIATIONS])
def test_both_epilogues_give_the_same_bits(inst):
    """M and N whole tiles: every tile is staged.  One column less: ldc = N - 1 is no multiple of four and every tile takes the
    per-element path (the same configuration: the tile counts do not change).  Every shared element bit for bit."""
    cfg, act, res, drop = inst
    m, n = (384, 640) if cfg == 0 else (8192, 2048)
    assert G.select_cfg(m, n) == cfg == G.select_cfg(m, n - 1) and G.tile_counts(m, n, cfg)[1] == 0 and (n - 1) % 4 != 0
    cell = G.Cell(f"epilogues-{G._name(*inst)}", "epilogues", cfg, act, res, drop, "both", m, n, 50, {})
    o = _operands(m, n, 50, res, 7 + _seed(cell))
    ref = _reference(o, act, drop)[0]
    c1, hl1 = _call(cell, o, "both")
    c2, hl2 = _call(cell, o, "both", n=n - 1)
    _check_f32(cell, c1, ref, "C staged")
    _check_f32(cell, c2, ref[:, :n - 1], "C per element")
    assert c2.shape == (m, n - 1)
    assert torch.equal(c1[:, :n - 1], c2), f"{_inst(cell)}: the staged and the per-element epilogue give different fp32 bits"
    h1, l1 = _images(hl1)
    h2, l2 = _images(hl2)
    assert hl1.kp == hl2.kp == n
    assert torch.equal(h1[:, :n - 1], h2[:, :n - 1]) and torch.equal(l1[:, :n - 1], l2[:, :n - 1]), \
        f"{_inst(cell)}: the staged and the per-element epilogue give different (hi, lo) images"
    assert float(h2[:, n - 1].abs().max()) == 0.0 and float(l2[:, n - 1].abs().max()) == 0.0
    _check_packed(cell, hl1, c1)


# ------------------------------------------------------------------------------------------------ c. beside the grid
@pytest.mark.parametrize("cid", EXTRA_IDS)
def test_beside_the_grid(cid):
    cell = G.BY_ID[cid]
    o = _operands(cell.m, cell.n, cell.k, cell.res, 3 + _seed(cell), k_a=cell.extra.get("k_a"))
    ref = _reference(o, cell.act)[0]
    if cell.kind in ("threshold", "unaligned", "wide_a"):
        if cell.kind == "wide_a":
            assert o.ahl.kp > G.kpad(cell.k)                      # (-> egnn_linear_hl_lda_f32)
        c, hl = _call(cell, o, "both")
        _check_f32(cell, c, ref)
        _check_packed(cell, hl, c)
    elif cell.kind == "split_cols":                               # as test_linear_hl_split_cols
        sc = cell.extra["split_cols"]
        plain, _ = _call(cell, o, "f32")
        mixed, _ = _call(cell, o, "f32", split_cols=sc)
        _check_f32(cell, plain, ref)
        assert torch.equal(mixed[:, sc:], plain[:, sc:]), f"{_inst(cell)}: columns behind split_cols differ from the plain call"
        halves = mixed[:, :sc].contiguous().view(torch.float16).float()      # a word = (fp16 hi | fp16 lo << 16), little endian
        hi, lo = halves[:, 0::2], halves[:, 1::2]
        assert torch.equal(hi, plain[:, :sc].half().float()), f"{_inst(cell)}: hi is not the fp16 rounding of the plain result"
        diff = ((hi + lo).double() - plain[:, :sc].double()).abs()
        assert float((diff - (SPLIT_ATOL + SPLIT_RTOL * plain[:, :sc].double().abs())).max()) <= 0.0, _inst(cell)
    else:                                                         # row_mask on the wide-A form
        bm = G.BM[cell.cfg]
        full, _ = _call(cell, o, "f32")
        _check_f32(cell, full, ref)
        rows = [5, cell.m - 1] + (list(range(700, 900)) if cell.m > 2000 else [])
        mask = torch.zeros(cell.m, dtype=torch.uint8)
        mask[rows] = 1
        got, _ = _call(cell, o, "f32", row_mask=mask.cuda())       # (C comes poisoned: tests/conftest.py)
        written = ~torch.isnan(got).any(dim=1)
        assert torch.equal(got[written], full[written]), _inst(cell)
        tiles = torch.zeros((cell.m + bm - 1) // bm, dtype=torch.bool)
        tiles[torch.tensor(rows) // bm] = True
        assert torch.equal(written.cpu(), tiles.repeat_interleave(bm)[:cell.m]), \
            f"{_inst(cell)}: the written rows are not the {bm}-row tiles that hold a set row"
        assert not bool(written.all()) and bool(written[mask.bool().cuda()].all())


@pytest.mark.parametrize("where", ["full_tile", "ragged_tile"])
@pytest.mark.parametrize("cfg", [0, 1])
def test_range_status_from_both_epilogues(cfg, where):
    """one value of the packed output beyond 65 504 (through the residual), in a staged tile and in a per-element one: the forward status
    raises; the same call with that value at 60 000 does not"""
    from egnn_pytorch_amd import _abi, _ops
    m, n = G.SHAPE[cfg]
    cell = G.Cell(f"range-cfg{cfg}-{where}", "range", cfg, 0, True, False, "hl", m, n, 29, {})
    i, j = (G.BM[cfg] + 3, G.BN + 5) if where == "full_tile" else (m - 1, n - 1)
    assert (i // G.BM[cfg] < m // G.BM[cfg] and j // G.BN < n // G.BN) == (where == "full_tile")
    o = _operands(m, n, 29, True, 99 + cfg)
    dev = o.a.device
    _ops.range_check_after_forward(dev, mode="sync")              # (nothing pending from earlier calls)
    o.r[i, j] = 6.0e4
    _, hl = _call(cell, o, "hl")
    _ops.range_check_after_forward(dev, mode="sync")
    assert 5.9e4 < float(hl.dense()[i, j]) < 6.1e4
    o.r[i, j] = 7.0e4
    _call(cell, o, "hl")
    with pytest.raises(_abi.EGNNRangeError) as exc:
        _ops.range_check_after_forward(dev, mode="sync")
    assert exc.value.bits & 1, exc.value.bits                     # EGNN_RANGE_A_OPERAND
    _ops.range_check_after_forward(dev, mode="sync")              # the word was cleared


# ------------------------------------------------------------------------------------------------ d. the block -> tile map
@pytest.mark.parametrize("ntm,ntn", G.TILE_MAP_CELLS)
def test_tile_map_under_every_group_size(ntm, ntn, monkeypatch):
    """asymmetric operands and a poisoned C: a tile no workgroup computes stays NaN, a tile computed in the wrong place is wrong"""
    m, n = G.tile_map_shape(ntm, ntn)
    cell = G.Cell(f"tilemap-{ntm}x{ntn}", "tile_map", 0, 0, False, False, "both", m, n, G.TILE_MAP_K, {})
    o = _operands(m, n, G.TILE_MAP_K, False, 31 * ntm + ntn)
    ref = _reference(o, 0)[0]
    first = None
    for env in G.TILE_MAP_GROUPS:
        if env is None:
            monkeypatch.delenv("EGNN_HL_GROUP_M", raising=False)
        else:
            monkeypatch.setenv("EGNN_HL_GROUP_M", str(env))
        c, hl = _call(cell, o, "both")
        _check_f32(cell, c, ref, f"C group_m={env}")
        if first is None:
            first = (c, hl)
            _check_packed(cell, hl, c)
        else:
            assert torch.equal(c, first[0]) and torch.equal(hl.hi, first[1].hi) and torch.equal(hl.lo, first[1].lo), \
                f"{_inst(cell)}: EGNN_HL_GROUP_M={env} changes the result"


# ------------------------------------------------------------------------------------------------ e. split-K
def _splitk_operands(c):
    g = torch.Generator().manual_seed(c.r + c.m + c.k_splits)
    grad = (torch.randn(c.r, c.m, generator=g) * torch.logspace(-9, -5, c.m)[None, :]).cuda()     # as test_gradient_gemms_match_float64
    x = torch.randn(c.r, c.n, generator=g).cuda()
    return grad, x


@pytest.mark.parametrize("cid", [c.id for c in G.SPLITK_CELLS])
def test_split_k(cid):
    """the bound of test_gradient_gemms_match_float64: 3e-6 of the result's scale"""
    from egnn_pytorch_amd import _ops
    c = [s for s in G.SPLITK_CELLS if s.id == cid][0]
    grad, x = _splitk_operands(c)
    want = grad.double().t() @ x.double()
    tol = 3e-6 * float(want.abs().max())
    got = _ops.grad_tn(grad, x, k_splits=c.k_splits)
    assert got.shape == (c.m, c.n) and torch.isfinite(got).all()
    err = float((got.double() - want).abs().max())
    print("GEMMVAR " + json.dumps(dict(cell=cid, parts=G.splitk_parts(c.r, c.k_splits), err=float(f"{err:.4e}"), bound=float(f"{tol:.4e}"))))
    assert err <= tol, (cid, err, tol)
    assert torch.equal(got, _ops.grad_tn(grad, x, k_splits=c.k_splits))                          # fixed-order partial sums
    one = _ops.grad_tn(grad, x, k_splits=1)
    assert float((one.double() - want).abs().max()) <= tol


def test_split_k_refuses_an_empty_part():
    """ceil(12 / 5) = 3 K-tiles per part leave the fifth part without one: EGNN_E_SHAPE, returned before the launch"""
    from egnn_pytorch_amd import _abi, _ops
    c = G.SPLITK_EMPTY_PART
    grad, x = _splitk_operands(c)
    with pytest.raises(_abi.EGNNHipError, match="egnn_linear_hl_splitk_f32 failed with code -2"):
        _ops.grad_tn(grad, x, k_splits=c.k_splits)
