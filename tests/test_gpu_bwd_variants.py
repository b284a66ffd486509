"""Every template instantiation of the register-contraction edge backward (csrc/edge_bwd.hip: 42 of `edge_bwd_kernel`, 5 of
`edge_bwd_prep_kernel`; tests/_bwd_variants.py) through a direct call of `_ops.edge_bwd_pass`, against the five contractions in float64:

  the bar        every output the variant produces -- the per-key sums of its partial rows, d/d W_s, d/d scalars, d/d W_2 -- within
                 5e-6 max|reference| + 1e-12 (the bar of tests/test_gpu_kernels.py::test_edge_bwd_pass_contractions_match_float64), with and
                 without dropout: at p = 0.5 the factor 2 is exact, at p = 0.2 the factor 1.25 costs one fp32 rounding of z; the cells
                 at the module's own initialisation (`init`) without the 1e-12: their scales are asserted > 0 on the host
  exact zeros    pad columns h >= H of the rows, of d/d W_s and of d/d W_2; rows c >= m_dim of d/d W_2; d/d s of every edge whose gU row
                 is zero; the partial rows of a key whose entries all carry gU = 0, and of the list's padding tiles
  no NaN         allocations are poisoned under test (tests/conftest.py): a forgotten element, chunk or slab shows
  rows_amax      the bits of max |rows|, exactly, wherever the entry accepts the by-product; refused where d/d W_s is on the matrix cores
  twice          the same bits from a second call (one cell per family, plain and dropout); the two cells with two slab groups equal, bit for bit in their
                 per-entry results, the same call with 8 rounds per slab

Each cell prints one `BWDVAR` JSON line: its worst error-to-bar ratio per output (EGNN_TEST_VERBOSE: one line per output as well)."""
import contextlib
import json
import os

import pytest
import torch

from tests import _bwd_variants as V

pytestmark = pytest.mark.gpu

IDS = [c.id for c in V.CELLS]
NAMES = dict(key_rows="rows", ws="ws", scal="scal", w2="w2")


@contextlib.contextmanager
def _entry_hook(mutate=None):
    """egnn_edge_bwd_pass_f32 behind a wrapper: `mutate(args)` changes the struct `_ops.edge_bwd_pass` built right before the call,
    and the return codes are recorded"""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    entry = lib.egnn_edge_bwd_pass_f32
    codes = []

    def wrapper(ref, stream):
        if mutate is not None:
            mutate(ref._obj)
        codes.append(entry(ref, stream))
        return codes[-1]
    lib.egnn_edge_bwd_pass_f32 = wrapper
    try:
        yield codes
    finally:
        lib.egnn_edge_bwd_pass_f32 = entry


class _Setup:
    pass


def _setup(cell):
    """the layer on the device, its packed weights, the P_i | P_j table and the entry list of a cell"""
    from egnn_pytorch_amd import _ops, _weights, autograd
    import copy
    p = V.prepare(cell.id)
    s = _Setup()
    s.p = p
    s.layer = copy.deepcopy(p.layer).cuda()
    s.w = s.layer.packed_weights()
    h, hp = s.w["H"], s.w["Hp"]
    assert hp == 32 * cell.steps and h == 2 * (2 * cell.kw["dim"] + cell.s) and s.w["S"] == cell.s
    s.h, s.hp = h, hp
    with torch.no_grad():
        s.proj = autograd._edge_tables(s.layer, s.w, p.feats.cuda(), False)
    s.idx32 = p.idx.to(torch.int32).cuda()
    s.gu16 = p.gu16.cuda()
    s.gu_scale = _weights.pow2_scale(float(p.gu16.abs().max()))
    s.scal = p.scal.cuda()
    s.w_s = torch.zeros(hp, cell.s, device="cuda")
    s.w_s[:h] = s.layer.edge_mlp[0].weight.detach()[:, 2 * cell.kw["dim"]:]
    if cell.by_dest:
        lists = _ops.dest_lists(s.idx32, cell.b, cell.n, cell.k, "cuda")
        s.ent = lists.ent
        # the list the host checks of tests/test_bwd_variants_table.py hold for -- compared before anything is launched on it
        assert torch.equal(s.ent.cpu(), p.ent) and torch.equal(lists.tile_seg.cpu(), p.seg), cell.id
    else:
        s.ent = p.ent.cuda()
    return s


def _call(cell, s, n_slabs=None, **over):
    from egnn_pytorch_amd import _ops
    kw = dict(by_dest=cell.by_dest, ws_nat=s.w_s if cell.want_s else None, want_w2=cell.want_w2, n_slabs=n_slabs or s.p.n_slabs,
              row_pairs=cell.row_pairs, drop=cell.drop, eid0=cell.eid0, want_amax=True)
    kw.update(over)
    with torch.no_grad():
        o = _ops.edge_bwd_pass(s.w, s.proj, s.idx32, s.gu16, s.gu_scale, s.scal, s.ent, cell.b, cell.n, cell.k, **kw)
    torch.cuda.synchronize()
    return o


def _what(cell):
    return f"{cell.id} (NM, ST, W2, SS, CH, PAIR, DROP, DSM) = {tuple(int(v) for v in cell.inst)}"


def _key_sums(cell, p, rows):
    """per-key sums of the partial rows on the host, float64 (row_pairs: the rows ARE the keys'); the rows behind the last key"""
    keys = cell.b * cell.n
    r = rows.cpu().double()
    if cell.row_pairs:
        return r[:keys], r[keys:]
    tiles = p.seg[1:] - p.seg[:-1]
    key_of_tile = torch.arange(keys).repeat_interleave(tiles)
    n_tiles = int(p.seg[-1])
    return torch.zeros(keys, r.shape[1], dtype=torch.float64).index_add_(0, key_of_tile, r[:n_tiles]), r[n_tiles:]


def _check(cell, s, o):
    """bar, exact zeros, no NaN, rows_amax.  Returns the worst error-to-bar ratio per output."""
    from egnn_pytorch_amd import _ops
    p, ref = s.p, V.reference(cell.id)
    h, hp, m = s.h, s.hp, cell.m_dim
    what = _what(cell)
    rows = o["rows"]
    assert rows.shape == ((p.ent.numel() // 32 if cell.row_pairs else p.ent.numel() // 16), hp), what
    sums, behind = _key_sums(cell, p, rows)
    got = dict(key_rows=sums[:, :h])
    assert set(k for k in ("w2", "ws", "scal") if k in o) == set(V.outputs_of(cell)) - {"key_rows"}, what
    for name in ("w2", "ws", "scal"):
        if name in o:
            assert bool(torch.isfinite(o[name]).all()), f"{what}: NaN in {name}"
    assert bool(torch.isfinite(rows).all()), f"{what}: NaN in the partial rows"
    # exact zeros
    if h < hp:
        assert float(rows[:, h:].abs().max()) == 0.0, f"{what}: pad columns of the rows"
    assert behind.numel() == 0 or float(behind.abs().max()) == 0.0, f"{what}: rows of the padding tiles"
    key = p.dst if cell.by_dest else p.src
    live_per_key = torch.zeros(cell.b * cell.n).index_add_(0, key, (~p.zero_rows).float())
    dead = live_per_key == 0
    assert bool(dead.any()) or (cell.hub and cell.k == 1), what
    if bool(dead.any()):
        assert float(sums[dead].abs().max()) == 0.0, f"{what}: a key without gradient"
    if cell.want_w2:
        w2 = o["w2"].cpu().double()
        assert w2.shape == (16, hp), what
        if m < 16:
            assert float(w2[m:].abs().max()) == 0.0, f"{what}: rows c >= m_dim of d/d W_2"
        if h < hp:
            assert float(w2[:, h:].abs().max()) == 0.0, f"{what}: pad columns of d/d W_2"
        got["w2"] = w2[:m, :h]
    if cell.want_s:
        ws, sc = o["ws"].cpu().double(), o["scal"].cpu().double()
        assert ws.shape == (hp, cell.s) and sc.shape == (cell.b * cell.n * cell.k, cell.s), what
        if h < hp:
            assert float(ws[h:].abs().max()) == 0.0, f"{what}: pad columns of d/d W_s"
        assert float(sc[p.zero_rows].abs().max()) == 0.0, f"{what}: d/d s of an edge without gradient"
        got["ws"], got["scal"] = ws[:h], sc
    # the by-product
    if V.accepts_rows_amax(cell.inst):
        assert o["amax_bits"] is not None, what
        assert _ops.bits_to_floats(o["amax_bits"])[0] == float(rows.abs().max()), f"{what}: rows_amax"
    else:
        assert o["amax_bits"] is None, what
    # the bar
    ratios, failed = {}, []
    for name in V.outputs_of(cell):
        r = ref[name]
        scale = float(r.abs().max())
        err = float((got[name] - r).abs().max())
        tol = 5e-6 * scale + (0.0 if cell.extra == "init" else 1e-12)     # (at the module's own initialisation the floor would be the bar)
        ratios[NAMES[name]] = err / tol
        if os.environ.get("EGNN_TEST_VERBOSE"):
            print(f"{cell.id:70s} {NAMES[name]:5s} err {err:.3e} bar {tol:.3e} ratio {err / tol:.3f}")
        if not err <= tol:
            failed.append(f"{NAMES[name]}: error {err:.3e} > bar {tol:.3e} ({err / tol:.2f} x)")
    print("BWDVAR " + json.dumps(dict(cell=cell.id, inst=[int(v) for v in cell.inst], drop=cell.drop is not None,
                                      ratios={k: round(v, 4) for k, v in ratios.items()})), flush=True)
    assert not failed, f"{what}: " + "; ".join(failed)
    return ratios


def _same_bits(a, b, names):
    return [n for n in names if n in a and a[n] is not None and not torch.equal(a[n], b[n])]


# the first cell of every family, without and with dropout, runs twice
TWICE = {next(c.id for c in V.CELLS if c.fam == fam and (c.drop is not None) == d) for fam in V.FAMILIES for d in (False, True)}


@pytest.mark.parametrize("cid", IDS)
def test_instantiation_matches_float64(cid):
    cell = V.BY_ID[cid]
    s = _setup(cell)
    with _entry_hook() as codes:
        o = _call(cell, s)
    assert codes == [0]
    _check(cell, s, o)
    if cid in TWICE:
        again = _call(cell, s)
        assert _same_bits(o, again, ("rows", "w2", "ws", "scal", "amax_bits")) == [], _what(cell)
    if cell.extra == "groups":
        # two slab groups (the second partial) against one: rows and d/d s are per-entry results, independent of the slabs; the all-edge
        # sums change their order
        n8 = V.n_slabs_of(s.p.rounds, V.ROUNDS_PER_SLAB)
        assert V.slabs(s.p.rounds, s.p.n_slabs)[2] == 2 and V.slabs(s.p.rounds, n8)[2] == 1
        o8 = _call(cell, s, n_slabs=n8)
        assert _same_bits(o, o8, ("rows", "scal", "amax_bits")) == [], _what(cell)
        _check(cell, s, o8)
    if not V.accepts_rows_amax(cell.inst):
        # asked for all the same: refused before anything is launched (launch_v)
        spare = torch.zeros(1, dtype=torch.int32, device="cuda")

        def ask(a):
            a.rows_amax = spare.data_ptr()
        _refused(cell, s, V.E_UNSUPPORTED, ask)


def _refused(cell, s, code, mutate=None, **over):
    from egnn_pytorch_amd import _abi
    with _entry_hook(mutate) as codes:
        with pytest.raises(_abi.EGNNHipError):
            _call(cell, s, **over)
    assert codes == [code], (_what(cell), codes, code)


def _first(**want):
    return next(c for c in V.CELLS if all(getattr(c, k) == v for k, v in want.items()))


def test_the_entry_refuses_before_any_launch():
    """egnn_edge_bwd_pass_f32's refusals (csrc/edge_bwd.hip:860-872, launch / launch_many / launch_v): the code the restated dispatcher
    names, and nothing launched -- the poisoned outputs are not looked at, the next valid call is unaffected."""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    # everything in one pass exists for S = 1 only
    for si in (1, 2, 3, 4):
        cell = next(c for c in V.CELLS if c.fam == "ss" and V.s_class(c.s) == si and not c.by_dest)
        s = _setup(cell)
        assert V.instantiation(cell.s, True, True, False, cell.drop is not None) == V.E_UNSUPPORTED
        _refused(cell, s, V.E_UNSUPPORTED, want_w2=True)
    # row_pairs: by destination, K <= 16, K > 32; and where the variant has no PAIR form
    cell = _first(fam="ss", by_dest=True, k=40)
    s = _setup(cell)
    _refused(cell, s, V.E_SHAPE, row_pairs=True)
    for k in (16, 33):
        cell = next(c for c in V.CELLS if c.fam == "ss" and not c.by_dest and c.k == k)
        s = _setup(cell)
        assert V.instantiation(cell.s, False, True, True, cell.drop is not None, False, k) == V.E_SHAPE
        _refused(cell, s, V.E_SHAPE, row_pairs=True)
    cell = next(c for c in V.CELLS if c.fam == "pair" and c.drop is None)
    s = _setup(cell)
    assert V.instantiation(cell.s, False, False, True, False, False, cell.k) == V.E_UNSUPPORTED
    _refused(cell, s, V.E_UNSUPPORTED, ws_nat=None)
    # the work area one byte short (the pair cell; then a d/d W_2 cell, whose records are larger)
    for c2 in (cell, _first(fam="w2", by_dest=True)):
        s2 = _setup(c2)
        need = lib.egnn_edge_bwd_work_bytes(s2.p.ent.numel(), c2.s, int(c2.want_w2), int(c2.want_s))

        def short(a, need=need):
            assert a.work_bytes == need
            a.work_bytes = need - 1
        _refused(c2, s2, V.E_SHAPE, short)
    # d/d W_s without d/d s
    def no_ds(a):
        a.ds_part = None
    _refused(cell, s, V.E_NULLPTR, no_ds)
    # more than five scalars: d/d s on the matrix cores needs the W_s^T fragments
    for si, code in ((3, V.E_NULLPTR), (4, V.E_NULLPTR)):
        c6 = next(c for c in V.CELLS if c.fam == "ss" and V.s_class(c.s) == si)
        s6 = _setup(c6)

        def no_wsth(a):
            a.WsTh = None
        assert V.instantiation(c6.s, False, True, False, c6.drop is not None, c6.by_dest, c6.k, has_wsth=False) == code
        _refused(c6, s6, code, no_wsth)
    # a dropout threshold with a scale below one
    cd = next(c for c in V.CELLS if c.drop is not None)
    sd = _setup(cd)

    def bad_keep(a):
        assert a.drop_thr > 0
        a.drop_inv_keep = 0.5
    _refused(cd, sd, V.E_SHAPE, bad_keep)
    # ... and the call as the table has it still answers
    with _entry_hook() as codes:
        o = _call(cell, s)
    assert codes == [0]
    _check(cell, s, o)
