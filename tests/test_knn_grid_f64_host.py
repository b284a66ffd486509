"""The float64 cell-grid entries without a GPU (csrc/knn_grid.hip; egnn_knn_select_grid_f64 / _grid_csr_f64 and their two queries):
declared in the header, bound in `_abi.SIGNATURES`, exported by the built library; the selection prototypes are the fp32 ones with
`double` for `float`; the size query and the row-flag offset; every argument check answers with made-up pointers, before any launch."""
import os

from egnn_pytorch_amd import _abi
from tests import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES, _, DEFINES = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip.h"))

ENTRIES = ("egnn_knn_grid_workspace_bytes_f64", "egnn_knn_grid_rowflag_offset_f64", "egnn_knn_select_grid_f64",
           "egnn_knn_select_grid_csr_f64")
E_NULLPTR, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -4
SHAPES = ((1, 1, 1), (3, 100, 7), (1, 70000, 32), (2, 262144, 128))


def test_entries_are_declared_bound_and_exported():
    lib = _abi.load()                                   # no compute call: loading needs no GPU
    for sym in ENTRIES:
        assert sym in PROTOTYPES and sym in _abi.SIGNATURES and sym in _abi.SYMBOLS, sym
        assert hasattr(lib, sym), sym
    assert int(DEFINES["EGNN_ABI_VERSION"]) == _abi.ABI_VERSION == 44        # additions only


def test_selection_prototypes_are_the_fp32_ones_with_double_for_float():
    lib = _abi.load()
    for f64 in ("egnn_knn_select_grid_f64", "egnn_knn_select_grid_csr_f64"):
        f32 = f64.replace("_f64", "_f32")
        ret32, params32 = PROTOTYPES[f32]
        assert PROTOTYPES[f64] == (ret32, [(ctype.replace("float", "double"), arg) for ctype, arg in params32]), f64
        assert any("double" in ctype for ctype, _ in PROTOTYPES[f64][1]), f64
        assert _abi.SIGNATURES[f64] == _abi.SIGNATURES[f32], f64
        assert getattr(lib, f64).argtypes == getattr(lib, f32).argtypes, f64
    assert PROTOTYPES["egnn_knn_grid_workspace_bytes_f64"] == PROTOTYPES["egnn_knn_grid_workspace_bytes"]
    assert PROTOTYPES["egnn_knn_grid_rowflag_offset_f64"] == ("size_t", [("int", "B"), ("int", "N")])


def test_size_query_is_positive_monotone_and_covers_the_fp32_layout_and_the_row_flags():
    lib = _abi.load()
    ws, ws32, off = lib.egnn_knn_grid_workspace_bytes_f64, lib.egnn_knn_grid_workspace_bytes, lib.egnn_knn_grid_rowflag_offset_f64
    for b, n, k in SHAPES:
        assert 0 < ws(b, n, k) <= ws(b + 1, n, k) and ws(b, n, k) <= ws(b, n + 1, k) <= ws(b, 2 * n, k)
        assert ws(b, n, k) <= ws(b, n, k + 1)
        assert ws(b, n, k) >= ws32(b, n, k)
        assert 0 < off(b, n) and off(b, n) + b * n <= ws(b, n, k)
    assert ws(0, 100, 8) > 0 and ws(1, 0, 8) > 0 and ws(1, 1, 1) > 0
    # the fp32 query keeps its values: the layout is 256-byte pieces of fixed sizes (header, chunk records, flags, cells, counters, starts,
    # 16-byte records)
    up = lambda x: (x + 255) // 256 * 256                                  # noqa: E731
    for b, n, k in SHAPES:
        cap = n // 4 + 64
        fixed = up(64 * b) + up(b * 64 * 16 * 8) + up(b * n) + up(4 * b * n) + up(4 * b * cap) + up(4 * b * (cap + 1))
        assert ws32(b, n, k) == fixed + up(16 * b * n)
        assert ws(b, n, k) == fixed + up(32 * b * n)


def test_grid_f64_argument_checks_need_no_device():
    lib = _abi.load()
    ws = lib.egnn_knn_grid_workspace_bytes_f64
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    n, k = 100, 8
    big = ws(1, n, k)

    def call(coors=fake, b=1, nn=n, kk=k, cdim=3, idx=fake, rank=fake, w=fake, wb=big):
        return lib.egnn_knn_select_grid_f64(coors, None, b, nn, kk, cdim, idx, rank, w, wb, None)

    for name in ("coors", "idx", "rank", "w"):
        assert call(**{name: None}) == E_NULLPTR, name
    assert call(b=0) == E_SHAPE and call(nn=0) == E_SHAPE and call(kk=0) == E_SHAPE and call(b=-1) == E_SHAPE
    assert call(kk=n + 1) == E_SHAPE                                      # K > N
    assert call(wb=big - 1) == E_SHAPE                                    # a workspace one byte short
    assert call(wb=lib.egnn_knn_grid_workspace_bytes(1, n, k)) == E_SHAPE  # (the fp32 workspace is too small)
    assert call(cdim=2) == E_UNSUPPORTED and call(cdim=4) == E_UNSUPPORTED
    assert call(nn=1000, kk=129, wb=ws(1, 1000, 129)) == E_UNSUPPORTED    # K beyond the kernel's limit
    assert call(b=65536, wb=ws(65536, n, k)) == E_UNSUPPORTED
    assert call(w=fake + 4) == E_ALIGN and call(w=fake + 8) == E_ALIGN
    # the fp32 entries' order: a NULL pointer before a bad shape, a bad shape before an unsupported one, that before the workspace
    assert call(coors=None, kk=0) == E_NULLPTR
    assert call(kk=0, cdim=2) == E_SHAPE
    assert call(cdim=2, wb=0) == E_UNSUPPORTED
    assert call(wb=0, w=fake + 4) == E_SHAPE


def test_grid_csr_f64_argument_checks_need_no_device():
    lib = _abi.load()
    ws = lib.egnn_knn_grid_workspace_bytes_f64
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    n, k = 100, 8
    big = ws(1, n, k)

    def call(coors=fake, rowptr=fake, col=fake, stride=0, b=1, nn=n, kk=k, cdim=3, idx=fake, rank=fake, w=fake, wb=big):
        return lib.egnn_knn_select_grid_csr_f64(coors, None, rowptr, col, stride, b, nn, kk, cdim, idx, rank, w, wb, None)

    for name in ("coors", "rowptr", "idx", "rank", "w"):
        assert call(**{name: None}) == E_NULLPTR, name
    assert call(kk=n + 1) == E_SHAPE
    assert call(b=0) == E_SHAPE and call(kk=0) == E_SHAPE and call(nn=0) == E_SHAPE
    assert call(wb=big - 1) == E_SHAPE
    assert call(stride=n) == E_SHAPE and call(stride=n + 2) == E_SHAPE and call(stride=-1) == E_SHAPE
    assert call(cdim=2) == E_UNSUPPORTED
    assert call(nn=1000, kk=129, wb=ws(1, 1000, 129)) == E_UNSUPPORTED
    assert call(b=65536, wb=ws(65536, n, k)) == E_UNSUPPORTED
    assert call(w=fake + 4) == E_ALIGN
