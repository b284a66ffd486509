"""Host-side agreement on the cell-grid selection with CSR rows (csrc/knn_grid.hip: egnn_knn_select_grid_csr_f32): the header declares
it, `_abi.py` requires it at load, the library exports it, the ABI version is unchanged -- a symbol is added and none altered -- and every
argument check returns before anything is launched or dereferenced."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "egnn_knn_select_grid_csr_f32"


def test_grid_csr_entry_in_header_binding_and_library():
    from egnn_pytorch_amd import _abi
    header = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    lib = _abi.load()
    assert re.search(r"\b" + NEW + r"\s*\(", header)
    assert NEW in _abi.SYMBOLS
    assert hasattr(lib, NEW)
    assert "#define EGNN_ABI_VERSION 44" in header
    assert _abi.ABI_VERSION == 44 and lib.egnn_abi_version() == 44


def test_grid_csr_argument_checks_need_no_device():
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    ws = lib.egnn_knn_grid_workspace_bytes
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    n, k = 100, 8
    big = ws(1, n, k)

    def call(coors=fake, rowptr=fake, col=fake, stride=0, b=1, nn=n, kk=k, cdim=3, idx=fake, rank=fake, w=fake, wb=big):
        return lib.egnn_knn_select_grid_csr_f32(coors, None, rowptr, col, stride, b, nn, kk, cdim, idx, rank, w, wb, None)

    for name in ("coors", "rowptr", "idx", "rank", "w"):                  # EGNN_E_NULLPTR
        assert call(**{name: None}) == -1, name
    assert call(kk=n + 1) == -2                                           # EGNN_E_SHAPE: K > N
    assert call(b=0) == -2 and call(kk=0) == -2 and call(nn=0) == -2
    assert call(wb=big - 1) == -2                                         # a workspace one byte short
    assert call(stride=n) == -2 and call(stride=n + 2) == -2 and call(stride=-1) == -2
    assert call(cdim=2) == -3                                             # EGNN_E_UNSUPPORTED
    assert call(nn=1000, kk=129, wb=ws(1, 1000, 129)) == -3
    assert call(b=65536, wb=ws(65536, n, k)) == -3
    assert call(w=fake + 4) == -4                                         # EGNN_E_ALIGN
