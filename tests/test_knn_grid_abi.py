"""Host-side agreement on the cell-grid selection's two entries (csrc/knn_grid.hip): the header declares them, `_abi.py` requires
them at load, the library exports them, and the ABI version is unchanged -- the change adds symbols and alters none."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egnn_knn_grid_workspace_bytes", "egnn_knn_select_grid_f32")


def test_grid_entries_in_header_binding_and_library():
    from egnn_pytorch_amd import _abi
    header = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    lib = _abi.load()
    for sym in NEW:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _abi.SYMBOLS, sym
        assert hasattr(lib, sym), sym
    assert "#define EGNN_ABI_VERSION 44" in header
    assert _abi.ABI_VERSION == 44 and lib.egnn_abi_version() == 44


def test_grid_workspace_size_and_argument_checks_need_no_device():
    """The size query and every argument check return before anything is launched: they run without a GPU."""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    ws = lib.egnn_knn_grid_workspace_bytes
    assert ws(1, 1, 1) > 0
    for b, n, k in ((1, 1, 1), (3, 100, 7), (1, 70000, 32), (2, 262144, 128)):
        assert 0 < ws(b, n, k) <= ws(b + 1, n, k) and ws(b, n, k) <= ws(b, n + 1, k) and ws(b, n, k) <= ws(b, n, k + 1)
    fake = 4096                                          # (never dereferenced: every call below is refused first)
    big = ws(1, 100, 8)
    sel = lib.egnn_knn_select_grid_f32
    assert sel(None, None, 1, 100, 8, 3, fake, fake, fake, big, None) == -1
    assert sel(fake, None, 1, 100, 8, 3, None, fake, fake, big, None) == -1
    assert sel(fake, None, 1, 100, 8, 3, fake, None, fake, big, None) == -1
    assert sel(fake, None, 1, 100, 8, 3, fake, fake, None, big, None) == -1
    assert sel(fake, None, 1, 100, 101, 3, fake, fake, fake, big, None) == -2          # K > N
    assert sel(fake, None, 0, 100, 8, 3, fake, fake, fake, big, None) == -2
    assert sel(fake, None, 1, 100, 0, 3, fake, fake, fake, big, None) == -2
    assert sel(fake, None, 1, 100, 8, 3, fake, fake, fake, big - 1, None) == -2        # a workspace one byte short
    assert sel(fake, None, 1, 100, 8, 2, fake, fake, fake, big, None) == -3            # coor_dim != 3
    assert sel(fake, None, 1, 1000, 129, 3, fake, fake, fake, ws(1, 1000, 129), None) == -3   # K beyond the kernel's limit
