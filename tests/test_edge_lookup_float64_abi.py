"""The float64 edge look-up entries of the C ABI (egnn_edge_features_gather_f64 / egnn_edge_features_grad_f64), without a GPU: the
built library exports them, the header declares them beside the _f32 pair, the ctypes bindings carry the _f32 signatures, the ABI
version of the library, the header and the Python side agree, and the argument checks that launch nothing answer as documented."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egnn_edge_features_gather_f64", "egnn_edge_features_grad_f64")


def _header():
    return open(os.path.join(ROOT, "include", "egnn_hip.h")).read()


def test_library_exports_and_header_declares_the_float64_entries():
    from egnn_pytorch_amd import _abi
    lib = _abi.load()                                   # no compute call: loading needs no GPU
    declared = set(re.findall(r"\b(egnn_[a-z0-9_]+)\s*\(", _header()))
    for sym in NEW:
        assert sym in declared, sym
        assert sym in _abi.SYMBOLS, sym
        assert hasattr(lib, sym), sym
        f32 = getattr(lib, sym.replace("_f64", "_f32"))
        assert getattr(lib, sym).argtypes == f32.argtypes and getattr(lib, sym).restype is ctypes.c_int


def test_abi_version_agrees_everywhere():
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    in_header = int(re.search(r"#define\s+EGNN_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert lib.egnn_abi_version() == _abi.ABI_VERSION == in_header
    assert in_header >= 43                              # (42 had no float64 look-up entries)


def test_float64_signatures_mirror_float32_in_the_header():
    """`double` for every `float`, nothing else changed."""
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for sym in NEW:
        f64 = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % sym, header, flags=re.S).group(1)
        f32 = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % sym.replace("_f64", "_f32"), header, flags=re.S).group(1)
        assert " ".join(f64.split()) == " ".join(f32.replace("float*", "double*").split())


def test_grad_size_query_and_limits_need_no_device():
    """work == NULL is a size query that launches nothing: G (E + 2047) / 2048 capped, the same for both dtypes (the partition does
    not depend on the element type); a table row wider than a wave's LDS table is unsupported: 2048 floats, 1024 doubles."""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    one = ctypes.c_void_p(16)                           # (a non-NULL pointer the size query never follows)

    def query(entry, d1, v1=6, e=(1, 4096, 16)):
        nw = ctypes.c_int64(-1)
        rc = entry(None, d1 + 8, one, v1, d1, one, 4, 8, one, e[0], e[1], e[2], one, one, None, None, ctypes.byref(nw), None)
        return rc, nw.value

    rc32, n32 = query(lib.egnn_edge_features_grad_f32, 8)
    rc64, n64 = query(lib.egnn_edge_features_grad_f64, 8)
    assert rc32 == rc64 == 0
    assert n32 == n64 == 32 * (6 * 8 + 4 * 8)           # E = 65 536: G = 32 partials of V1 d1 + V2 d2 elements
    assert query(lib.egnn_edge_features_grad_f32, 2048)[0] == 0
    assert query(lib.egnn_edge_features_grad_f64, 1024)[0] == 0
    assert query(lib.egnn_edge_features_grad_f64, 1025)[0] == query(lib.egnn_edge_features_grad_f32, 2049)[0] != 0
    assert b"outside what the gfx950 kernels are built for" in lib.egnn_error_string(query(lib.egnn_edge_features_grad_f64, 1025)[0])
