"""egnn_forward_opts carries the status-publish fields (ABI 44), without a GPU: the ctypes mirror has the header's fields in the header's
order, its size is the library's, and the three ABI version numbers agree."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "egnn_hip.h")).read()


def test_forward_opts_mirror_matches_the_header_and_the_library():
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    body = re.search(r"typedef struct egnn_forward_opts \{(.*?)\} egnn_forward_opts;", _header(), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    assert names == [f[0] for f in _abi.ForwardOpts._fields_]
    for decl, (name, ctype) in zip(decls, _abi.ForwardOpts._fields_):
        assert ("*" in decl) == (ctype is ctypes.c_void_p), decl
        if "*" not in decl:
            assert decl.startswith("int32_t ") and ctype is ctypes.c_int32, decl
    for name in ("status_pub", "status_words", "status_seq"):
        assert name in names
    assert lib.egnn_struct_bytes(8) == ctypes.sizeof(_abi.ForwardOpts)


def test_abi_version_is_44_everywhere():
    from egnn_pytorch_amd import _abi
    in_header = int(re.search(r"#define\s+EGNN_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert _abi.load().egnn_abi_version() == _abi.ABI_VERSION == in_header == 44


def test_status_request_is_refused_outside_a_module_forward():
    """No `early_publish` scope, no request: a bare `_forward_c` (or any other caller of the C entry) keeps today's path."""
    from egnn_pytorch_amd import _ops
    assert _ops._early.get() is None
    assert _ops.status_request("cuda:0") is None
    with _ops.early_publish(last=False):
        assert _ops.status_request("cuda:0") is None                      # (layers that can still write the word follow)
