"""The C ABI and its ctypes binding agree, without a GPU: every prototype of include/egnn_hip.h against `_abi.SIGNATURES` (count,
order and type of every argument, the return type), every argument struct against its mirror (field names, order and types), the
order of `egnn_struct_bytes` in csrc/node_ops.hip against `_abi.STRUCTS`, the built library against all three (sizes, version), and
include/egnn_hip_ref.h against tests/_reflib.py.  The header is parsed once (tests/_cheader.py); the parts that compare it with the
tables do not load the library.  Behind them: the entries whose argument checks answer before any launch, called with made-up pointers."""
import ctypes
import os
import re

import pytest

from egnn_pytorch_amd import _abi
from tests import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES, STRUCTS, DEFINES = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip.h"))
MIRRORS = dict(_abi.STRUCTS, egnn_layer_params=_abi.LayerParams)       # header struct name -> ctypes mirror

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
POINTEES = dict(SCALARS, uint8_t=ctypes.c_uint8)                       # what a typed POINTER(T) may point to
SAME = ({ctypes.c_int, ctypes.c_int32},)                               # the one substitution allowed: int <-> int32_t

# the entries the feature pull requests since ABI 37 added, each once pinned by a test of its own
NAMED_ENTRIES = (
    "egnn_knn_grid_workspace_bytes", "egnn_knn_select_grid_f32", "egnn_knn_select_grid_csr_f32",
    "egnn_knn_select_csr_f32", "egnn_knn_select_csr_f64", "egnn_adj_csr_workspace_bytes", "egnn_adj_csr_square_count",
    "egnn_adj_csr_square_fill", "egnn_csr_slot_labels_u8", "egnn_edge_features_gather_slot_f32", "egnn_edge_features_gather_slot_f64",
    "egnn_edge_features_grad_slot_f32", "egnn_edge_features_grad_slot_f64",
    "egnn_edge_features_gather_f64", "egnn_edge_features_grad_f64", "egnn_status_publish",
    "egnn_edge_hidden_fwd_f32", "egnn_edge_hidden_fwd_f64", "egnn_edge_hidden_bwd_f32", "egnn_edge_hidden_bwd_f64",
    "egnn_edge_hidden_bwd2_f32", "egnn_edge_hidden_bwd2_f64",
)


def _same(a, b):
    return a is b or any(a in s and b in s for s in SAME)


def agrees(ctype, cls, returned=False):
    """Is `cls` the ctypes class of the declared C type?  Scalars by the fixed table; `const char*` returned -> c_char_p; a pointer to
    an argument struct -> POINTER(its mirror); any other pointer -> c_void_p or POINTER(the pointed-to scalar)."""
    if not ctype.endswith("*"):
        return ctype in SCALARS and _same(SCALARS[ctype], cls)
    target = ctype[:-1]
    if target == "char" and returned:
        return cls is ctypes.c_char_p
    if target in MIRRORS:
        return cls is ctypes.POINTER(MIRRORS[target])
    if cls is ctypes.c_void_p:
        return True
    return target in POINTEES and any(cls is ctypes.POINTER(c) for c in POINTEES.values() if _same(c, POINTEES[target]))


def prototype_mismatches(prototypes, signatures):
    """every disagreement between a header's prototypes and a name -> (restype, argtypes) table, one line each"""
    out = ["%s: declared in the header, no signature" % n for n in prototypes if n not in signatures]
    out += ["%s: has a signature, not declared in the header" % n for n in signatures if n not in prototypes]
    for name in sorted(set(prototypes) & set(signatures)):
        (ret, params), (restype, argtypes) = prototypes[name], signatures[name]
        if not agrees(ret, restype, returned=True):
            out.append("%s: returns %s, restype %s" % (name, ret, getattr(restype, "__name__", restype)))
        if len(params) != len(argtypes):
            out.append("%s: %d arguments in the header, %d argtypes" % (name, len(params), len(argtypes)))
            continue
        out += ["%s: argument %d, `%s %s`, is bound as %s" % (name, i, ctype, arg, cls.__name__)
                for i, ((ctype, arg), cls) in enumerate(zip(params, argtypes)) if not agrees(ctype, cls)]
    return out


# ------------------------------------------------------------------ (a) prototypes
def test_every_prototype_has_its_signature_type_by_type():
    assert len(PROTOTYPES) > 100 and _abi.SYMBOLS == tuple(_abi.SIGNATURES)
    bad = prototype_mismatches(PROTOTYPES, _abi.SIGNATURES)
    assert not bad, "\n".join(bad)


def test_named_entries_are_declared_bound_and_exported():
    lib = _abi.load()                                   # no compute call: loading needs no GPU
    for sym in NAMED_ENTRIES:
        assert sym in PROTOTYPES and sym in _abi.SIGNATURES and sym in _abi.SYMBOLS, sym
        assert hasattr(lib, sym), sym


def test_float64_entries_have_the_float32_entries_signatures():
    """In the header `double` for every `float` and nothing else changed, argument names included; in the binding one signature."""
    lib = _abi.load()
    for f64 in ("egnn_edge_features_gather_f64", "egnn_edge_features_grad_f64"):
        f32 = f64.replace("_f64", "_f32")
        ret32, params32 = PROTOTYPES[f32]
        assert PROTOTYPES[f64] == (ret32, [(ctype.replace("float", "double"), arg) for ctype, arg in params32]), f64
        assert _abi.SIGNATURES[f64] == _abi.SIGNATURES[f32], f64
        assert getattr(lib, f64).argtypes == getattr(lib, f32).argtypes and getattr(lib, f64).restype is ctypes.c_int, f64


# ------------------------------------------------------------------ (b) structs
def test_every_argument_struct_of_the_header_has_a_mirror():
    assert set(STRUCTS) == set(MIRRORS) and len(MIRRORS) == len(_abi.STRUCTS) + 1
    assert len({m for _, m in _abi.STRUCTS}) == len(_abi.STRUCTS)


@pytest.mark.parametrize("name", sorted(MIRRORS))
def test_struct_mirror_has_the_headers_fields_in_order_and_type(name):
    declared, mirror = STRUCTS[name], MIRRORS[name]
    fields = [(f[0], f[1]) for f in mirror._fields_]
    assert [n for _, n in declared] == [n for n, _ in fields], "%s: field names / order differ from %s" % (mirror.__name__, name)
    bad = ["%s.%s: `%s` in the header, %s in %s" % (name, field, ctype, cls.__name__, mirror.__name__)
           for (ctype, field), (_, cls) in zip(declared, fields) if not agrees(ctype, cls)]
    assert not bad, "\n".join(bad)
    if name == "egnn_forward_opts":                     # the status-publish fields (ABI 44)
        assert {"status_pub", "status_words", "status_seq"} <= {n for n, _ in fields}


# ------------------------------------------------------------------ (c) the order of egnn_struct_bytes
def test_struct_bytes_switch_names_the_structs_in_order():
    src = open(os.path.join(ROOT, "egnn_pytorch_amd", "csrc", "node_ops.hip")).read()
    body = src[src.index("int64_t egnn_struct_bytes(int which)"):]
    body = body[:body.index("default:")]
    cases = re.findall(r"case\s+(\d+)\s*:\s*return\s*\(int64_t\)\s*sizeof\((\w+)\)\s*;", body)
    assert cases == [(str(i), name) for i, (name, _) in enumerate(_abi.STRUCTS)]


# ------------------------------------------------------------------ (d) the loaded library
def test_loaded_library_has_the_mirrors_sizes():
    lib = _abi.load()
    for i, (name, mirror) in enumerate(_abi.STRUCTS):
        assert lib.egnn_struct_bytes(i) == ctypes.sizeof(mirror), name
    assert lib.egnn_struct_bytes(len(_abi.STRUCTS)) == -1 and lib.egnn_struct_bytes(-1) == -1
    assert _abi.STRUCTS[8][1] is _abi.ForwardOpts and lib.egnn_struct_bytes(8) == ctypes.sizeof(_abi.ForwardOpts)
    assert _abi.STRUCTS[9][1] is _abi.EdgeHiddenArgs and lib.egnn_struct_bytes(9) == ctypes.sizeof(_abi.EdgeHiddenArgs)
    for sym in _abi.SYMBOLS:
        assert hasattr(lib, sym), sym


def test_abi_version_is_44_everywhere():
    assert int(DEFINES["EGNN_ABI_VERSION"]) == _abi.ABI_VERSION == _abi.load().egnn_abi_version() == 44


# ------------------------------------------------------------------ (e) the test-only library's header
def test_reference_header_matches_reflib():
    from tests import _reflib
    prototypes, structs, _ = _cheader.parse(os.path.join(ROOT, "include", "egnn_hip_ref.h"))
    assert prototypes and not structs
    bad = prototype_mismatches(prototypes, _reflib.SIGNATURES)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ argument checks that answer before any launch
def test_grid_workspace_size_and_argument_checks_need_no_device():
    """The size query and every argument check return before anything is launched: they run without a GPU."""
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


def test_grid_csr_argument_checks_need_no_device():
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


def test_grad_size_query_and_limits_need_no_device():
    """work == NULL is a size query that launches nothing: G (E + 2047) / 2048 capped, the same for both dtypes (the partition does
    not depend on the element type); a table row wider than a wave's LDS table is unsupported: 2048 floats, 1024 doubles."""
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
