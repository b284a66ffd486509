"""The declarations of a plain C header (include/egnn_hip.h, include/egnn_hip_ref.h) for tests/test_abi_agreement.py: comments
stripped, then prototypes and `typedef struct` bodies split with regular expressions.  No C parser: the headers hold nothing but
scalar and pointer declarations, and anything else (an array, a function pointer, a nested struct) is refused, not guessed."""
import re

_DECLARATOR = re.compile(r"^(.*?)([\s*]*)(\w+)$", re.S)


def _ctype(base, stars):
    """`const float` + `*` -> "float*": const dropped, blanks collapsed."""
    words = [w for w in base.split() if w != "const"]
    assert words and all(re.fullmatch(r"\w+", w) for w in words), base
    return " ".join(words) + "*" * stars.count("*")


def _declarations(decl):
    """`const float *a, *b` -> [("float*", "a"), ("float*", "b")]: the base type is the first declarator's, the stars are each one's own."""
    assert not re.search(r"[\[\](){}:]", decl), decl
    first, *rest = decl.split(",")
    base, stars, name = _DECLARATOR.match(first.strip()).groups()
    out = [(_ctype(base, stars), name)]
    for part in rest:
        stars, name = re.fullmatch(r"([\s*]*)(\w+)", part.strip()).groups()
        out.append((_ctype(base, stars), name))
    return out


def parse(path):
    """-> (prototypes {name: (return type, [(argument type, argument name), ...])}, structs {name: [(field type, field name), ...]},
    defines {name: text}), every type as `_ctype` writes it."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\benum\s*\w*\s*\{[^{}]*\}\s*;", " ", text)
    structs = {}

    def take_struct(m):
        tag, body, name = m.groups()
        assert tag == name and name not in structs, (tag, name)
        structs[name] = [f for decl in body.split(";") if decl.strip() for f in _declarations(decl)]
        return " "

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    prototypes = {}
    for stmt in text.split(";"):
        stmt = stmt.strip().lstrip("}").strip()                     # (the closing brace of extern "C")
        if not stmt:
            continue
        m = re.fullmatch(r"([\w\s*]+?)\s*\(([^()]*)\)", stmt, flags=re.S)
        assert m, "not a prototype: %r" % stmt
        (ret, name), = _declarations(m.group(1))
        assert name not in prototypes, name
        params = m.group(2).strip()
        prototypes[name] = (ret, [] if params in ("", "void") else [f for p in params.split(",") for f in _declarations(p)])
    return prototypes, structs, defines
