"""Strict reader of include/dsu_hip.h: the header is the one statement of the C ABI, and the ctypes
binding (_lib.py) is derived from what this module reads in it.

Accepted, after comments and preprocessor lines are stripped:
    #define DSU_NAME <integer> | (<-integer>)                     -> defines
    typedef struct [tag] { fields } name;                           -> structs (ctypes.Structure classes)
        fields: type a;  type a, b;  type* a;  type a[N];  <earlier struct> a;   ([const] allowed)
    typedef struct tag name;                                        -> opaque
    ret dsu_name(void | [const] type [*[*]] ident, ...);            -> protos: name -> (restype, argtypes)
Anything else raises DsuError with the offending text; nothing is skipped or guessed.
"""
import collections
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dsu_hip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_POINTEES = set(SCALARS) | {"void", "char", "uint8_t", "uint16_t"}     # may stand left of a `*` only
_RETURNS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}

Header = collections.namedtuple("Header", "defines structs opaque protos")


class DsuError(RuntimeError):
    pass


def _bad(what, text):
    raise DsuError(f"dsu_hip.h: {what}: {' '.join(text.split())!r}")


def _statements(text):
    """Split at the `;` outside braces."""
    depth, start = 0, 0
    for m in re.finditer(r"[{};]", text):
        depth += (m.group() == "{") - (m.group() == "}")
        if depth < 0:
            _bad("unbalanced brace", text[start:m.end()])
        if m.group() == ";" and depth == 0:
            yield text[start:m.start()].strip()
            start = m.end()
    if depth or text[start:].strip():
        _bad("text after the last `;`", text[start:])


def parse(text):
    h = Header({}, {}, set(), {})
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)

    def define(m):
        d = re.fullmatch(r"#\s*define\s+(DSU_\w+)\s+(?:(\d+)|\(\s*(-\d+)\s*\))\s*", m.group())
        if d:
            h.defines[d.group(1)] = int(d.group(2) or d.group(3))
        elif not re.fullmatch(r"#\s*(if|ifdef|ifndef|endif|include|define\s+\w+\s*$).*", m.group()):
            _bad("preprocessor line outside the grammar", m.group())
        return ""
    text = re.sub(r"^[ \t]*#.*$", define, text, flags=re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    text = m.group(1) if m else text

    def pointee(word, stmt):
        if word not in _POINTEES and word not in h.structs and word not in h.opaque:
            _bad(f"unknown type word {word!r}", stmt)

    def extent(expr, stmt):                       # literal | define [+ literal]
        m = re.fullmatch(r"(\w+)(?:\s*\+\s*(\d+))?", expr.strip())
        if not m or not (m.group(1).isdigit() or m.group(1) in h.defines):
            _bad("array extent", stmt)
        n = m.group(1)
        return (int(n) if n.isdigit() else h.defines[n]) + int(m.group(2) or 0)

    def fields(body, stmt):
        if re.search(r"[{}():]", body) or not body.rstrip().endswith(";"):
            _bad("struct body outside the grammar", stmt)
        out = []
        for decl in body.rstrip().rstrip(";").split(";"):
            m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\b\s*(.*?)\s*", decl, flags=re.S)
            if not m:
                _bad("field", decl)
            base = m.group(1)
            for d in m.group(2).split(","):
                dm = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[([^\]]*)\])?\s*", d)
                if not dm:
                    _bad("field", decl)
                if dm.group(1):
                    pointee(base, decl)
                    t = C.c_void_p
                elif base in SCALARS or base in h.structs:
                    t = SCALARS.get(base) or h.structs[base]
                else:
                    _bad(f"unknown type word {base!r}", decl)
                out.append((dm.group(2), t * extent(dm.group(3), decl) if dm.group(3) is not None else t))
        return out

    def param(p, stmt):
        m = re.fullmatch(r"\s*(?:const\s+)?(\w+)(\s*\*{1,2}\s*|\s+)(\w+)\s*", p)
        if not m:
            _bad("parameter", stmt)
        base, stars = m.group(1), m.group(2).strip()
        if not stars:
            if base not in SCALARS:
                _bad(f"unknown type word {base!r}", stmt)
            return SCALARS[base]
        pointee(base, stmt)
        return C.POINTER(h.structs[base]) if stars == "*" and base in h.structs else C.c_void_p

    for stmt in _statements(text):
        m = re.fullmatch(r"typedef\s+struct\s*(\w+)?\s*\{(.*)\}\s*(\w+)", stmt, flags=re.S)
        if m:
            if m.group(3) in h.structs or m.group(3) in h.opaque:
                _bad("redefinition", stmt)
            h.structs[m.group(3)] = type(m.group(3), (C.Structure,), {"_fields_": fields(m.group(2), stmt)})
            continue
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)", stmt)
        if m:
            h.opaque.add(m.group(2))
            continue
        m = re.fullmatch(r"(const\s+)?(\w+)(\s*\*\s*|\s+)(dsu_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m or re.search(r"[()\[\]{}]", m.group(5)) or m.group(4) in h.protos:
            _bad("statement outside the grammar", stmt)
        const, ret, star, name, params = m.groups()
        if star.strip():
            pointee(ret, stmt)
            restype = C.c_char_p if (const and ret == "char") else C.c_void_p
        elif const or ret not in _RETURNS:
            _bad(f"return type {ret!r}", stmt)
        else:
            restype = _RETURNS[ret]
        args = [] if params.strip() == "void" else [param(p, stmt) for p in params.split(",")]
        h.protos[name] = (restype, args)
    return h


def read(path=HEADER_PATH):
    if not os.path.exists(path):
        raise DsuError(f"{os.path.normpath(path)} is missing: the ctypes binding is derived from it")
    with open(path) as f:
        return parse(f.read())
