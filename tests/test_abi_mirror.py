"""causal-gen_amd/_lib.py mirrors include/cgen_hip.h by hand; this holds the whole mirror to the header, without a GPU.

The header is read twice.  Its TEXT (comments removed) gives the names: every typedef'd struct with its fields in order, every
`#define CGEN_*` and enumerator, every `cgen_*(...)` declaration with its parameter types.  ONE C program, built from those names,
compiled with gcc against include/ and run once, gives the numbers: sizeof and, per field, offsetof and sizeof; each constant's
value.  A wrong offset in one of these records is not a failing assertion on the GPU but a pointer read from the wrong slot, so
everything is compared -- a struct, constant or entry point added to the header is covered once it is mirrored, and fails here
until it is."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT

from causal_gen_amd import _lib

# header constants that deliberately have no mirror in _lib
UNMIRRORED = set()

INT64_TYPES, INT32_TYPES = {"int64_t", "uint64_t", "size_t"}, {"int32_t", "uint32_t", "int", "unsigned"}


@functools.lru_cache(maxsize=None)
def header_text():
    src = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def header_structs():
    """{struct name: [field names in order]}; `int32_t a, b[4];` declares a and b."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", header_text()):
        decls = [d for d in body.split(";") if d.strip()]
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", piece).group(1) for d in decls for piece in d.split(",")]
    return out


def header_constants():
    """Names of every `#define CGEN_*` (but the include guard) and every CGEN_* enumerator."""
    src = header_text()
    names = [n for n in re.findall(r"^\s*#\s*define\s+(CGEN_\w+)\b(?!\()", src, re.M) if n != "CGEN_HIP_H"]
    for body in re.findall(r"\benum\s+\w*\s*\{([^{}]*)\}", src):
        names += re.findall(r"\b(CGEN_\w+)\b", body)
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    return names


def header_prototypes():
    """{entry point: (return type, [parameter declarations])}, a parameter declaration as written (`const cgen_view* a`, `cgen_stream_t`)."""
    src = header_text()
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(cgen_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src, re.M):
        params = " ".join(params.split())
        out[name] = (ret.replace(" ", ""), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    # (the pattern of tests/test_abi.py: nothing that looks like a declaration was left out by the stricter one above)
    assert sorted(out) == sorted(set(re.findall(r"\b(cgen_[a-z0-9_]+)\s*\(", src)))
    return out


@functools.lru_cache(maxsize=None)
def gcc_says():
    """({struct: sizeof}, {(struct, field): (offsetof, sizeof)}, {constant: value}) of the header, from one compiled program."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "cgen_hip.h"', "int main(void) {"]
    for s, fields in header_structs().items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f) for f in fields]
    lines += ['printf("K %s %%lld\\n", (long long)(%s));' % (k, k) for k in header_constants()]
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "mirror.c"), os.path.join(d, "mirror")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        rows = [r.split() for r in subprocess.check_output([exe], text=True).splitlines()]
    sizes = {r[1]: int(r[2]) for r in rows if r[0] == "S"}
    fields = {(r[1], r[2]): (int(r[3]), int(r[4])) for r in rows if r[0] == "F"}
    consts = {r[1]: int(r[2]) for r in rows if r[0] == "K"}
    return sizes, fields, consts


def test_every_struct_is_registered():
    assert set(header_structs()) == set(_lib.STRUCTS)
    mirrors = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == _lib.__name__}
    assert mirrors == set(_lib.STRUCTS.values()), sorted(m.__name__ for m in mirrors ^ set(_lib.STRUCTS.values()))
    assert len(_lib.STRUCTS) >= 26


def test_struct_layouts_match_header():
    """sizeof of every struct; name, order, offset and size of every field (`in_` in Python stands for `in`, a keyword)."""
    sizes, fields, _ = gcc_says()
    wrong = []
    for cname, names in header_structs().items():
        cls = _lib.STRUCTS.get(cname)
        if cls is None:
            wrong.append((cname, "no mirror"))
            continue
        mine = [f[0] for f in cls._fields_]
        if [re.sub(r"_$", "", f) for f in mine] != names:
            wrong.append((cname, "fields", mine, names))
            continue
        if C.sizeof(cls) != sizes[cname]:
            wrong.append((cname, "sizeof", C.sizeof(cls), sizes[cname]))
        for py, f in zip(mine, names):
            d = getattr(cls, py)
            if (d.offset, d.size) != fields[cname, f]:
                wrong.append((cname, f, "offset, size", (d.offset, d.size), fields[cname, f]))
    assert not wrong, wrong
    assert len(fields) >= 393


def test_constants_match_header():
    """CGEN_X of the header is X of _lib with the header's value; ABI_VERSION is one of them."""
    _, _, consts = gcc_says()
    assert set(consts) == set(header_constants()) and len(consts) >= 61
    wrong = []
    for cname, value in consts.items():
        name = cname[len("CGEN_"):]
        if not hasattr(_lib, name):
            if cname not in UNMIRRORED:
                wrong.append((cname, "no mirror"))
        elif cname in UNMIRRORED:
            wrong.append((cname, "mirrored, yet listed in UNMIRRORED"))
        elif getattr(_lib, name) != value:
            wrong.append((cname, getattr(_lib, name), value))
    assert not wrong, wrong
    assert UNMIRRORED <= set(consts), sorted(UNMIRRORED - set(consts))


def _c_class(decl):
    """The class of a C parameter declaration, as the table of classes below names it."""
    words = set(re.findall(r"\w+", decl))
    if "*" in decl or "[" in decl or "cgen_stream_t" in words:
        return "pointer"
    for cls, names in (("view", {"cgen_view"}), ("float", {"float"}), ("double", {"double"}), ("int64", INT64_TYPES), ("int32", INT32_TYPES)):
        if words & names:
            return cls
    raise AssertionError("a parameter type this test does not know: %r" % decl)


def _ctypes_class(t):
    if t is _lib.View:
        return "view"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    if t in (C.c_float, C.c_double):
        return "float" if t is C.c_float else "double"
    if issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ":
        return {4: "int32", 8: "int64"}.get(C.sizeof(t), "int%d" % (8 * C.sizeof(t)))
    return repr(t)


def test_prototypes_match_header():
    """Argument count and, per argument, its class: pointer (any `*`, or cgen_stream_t) / cgen_view by value / float / double /
    8-byte integer / 4-byte integer.  `const char*` functions are exactly _RESTYPES; everything else returns int."""
    protos = header_prototypes()
    assert set(protos) == set(_lib.PROTOTYPES) and len(protos) >= 123
    wrong = []
    for name, (ret, params) in protos.items():
        want, got = [_c_class(p) for p in params], [_ctypes_class(t) for t in _lib.PROTOTYPES[name]]
        if want != got:
            wrong.append((name, [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g] or (len(want), len(got))))
        if ret not in ("int", "constchar*"):
            wrong.append((name, "returns", ret))
    assert not wrong, wrong
    assert {n for n, (ret, _) in protos.items() if ret == "constchar*"} == set(_lib._RESTYPES)
    assert all(t is C.c_char_p for t in _lib._RESTYPES.values())
