"""The ctypes table in fastmax_experiments_amd/_lib.py against the prototypes in include/fastmax_hip.h: same functions in
the same order, and for each one the same number of parameters and the same kind of every parameter and of the return type.
A wrong entry would hand a kernel garbage without any error, so this is checked from the header's text (no library needed)."""
import ctypes
import os
import re

from fastmax_experiments_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_kind(decl):
    """kind of one C parameter or return type: 'pointer', 'const char*', 'int', 'int64_t', 'size_t' or 'float'"""
    decl = " ".join(decl.split())
    if "*" in decl:
        return "const char*" if re.match(r"const char ?\*", decl) else "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words[0] in ("int", "int64_t", "size_t", "float"), decl
    return words[0]


def ctypes_kind(t):
    if t is ctypes.c_char_p:
        return "const char*"
    if t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float"}[t]


def header_prototypes():
    """[(name, return kind, [parameter kinds])] in the header's order"""
    text = open(os.path.join(ROOT, "include", "fastmax_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(fastmax_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        kinds = [] if params in ("", "void") else [c_kind(p) for p in params.split(",")]
        protos.append((name, c_kind(ret), kinds))
    return protos


def test_parser_reads_the_header():
    protos = dict((n, (r, k)) for n, r, k in header_prototypes())
    assert len(protos) == 59
    assert protos["fastmax_hip_error_string"] == ("const char*", ["int"])
    assert protos["fastmax_hip_tune"] == ("int", ["const char*", "int"])
    assert protos["fastmax_hip_build_flags"] == ("int", [])
    assert protos["fastmax_hip_lora_tn_workspace"] == ("int64_t", ["int", "int", "int"])
    assert protos["fastmax_hip_forward_workspace"] == ("size_t", ["pointer"])
    assert protos["fastmax_hip_cross_entropy_backward"][1][:6] == ["pointer", "int64_t", "pointer", "pointer", "pointer", "float"]


def test_binding_table_matches_every_prototype():
    protos = header_prototypes()
    assert [n for n, _, _ in protos] == list(_lib.ABI) == _lib.SYMBOLS
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI[name]
        assert ctypes_kind(restype) == ret, name
        assert len(argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(argtypes, kinds)):
            assert ctypes_kind(t) == kind, f"{name}: parameter {i} is bound as {ctypes_kind(t)}, the header says {kind}"


def test_error_codes_and_abi_version_match_the_header():
    text = open(os.path.join(ROOT, "include", "fastmax_hip.h")).read()
    codes = dict(re.findall(r"FASTMAX_(E_[A-Z_]+) = (-\d+)", text))
    assert len(codes) == 6
    for name, value in codes.items():
        assert getattr(_lib, name) == int(value), name
    assert _lib.ABI_VERSION == int(re.search(r"#define FASTMAX_ABI_VERSION (\d+)", text).group(1))
