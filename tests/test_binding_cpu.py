"""The ctypes table in fastmax_experiments_amd/_lib.py against the prototypes in the public headers under include/
(_lib.HEADERS): same functions in the same order, and for each one the same number of parameters and the same kind of every
parameter and of the return type.  A wrong entry would hand a kernel garbage without any error, so this is checked from the
headers' text (no library needed).  This is the only place that parses the headers."""
import ctypes
import os
import re
import zlib

from fastmax_experiments_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text(header):
    return open(os.path.join(ROOT, "include", header)).read()


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


def header_prototypes(header):
    """[(name, return kind, [parameter kinds])] in the header's order"""
    text = re.sub(r"/\*.*?\*/", " ", header_text(header), flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(fastmax_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        kinds = [] if params in ("", "void") else [c_kind(p) for p in params.split(",")]
        protos.append((name, c_kind(ret), kinds))
    return protos


def test_parser_reads_the_header():
    protos = dict((n, (r, k)) for n, r, k in header_prototypes("fastmax_hip.h"))
    assert len(protos) == 59
    assert protos["fastmax_hip_error_string"] == ("const char*", ["int"])
    assert protos["fastmax_hip_tune"] == ("int", ["const char*", "int"])
    assert protos["fastmax_hip_build_flags"] == ("int", [])
    assert protos["fastmax_hip_lora_tn_workspace"] == ("int64_t", ["int", "int", "int"])
    assert protos["fastmax_hip_forward_workspace"] == ("size_t", ["pointer"])
    assert protos["fastmax_hip_cross_entropy_backward"][1][:6] == ["pointer", "int64_t", "pointer", "pointer", "pointer", "float"]


def test_each_header_declares_its_own_entry_points():
    assert _lib.HEADERS == ("fastmax_hip.h", "fastmax_hip_generate.h", "fastmax_hip_linearmax_decode.h", "fastmax_hip_block.h")
    names = {h: [n for n, _, _ in header_prototypes(h)] for h in _lib.HEADERS}
    assert len(names["fastmax_hip.h"]) == 59
    assert names["fastmax_hip_generate.h"] == ["fastmax_hip_p2_decode_step_qkv_supported", "fastmax_hip_p2_decode_step_qkv"]
    assert names["fastmax_hip_linearmax_decode.h"] == ["fastmax_hip_linearmax_decode_state_bytes",
                                                       "fastmax_hip_linearmax_decode_advance"]
    assert len(names["fastmax_hip_block.h"]) == 5
    assert [len(_lib.ABI[n][1]) for n in names["fastmax_hip_generate.h"]] == [5, 15]
    assert [len(_lib.ABI[n][1]) for n in names["fastmax_hip_linearmax_decode.h"]] == [4, 15]
    # q, q_strides, k, k_strides, v, v_strides: the strides are bound as int64 pointers, not as untyped ones
    assert [t is _lib.i64p for t in _lib.ABI["fastmax_hip_linearmax_decode_advance"][1][:6]] == [False, True] * 3
    for side in _lib.HEADERS[1:]:
        assert '#include "fastmax_hip.h"' in header_text(side), side


def test_binding_table_matches_every_prototype():
    protos = [proto for h in _lib.HEADERS for proto in header_prototypes(h)]
    assert [n for n, _, _ in protos] == list(_lib.ABI) == _lib.SYMBOLS
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI[name]
        assert ctypes_kind(restype) == ret, name
        assert len(argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(argtypes, kinds)):
            assert ctypes_kind(t) == kind, f"{name}: parameter {i} is bound as {ctypes_kind(t)}, the header says {kind}"


# crc32 of the (name, return kind, parameter kinds) rows, taken on the commit before the four tables became one: its tables
# concatenated in HEADERS order (68 rows), and its ABI alone (the 59 rows of fastmax_hip.h)
PINNED_ABI_CRC, PINNED_FIRST_HEADER_CRC = 1240384090, 329697078


def test_pinned_table_and_abi_version_are_unchanged():
    """names in order and their signatures, as a checksum taken from the parent commit: no signature moved in the merge"""
    def digest(table):
        rows = [(n, ctypes_kind(r), [ctypes_kind(a) for a in args]) for n, (r, args) in table.items()]
        return zlib.crc32(repr(rows).encode())
    assert _lib.ABI_VERSION == 9
    assert len(_lib.ABI) == 68 and _lib.SYMBOLS == list(_lib.ABI)
    assert digest(_lib.ABI) == PINNED_ABI_CRC
    assert digest(dict(list(_lib.ABI.items())[:59])) == PINNED_FIRST_HEADER_CRC


def test_error_codes_and_abi_version_match_the_header():
    text = header_text("fastmax_hip.h")
    codes = dict(re.findall(r"FASTMAX_(E_[A-Z_]+) = (-\d+)", text))
    assert len(codes) == 6
    for name, value in codes.items():
        assert getattr(_lib, name) == int(value), name
    assert _lib.ABI_VERSION == int(re.search(r"#define FASTMAX_ABI_VERSION (\d+)", text).group(1))
    acts = dict(re.findall(r"FASTMAX_(ACT_[A-Z]+) = (\d+)", header_text("fastmax_hip_block.h")))
    assert {k: int(v) for k, v in acts.items()} == {"ACT_SILU": _lib.ACT_SILU, "ACT_GELU": _lib.ACT_GELU}
