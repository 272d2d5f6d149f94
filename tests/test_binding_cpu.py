"""The ctypes table in fastmax_experiments_amd/_lib.py against the prototypes in the public headers under include/
(_lib.HEADERS): same functions in the same order, and for each one the same number of parameters and the same kind of every
parameter and of the return type.  A wrong entry would hand a kernel garbage without any error, so this is checked from the
headers' text; per header, also that the library exports every name and that the bound types are the table's, and that the build
watches the header.  This is the only place that parses the headers and the only one that checks the table against them: a new
header needs a name in _lib.HEADERS, rows at the end of _lib.ABI and a new checksum below, and no test of its own for this."""
import ctypes
import os
import re
import zlib

import pytest

from fastmax_experiments_amd import _lib, build

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
    assert _lib.HEADERS == ("fastmax_hip.h", "fastmax_hip_generate.h", "fastmax_hip_linearmax_decode.h", "fastmax_hip_block.h",
                            "fastmax_hip_optim.h", "fastmax_hip_next_token.h", "fastmax_hip_neox.h", "fastmax_hip_cursor.h",
                            "fastmax_hip_nucleus.h", "fastmax_hip_moe.h", "fastmax_hip_moe_decode.h", "fastmax_hip_head.h",
                            "fastmax_hip_adapter.h", "fastmax_hip_kv_decode.h")
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
    assert len(names["fastmax_hip_adapter.h"]) == 3 and len(names["fastmax_hip_kv_decode.h"]) == 5
    assert [t is _lib.i64p for t in _lib.ABI["fastmax_hip_kv_decode_append_attend"][1][:6]] == [False, True] * 3
    assert [t is _lib.i64p for t in _lib.ABI["fastmax_hip_kv_decode_load"][1][:4]] == [False, True] * 2
    every = [n for h in _lib.HEADERS for n in names[h]]
    assert len(every) == len(set(every)), "a name is declared in two headers"


@pytest.mark.parametrize("header", _lib.HEADERS)
def test_table_rows_match_the_header_and_the_library(header):
    """the header's prototypes against their slice of the table, the library's exports and the types bound on the handle"""
    protos = header_prototypes(header)
    start = sum(len(header_prototypes(h)) for h in _lib.HEADERS[:_lib.HEADERS.index(header)])
    rows = list(_lib.ABI.items())[start:start + len(protos)]
    assert protos and [n for n, _, _ in protos] == [n for n, _ in rows], "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for (name, ret, kinds), (_, (restype, argtypes)) in zip(protos, rows):
        assert ctypes_kind(restype) == ret, name
        assert [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    if header != _lib.HEADERS[0]:
        assert '#include "fastmax_hip.h"' in header_text(header)
    assert os.path.join("..", "..", "include", header) in build.HEADERS, "the build does not watch the header"
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9


def test_binding_table_matches_every_prototype():
    protos = [proto for h in _lib.HEADERS for proto in header_prototypes(h)]
    assert [n for n, _, _ in protos] == list(_lib.ABI) == _lib.SYMBOLS
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI[name]
        assert ctypes_kind(restype) == ret, name
        assert len(argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(argtypes, kinds)):
            assert ctypes_kind(t) == kind, f"{name}: parameter {i} is bound as {ctypes_kind(t)}, the header says {kind}"


# crc32 of the (name, return kind, parameter kinds) rows.  The first two were taken on the commit before the four tables became
# one: its ABI alone (the 59 rows of fastmax_hip.h) and its tables concatenated in HEADERS order (68 rows).  The third on the commit
# before the eight side headers' tables joined them: its nine tables concatenated in HEADERS order (98 rows).  The fourth on the
# commit before the last two side tables joined them: its ABI, then its adapter-v2 table, then its KV-cache decode table (106 rows).
PINNED_FIRST_HEADER_CRC, PINNED_FOUR_HEADERS_CRC, PINNED_TWELVE_HEADERS_CRC = 329697078, 1240384090, 3488605058
PINNED_ABI_CRC = 1128403750


def test_pinned_table_and_abi_version_are_unchanged():
    """names in order and their signatures, as checksums taken from the parent commits: no signature moved in the merges"""
    def digest(rows):
        return zlib.crc32(repr([(n, ctypes_kind(r), [ctypes_kind(a) for a in args]) for n, (r, args) in rows]).encode())
    rows = list(_lib.ABI.items())
    assert _lib.ABI_VERSION == 9
    assert len(rows) == 106 and _lib.SYMBOLS == list(_lib.ABI)
    assert digest(rows[:59]) == PINNED_FIRST_HEADER_CRC
    assert digest(rows[:68]) == PINNED_FOUR_HEADERS_CRC
    assert digest(rows[:98]) == PINNED_TWELVE_HEADERS_CRC
    assert digest(rows) == PINNED_ABI_CRC


def test_rows_that_their_headers_define_by_another_row():
    kinds = {n: [ctypes_kind(t) for t in args] for n, (_, args) in _lib.ABI.items()}
    # the dense entry point with a bias is fastmax_hip_last_logits with one more pointer, behind w and its stride
    plain = _lib.ABI["fastmax_hip_last_logits"][1]
    assert _lib.ABI["fastmax_hip_last_logits_bias"][1] == plain[:4] + [_lib.vp] + plain[4:]
    # sample_cursor_nucleus: sample_cursor's arguments plus top_p ahead of the stream; sample_nucleus: sample's plus top_p;
    # nucleus_mask: topk_mask's plus top_p and the temperature
    assert kinds["fastmax_hip_sample_cursor_nucleus"] == kinds["fastmax_hip_sample_cursor"][:-1] + ["float", "pointer"]
    assert len(kinds["fastmax_hip_sample_nucleus"]) == len(kinds["fastmax_hip_sample"]) + 1
    assert len(kinds["fastmax_hip_nucleus_mask"]) == len(kinds["fastmax_hip_topk_mask"]) + 2
    # from fastmax_hip_optim.h on, whatever returns an error code takes the stream last
    for header in _lib.HEADERS[4:]:
        for name, ret, params in header_prototypes(header):
            if ret == "int" and params:
                assert params[-1] == "pointer", f"{name}: the stream comes last"


def test_error_codes_and_abi_version_match_the_header():
    text = header_text("fastmax_hip.h")
    codes = dict(re.findall(r"FASTMAX_(E_[A-Z_]+) = (-\d+)", text))
    assert len(codes) == 6
    for name, value in codes.items():
        assert getattr(_lib, name) == int(value), name
    assert _lib.ABI_VERSION == int(re.search(r"#define FASTMAX_ABI_VERSION (\d+)", text).group(1))
    acts = dict(re.findall(r"FASTMAX_(ACT_[A-Z]+) = (\d+)", header_text("fastmax_hip_block.h")))
    assert {k: int(v) for k, v in acts.items()} == {"ACT_SILU": _lib.ACT_SILU, "ACT_GELU": _lib.ACT_GELU}
