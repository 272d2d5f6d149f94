"""The fp8 softmax KV cache without a GPU: its header's rows of the binding table against the prototypes, the size arithmetic, the
C ABI's host-side refusals, the class's own refusals and its place among the caches."""
import ctypes
import os

import pytest
import torch

from fastmax_experiments_amd import _lib, build, decode
from test_binding_cpu import ctypes_kind, header_prototypes

HEADER = "fastmax_hip_kv_fp8.h"
P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host


def test_rows_match_the_header_and_the_library():
    protos = header_prototypes(HEADER)
    assert [n for n, _, _ in protos] == list(_lib.ABI_EXT4), "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI_EXT4[name]
        assert ctypes_kind(restype) == ret and [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    earlier = set(_lib.ABI) | set(_lib.ABI_EXT) | set(_lib.ABI_EXT2) | set(_lib.ABI_EXT3)
    assert _lib.HEADERS_EXT4 == (HEADER,) and not set(_lib.ABI_EXT4) & earlier
    assert os.path.join("..", "..", "include", HEADER) in build.HEADERS and "softmax_kv_fp8.hip" in build.SOURCES
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9


def test_sizes():
    sb, ws = _lib.lib().fastmax_hip_kv_fp8_state_bytes, _lib.lib().fastmax_hip_kv_fp8_workspace
    assert sb(2, 4, 64, 300) == 64 + 2 * 4 * 384 * (2 * 64 + 8) and sb(1, 1, 256, 128) == 64 + 128 * (2 * 256 + 8)
    assert ws(2, 8, 2, 1, 64, 300) == 2 * 8 * (3 * 66 + 2) * 4 and ws(1, 20, 1, 50, 16, 128) == 20 * 8 * (18 + 2) * 4
    assert sb(1, 1, 24, 16) == 0 and sb(1, 1, 264, 16) == 0 and sb(1, 1, 64, 0) == 0 and sb(65536, 1, 64, 16) == 0
    assert ws(1, 2, 2, 1, 24, 16) == 0 and ws(1, 3, 2, 1, 64, 16) == 0 and ws(1, 2, 2, 0, 64, 16) == 0


def _call(fn, kw):
    a = {**dict(q=P, k=P, v=P, o=P, state=P, B=1, H=2, Hkv=1, T=3, D=64, dtype=_lib.BF16, ws_bytes=1 << 30, st=(640, 640, 64)), **kw}
    s = (ctypes.c_int64 * 3)(*a["st"])
    if fn == "load":
        return _lib.lib().fastmax_hip_kv_fp8_load(a["k"], s, a["v"], s, a["state"], a["B"], a["Hkv"], a["T"], a["D"], 16, a["dtype"], None)
    return _lib.lib().fastmax_hip_softmax_kv_fp8_append_attend(a["q"], s, a["k"], s, a["v"], s, a["state"], a["o"], None, a["B"], a["H"],
                                                               a["Hkv"], a["T"], a["D"], 16, a["dtype"], 0.125, P, a["ws_bytes"], None)


@pytest.mark.parametrize("fn", ["load", "append_attend"])
@pytest.mark.parametrize("kw, code", [
    (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(dtype=_lib.F64), _lib.E_BAD_DTYPE), (dict(D=24), _lib.E_BAD_SHAPE),
    (dict(D=264), _lib.E_BAD_SHAPE), (dict(T=0), _lib.E_BAD_SHAPE), (dict(Hkv=0), _lib.E_BAD_SHAPE), (dict(k=None), _lib.E_NULL),
    (dict(state=None), _lib.E_NULL), (dict(v=P + 2), _lib.E_ALIGNMENT), (dict(state=P + 4), _lib.E_ALIGNMENT),
    (dict(st=(640, 640, 68)), _lib.E_ALIGNMENT)])
def test_host_side_refusals(fn, kw, code):
    assert _call(fn, kw) == code


@pytest.mark.parametrize("fn, kw, code", [("append_attend", dict(ws_bytes=64), _lib.E_WORKSPACE), ("append_attend", dict(Hkv=3), _lib.E_BAD_SHAPE),
                                          ("append_attend", dict(o=None), _lib.E_NULL), ("load", dict(T=17), _lib.E_BAD_SHAPE)])
def test_refusals_of_one_entry_point(fn, kw, code):
    assert _call(fn, kw) == code


def test_the_class_refuses_and_is_a_softmax_cache():
    kw0 = dict(B=1, H=2, D=64, device="cpu", max_len=16, dtype=torch.bfloat16)
    for kw, err in ((dict(D=24), NotImplementedError), (dict(D=264), NotImplementedError), (dict(dtype=torch.float32), ValueError),
                    (dict(), RuntimeError)):
        with pytest.raises(err):
            decode.SoftmaxFP8KVDecodeState(**{**kw0, **kw})
    st = object.__new__(decode.SoftmaxFP8KVDecodeState)          # nothing is run: check_block_cache looks at the class and p only
    decode.check_block_cache("quadratic", st)
    with pytest.raises(TypeError, match="FastmaxKVDecodeState"):
        decode.check_block_cache("fastmax", st)
