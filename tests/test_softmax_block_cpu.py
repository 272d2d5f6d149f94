"""The many-tokens-at-once route onto the softmax KV cache without a GPU: its header's rows of the binding table against the
prototypes, the workspace formula, the C ABI's host-side refusals in their documented order and the classes' switches."""
import ctypes
import os

import pytest
import torch

from fastmax_experiments_amd import _lib, build, decode
from test_binding_cpu import ctypes_kind, header_prototypes

HEADER = "fastmax_hip_softmax_block.h"
P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host


def test_rows_match_the_header_and_the_library():
    protos = header_prototypes(HEADER)
    assert [n for n, _, _ in protos] == list(_lib.ABI_EXT5), "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI_EXT5[name]
        assert ctypes_kind(restype) == ret and [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    earlier = set(_lib.ABI) | set(_lib.ABI_EXT) | set(_lib.ABI_EXT2) | set(_lib.ABI_EXT3) | set(_lib.ABI_EXT4)
    assert _lib.HEADERS_EXT5 == (HEADER,) and not set(_lib.ABI_EXT5) & earlier
    assert os.path.join("..", "..", "include", HEADER) in build.HEADERS and "softmax_kv_block.hip" in build.SOURCES
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9
    text = open(os.path.join(os.path.dirname(build.HERE), "include", HEADER)).read()
    for name in ("ROWS", "ROWS_D256", "SPAN", "TOKENS"):          # the constants mirror the header's defines
        assert f"#define FASTMAX_KV_BLOCK_{name} {getattr(_lib, 'KV_BLOCK_' + name)}\n" in text


@pytest.mark.parametrize("B, H, Hkv, T, D, max_len, taken", [
    (2, 8, 2, 1, 64, 300, 1), (1, 20, 1, 500, 16, 128, 1), (3, 32, 4, 64, 128, 5000, 1), (1, 4, 4, 65, 256, 513, 1), (1, 2, 2, 1, 12, 16, 0),
    (1, 2, 2, 1, 264, 16, 0), (1, 3, 2, 1, 64, 16, 0), (1, 2, 2, 0, 64, 16, 0), (1, 2, 2, 1, 64, 0, 0), (65536, 1, 1, 1, 64, 16, 0), (1, 2, 0, 1, 64, 16, 0)])
def test_workspace_formula_and_zero_for_a_rejected_shape(B, H, Hkv, T, D, max_len, taken):
    chunks = -(-max_len // _lib.KV_CHUNK)
    want = taken * B * H * min(T, _lib.KV_BLOCK_TOKENS) * (-(-chunks // _lib.KV_BLOCK_SPAN) * (D + 2) + 1) * 4
    assert _lib.lib().fastmax_hip_softmax_kv_block_workspace(B, H, Hkv, T, D, max_len) == want


def _call(kw):
    a = {**dict(q=P, k=P, v=P, o=P, state=P, lse=None, ws=P, B=1, H=2, Hkv=1, T=3, D=64, dtype=_lib.BF16, scale=0.125, ws_bytes=1 << 30,
                st=(640, 640, 64)), **kw}
    s = (ctypes.c_int64 * 3)(*a["st"])
    return _lib.lib().fastmax_hip_softmax_kv_append_attend_block(a["q"], s, a["k"], s, a["v"], s, a["state"], a["o"], a["lse"], a["B"], a["H"],
                                                                 a["Hkv"], a["T"], a["D"], 16, a["dtype"], a["scale"], a["ws"],
                                                                 a["ws_bytes"], None)


# each refusal alone, then each with every later kind of mistake in the same call: the earlier one in the documented order wins
MISTAKES = [(dict(k=None), _lib.E_NULL), (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(D=12), _lib.E_BAD_SHAPE),
            (dict(v=P + 2), _lib.E_ALIGNMENT), (dict(ws_bytes=64), _lib.E_WORKSPACE)]


@pytest.mark.parametrize("kw, code", MISTAKES + [({**MISTAKES[i][0], **MISTAKES[j][0]}, MISTAKES[i][1]) for i in range(5) for j in range(i + 1, 5)] + [
    (dict(state=None), _lib.E_NULL), (dict(ws=None), _lib.E_NULL), (dict(dtype=_lib.F64), _lib.E_BAD_DTYPE), (dict(D=264), _lib.E_BAD_SHAPE),
    (dict(T=0), _lib.E_BAD_SHAPE), (dict(Hkv=3), _lib.E_BAD_SHAPE), (dict(scale=float("inf")), _lib.E_BAD_SHAPE),
    (dict(state=P + 4), _lib.E_ALIGNMENT), (dict(st=(640, 640, 68)), _lib.E_ALIGNMENT), (dict(lse=P + 2), _lib.E_ALIGNMENT)])
def test_host_side_refusals_in_the_documented_order(kw, code):
    assert _call(kw) == code


def test_the_switch_is_off_and_the_fp8_cache_refuses():
    assert decode.SoftmaxKVDecodeState.block_extend is False
    st = object.__new__(decode.SoftmaxKVDecodeState)          # nothing is run: the attribute alone
    assert st.block_extend is False
    st.block_extend = True
    assert st.block_extend is True and decode.SoftmaxKVDecodeState.block_extend is False
    st._append_attend = lambda q, k, v, T, lse=False, block=False: (T, block)          # which route a call would take
    many, one = torch.zeros(1, 2, 3, 64), torch.zeros(1, 2, 1, 64)
    assert st.extend(many, many, many) == (3, True) and st.extend(one, one, one) == (1, False) and st.step(one, one, one) == (1, False)
    st.block_extend = False
    assert st.extend(many, many, many) == (3, False) and st.extend_block(one, one, one) == (1, True)
    f8 = object.__new__(decode.SoftmaxFP8KVDecodeState)
    assert f8.block_extend is False
    f8.block_extend = False
    with pytest.raises(NotImplementedError, match="SoftmaxKVDecodeState"):
        f8.block_extend = True
    with pytest.raises(NotImplementedError, match="16-bit"):
        f8.extend_block(*(torch.zeros(1, 2, 3, 64),) * 3)
    assert f8.block_extend is False
