"""Softmax attention without a GPU: the block accepts attn_alg="quadratic" and plans "softmax", the caches are told apart, the new
header's rows of the binding table against its prototypes, the C ABI's host-side refusals, the float64 reference against torch's."""
import ctypes
import os

import pytest
import torch

import softmax_ref
from fastmax_experiments_amd import _lib, build, decode
from fastmax_experiments_amd.attention_block import CausalSelfAttention
from test_binding_cpu import ctypes_kind, header_prototypes

HEADER = "fastmax_hip_softmax.h"
P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host


class _Cache:
    """a cache of a class where nothing is run: check_block_cache looks at the class and p only"""
    def __new__(cls, kind, p=2):
        st = object.__new__(kind)
        st.p = p
        return st


def test_the_block_accepts_quadratic_and_plans_softmax():
    kw = dict(n_embd=64, n_head=4, n_query_groups=1, head_size=16, r=0)
    attn = CausalSelfAttention(attn_alg="quadratic", **kw)
    x = torch.zeros(2, 3, 64)
    assert attn.plan(x) == CausalSelfAttention(attn_alg="fastmax", **kw).plan(x)._replace(operator="softmax")
    with pytest.raises(ValueError, match="performer not supported"):
        CausalSelfAttention(attn_alg="performer", **kw)
    cos = sin = torch.zeros(3, 16)
    with pytest.raises(NotImplementedError, match="SoftmaxKVDecodeState"):          # input_pos without a state points to the cache
        attn(x, cos, sin, input_pos=torch.arange(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            attn.bfloat16()(x.bfloat16(), cos, sin)
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.neox_block import NeoXBlock
    for blk in (Block.from_config("tiny-llama-1.1b", attn_alg="quadratic"), NeoXBlock.from_config("pythia-14m", attn_alg="quadratic"),
                Block.from_config("Mixtral-8x7B-v0.1", attn_alg="quadratic", intermediate_size=64, n_expert=2, n_expert_per_token=1)):
        assert blk.attn.attn_alg == "quadratic"


def test_check_block_cache_tells_the_caches_apart():
    soft, kv, lin = (_Cache(k) for k in (decode.SoftmaxKVDecodeState, decode.FastmaxKVDecodeState, decode.LinearmaxDecodeState))
    decode.check_block_cache("quadratic", soft)
    decode.check_block_cache("fastmax", kv)
    decode.check_block_cache("linearmax", lin)
    for wrong in (kv, lin, _Cache(decode.FastmaxDecodeState)):
        with pytest.raises(TypeError, match="SoftmaxKVDecodeState"):
            decode.check_block_cache("quadratic", wrong)
    with pytest.raises(TypeError, match="FastmaxKVDecodeState, not on a SoftmaxKVDecodeState"):
        decode.check_block_cache("fastmax", soft)
    with pytest.raises(TypeError, match="LinearmaxDecodeState, not on a SoftmaxKVDecodeState"):
        decode.check_block_cache("linearmax", soft)
    for kw, err in ((dict(D=12), NotImplementedError), (dict(D=264), NotImplementedError), (dict(dtype=torch.float32), ValueError)):
        with pytest.raises(err):
            decode.SoftmaxKVDecodeState(**{**dict(B=1, H=2, D=64, device="cpu", max_len=16, dtype=torch.bfloat16), **kw})


def test_rows_match_the_header_and_the_library():
    protos = header_prototypes(HEADER)
    assert [n for n, _, _ in protos] == list(_lib.ABI_EXT2), "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI_EXT2[name]
        assert ctypes_kind(restype) == ret and [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert _lib.HEADERS_EXT2 == (HEADER,) and not set(_lib.ABI_EXT2) & (set(_lib.ABI) | set(_lib.ABI_EXT))
    assert os.path.join("..", "..", "include", HEADER) in build.HEADERS
    assert {"softmax_attention.hip", "softmax_kv_decode.hip"} <= set(build.SOURCES)
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9
    ws = bound.fastmax_hip_softmax_kv_workspace
    assert ws(2, 8, 2, 1, 64, 300) == 2 * 8 * (3 * 66 + 2) * 4 and ws(2, 8, 2, 50, 64, 300) == 8 * ws(2, 8, 2, 1, 64, 300)
    assert ws(1, 2, 2, 1, 12, 16) == 0 and ws(1, 2, 2, 1, 264, 16) == 0 and ws(1, 3, 2, 1, 64, 16) == 0


def _call(fn, kw):
    a = {**dict(q=P, k=P, v=P, o=P, B=1, H=2, Hkv=1, T=3, D=64, dtype=_lib.BF16, ws_bytes=1 << 30, st=(640, 640, 64)), **kw}
    s = (ctypes.c_int64 * 3)(*a["st"])
    qkv = (a["q"], s, a["k"], s, a["v"], s)
    if fn == "forward":
        return _lib.lib().fastmax_hip_softmax_forward(*qkv, a["o"], None, a["B"], a["H"], a["Hkv"], a["T"], a["D"], a["dtype"], 0.125, None)
    return _lib.lib().fastmax_hip_softmax_kv_append_attend(*qkv, P, a["o"], None, a["B"], a["H"], a["Hkv"], a["T"], a["D"], 16, a["dtype"],
                                                           0.125, P, a["ws_bytes"], None)


@pytest.mark.parametrize("fn", ["forward", "kv_append_attend"])
@pytest.mark.parametrize("kw, code", [
    (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(dtype=_lib.F64), _lib.E_BAD_DTYPE), (dict(D=12), _lib.E_BAD_SHAPE),
    (dict(D=264), _lib.E_BAD_SHAPE), (dict(T=0), _lib.E_BAD_SHAPE), (dict(Hkv=3), _lib.E_BAD_SHAPE), (dict(q=None), _lib.E_NULL),
    (dict(o=None), _lib.E_NULL), (dict(k=P + 2), _lib.E_ALIGNMENT), (dict(st=(640, 640, 68)), _lib.E_ALIGNMENT)])
def test_host_side_refusals(fn, kw, code):
    assert _call(fn, kw) == code


def test_a_short_workspace_is_refused():
    assert _call("kv_append_attend", dict(ws_bytes=64)) == _lib.E_WORKSPACE


def test_reference_agrees_with_torch():
    q, k, v = softmax_ref.inputs(2, 4, 2, 37, 16, torch.bfloat16, 0)
    ref = softmax_ref.reference(q, k, v)
    kx, vx = (t.double().repeat_interleave(2, dim=1) for t in (k, v))
    want = torch.nn.functional.scaled_dot_product_attention(q.double(), kx, vx, is_causal=True)
    assert (ref["o"] - want).abs().max() < 1e-13
    lse = torch.logsumexp((q.double() @ kx.transpose(-1, -2) / 4).masked_fill(~torch.ones(37, 37, dtype=torch.bool).tril(), -1e300), -1)
    assert (ref["lse"] - lse).abs().max() < 1e-13 and (ref["allow_o"] > 0).all() and (ref["allow_lse"] > 0).all()
