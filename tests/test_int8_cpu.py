"""The int8 linear without a GPU: _lib.ABI_EXT against its header, the C ABI's host-side refusals, Int8Linear / quantize_base on the CPU."""
import ctypes
import os

import pytest
import torch

from fastmax_experiments_amd import _lib, build
from test_binding_cpu import ctypes_kind, header_prototypes, header_text

HEADER = "fastmax_hip_int8.h"
P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host


def test_ext_rows_match_the_header_and_the_library():
    protos = header_prototypes(HEADER)
    assert [n for n, _, _ in protos] == list(_lib.ABI_EXT), "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI_EXT[name]
        assert ctypes_kind(restype) == ret and [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert _lib.HEADERS_EXT == (HEADER,) and HEADER not in _lib.HEADERS and not set(_lib.ABI_EXT) & set(_lib.ABI)
    assert '#include "fastmax_hip.h"' in header_text(HEADER)
    assert os.path.join("..", "..", "include", HEADER) in build.HEADERS and "int8_linear.hip" in build.SOURCES
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9
    sizes = [bound.fastmax_hip_int8_linear_workspace(M, 192) for M in (1, 2, 16, 17, 129, 4096)]          # monotone in M
    assert sizes == sorted(sizes) and sizes[0] >= 192 * 6 + 8 and all(s % 16 == 0 for s in sizes)
    assert bound.fastmax_hip_int8_linear_workspace(4, 96) == 0 and bound.fastmax_hip_int8_linear_workspace(0, 64) == 0


def _linear(x=P, ldx=64, cb=P, scb=P, y=P, ldy=16, M=1, N=16, K=64, dtype=_lib.BF16, ws=P, ws_bytes=1 << 30):
    return _lib.lib().fastmax_hip_int8_linear(x, ldx, cb, scb, None, y, ldy, M, N, K, dtype, 6.0, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code", [
    (dict(K=96, ldx=96), _lib.E_BAD_SHAPE), (dict(N=24, ldy=24), _lib.E_BAD_SHAPE), (dict(M=0), _lib.E_BAD_SHAPE),
    (dict(K=133184, ldx=133184), _lib.E_BAD_SHAPE),                        # K * 16129 >= 2^31
    (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(ldx=56), _lib.E_BAD_SHAPE), (dict(ldy=8), _lib.E_BAD_SHAPE),
    (dict(x=None), _lib.E_NULL), (dict(cb=None), _lib.E_NULL), (dict(scb=None), _lib.E_NULL), (dict(y=None), _lib.E_NULL),
    (dict(ws=None), _lib.E_NULL), (dict(x=P + 2), _lib.E_ALIGNMENT), (dict(ws_bytes=16), _lib.E_WORKSPACE)])
def test_host_side_refusals(kw, code):
    assert _linear(**kw) == code


def test_int8_linear_on_the_cpu():
    from fastmax_experiments_amd.lora import Int8Linear
    torch.manual_seed(0)
    lin = torch.nn.Linear(128, 48)
    lin.weight.data[5] = 0.0
    q = Int8Linear.from_linear(lin, threshold=5.0)
    assert q.weight.dtype == torch.int8 and not q.weight.requires_grad and q.SCB.dtype == q.bias.dtype == torch.float32
    err = (q.dequantize(torch.float32) - lin.weight.data).abs()          # within the codec's own half step, element by element
    assert (err <= q.SCB[:, None] / 254 * (1 + 2.0 ** -20)).all() and q.SCB[5] == 0 and not q.weight[5].any()
    fresh = Int8Linear(128, 48)
    fresh.load_state_dict(q.state_dict())
    assert torch.equal(fresh.weight, q.weight) and torch.equal(fresh.SCB, q.SCB) and torch.equal(fresh.bias, q.bias)
    assert set(q.state_dict()) == {"weight", "SCB", "bias"} and q.threshold == 5.0
    for cast in (fresh.half(), fresh.to(torch.bfloat16), fresh.to("cpu", torch.float16)):          # the values survive, not only the dtypes
        assert torch.equal(cast.SCB, q.SCB) and torch.equal(cast.bias, q.bias) and torch.equal(cast.weight, q.weight)
    with pytest.raises(TypeError):
        q(torch.zeros(2, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q(torch.zeros(2, 128, dtype=torch.bfloat16))


def test_quantize_base_modes():
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.generate import NextTokenHead
    from fastmax_experiments_amd.lora import Int8Linear, LoRALinear, NF4Linear, merged_state_dict
    assert isinstance(LoRALinear(128, 64, r=4).quantize_base().linear, NF4Linear)
    assert LoRALinear(128, 64, r=4).quantize_base(mode="bnb.nf4-dq").linear.double_quant
    lin = LoRALinear(128, 64, r=4).quantize_base(mode="bnb.int8")
    assert isinstance(lin.linear, Int8Linear) and lin.plan(torch.zeros(2, 128, dtype=torch.bfloat16)).route == "tensor_ops"
    with pytest.raises(ValueError, match=r"bnb\.nf4, bnb\.nf4-dq, bnb\.int8"):
        LoRALinear(128, 64).quantize_base(mode="bnb.fp4")
    with pytest.raises(ValueError, match="already quantised as bnb.int8"):
        lin.quantize_base(mode="bnb.nf4")
    assert lin.quantize_base().linear is lin.linear and lin.quantize_base(mode="bnb.int8").linear is lin.linear
    dense = merged_state_dict(torch.nn.ModuleDict({"fc": lin}), torch.float32)          # int8 bases are written dense
    assert set(dense) == {"fc.weight", "fc.bias"} and torch.equal(dense["fc.weight"], lin.linear.dequantize())
    blk = Block.from_config("pythia-14m").quantize_base(mode="bnb.int8")
    assert [type(m.linear) for m in blk.modules() if isinstance(m, LoRALinear)] == [Int8Linear] * 5
    with pytest.raises(NotImplementedError, match="int8 lm_head"):
        NextTokenHead(128, 512).quantize_base(mode="bnb.int8")
