"""The decode-size expert kernels on device-side row counts (include/fastmax_hip_moe_decode.h, csrc/moe_decode.hip,
fastmax_experiments_amd/moe.py ``device_routed``), everything that needs no device:

1. the row limit against the header, source and shared headers in the build's lists (the binding table against this header:
   test_binding_cpu);
2. the packer's entry size against the library's ``sizeof``;
3. every rejection of the C ABI, returned before any launch (null streams, made-up addresses);
4. what the ``device_routed`` setter refuses, each with its own message, and what ``GraphedDecoder`` refuses before it touches a
   device."""
import ctypes

import pytest
import torch

from fastmax_experiments_amd import _lib, build
from fastmax_experiments_amd.decode import _DecodeState
from test_binding_cpu import header_text



# ---- 1. limit, build ------------------------------------------------------------------------------------------------------------
def test_the_limit_is_the_headers_and_it_builds_on_the_moe_header():
    text = header_text("fastmax_hip_moe_decode.h")
    assert '#include "fastmax_hip_moe.h"' in text
    assert f"#define FASTMAX_MOE_DECODE_MAX_ROWS {_lib.MOE_DECODE_MAX_ROWS}" in text


def test_the_build_lists_the_source_and_the_headers():
    assert "moe_decode.hip" in build.SOURCES and "nf4_lora.hip" in build.SOURCES
    assert "nf4_gemv.h" in build.HEADERS and "row_kernels.h" in build.HEADERS


# ---- 2. the table's entry ---------------------------------------------------------------------------------------------------
def test_the_packer_s_entry_is_the_library_s():
    from fastmax_experiments_amd import lora, moe
    assert _lib.lib().fastmax_hip_moe_expert_entry_bytes() == moe.ENTRY_BYTES == ctypes.sizeof(moe._ExpertEntry)
    # three linears, each a code pointer, the fastmax_nf4_scales fields and a bias pointer
    assert moe.ENTRY_BYTES == 3 * (2 * ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(lora.NF4Scales._C))
    assert [n for n, _ in moe._ExpertEntry._fields_] == ["fc_1", "fc_2", "proj"]
    assert [n for n, _ in moe._LinearEntry._fields_] == ["wq", "scales", "bias"]


# ---- 3. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _call(name, defaults, over):
    a = dict(defaults)
    a.update(over)
    return getattr(_lib.lib(), name)(*a.values())


def _up(**over):
    return _call("fastmax_hip_moe_experts_up", dict(x=A, xs=256, table=A, offsets=A, row_of=A, h=A, hs=384, M=5, E=8, k=2, C=256,
                                                    I=384, dtype=_lib.BF16, stream=None), over)


def _down(**over):
    return _call("fastmax_hip_moe_experts_down", dict(h=A, hs=384, table=A, offsets=A, ys=A, yss=256, M=5, E=8, k=2, C=256, I=384,
                                                      dtype=_lib.BF16, stream=None), over)


POINTERS = {_up: ("x", "table", "offsets", "row_of", "h"), _down: ("h", "table", "offsets", "ys")}
MISALIGNED = {"x": 8, "h": 8, "ys": 8, "table": 4, "offsets": 2, "row_of": 2}       # off 16 bytes / 8 bytes / a 4-byte element
STRIDES = {_up: (("xs", 256), ("hs", 384)), _down: (("hs", 384), ("yss", 256))}


def test_the_entry_points_reject_bad_calls_before_any_launch():
    for call, names in POINTERS.items():
        for n in names:
            assert call(**{n: None}) == _lib.E_NULL, (call.__name__, n)
            assert call(**{n: A + MISALIGNED[n]}) == _lib.E_ALIGNMENT, (call.__name__, n)
        for d in (-1, _lib.F16, 3):
            assert call(dtype=d) == _lib.E_BAD_DTYPE, (call.__name__, d)
        for bad in (dict(M=0), dict(M=17), dict(M=-1), dict(E=0), dict(E=_lib.MOE_MAX_EXPERTS + 1), dict(k=0),
                    dict(k=_lib.MOE_MAX_PER_TOKEN + 1, E=16), dict(k=3, E=2), dict(C=0), dict(C=64), dict(C=192), dict(C=-128),
                    dict(I=0), dict(I=320), dict(I=64)):
            assert call(**bad) == _lib.E_BAD_SHAPE, (call.__name__, bad)
        for s, width in STRIDES[call]:
            assert call(**{s: width - 1}) == _lib.E_BAD_SHAPE, (call.__name__, s)
            assert call(**{s: width + 4}) == _lib.E_ALIGNMENT, (call.__name__, s)      # bf16: 8 bytes off a 16-byte row
    # float32 rows: a stride of width + 2 elements is 8 bytes off
    assert _up(dtype=_lib.F32, xs=258) == _lib.E_ALIGNMENT and _down(dtype=_lib.F32, yss=258) == _lib.E_ALIGNMENT
    # M = 16, E = 64, k = 8 are inside the limits: the next check (a misaligned pointer) is what refuses these
    assert _up(M=16, E=64, k=8, x=A + 8) == _lib.E_ALIGNMENT and _down(M=16, E=64, k=8, ys=A + 8) == _lib.E_ALIGNMENT
    assert _up(M=1, E=1, k=1, x=A + 8) == _lib.E_ALIGNMENT


# ---- 4. the host contract ------------------------------------------------------------------------------------------------------
def test_device_routed_is_off_by_default_and_the_setter_names_what_it_refuses():
    from fastmax_experiments_amd.moe import LLaMAMoE
    dense = LLaMAMoE(128, 128, 4, 2)
    assert dense.device_routed is False
    with pytest.raises(ValueError, match="dense.*quantize_base"):
        dense.device_routed = True
    assert dense.device_routed is False
    dense.device_routed = False                                           # off is always allowed
    with pytest.raises(ValueError, match="active LoRA branch"):
        LLaMAMoE(128, 128, 4, 2, r=4, alpha=8, to_mlp=True).quantize_base().device_routed = True
    for n_embd, inter in ((192, 128), (128, 192)):
        with pytest.raises(ValueError, match="multiples of 128"):
            LLaMAMoE(n_embd, inter, 4, 2).quantize_base().device_routed = True
    for double_quant in (False, True):
        ok = LLaMAMoE(128, 256, 4, 2).quantize_base(double_quant)
        ok.device_routed = True
        assert ok.device_routed is True
    # to_mlp = False (the reference's default lora_mlp = False): r reaches neither the gate nor the experts
    lora_elsewhere = LLaMAMoE(128, 128, 4, 2, r=4, alpha=8, to_mlp=False).quantize_base()
    lora_elsewhere.device_routed = True
    assert lora_elsewhere.device_routed and list(lora_elsewhere.state_dict()) == list(LLaMAMoE(128, 128, 4, 2).quantize_base().state_dict())


def test_the_device_route_leaves_every_other_call_where_it_was():
    """no device here: a CPU tensor still meets the fused route's own error, and the tensor-op route ignores the switch"""
    from fastmax_experiments_amd.moe import LLaMAMoE
    layer = LLaMAMoE(128, 128, 4, 2).quantize_base()
    layer.device_routed = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.randn(2, 128))
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer.expert_table()


class _State(_DecodeState):
    """what GraphedDecoder reads of a state cache before it touches a device"""
    def __init__(self, B):
        self.B, self.count = B, 0


def test_graphed_decoder_takes_moe_blocks_only_when_every_layer_is_device_routed():
    from fastmax_experiments_amd import generate
    from fastmax_experiments_amd.block import Block
    blocks = [Block(n_embd=128, n_head=4, intermediate_size=128, mlp_class="LLaMAMoE", n_expert=4, n_expert_per_token=2).quantize_base()
              for _ in range(2)]
    head = generate.NextTokenHead(128, 40)
    kw = dict(cos=torch.zeros(12, 32), sin=torch.zeros(12, 32), max_len=11)

    def build(B, wte=torch.zeros(40, 128)):
        return generate.GraphedDecoder(wte, blocks, head, [_State(B), _State(B)], **kw)

    with pytest.raises(NotImplementedError, match="row counts.*device_routed = True"):
        build(2)
    blocks[0].mlp.device_routed = True                                    # one of two
    with pytest.raises(NotImplementedError, match="row counts"):
        build(2)
    blocks[1].mlp.device_routed = True
    with pytest.raises(NotImplementedError, match="at most 16 rows"):
        build(17)
    with pytest.raises(NotImplementedError, match="bfloat16 or float32"):
        build(2, torch.zeros(40, 128, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="no CPU path"):                # past the MoE checks: the first thing that needs a device
        build(16)
    blocks[1].mlp.fused_neighbours = False                                # the tensor-op route reads per expert
    with pytest.raises(NotImplementedError, match="row counts"):
        build(2)
