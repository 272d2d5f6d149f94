"""The next-token head on a biased or NF4-quantised lm_head (include/fastmax_hip_head.h, csrc/last_logits.hip,
fastmax_experiments_amd/generate.py), everything that needs no device:

1. (the binding table against this header, and the bias entry point's row against the plain one's: test_binding_cpu);
2. every rejection the header lists, returned before any launch;
3. NextTokenHead.quantize_base on host tensors: sizes, state-dict keys, a round trip, the refusals; the default head unchanged."""
import ctypes

import pytest
import torch

from fastmax_experiments_amd import _lib
from fastmax_experiments_amd.generate import NextTokenHead, last_logits
from fastmax_experiments_amd.lora import NF4Linear, NF4Scales


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it
PLAIN = NF4Scales._C(A, None, None, None, 0.0)
DOUBLE = NF4Scales._C(None, A, A, A, 0.25)


def _bias(**over):
    a = dict(x=A, ldx=640, w=A, ldw=128, bias=A, out=A, ldo=515, B=2, V=515, C=128, dtype=_lib.BF16, out_dtype=_lib.F32, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_last_logits_bias(*a.values())


def _nf4(form=PLAIN, **over):
    a = dict(x=A, ldx=640, codes=A, scales=ctypes.byref(form), bias=A, out=A, ldo=515, B=2, V=515,
             C=128, dtype=_lib.BF16, out_dtype=_lib.F32, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_last_logits_nf4(*a.values())


def test_last_logits_bias_rejects_bad_calls_before_any_launch():
    for missing in ("x", "w", "out"):
        assert _bias(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _bias(dtype=dt) == _lib.E_BAD_DTYPE
    assert _bias(dtype=_lib.BF16, out_dtype=_lib.F16) == _lib.E_BAD_DTYPE
    assert _bias(dtype=_lib.F32, out_dtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(B=0), dict(V=0), dict(C=0), dict(B=-1), dict(V=-3), dict(ldw=127), dict(ldo=514), dict(ldx=-1),
                dict(C=2 ** 30 + 8, ldw=2 ** 30 + 8)):
        assert _bias(**bad) == _lib.E_BAD_SHAPE, bad
    for off in (dict(x=A + 1), dict(w=A + 1), dict(bias=A + 1), dict(out=A + 2), dict(dtype=_lib.F32, x=A + 2),
                dict(dtype=_lib.F32, bias=A + 2)):
        assert _bias(**off) == _lib.E_ALIGNMENT, off


@pytest.mark.parametrize("scales", [PLAIN, DOUBLE], ids=["plain", "double"])
def test_last_logits_nf4_rejects_bad_calls_before_any_launch(scales):
    for missing in ("x", "codes", "scales", "out"):
        assert _nf4(scales, **{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _nf4(scales, dtype=dt) == _lib.E_BAD_DTYPE
    assert _nf4(scales, dtype=_lib.BF16, out_dtype=_lib.F16) == _lib.E_BAD_DTYPE
    assert _nf4(scales, dtype=_lib.F32, out_dtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(B=0), dict(V=0), dict(C=0), dict(B=-1), dict(V=-3), dict(C=-64), dict(ldo=514), dict(ldx=-1), dict(C=32),
                dict(C=96), dict(C=100), dict(C=2 ** 30, V=1024, ldo=1024), dict(C=2 ** 20, V=2 ** 20, ldo=2 ** 20)):
        assert _nf4(scales, **bad) == _lib.E_BAD_SHAPE, bad
    for off in (dict(x=A + 1), dict(bias=A + 1), dict(out=A + 2), dict(dtype=_lib.F32, x=A + 2), dict(codes=A + 8),
                dict(codes=A + 4)):
        assert _nf4(scales, **off) == _lib.E_ALIGNMENT, off


def test_a_scales_struct_with_neither_form_filled_is_a_missing_pointer():
    assert _nf4(NF4Scales._C(None, None, None, None, 0.0)) == _lib.E_NULL
    assert _nf4(NF4Scales._C(None, None, A, A, 0.0)) == _lib.E_NULL              # no codes of the scales: the plain form, without absmax
    assert _nf4(NF4Scales._C(A, A, None, A, 0.0)) == _lib.E_NULL                 # double-quantised without absmax2
    assert _nf4(NF4Scales._C(A, A, A, None, 0.0)) == _lib.E_NULL                 # ... without the map
    assert _nf4(NF4Scales._C(A + 2, None, None, None, 0.0)) == _lib.E_ALIGNMENT
    assert _nf4(NF4Scales._C(None, A + 1, A + 2, A, 0.0)) == _lib.E_ALIGNMENT    # the 8-bit codes may sit anywhere, absmax2 not
    assert _nf4(NF4Scales._C(None, A + 1, A, A + 2, 0.0)) == _lib.E_ALIGNMENT


# ---- 3. the head's bookkeeping -------------------------------------------------------------------------------------------------
C, PADDED, VOCAB = 128, 576, 515


def _head(bias, double_quant=None, seed=5):
    torch.manual_seed(seed)
    head = NextTokenHead(C, PADDED, VOCAB, lm_head_bias=bias)
    return head if double_quant is None else head.quantize_base(double_quant)


def test_the_default_head_is_todays_module():
    head = NextTokenHead(C, PADDED, VOCAB)
    assert list(head.state_dict().keys()) == ["ln_f.weight", "lm_head.weight"]
    assert type(head.lm_head) is torch.nn.Linear and head.lm_head.bias is None
    assert list(NextTokenHead(C, PADDED, VOCAB, lm_head_bias=False).state_dict().keys()) == ["ln_f.weight", "lm_head.weight"]
    assert list(NextTokenHead(C, PADDED, norm_class="LayerNorm").state_dict().keys()) == ["ln_f.weight", "ln_f.bias", "lm_head.weight"]


def test_the_bias_takes_the_references_state_dict_key():
    head = _head(True)
    assert list(head.state_dict().keys()) == ["ln_f.weight", "lm_head.weight", "lm_head.bias"]
    assert head.state_dict()["lm_head.bias"].shape == (PADDED,)


@pytest.mark.parametrize("double_quant", [False, True], ids=["plain", "double"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_quantize_base_sizes_and_state_dict_keys(bias, double_quant):
    dense = _head(bias)
    w, b = dense.lm_head.weight.detach().clone(), None if not bias else dense.lm_head.bias.detach().clone()
    head = dense.quantize_base(double_quant)
    assert head is dense and isinstance(head.lm_head, NF4Linear) and head.lm_head.double_quant == double_quant
    qs = head.lm_head.weight.quant_state
    assert head.lm_head.weight.dtype == torch.uint8 and head.lm_head.weight.shape == (PADDED * C // 2,)
    assert qs[0].shape == (PADDED * C // 64,) and qs[0].dtype == (torch.uint8 if double_quant else torch.float32)
    assert tuple(qs[1]) == (PADDED, C)
    if double_quant:
        offset, (absmax2, code2) = qs[4]
        assert absmax2.shape == (-(-PADDED * C // 64 // 256),) and code2.shape == (256,) and offset.shape == ()
    keys = ["ln_f.weight", "lm_head.weight"] + (["lm_head.bias"] if bias else []) + ["lm_head._extra_state"]
    assert list(head.state_dict().keys()) == keys
    assert (head.lm_head.bias is None) == (not bias)
    if bias:
        assert torch.equal(head.lm_head.bias, b.float())
    # NF4 at block 64: every weight within half the widest codebook gap (0.304 / 2) of its block's absmax, plus the scale's own error
    err = (head.lm_head.dequantize() - w).abs().reshape(-1, 64)
    slack = 0.153 if not double_quant else 0.2
    assert (err <= slack * w.abs().reshape(-1, 64).amax(1, keepdim=True)).all()


@pytest.mark.parametrize("double_quant", [False, True], ids=["plain", "double"])
def test_a_state_dict_round_trip_into_a_fresh_quantised_head(double_quant):
    src = _head(True, double_quant)
    with torch.no_grad():
        src.lm_head.bias.copy_(torch.randn(PADDED))
    dst = _head(True, double_quant, seed=6)
    assert not torch.equal(dst.lm_head.weight, src.lm_head.weight)
    result = dst.load_state_dict(src.state_dict())
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(dst.lm_head.weight, src.lm_head.weight) and torch.equal(dst.lm_head.bias, src.lm_head.bias)
    assert torch.equal(dst.lm_head.dequantize(), src.lm_head.dequantize())
    assert dst.lm_head.double_quant == double_quant


def test_quantize_base_refusals_and_the_second_call():
    with pytest.raises(ValueError, match="multiple of 64"):
        NextTokenHead(96, PADDED).quantize_base()
    for dq in (False, True):
        head = _head(True, dq)
        lm = head.lm_head
        assert head.quantize_base(dq) is head and head.lm_head is lm            # a second call: nothing happens
        with pytest.raises(ValueError, match="already quantised"):
            head.quantize_base(not dq)
        assert head.lm_head is lm


def test_last_logits_checks_its_arguments_before_any_call():
    x = torch.zeros(2, C)
    w = torch.zeros(PADDED, C)
    lm = _head(False, False).lm_head
    for weight in (w, lm, lm.weight):
        with pytest.raises(ValueError, match="rows should lie"):
            last_logits(x, weight, rows=PADDED + 1)
        with pytest.raises(ValueError, match="rows should lie"):
            last_logits(x, weight, rows=0)
        with pytest.raises(ValueError, match="bias should hold"):
            last_logits(x, weight, bias=torch.zeros(VOCAB - 1), rows=VOCAB)
        with pytest.raises(ValueError, match="bias should hold"):
            last_logits(x, weight, bias=torch.zeros(PADDED, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="x should be"):
            last_logits(torch.zeros(2, C + 64), weight)
        with pytest.raises(RuntimeError, match="no CPU path"):
            last_logits(x, weight, bias=torch.zeros(PADDED), rows=VOCAB)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        last_logits(x.double(), lm)
    odd = NF4Linear(96, 64, bias=False)                     # 96 x 64 weights are whole blocks, a row of 96 is not
    with pytest.raises(ValueError, match="C % 64 == 0"):
        last_logits(torch.zeros(1, 96), odd)
