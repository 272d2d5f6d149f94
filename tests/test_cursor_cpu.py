"""The decode cursor (include/fastmax_hip_cursor.h, csrc/decode_cursor.hip, generate.DecodeCursor / GraphedDecoder), everything that
needs no device:

1. the record's size and word numbers against the header, the source and the shared sampler header in the build's lists (the
   binding table against this header: test_binding_cpu);
2. every rejection the header lists, returned before any launch;
3. the host contract: what GraphedDecoder refuses, before it touches a device, and ``generate(graphed=...)``."""

import pytest
import torch

from fastmax_experiments_amd import _lib, build, generate
from fastmax_experiments_amd.decode import _DecodeState
from test_binding_cpu import header_text


# ---- 1. the record ------------------------------------------------------------------------------------------------------------
def test_the_record_is_whole_int64_words_and_the_word_numbers_are_the_headers():
    nbytes = _lib.lib().fastmax_hip_cursor_bytes()
    assert nbytes % 8 == 0 and nbytes // 8 > _lib.CURSOR_OVERFLOW
    text = header_text("fastmax_hip_cursor.h")
    for word, number in (("POS", _lib.CURSOR_POS), ("NEXT", _lib.CURSOR_NEXT), ("DRAW_BASE", _lib.CURSOR_DRAW_BASE),
                         ("SEED", _lib.CURSOR_SEED), ("OVERFLOW", _lib.CURSOR_OVERFLOW), ("WORDS", nbytes // 8)):
        assert f"FASTMAX_CURSOR_{word} = {number}" in text, word


def test_the_build_compiles_the_source_and_watches_the_headers():
    assert "decode_cursor.hip" in build.SOURCES and "next_token.hip" in build.SOURCES
    assert "next_token_sample.h" in build.HEADERS


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _feed(**over):
    a = dict(cursor=A, tok=A, wte=A, ldw=128, n_wte_rows=515, x=A, ldx=128, B=2, C=128, dtype=_lib.BF16, cos=A, sin=A, ld_rope=16,
             n_rope_rows=13, cos_row=A, sin_row=A, n_cols=8, rope_dtype=_lib.F32, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_cursor_feed(*a.values())


def _sample(**over):
    a = dict(logits=A, ld=515, cursor=A, tok=A, out=A, ldo=13, L=13, done=A, eos_id=-1, B=2, V=515, top_k=50, temperature=0.8,
             stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_sample_cursor(*a.values())


def test_feed_rejects_bad_calls_before_any_launch():
    for missing in ("cursor", "tok", "wte", "x", "cos", "sin", "cos_row", "sin_row"):
        assert _feed(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _feed(dtype=dt) == _lib.E_BAD_DTYPE and _feed(rope_dtype=dt) == _lib.E_BAD_DTYPE
    for bad in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(n_cols=0), dict(n_wte_rows=0), dict(n_rope_rows=0), dict(ldw=127),
                dict(ldx=127), dict(ld_rope=7), dict(C=2 ** 30 + 8, ldw=2 ** 30 + 8, ldx=2 ** 30 + 8)):
        assert _feed(**bad) == _lib.E_BAD_SHAPE, bad
    for odd in (dict(cursor=A + 4), dict(tok=A + 4), dict(wte=A + 1), dict(x=A + 1), dict(cos=A + 2), dict(sin=A + 2),
                dict(cos_row=A + 2), dict(sin_row=A + 2), dict(dtype=_lib.F32, wte=A + 2)):
        assert _feed(**odd) == _lib.E_ALIGNMENT, odd


def test_sample_cursor_rejects_bad_calls_before_any_launch():
    for missing in ("logits", "cursor", "tok", "out"):
        assert _sample(**{missing: None}) == _lib.E_NULL, missing
    assert _sample(done=None, eos_id=3) == _lib.E_NULL                      # done is needed only where an eos is looked for
    for bad in (dict(B=0), dict(V=0), dict(L=0), dict(L=-2), dict(top_k=-1), dict(ld=514), dict(ldo=12), dict(V=2 ** 30 + 1, ld=2 ** 31)):
        assert _sample(**bad) == _lib.E_BAD_SHAPE, bad
    for t in (-0.5, float("nan"), float("inf")):
        assert _sample(temperature=t) == _lib.E_BAD_SHAPE, t
    for odd in (dict(logits=A + 2), dict(cursor=A + 4), dict(tok=A + 4), dict(out=A + 4)):
        assert _sample(**odd) == _lib.E_ALIGNMENT, odd


# ---- 3. the host contract ------------------------------------------------------------------------------------------------------
class _State(_DecodeState):
    """stands for a decode state cache where nothing is run"""
    B, count = 2, 0

    def __init__(self):
        pass


def test_generate_refuses_a_decoder_built_for_another_loop():
    class Decoder:
        def serves(self, *a):
            return False
    head = generate.NextTokenHead(16, 40)
    with pytest.raises(ValueError, match="graphed was built from other"):
        generate.generate(torch.zeros(40, 16), [], head, [], torch.zeros(2, 3, dtype=torch.int64), 6, cos=torch.zeros(8, 4),
                          sin=torch.zeros(8, 4), graphed=Decoder())


def test_graphed_decoder_refusals_come_before_any_device_work():
    from fastmax_experiments_amd.block import Block
    blocks = [Block.from_config("pythia-14m")]
    head = generate.NextTokenHead(128, 40)
    kw = dict(cos=torch.zeros(8, 8), sin=torch.zeros(8, 8), max_len=9)
    wte = torch.zeros(40, 128)
    with pytest.raises(ValueError, match="state caches"):
        generate.GraphedDecoder(wte, blocks, head, [], **kw)
    with pytest.raises(ValueError, match="top_k"):
        generate.GraphedDecoder(wte, blocks, head, [_State()], top_k=0, **kw)
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    with pytest.raises(NotImplementedError, match="by value"):
        generate.GraphedDecoder(wte, blocks, head, [FastmaxDecodeState(2, 4, 32, "cpu", p=1)], **kw)
    head.fused = False
    with pytest.raises(ValueError, match="torch's generator"):
        generate.GraphedDecoder(wte, blocks, head, [_State()], **kw)
    head.fused = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        generate.GraphedDecoder(wte, blocks, head, [_State()], **kw)
    with pytest.raises(ValueError, match="max_len"):
        generate.GraphedDecoder(wte, blocks, head, [_State()], cos=torch.zeros(8, 8), sin=torch.zeros(8, 8), max_len=10)
