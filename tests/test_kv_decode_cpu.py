"""KV-cache decode, everything that needs no device (include/fastmax_hip_kv_decode.h, csrc/fastmax_kv_decode.hip,
fastmax_experiments_amd/decode.py FastmaxKVDecodeState):

1. the source in the build's list and the header's constants against _lib's (the header's rows of _lib.ABI are checked where
   every header's are, in test_binding_cpu.py);
2. the state and workspace sizes against the header's formulas, and 0 for what the route does not take;
3. every rejection the header lists, with its code, returned on made-up aligned addresses before any launch;
4. the constructor's refusals and the host-side refusals of generate() and the block."""
import ctypes
import re

import pytest
import torch

from fastmax_experiments_amd import _lib, build, decode
from test_binding_cpu import header_text

ES = {_lib.F32: 4, _lib.BF16: 2, _lib.F16: 2}


# ---- 1. the build and the binding ------------------------------------------------------------------------------------------------
def test_the_build_compiles_the_source_and_watches_the_header():
    assert "fastmax_kv_decode.hip" in build.SOURCES


def test_constants_match_the_header():
    text = header_text("fastmax_hip_kv_decode.h")

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", text).group(1))

    assert (define("FASTMAX_KV_CHUNK"), define("FASTMAX_KV_SLICE"), define("FASTMAX_KV_MAX_D")) == \
        (_lib.KV_CHUNK, _lib.KV_SLICE, _lib.KV_MAX_D) == (128, 8, 256)
    words = dict(re.findall(r"FASTMAX_KV_(LEN|OVERFLOW|HEADER_WORDS) = (\d+)", text))
    assert (int(words["LEN"]), int(words["OVERFLOW"]), int(words["HEADER_WORDS"])) == \
        (_lib.KV_LEN, _lib.KV_OVERFLOW, _lib.KV_HEADER_WORDS) == (0, 1, 16)


# ---- 2. sizes ----------------------------------------------------------------------------------------------------------------------
def _cap(max_len):
    return -(-max_len // _lib.KV_CHUNK) * _lib.KV_CHUNK


def test_state_bytes_follow_the_formula():
    q = _lib.lib().fastmax_hip_kv_decode_state_bytes
    for B, Hkv, D, max_len in ((1, 1, 256, 1), (2, 3, 64, 127), (2, 3, 64, 128), (1, 2, 33, 129), (8, 32, 128, 2048), (1, 1, 1, 5),
                               (8, 4, 80, 32768), (1, 1, 256, 2 ** 31 - 1)):
        for dt in (_lib.F32, _lib.BF16, _lib.F16):
            want = 4 * _lib.KV_HEADER_WORDS + 2 * B * Hkv * _cap(max_len) * D * ES[dt]
            assert q(B, Hkv, D, max_len, dt) == want and want % 16 == 0, (B, Hkv, D, max_len, dt)
    # slot max_len lies inside the allocation whenever max_len is not a whole number of chunks
    assert _cap(300) == 384 and _cap(128) == 128 and _cap(1) == 128


def test_state_bytes_are_zero_for_what_the_route_does_not_take():
    q = _lib.lib().fastmax_hip_kv_decode_state_bytes
    assert q(1, 1, 256, 64, _lib.BF16) > 0
    for bad in ((1, 1, 257, 64, _lib.BF16), (1, 1, 512, 64, _lib.F32), (1, 1, 0, 64, _lib.BF16), (1, 1, -4, 64, _lib.BF16),
                (1, 1, 64, 0, _lib.BF16), (1, 1, 64, -1, _lib.BF16), (0, 1, 64, 64, _lib.BF16), (1, 0, 64, 64, _lib.BF16),
                (1, 1, 64, 64, 3), (1, 1, 64, 64, -1), (256, 256, 64, 64, _lib.BF16)):
        assert q(*bad) == 0, bad


def test_workspace_follows_the_formula():
    q = _lib.lib().fastmax_hip_kv_decode_workspace
    for B, H, Hkv, T, D, max_len in ((1, 8, 1, 1, 256, 2048), (2, 3, 3, 7, 64, 300), (2, 8, 2, 8, 40, 100), (1, 2, 2, 9, 33, 129),
                                     (8, 32, 32, 1, 128, 32768), (1, 4, 2, 500, 80, 1000)):
        want = B * H * min(T, _lib.KV_SLICE) * (_cap(max_len) // _lib.KV_CHUNK) * (D + 1) * 4
        assert q(B, H, Hkv, T, D, max_len) == want, (B, H, Hkv, T, D, max_len)
    for bad in ((1, 8, 3, 1, 64, 100), (1, 0, 1, 1, 64, 100), (1, 8, 1, 0, 64, 100), (1, 8, 1, 1, 257, 100), (1, 8, 1, 1, 64, 0)):
        assert q(*bad) == 0, bad


# ---- 3. rejections ---------------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it
S3 = (ctypes.c_int64 * 3)(64 * 4 * 8, 64 * 8, 64)


def _attend(**over):
    a = dict(q=A, qs=S3, k=A, ks=S3, v=A, vs=S3, state=A, o=A, B=2, H=8, Hkv=4, T=1, D=64, max_len=300, dtype=_lib.BF16, p=2,
             inv_nt=0.125, ws=A, wsb=1 << 30, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_kv_decode_append_attend(*a.values())


def _load(**over):
    a = dict(k=A, ks=S3, v=A, vs=S3, state=A, B=2, Hkv=4, T=5, D=64, max_len=300, dtype=_lib.BF16, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_kv_decode_load(*a.values())


def test_append_attend_rejects_bad_calls_before_any_launch():
    for missing in ("q", "qs", "k", "ks", "v", "vs", "state", "o", "ws"):
        assert _attend(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _attend(dtype=dt) == _lib.E_BAD_DTYPE
    for p in (0, 3):
        assert _attend(p=p) == _lib.E_BAD_P
    for bad in (dict(T=0), dict(T=-1), dict(H=7), dict(H=8, Hkv=3), dict(H=0), dict(Hkv=0), dict(B=0), dict(D=0), dict(D=257),
                dict(max_len=0), dict(inv_nt=float("nan")), dict(inv_nt=float("inf"))):
        assert _attend(**bad) == _lib.E_BAD_SHAPE, bad
    for odd in (dict(state=A + 8), dict(state=A + 4), dict(ws=A + 8), dict(q=A + 1), dict(k=A + 1), dict(v=A + 1), dict(o=A + 1)):
        assert _attend(**odd) == _lib.E_ALIGNMENT, odd
    assert _attend(dtype=_lib.F32, q=A + 2) == _lib.E_ALIGNMENT and _attend(dtype=_lib.F32, o=A + 2) == _lib.E_ALIGNMENT
    need = _lib.lib().fastmax_hip_kv_decode_workspace(2, 8, 4, 1, 64, 300)
    assert need == 2 * 8 * 3 * 65 * 4 and _attend(wsb=need - 1) == _lib.E_WORKSPACE
    # the order the header gives: a missing pointer before the dtype, the dtype before p, p before the shape
    assert _attend(q=None, dtype=7, p=5, T=0) == _lib.E_NULL and _attend(dtype=7, p=5, T=0) == _lib.E_BAD_DTYPE
    assert _attend(p=5, T=0) == _lib.E_BAD_P and _attend(T=0, state=A + 4) == _lib.E_BAD_SHAPE


def test_load_and_set_len_reject_bad_calls_before_any_launch():
    for missing in ("k", "ks", "v", "vs", "state"):
        assert _load(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _load(dtype=dt) == _lib.E_BAD_DTYPE
    for bad in (dict(T=0), dict(T=-3), dict(T=301), dict(B=0), dict(Hkv=0), dict(D=300), dict(max_len=0)):
        assert _load(**bad) == _lib.E_BAD_SHAPE, bad
    for odd in (dict(state=A + 8), dict(k=A + 1), dict(v=A + 1)):
        assert _load(**odd) == _lib.E_ALIGNMENT, odd
    set_len = _lib.lib().fastmax_hip_kv_decode_set_len
    assert set_len(None, 0, 5, None) == _lib.E_NULL
    for new_len, max_len in ((-1, 5), (6, 5), (0, 0), (0, -2)):
        assert set_len(A, new_len, max_len, None) == _lib.E_BAD_SHAPE, (new_len, max_len)
    assert set_len(A + 4, 0, 5, None) == _lib.E_ALIGNMENT


# ---- 4. the host contract --------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    K = decode.FastmaxKVDecodeState
    with pytest.raises(ValueError, match="p should be 1 or 2"):
        K(1, 2, 64, "cpu", 16, torch.bfloat16, p=3)
    with pytest.raises(ValueError, match="does not divide"):
        K(1, 8, 64, "cpu", 16, torch.bfloat16, n_query_groups=3)
    with pytest.raises(ValueError, match="does not divide"):
        K(1, 8, 64, "cpu", 16, torch.bfloat16, n_query_groups=0)
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        K(1, 2, 64, "cpu", 16, torch.float64)
    for bad in (0, -5, 2.5, 2 ** 31):
        with pytest.raises(ValueError, match="max_len"):
            K(1, 2, 64, "cpu", bad, torch.bfloat16)
    for D in (257, 512, 0):
        with pytest.raises(NotImplementedError, match="not supported"):
            K(1, 2, D, "cpu", 16, torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K(1, 2, 256, "cpu", 16, torch.bfloat16)
    # the state caches keep their refusal above 128
    with pytest.raises(NotImplementedError, match="head size 256"):
        decode.FastmaxDecodeState(1, 2, 256, "cpu", p=2)


class _KV(decode.FastmaxKVDecodeState):
    """a cache where nothing is run: the refusals below look at max_len and p only"""

    def __init__(self, max_len, p=2, B=2):
        self.max_len, self.p, self.B = max_len, p, B


def test_generate_refuses_a_cache_that_is_too_small_up_front():
    from fastmax_experiments_amd import generate
    from fastmax_experiments_amd.block import Block
    blocks = [Block.from_config("pythia-14m")]
    head = generate.NextTokenHead(128, 40)
    wte, prompt = torch.zeros(40, 128), torch.zeros(2, 3, dtype=torch.int64)
    kw = dict(cos=torch.zeros(16, 8), sin=torch.zeros(16, 8))
    with pytest.raises(ValueError, match="holds at most 7"):
        generate.generate(wte, blocks, head, [_KV(7)], prompt, 9, **kw)                # 8 tokens are fed
    with pytest.raises(ValueError, match="holds at most 7"):
        generate.GraphedDecoder(wte, blocks, head, [_KV(7)], max_len=9, **kw)
    with pytest.raises(ValueError, match="max_len > 3"):
        generate.GraphedDecoder(wte, blocks, head, [_KV(3)], max_len=4, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):                             # enough room: the next refusal is the device's
        generate.GraphedDecoder(wte, blocks, head, [_KV(8)], max_len=9, **kw)


def test_the_block_takes_the_cache_for_fastmax_at_p2_only():
    from fastmax_experiments_amd.attention_block import CausalSelfAttention
    x, cos, sin = torch.zeros(2, 1, 64), torch.zeros(1, 8), torch.zeros(1, 8)
    fast = CausalSelfAttention(n_embd=64, n_head=2, n_query_groups=1, head_size=32, attn_alg="fastmax", r=0)
    with pytest.raises(ValueError, match="p=1"):
        fast.attend_cached(x, cos, sin, _KV(8, p=1))
    lin = CausalSelfAttention(n_embd=64, n_head=2, n_query_groups=1, head_size=32, attn_alg="linearmax", r=0)
    with pytest.raises(TypeError, match="LinearmaxDecodeState"):
        lin.attend_cached(x, cos, sin, _KV(8))
