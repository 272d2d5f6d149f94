"""CPU-side checks of generation through the attention block (include/fastmax_hip_generate.h, csrc/fastmax_decode_qkv.hip,
decode.py step_qkv / extend_qkv, attention_block.py forward(..., state=...)): the entry points are bound and exported (their rows
against the header's prototypes: test_binding_cpu.py), `_supported` follows the documented conditions, every
rejected argument comes back as its error code before anything is launched (host pointers stand in for device buffers: a
rejected call never touches them), and the block's host-side contract."""
import ctypes
import inspect

import pytest
import torch

E_BAD_SHAPE, E_BAD_DTYPE, E_NULL = -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from fastmax_experiments_amd import _lib, build
    build.build()
    return _lib.lib()


def test_generate_entry_points_are_bound_and_exported(lib):
    from fastmax_experiments_amd import _lib
    for name in ("fastmax_hip_p2_decode_step_qkv_supported", "fastmax_hip_p2_decode_step_qkv"):
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib.ABI[name][0], _lib.ABI[name][1]), name
    assert lib.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("G,qpk,D,rope", [(4, 8, 64, 64), (32, 1, 128, 128), (1, 8, 128, 128), (4, 1, 32, 8)])
def test_supported_shapes(lib, G, qpk, D, rope, dt):
    assert lib.fastmax_hip_p2_decode_step_qkv_supported(G, qpk, D, rope, dt) == 1


def test_unsupported_shapes(lib):
    f = lib.fastmax_hip_p2_decode_step_qkv_supported
    assert f(4, 8, 64, 64, 1) == 1
    for G, qpk, D, rope, dt in ((4, 8, 136, 64, 1), (4, 8, 64, 63, 1), (4, 8, 64, 7, 0), (4, 8, 64, 66, 1), (4, 257, 64, 64, 1),
                                (4, 8, 64, 64, 3), (4, 8, 64, 64, -1), (0, 8, 64, 64, 1), (4, 0, 64, 64, 1), (4, 8, 0, 0, 1),
                                (4, 8, 64, -2, 1)):
        assert f(G, qpk, D, rope, dt) == 0, (G, qpk, D, rope, dt)
    assert f(4, 256, 64, 64, 1) == 1 and f(4, 8, 128, 0, 2) == 1


def test_step_qkv_rejects_bad_arguments_before_any_launch(lib):
    keep = [ctypes.create_string_buffer(4096) for _ in range(5)]
    qkv, cos, sin, state, o = (ctypes.cast(b, ctypes.c_void_p) for b in keep)
    step = lib.fastmax_hip_p2_decode_step_qkv

    def call(qkv=qkv, cos=cos, sin=sin, state=state, o=o, B=1, G=2, qpk=2, D=64, rope=64, t16=0, dt=1, odt=1):
        return step(qkv, cos, sin, state, o, B, G, qpk, D, rope, t16, dt, odt, 0.125, None)

    for kw in (dict(qkv=None), dict(cos=None), dict(sin=None), dict(state=None), dict(o=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(dt=3), dict(dt=-1), dict(odt=7), dict(odt=-1)):
        assert call(**kw) == E_BAD_DTYPE, kw
    for kw in (dict(D=136), dict(D=129), dict(D=0), dict(rope=63), dict(rope=66), dict(rope=-2), dict(qpk=257), dict(qpk=0),
               dict(G=0), dict(B=0), dict(B=-1), dict(B=65536, G=1), dict(B=256, G=256)):
        assert call(**kw) == E_BAD_SHAPE, kw


def test_forward_takes_a_state_and_linearmax_refuses_it():
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    sig = inspect.signature(CausalSelfAttention.forward)
    assert list(sig.parameters) == ["self", "x", "cos", "sin", "input_pos", "state"]
    assert sig.parameters["state"].default is None and sig.parameters["input_pos"].default is None
    assert callable(getattr(CausalSelfAttention, "attend_cached"))
    blk = CausalSelfAttention(n_embd=64, n_head=4, n_query_groups=2, head_size=16, attn_alg="linearmax")
    st = FastmaxDecodeState(1, 4, 16, "cpu", p=2, n_query_groups=2)
    cos, sin = build_rope_cache(4, 16)
    with pytest.raises(NotImplementedError, match="whole sequence"):
        blk(torch.zeros(1, 1, 64), cos[:1], sin[:1], torch.tensor([0]), st)
    with pytest.raises(NotImplementedError, match="whole sequence"):
        blk.attend_cached(torch.zeros(1, 3, 64), cos[:3], sin[:3], st)


def test_state_host_side_contract():
    """reset keeps the allocation; the qkv entry points refuse a first-order state and malformed operands on the host"""
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    st = FastmaxDecodeState(1, 4, 16, "cpu", p=2, n_query_groups=2)
    assert st.prefill_chunk is None and isinstance(st.fused_step, bool)
    ptr = st.state.data_ptr()
    st.state.fill_(1.0)
    st.count = 7
    st.reset()
    assert st.count == 0 and st.state.data_ptr() == ptr and not st.state.any()
    qkv = torch.zeros(1, 1, 2, 4, 16)
    row = torch.zeros(1, 16)
    for bad in (torch.zeros(1, 1, 2, 3, 16), torch.zeros(1, 1, 4, 4, 16), torch.zeros(1, 1, 2, 4, 8), torch.zeros(1, 2, 4, 16)):
        with pytest.raises(ValueError):
            st.step_qkv(bad, row, row, 16)
        with pytest.raises(ValueError):
            st.extend_qkv(bad, row, row, 16)
    with pytest.raises(ValueError):
        st.step_qkv(torch.zeros(1, 2, 2, 4, 16), torch.zeros(2, 16), torch.zeros(2, 16), 16)      # two tokens
    with pytest.raises(ValueError):
        st.step_qkv(qkv, torch.zeros(2, 16), row, 16)                                             # rows of two positions
    with pytest.raises(ValueError):
        st.extend_qkv(qkv, torch.zeros(1, 8), torch.zeros(1, 8), 16)                              # rows shorter than rope_n_elem
    p1 = FastmaxDecodeState(1, 4, 16, "cpu", p=1)
    for f in (p1.step_qkv, p1.extend_qkv):
        with pytest.raises(NotImplementedError):
            f(torch.zeros(1, 1, 4, 3, 16), row, row, 16)


def test_any_bounded_cache_is_refused_up_front_by_its_own_max_len():
    """the generation loops ask the cache how much it holds; they do not decide by its class.  Nothing runs on a device."""
    from fastmax_experiments_amd import decode, generate
    from fastmax_experiments_amd.block import Block

    class Ring(decode._DecodeState):
        """a cache kind of the test's own: nothing but a capacity"""
        max_len = 5

        def __init__(self, B):
            self.B = B

    assert not issubclass(Ring, decode.FastmaxKVDecodeState) and decode._DecodeState.max_len is None
    blocks = [Block.from_config("pythia-14m")]
    head = generate.NextTokenHead(128, 40)
    wte, prompt = torch.zeros(40, 128), torch.zeros(2, 3, dtype=torch.int64)
    kw = dict(cos=torch.zeros(16, 8), sin=torch.zeros(16, 8))
    with pytest.raises(ValueError, match="holds at most 5"):
        generate.generate(wte, blocks, head, [Ring(2)], prompt, 7, **kw)                # 6 tokens are fed
    with pytest.raises(ValueError, match="holds at most 5"):
        generate.GraphedDecoder(wte, blocks, head, [Ring(2)], max_len=7, **kw)


@pytest.mark.parametrize("dtype,table_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                               (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("B,T,G,qpk,hs,rope_n", [(2, 5, 2, 3, 16, 16), (1, 3, 1, 4, 16, 4), (2, 1, 4, 1, 8, 8)])
def test_shared_eager_split_is_the_forward_fallback_bit_for_bit(B, T, G, qpk, hs, rope_n, dtype, table_dtype):
    """forward's eager fallback used to slice, repeat K and V per query head, then rotate; it now takes the eager split the
    decode state caches use (K, V at their G heads) and repeats afterwards.  RoPE acts on each row alone: identical bits."""
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.attention_block import apply_rope, build_rope_cache
    gen = torch.Generator().manual_seed(B * 1000 + T * 100 + G * 10 + qpk)
    qkv = torch.randn(B, T, G * (qpk + 2) * hs, generator=gen).to(dtype)
    cos, sin = (t.to(table_dtype) for t in build_rope_cache(T, rope_n))
    n_head, n_query_groups, q_per_kv, total_qkv, head_size = G * qpk, G, qpk, qpk + 2, hs

    # the earlier inline expression of CausalSelfAttention.forward, verbatim but for `self.`
    qkv5 = qkv.view(B, T, n_query_groups, total_qkv, head_size)
    q = qkv5[:, :, :, :q_per_kv].permute(0, 2, 3, 1, 4).reshape(B, n_head, T, head_size)
    k, v = (qkv5[:, :, :, q_per_kv + i].permute(0, 2, 1, 3).repeat_interleave(q_per_kv, dim=1) for i in (0, 1))
    n = rope_n
    q = torch.cat((apply_rope(q[..., :n], cos, sin), q[..., n:]), dim=-1)
    k = torch.cat((apply_rope(k[..., :n], cos, sin), k[..., n:]), dim=-1)

    q2, k2, v2 = ops.eager_rope_qkv_split(qkv5, cos, sin, rope_n)
    k2, v2 = (t.repeat_interleave(qpk, dim=1) for t in (k2, v2))
    for got, want in ((q2, q), (k2, k), (v2, v)):
        assert got.dtype == want.dtype == dtype and got.shape == want.shape
        assert torch.equal(got, want)
    # on the CPU the decode state caches' split is this eager one
    for got, want in zip(ops.rope_qkv_split(qkv5, cos, sin, rope_n), ops.eager_rope_qkv_split(qkv5, cos, sin, rope_n)):
        assert torch.equal(got, want)
