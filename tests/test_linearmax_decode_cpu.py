"""CPU-side checks of the first-order linearmax decode state cache (include/fastmax_hip_linearmax_decode.h,
csrc/linearmax_decode.hip, decode.LinearmaxDecodeState, attention_block.attend_cached):

* the entry points are bound and exported (their rows against the header's prototypes: test_binding_cpu.py);
* the state-size query returns the documented record size and 0 for what it refuses;
* the advance call turns every bad argument into its error code on the host (host pointers stand in for device buffers: a
  rejected call never touches them);
* the recurrence the kernel implements -- sums of centred, UNSCALED rows and two running maxima -- written out in float64
  numpy reproduces oracle.fastmax_oracle.linearmax_fwd for prefill, steps and a multi-token extend, with grouped heads and
  inputs whose maxima move after the prompt;
* the block's dispatch errors."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fastmax_oracle as orc

E_BAD_SHAPE, E_BAD_DTYPE, E_ALIGNMENT, E_NULL = -2, -3, -5, -6


@pytest.fixture(scope="module")
def lib():
    from fastmax_experiments_amd import _lib, build
    build.build()
    return _lib.lib()


def test_entry_points_are_bound_and_exported(lib):
    from fastmax_experiments_amd import _lib
    for name in ("fastmax_hip_linearmax_decode_state_bytes", "fastmax_hip_linearmax_decode_advance"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib.ABI[name][0], _lib.ABI[name][1]), name
    assert lib.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9


def _record_bytes(H, G, D):
    """the documented record of one (b, kv head): 8 slab blocks of S2 part, S1 part, own ksum, own padded statistics"""
    dp = 64 if D <= 64 else 128
    w = dp // 8
    return 4 * 8 * (dp * w + w + dp + 4 * ((2 + H // G + 3) // 4))


@pytest.mark.parametrize("D", [16, 64, 72, 128])
@pytest.mark.parametrize("G,qpk", [(2, 1), (2, 4)])
def test_state_bytes_is_the_documented_record(lib, D, G, qpk):
    f = lib.fastmax_hip_linearmax_decode_state_bytes
    H = G * qpk
    for B in (1, 3):
        assert f(B, H, G, D) == B * G * _record_bytes(H, G, D)
    dp = 64 if D <= 64 else 128
    # S2 (DP x DP) and S1 (DP) once, ksum and the statistics once per slab
    assert _record_bytes(H, G, D) == 4 * (dp * dp + dp + 8 * (dp + 4 * ((2 + qpk + 3) // 4)))


def test_state_bytes_refuses_unsupported_shapes(lib):
    f = lib.fastmax_hip_linearmax_decode_state_bytes
    assert f(1, 4, 2, 128) > 0 and f(1, 64, 1, 64) > 0
    for B, H, G, D in ((1, 4, 2, 129), (1, 5, 2, 64), (1, 4, 3, 64), (0, 4, 2, 64), (-1, 4, 2, 64), (1, 0, 2, 64), (1, 4, 0, 64),
                       (1, 4, -2, 64), (1, 4, 2, 0), (1, 4, 2, -8), (1, 65, 1, 64)):
        assert f(B, H, G, D) == 0, (B, H, G, D)


def test_advance_rejects_bad_arguments_before_any_launch(lib):
    keep = [ctypes.create_string_buffer(1 << 16) for _ in range(5)]
    q, k, v, state, o = (ctypes.c_void_p((ctypes.addressof(b) + 15) & ~15) for b in keep)
    strides = (ctypes.c_int64 * 3)(64 * 4, 64, 64)
    adv = lib.fastmax_hip_linearmax_decode_advance

    def call(q=q, qs=strides, k=k, ks=strides, v=v, vs=strides, state=state, o=o, B=1, H=4, G=2, T=1, D=64, dt=1):
        return adv(q, qs, k, ks, v, vs, state, o, B, H, G, T, D, dt, None)

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(state=None), dict(qs=None), dict(ks=None), dict(vs=None),
               dict(q=None, o=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(dt=3), dict(dt=-1), dict(dt=3, T=0)):
        assert call(**kw) == E_BAD_DTYPE, kw
    for kw in (dict(T=0), dict(T=-3), dict(H=5), dict(H=3, G=2), dict(G=3), dict(G=0), dict(H=0), dict(B=0), dict(B=-1), dict(D=0),
               dict(D=129), dict(H=130, G=2), dict(B=1 << 20, H=1 << 10, G=1 << 10)):
        assert call(**kw) == E_BAD_SHAPE, kw
    assert call(state=ctypes.c_void_p(state.value + 4)) == E_ALIGNMENT


# ---- the recurrence in float64 ---------------------------------------------------------------------------------------
class _Recurrence:
    """the state of "Semantics": per KV head S2 = sum kc v^T, S1 = sum v, ksum = sum kc, the count and Mk; per query head Mq.
    Sums of centred UNSCALED rows; a = 1 / (Mq Mk) only at read-out."""

    def __init__(self, B, H, G, D):
        self.r = H // G
        self.S2, self.S1, self.ks = np.zeros((B, G, D, D)), np.zeros((B, G, D)), np.zeros((B, G, D))
        self.count, self.Mk, self.Mq = 0, np.zeros((B, G)), np.zeros((B, H))

    def extend(self, q, k, v):
        B, H, T, D = q.shape
        G, r = k.shape[1], self.r
        qc, kc = q - q.mean(-1, keepdims=True), k - k.mean(-1, keepdims=True)
        # both maxima over the whole chunk before any row is read out
        self.Mq = np.maximum(self.Mq, np.sqrt((qc * qc).sum(-1)).max(-1))
        self.Mk = np.maximum(self.Mk, np.sqrt((kc * kc).sum(-1)).max(-1))
        a = 1.0 / (self.Mq.reshape(B, G, r) * self.Mk[:, :, None])
        o = np.empty((B, G, r, T, D))
        for t in range(T):
            self.S2 += kc[:, :, t, :, None] * v[:, :, t, None, :]
            self.S1 += v[:, :, t]
            self.ks += kc[:, :, t]
            self.count += 1
            qt = qc[:, :, t].reshape(B, G, r, D)
            num = self.S1[:, :, None] + a[..., None] * np.einsum("bgrm,bgmd->bgrd", qt, self.S2)
            den = self.count + a * np.einsum("bgrm,bgm->bgr", qt, self.ks)
            o[:, :, :, t] = num / den[..., None]
        return o.reshape(B, H, T, D)


def _moving_maxima_case(B, H, G, D, P, S, seed):
    """P prompt tokens + S later ones; after the prompt one k row is multiplied by 3 and a later q row by 4, so both running
    maxima change during generation"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, H, P + S, D))
    k, v = rng.standard_normal((B, G, P + S, D)), rng.standard_normal((B, G, P + S, D))
    k[:, :, P + 1] *= 3.0
    q[:, :, P + 3] *= 4.0
    return q, k, v


def _L(q, k, v):
    r = q.shape[1] // k.shape[1]
    return orc.linearmax_fwd(q, np.repeat(k, r, axis=1), np.repeat(v, r, axis=1), p=1, mask=True)


@pytest.mark.parametrize("B,H,G,D,P", [(2, 4, 2, 16, 5), (1, 6, 2, 24, 1), (1, 2, 2, 72, 70)])
def test_float64_recurrence_reproduces_the_oracle(B, H, G, D, P):
    S = 12
    q, k, v = _moving_maxima_case(B, H, G, D, P, S, seed=D + P)
    st = _Recurrence(B, H, G, D)
    # prefill = extend on an empty state: L over the prompt
    o = st.extend(q[:, :, :P], k[:, :, :P], v[:, :, :P])
    assert np.abs(o - _L(q[:, :, :P], k[:, :, :P], v[:, :, :P])).max() < 1e-12
    # six steps: each the last row of L over its prefix (the maxima move at P + 1 and P + 3)
    mk0, mq0 = st.Mk.copy(), st.Mq.copy()
    for t in range(P, P + 6):
        o = st.extend(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1])
        ref = _L(q[:, :, :t + 1], k[:, :, :t + 1], v[:, :, :t + 1])[:, :, t:]
        assert np.abs(o - ref).max() < 1e-12, t
    assert (st.Mk > mk0).all() and (st.Mq > mq0).all()
    # a multi-token extend: rows of L over the WHOLE sequence, which T single steps would not give
    o = st.extend(q[:, :, P + 6:], k[:, :, P + 6:], v[:, :, P + 6:])
    assert np.abs(o - _L(q, k, v)[:, :, P + 6:]).max() < 1e-12
    assert st.count == P + S


def test_extend_is_not_a_sequence_of_steps():
    """the chunk's statistics reach its earlier rows: with a large k row late in the chunk, stepping gives other rows"""
    B, H, G, D, P = 1, 2, 1, 16, 4
    q, k, v = _moving_maxima_case(B, H, G, D, P, 6, seed=3)
    a, b = _Recurrence(B, H, G, D), _Recurrence(B, H, G, D)
    for st in (a, b):
        st.extend(q[:, :, :P], k[:, :, :P], v[:, :, :P])
    whole = a.extend(q[:, :, P:], k[:, :, P:], v[:, :, P:])
    steps = np.concatenate([b.extend(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1]) for t in range(P, P + 6)], axis=2)
    assert np.abs(whole[:, :, -1] - steps[:, :, -1]).max() < 1e-12          # the last row has seen everything either way
    assert np.abs(whole[:, :, 0] - steps[:, :, 0]).max() > 1e-3


# ---- host-side contract of the class and the block --------------------------------------------------------------------
def test_state_host_side_contract(lib):
    from fastmax_experiments_amd.decode import LinearmaxDecodeState
    st = LinearmaxDecodeState(2, 4, 16, "cpu", n_query_groups=2)
    assert st.count == 0 and st.state.dtype == torch.float32
    assert st.state.numel() * 4 == lib.fastmax_hip_linearmax_decode_state_bytes(2, 4, 2, 16) and not st.state.any()
    ptr = st.state.data_ptr()
    st.state.fill_(1.0)
    st.count = 7
    st.reset()
    assert st.count == 0 and st.state.data_ptr() == ptr and not st.state.any()
    for name in ("prefill", "step", "extend", "step_qkv", "extend_qkv", "reset"):
        assert callable(getattr(st, name)), name
    assert LinearmaxDecodeState(1, 4, 16, "cpu").Hkv == 4
    with pytest.raises(ValueError):
        LinearmaxDecodeState(1, 4, 16, "cpu", n_query_groups=3)
    with pytest.raises(NotImplementedError):
        LinearmaxDecodeState(1, 4, 129, "cpu")
    z = torch.zeros
    with pytest.raises(ValueError):
        st.step(z(2, 4, 2, 16), z(2, 2, 2, 16), z(2, 2, 2, 16))                 # two tokens
    with pytest.raises(ValueError):
        st.step(z(2, 4, 1, 16), z(2, 4, 1, 16), z(2, 4, 1, 16))                 # K, V not at their G heads
    with pytest.raises(ValueError):
        st.extend(z(2, 4, 0, 16), z(2, 2, 0, 16), z(2, 2, 0, 16))               # T = 0
    with pytest.raises(ValueError):
        st.extend(z(2, 4, 3, 16), z(2, 2, 3, 16), z(2, 2, 2, 16))
    row = z(1, 16)
    for bad in (z(2, 1, 2, 3, 16), z(2, 1, 4, 4, 16), z(2, 1, 2, 4, 8), z(2, 2, 4, 16)):
        with pytest.raises(ValueError):
            st.step_qkv(bad, row, row, 16)
        with pytest.raises(ValueError):
            st.extend_qkv(bad, row, row, 16)
    with pytest.raises(ValueError):
        st.step_qkv(z(2, 2, 2, 4, 16), z(2, 16), z(2, 16), 16)                  # two tokens
    with pytest.raises(ValueError):
        st.extend_qkv(z(2, 1, 2, 4, 16), z(1, 8), z(1, 8), 16)                  # rope rows shorter than rope_n_elem
    assert st.count == 0 and not st.state.any()


def test_fastmax_state_keeps_refusing_first_order_extend():
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    p1 = FastmaxDecodeState(1, 4, 16, "cpu", p=1)
    with pytest.raises(NotImplementedError, match="LinearmaxDecodeState"):
        p1.extend(torch.zeros(1, 4, 2, 16), torch.zeros(1, 4, 2, 16), torch.zeros(1, 4, 2, 16))


def test_block_dispatch_errors():
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    kw = dict(n_embd=64, n_head=4, n_query_groups=2, head_size=16)
    lin, fm = CausalSelfAttention(attn_alg="linearmax", **kw), CausalSelfAttention(attn_alg="fastmax", **kw)
    cos, sin = build_rope_cache(4, 16)
    x1, x3 = torch.zeros(1, 1, 64), torch.zeros(1, 3, 64)
    p2 = FastmaxDecodeState(1, 4, 16, "cpu", p=2, n_query_groups=2)
    lm = LinearmaxDecodeState(1, 4, 16, "cpu", n_query_groups=2)
    # a linearmax block on a fastmax state: still NotImplementedError, still "whole sequence", and it names the class to use
    for call in (lambda: lin(x1, cos[:1], sin[:1], torch.tensor([0]), p2), lambda: lin.attend_cached(x3, cos[:3], sin[:3], p2)):
        with pytest.raises(NotImplementedError, match="whole sequence") as e:
            call()
        assert "LinearmaxDecodeState" in str(e.value)
    # a fastmax block on a linearmax state
    for call in (lambda: fm(x1, cos[:1], sin[:1], torch.tensor([0]), lm), lambda: fm.attend_cached(x3, cos[:3], sin[:3], lm)):
        with pytest.raises(TypeError, match="FastmaxDecodeState"):
            call()
    with pytest.raises(TypeError, match="LinearmaxDecodeState"):
        lin.attend_cached(x1, cos[:1], sin[:1], object())
    assert p2.count == 0 and lm.count == 0 and not lm.state.any()
