"""First-order linearmax decode state cache (decode.LinearmaxDecodeState, csrc/linearmax_decode.hip) on an MI355X against
L(q, k, v) = masked first-order linearmax over the whole sequence (oracle.fastmax_oracle.linearmax_fwd, float64, on the
up-cast inputs; K and V expanded from their KV heads as the model expands them).

In every case one k row is multiplied by 3 and one later q row by 4 at positions after the prompt, so both running maxima
change during generation: an implementation that freezes the statistics at prefill fails.

Tolerances and the row-error measure are those of test_decode_p2_gpu.py: fp32 2e-4, bf16 8e-3, f16 2e-3, each row against
that row's own magnitude."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import fastmax_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-4, torch.bfloat16: 8e-3, torch.float16: 2e-3}
# (B, H, G, D): grouped heads with D < 64 (DP padding); D = 64; D = 128; D not a multiple of 16 (DP = 128); D = 24
SHAPES = [((2, 4, 2, 16), torch.float32), ((1, 4, 4, 64), torch.bfloat16), ((1, 2, 1, 128), torch.bfloat16),
          ((1, 4, 2, 72), torch.float16), ((1, 2, 2, 24), torch.float32)]
SHAPE_IDS = ["B2H4G2D16-f32", "B1H4G4D64-bf16", "B1H2G1D128-bf16", "B1H4G2D72-f16", "B1H2G2D24-f32"]
PROMPTS = [1, 5, 70]
STEPS = 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _state(B, H, D, G):
    from fastmax_experiments_amd.decode import LinearmaxDecodeState
    return LinearmaxDecodeState(B, H, D, "cuda", n_query_groups=G)


def _row_err(got, ref):
    """worst over the rows (last axis = D) of max|got - ref| / max|ref| of that row"""
    got = np.asarray(got, np.float64).reshape(-1, ref.shape[-1])
    ref = np.asarray(ref, np.float64).reshape(-1, ref.shape[-1])
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-6)).max())


def _np(t):
    return t.float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(shape, dt, P, S, ik, iq):
    """P prompt tokens + S later ones in dtype dt on the device; k row P + ik times 3, q row P + iq times 4 (before the cast)"""
    B, H, G, D = shape
    g = torch.Generator().manual_seed(1000 * D + 10 * P + S)
    q = torch.randn(B, H, P + S, D, generator=g)
    k, v = (torch.randn(B, G, P + S, D, generator=g) for _ in range(2))
    k[:, :, P + ik] *= 3.0
    q[:, :, P + iq] *= 4.0
    return tuple(t.to(dt).cuda() for t in (q, k, v))


@functools.lru_cache(maxsize=None)
def _L(shape, dt, P, S, ik, iq, n):
    """L over the first n tokens of _inputs(...), float64 on the up-cast inputs; computed once, read-only"""
    q, k, v = (t[:, :, :n].double().cpu().numpy() for t in _inputs(shape, dt, P, S, ik, iq))
    r = shape[1] // shape[2]
    ref = orc.linearmax_fwd(q, np.repeat(k, r, axis=1), np.repeat(v, r, axis=1), p=1, mask=True)
    ref.setflags(write=False)
    return ref


def _tok(tensors, a, b):
    return tuple(t[:, :, a:b] for t in tensors)


# ---- 1. prefill and steps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PROMPTS)
@pytest.mark.parametrize("shape,dt", SHAPES, ids=SHAPE_IDS)
def test_prefill_and_steps_match_L_over_each_prefix(shape, dt, P):
    B, H, G, D = shape
    key = (shape, dt, P, STEPS, 1, 3)
    qkv = _inputs(*key)
    st = _state(B, H, D, G)
    o = st.prefill(*_tok(qkv, 0, P))
    assert o.shape == (B, H, P, D) and o.dtype == dt and st.count == P
    err = rel_err(_np(o), _L(*key, P))
    print(f"linearmax decode {shape} {dt} prompt {P}: prefill {err:.3e} (bound {TOL[dt]:.0e})")
    assert err < TOL[dt]
    for t in range(P, P + STEPS):
        o = st.step(*_tok(qkv, t, t + 1))
        assert o.shape == (B, H, 1, D) and o.dtype == dt and st.count == t + 1
        err = _row_err(_np(o), _L(*key, t + 1)[:, :, t:])
        print(f"  step at {t}: worst row {err:.3e}")
        assert err < TOL[dt], t


# ---- 2. extend ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PROMPTS)
@pytest.mark.parametrize("shape,dt", SHAPES, ids=SHAPE_IDS)
def test_extend_matches_rows_of_L_over_the_whole_sequence(shape, dt, P):
    B, H, G, D = shape
    for T in (1, 3, 33):
        key = (shape, dt, P, T, T // 3, (2 * T) // 3)          # T = 3: rows P + 1, P + 2; T = 33: P + 11, P + 22; T = 1: both P
        qkv = _inputs(*key)
        st = _state(B, H, D, G)
        st.prefill(*_tok(qkv, 0, P))
        before = st.state.clone()
        o = st.extend(*_tok(qkv, P, P + T))
        assert o.shape == (B, H, T, D) and o.dtype == dt and st.count == P + T
        err = _row_err(_np(o), _L(*key, P + T)[:, :, P:])
        print(f"linearmax extend {shape} {dt} prompt {P} T={T}: worst row {err:.3e} (bound {TOL[dt]:.0e})")
        assert err < TOL[dt], T
        if T == 1:
            # extend(T = 1) is step, bit for bit, in the output and in the state
            other = _state(B, H, D, G)
            other.state.copy_(before)
            other.count = P
            o_s = other.step(*_tok(qkv, P, P + 1))
            assert torch.equal(o, o_s) and torch.equal(st.state, other.state) and other.count == P + 1


@pytest.mark.parametrize("P", PROMPTS)
@pytest.mark.parametrize("shape,dt", SHAPES, ids=SHAPE_IDS)
def test_extend_on_an_empty_state_agrees_with_prefill(shape, dt, P):
    B, H, G, D = shape
    key = (shape, dt, P, STEPS, 1, 3)
    qkv = _inputs(*key)
    a, b = _state(B, H, D, G), _state(B, H, D, G)
    o_a = a.prefill(*_tok(qkv, 0, P))
    o_b = b.extend(*_tok(qkv, 0, P))
    assert a.count == b.count == P and o_b.shape == (B, H, P, D) and o_b.dtype == dt
    ref = _L(*key, P)
    assert rel_err(_np(o_a), ref) < TOL[dt] and _row_err(_np(o_b), ref) < TOL[dt]
    nxt = _L(*key, P + 1)[:, :, P:]
    for st in (a, b):
        assert _row_err(_np(st.step(*_tok(qkv, P, P + 1))), nxt) < TOL[dt]


# ---- 3. the QKV entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,G,qpk,hs,rope_n,dt", [(2, 2, 2, 32, 8, torch.bfloat16), (2, 2, 2, 32, 8, torch.float32),
                                                   (1, 4, 1, 64, 64, torch.bfloat16), (2, 1, 4, 72, 72, torch.float16)])
def test_qkv_entry_points_bit_identical_to_split_then_step_or_extend(B, G, qpk, hs, rope_n, dt):
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.attention_block import build_rope_cache
    P, T, S, H = 9, 4, 3, G * qpk
    N = P + T + S
    gen = torch.Generator().manual_seed(100 * hs + qpk)
    big = torch.randn(B, N, G, qpk + 2, hs, generator=gen)
    big[:, P + 1, :, qpk] *= 3.0
    big[:, P + T + 1, :, :qpk] *= 4.0
    big = big.to(dt).cuda()
    cos, sin = build_rope_cache(N, rope_n, device="cuda")
    a, b = _state(B, H, hs, G), _state(B, H, hs, G)
    views = 0
    for lo, hi in [(0, P), (P, P + T)] + [(t, t + 1) for t in range(P + T, N)]:
        qkv, c, s = big[:, lo:hi], cos[lo:hi], sin[lo:hi]
        assert B == 1 or not qkv.is_contiguous()
        q, k, v = b._split_qkv(qkv, c, s, rope_n)
        assert q.shape == (B, H, hi - lo, hs) and k.shape == (B, G, hi - lo, hs) and v.shape == k.shape
        views += sum(not t.is_contiguous() for t in (q, k, v))
        if hi - lo == 1:
            o_a, o_b = a.step_qkv(qkv, c, s, rope_n), b.step(q, k, v)
        else:
            o_a = a.extend_qkv(qkv, c, s, rope_n)
            o_b = b.prefill(q, k, v) if lo == 0 else b.extend(q, k, v)
        assert o_a.shape == (B, H, hi - lo, hs) and o_a.dtype == dt
        assert torch.equal(o_a, o_b), (lo, hi)
        assert torch.equal(a.state, b.state), (lo, hi)
    assert a.count == b.count == N
    if not ops.rope_qkv_supported(dt, hs, rope_n):
        assert views > 0, "the slicing route's V is a permuted view: the kernel should have been handed one"


def test_strided_views_bit_identical_to_contiguous():
    B, H, G, P, T, D = 2, 4, 2, 20, 5, 64
    g = torch.Generator().manual_seed(7)
    packed = torch.randn(B, P + T + 1, H + 2 * G, D, generator=g).to(torch.bfloat16).cuda()      # (B, N, heads, D) storage
    q, k, v = (packed[:, :, a:b].transpose(1, 2) for a, b in ((0, H), (H, H + G), (H + G, H + 2 * G)))
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    s1, s2 = _state(B, H, D, G), _state(B, H, D, G)
    for lo, hi in ((0, P), (P, P + T), (P + T, P + T + 1)):
        f1, f2 = (s1.extend, s2.extend) if hi - lo > 1 else (s1.step, s2.step)
        o1 = f1(*_tok((q, k, v), lo, hi))
        o2 = f2(*(t.contiguous() for t in _tok((q, k, v), lo, hi)))
        assert torch.equal(o1, o2) and torch.equal(s1.state, s2.state)


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_bitwise_reproducible_and_reset_is_a_fresh_state(shape, dt):
    B, H, G, D = shape
    P = 70
    qkv = _inputs(shape, dt, P, 8, 1, 3)

    def run(st):
        outs = [st.prefill(*_tok(qkv, 0, P))]
        outs += [st.step(*_tok(qkv, t, t + 1)) for t in range(P, P + 4)]
        outs.append(st.extend(*_tok(qkv, P + 4, P + 8)))
        torch.cuda.synchronize()
        return outs, st.state.clone()

    st = _state(B, H, D, G)
    ptr = st.state.data_ptr()
    first = run(st)
    st.reset()
    assert st.count == 0 and st.state.data_ptr() == ptr and not st.state.any()
    second = run(st)
    fresh = run(_state(B, H, D, G))
    for other in (second, fresh):
        assert torch.equal(first[1], other[1])
        for x, y in zip(first[0], other[0]):
            assert torch.equal(x, y)


# ---- 5. the block, token by token ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [2, 4], ids=["grouped", "H=G"])
def test_block_generates_token_by_token(G, dt):
    """attend_cached = the last row of fastmax_hack over the split, rotated prefix; forward = proj of that row laid head by head"""
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    from fastmax_experiments_amd.attention_mechanisms.fastmax_hack import fastmax_hack
    B, H, hs, N, C = 2, 4, 32, 10, 128
    qpk = H // G
    torch.manual_seed(5)
    blk = CausalSelfAttention(n_embd=C, n_head=H, n_query_groups=G, head_size=hs, attn_alg="linearmax").to("cuda", dt).eval()
    x = torch.randn(B, N, C, generator=torch.Generator().manual_seed(6))
    x[:, 4] *= 3.0          # larger q and k rows late in the sequence: both maxima move while generating
    x[:, 7] *= 4.0
    x = x.to(dt).cuda()
    cos, sin = build_rope_cache(N, blk.rope_n_elem, device="cuda")
    s_att, s_fwd = _state(B, H, hs, G), _state(B, H, hs, G)
    qs, ks, vs = [], [], []
    worst_a = worst_f = 0.0
    with torch.no_grad():
        for t in range(N):
            xt, c, s = x[:, t:t + 1], cos[t:t + 1], sin[t:t + 1]
            o = blk.attend_cached(xt, c, s, s_att)
            y = blk(xt, c, s, torch.tensor([t], device="cuda"), s_fwd)
            assert o.shape == (B, H, 1, hs) and o.dtype == dt and y.shape == (B, 1, C) and y.dtype == dt
            assert s_att.count == s_fwd.count == t + 1
            q, k, v = s_att._split_qkv(blk.attn(xt).view(B, 1, G, qpk + 2, hs), c, s, blk.rope_n_elem)
            qs.append(q), ks.append(k.repeat_interleave(qpk, dim=1)), vs.append(v.repeat_interleave(qpk, dim=1))
            row = fastmax_hack(torch.cat(qs, 2), torch.cat(ks, 2), torch.cat(vs, 2), p=1, mask=True)[:, :, t:]
            worst_a = max(worst_a, _row_err(_np(o), _np(row).astype(np.float64)))
            ref_y = blk.proj(row.reshape(B, 1, H * hs))
            worst_f = max(worst_f, _row_err(_np(y), _np(ref_y).astype(np.float64)))
    print(f"linearmax block G={G} {dt}: attend_cached worst row {worst_a:.3e}, forward worst row {worst_f:.3e} (bound {TOL[dt]:.0e})")
    assert worst_a < TOL[dt] and worst_f < TOL[dt]
