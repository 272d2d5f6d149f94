"""Generation through the attention block on the second-order decode state cache, on an MI355X
(attention_block.py forward(..., state=...) / attend_cached, decode.py step_qkv / extend_qkv, csrc/fastmax_decode_qkv.hip).

1. the step taken straight from the QKV projection's output is BIT-identical, in every output and in the state, to the split +
   RoPE pass (K, V at their G heads) followed by `step`;
2. `attend_cached` over a prompt, a 5-token call and single tokens against masked p=2 fastmax over all 48 positions (C oracle,
   float64), fed the block's own QKV projection de-interleaved and rotated in float64;
3. `forward(..., state=...)` at T = 1 against the output projection of the oracle's heads laid side by side; `reset()` and the
   same sequence again reproduce every output bitwise;
4. without a state, `input_pos` still takes the documented slicing path.

Tolerances are those of test_decode_p2_gpu.py, each row against that row's own magnitude: fp32 2e-4, bf16 8e-3, f16 2e-3."""
import numpy as np
import pytest
import torch

from oracle import c_oracle

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-4, torch.bfloat16: 8e-3, torch.float16: 2e-3}
CALLS = [(0, 37), (37, 42)] + [(t, t + 1) for t in range(42, 48)]      # the prompt, one call of 5 tokens, 6 single tokens
N = 48


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _state(B, H, D, G):
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    return FastmaxDecodeState(B, H, D, "cuda", p=2, n_query_groups=G)


def _row_err(got, ref):
    """worst over the rows (last axis) of max|got - ref| / max|ref| of that row"""
    got = np.asarray(got, np.float64).reshape(-1, ref.shape[-1])
    ref = np.asarray(ref, np.float64).reshape(-1, ref.shape[-1])
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-6)).max())


def _slice_split(qkv, cos, sin, n):
    """the tensor-op de-interleave + RoPE of model.py:397-425 with K and V left at their G heads"""
    from fastmax_experiments_amd.attention_block import apply_rope
    B, T, G, total, hs = qkv.shape
    qpk = total - 2
    q = qkv[:, :, :, :qpk].permute(0, 2, 3, 1, 4).reshape(B, G * qpk, T, hs)
    k, v = (qkv[:, :, :, qpk + i].permute(0, 2, 1, 3) for i in (0, 1))
    q = torch.cat((apply_rope(q[..., :n], cos, sin), q[..., n:]), dim=-1)
    k = torch.cat((apply_rope(k[..., :n], cos, sin), k[..., n:]), dim=-1)
    return q, k, v


# ---- 1. bit identity at the state level -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,tables16", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True),
                                         (torch.float16, False), (torch.float16, True)])
@pytest.mark.parametrize("B,G,qpk,hs,rope_n", [(2, 4, 8, 64, 64), (1, 2, 1, 128, 128), (2, 1, 8, 64, 64), (1, 4, 1, 32, 8),
                                               (1, 2, 3, 40, 16)])
def test_step_qkv_bit_identical_to_split_then_step(B, G, qpk, hs, rope_n, dt, tables16):
    from fastmax_experiments_amd import _lib, ops
    from fastmax_experiments_amd.attention_block import build_rope_cache
    T0, S, H = 40, 4, G * qpk
    gen = torch.Generator().manual_seed(1000 * hs + 10 * qpk + G)
    qkv = torch.randn(B, T0 + S, G, qpk + 2, hs, generator=gen).to(dt).cuda()
    cos, sin = build_rope_cache(T0 + S, rope_n, device="cuda")
    if tables16:
        cos, sin = cos.to(dt), sin.to(dt)          # a rope cache kept in the tensors' own dtype: products rounded to it
    assert _lib.lib().fastmax_hip_p2_decode_step_qkv_supported(G, qpk, hs, rope_n, ops._DT[dt]) == 1
    fused, split, unfused = (_state(B, H, hs, G) for _ in range(3))
    assert fused.fused_step in (True, False)
    fused.fused_step, unfused.fused_step = True, False
    for st in (fused, split, unfused):
        st.extend_qkv(qkv[:, :T0], cos[:T0], sin[:T0], rope_n)
    assert torch.equal(fused.state, split.state) and fused.count == T0
    for t in range(T0, T0 + S):
        tok, c, s = qkv[:, t:t + 1], cos[t:t + 1], sin[t:t + 1]
        o_f = fused.step_qkv(tok, c, s, rope_n)
        if ops.rope_qkv_supported(dt, hs, rope_n):
            q, k, v = ops.RopeQKVSplit.apply(tok, c, s, rope_n, 0)
        else:
            q, k, v = _slice_split(tok, c, s, rope_n)      # the split kernel wants whole 16-byte pieces
        assert k.shape == (B, G, 1, hs) and v.shape == (B, G, 1, hs)
        o_s = split.step(q, k, v)
        o_u = unfused.step_qkv(tok, c, s, rope_n)
        assert o_f.shape == (B, H, 1, hs) and o_f.dtype == dt
        assert torch.equal(o_f, o_s), f"token {t}: fused step differs from split + step"
        assert torch.equal(o_u, o_s), f"token {t}: two-launch step_qkv differs from split + step"
        assert torch.equal(fused.state, split.state), f"token {t}: states differ"
        assert torch.equal(unfused.state, split.state)
    assert fused.count == split.count == unfused.count == T0 + S


# ---- 2., 3. the block against float64 ------------------------------------------------------------------------------------
def _rope64(x, cos, sin):
    half = x.shape[-1] // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * sin


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def case(request):
    """the block, 48 tokens, and the float64 reference over all 48 positions, computed once per dtype and left unchanged.  The
    reference is fed the block's own QKV projection, one `attn` call per call of CALLS (the calls the block itself makes)."""
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    dt = request.param
    torch.manual_seed(5)
    blk = CausalSelfAttention(n_embd=256, n_head=8, n_query_groups=2, head_size=32).to("cuda", dt).eval()
    B, H, G, hs, qpk = 2, 8, 2, 32, 4
    x = torch.randn(B, N, 256, generator=torch.Generator().manual_seed(6)).to(dt).cuda()
    cos, sin = build_rope_cache(N, blk.rope_n_elem, device="cuda")
    with torch.no_grad():
        qkv = torch.cat([blk.attn(x[:, a:b]) for a, b in CALLS], dim=1)
    qkv = qkv.double().cpu().view(B, N, G, qpk + 2, hs)
    c64, s64 = cos.double().cpu(), sin.double().cpu()
    q = _rope64(qkv[:, :, :, :qpk].permute(0, 2, 3, 1, 4).reshape(B, H, N, hs), c64, s64)
    k = _rope64(qkv[:, :, :, qpk].permute(0, 2, 1, 3), c64, s64).repeat_interleave(qpk, dim=1)
    v = qkv[:, :, :, qpk + 1].permute(0, 2, 1, 3).repeat_interleave(qpk, dim=1)
    ref, _ = c_oracle.fwd(q.numpy(), k.numpy(), v.numpy(), mask=True, p=2)
    ref.setflags(write=False)
    return dict(dt=dt, blk=blk, x=x, cos=cos, sin=sin, ref=ref, dims=(B, H, G, hs))


def test_attend_cached_matches_float64(case):
    blk, x, cos, sin, ref, dt = (case[n] for n in ("blk", "x", "cos", "sin", "ref", "dt"))
    B, H, G, hs = case["dims"]
    st = _state(B, H, hs, G)
    with torch.no_grad():
        outs = [blk.attend_cached(x[:, a:b], cos[a:b], sin[a:b], st) for a, b in CALLS]
    for (a, b), o in zip(CALLS, outs):
        assert o.shape == (B, H, b - a, hs) and o.dtype == dt
    assert st.count == N
    got = torch.cat(outs, dim=2).float().cpu().numpy()
    for name, sl in (("prompt", slice(0, 37)), ("5-token call", slice(37, 42)), ("single tokens", slice(42, 48))):
        print(f"attend_cached {dt} {name}: worst row {_row_err(got[:, :, sl], ref[:, :, sl]):.3e} (bound {TOL[dt]:.0e})")
    assert _row_err(got, ref) < TOL[dt]


def test_forward_single_tokens_match_projected_oracle_and_reset_reproduces(case):
    blk, x, cos, sin, ref, dt = (case[n] for n in ("blk", "x", "cos", "sin", "ref", "dt"))
    B, H, G, hs = case["dims"]
    st = _state(B, H, hs, G)

    def run():
        with torch.no_grad():
            return [blk(x[:, a:b], cos[a:b], sin[a:b], torch.arange(a, b, device="cuda"), st) for a, b in CALLS]

    outs = run()
    assert st.count == N
    w = blk.proj.linear.weight.detach().double().cpu().numpy()                      # (n_embd, n_head * hs); no bias, no LoRA on proj
    worst = 0.0
    for (a, b), y in zip(CALLS, outs):
        assert y.shape == (B, b - a, 256) and y.dtype == dt
        if b - a == 1:
            heads = ref[:, :, a, :].reshape(B, 1, H * hs)                  # T = 1: the reshape lays the heads side by side
            worst = max(worst, _row_err(y.float().cpu().numpy(), heads @ w.T))
    print(f"forward(state) {dt} T=1: worst row {worst:.3e} (bound {TOL[dt]:.0e})")
    assert worst < TOL[dt]
    ptr = st.state.data_ptr()
    st.reset()
    assert st.count == 0 and st.state.data_ptr() == ptr
    again = run()
    assert st.count == N
    for y0, y1 in zip(outs, again):
        assert torch.equal(y0, y1)


# ---- 4. without a state nothing changed -------------------------------------------------------------------------------
def test_input_pos_without_state_takes_the_slicing_path():
    from attention_mechanisms.fastmax import fastmax
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    torch.manual_seed(9)
    blk = CausalSelfAttention(n_embd=256, n_head=8, n_query_groups=2, head_size=32).to("cuda").eval()
    B, T, G, qpk, hs = 2, 5, 2, 4, 32
    x = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(10)).cuda()
    cos, sin = build_rope_cache(16, hs, device="cuda")
    pos = torch.arange(3, 3 + T, device="cuda")
    c, s = cos.index_select(0, pos), sin.index_select(0, pos)
    with torch.no_grad():
        y_kw = blk(x, c, s, pos, state=None)
        y_pos = blk(x, c, s, pos)
        # the documented path: slices of the (B, T, group, slot, hs) view, K and V repeated per query head, apply_rope,
        # UNMASKED p=2 attention over the T tokens of the call, the reshape without a transpose, the output projection
        q, k, v = _slice_split(blk.attn(x).view(B, T, G, qpk + 2, hs), c, s, hs)
        k, v = (t.repeat_interleave(qpk, dim=1) for t in (k, v))
        y_ref = blk.proj(fastmax(q, k, v, p=2, mask=False).reshape(B, T, 8 * hs))
    assert torch.equal(y_kw, y_pos)
    assert torch.equal(y_kw, y_ref)
