"""KV-cache decode (decode.py FastmaxKVDecodeState, csrc/fastmax_kv_decode.hip, include/fastmax_hip_kv_decode.h) on an MI355X.

The reference is the C oracle's masked forward over the whole sequence on the dtype-rounded inputs (float64 blockwise rows after a
long prefill, the float64 projection-and-oracle reference for the block); every step row is measured against that row's own
magnitude as tests/test_decode_p2_gpu.py does, with that file's tolerances: fp32 2e-4, bf16 8e-3, f16 2e-3.  `randn` inputs keep
s = q.k / nt at a standard deviation of 0.125 at every D, so 1 + s stays well away from 0 for p = 1 too.

1. prefill + 6 single steps, three dtypes, head sizes 32 .. 256, across a chunk boundary;  2. p = 1;  3. D = 33 (element loads);
4. grouped queries against the oracle and against a per-query-head cache;  5. steps after a 4096-token prefill;  6. extend against
single steps, bit for bit;  7. bits do not depend on strides, the run, B, the batch row or max_len;  8. truncation;  9. the
capacity guard on the host and on the device;  10. a two-block stack at head size 256 against float64, and at 64 against the
second-order state;  11. generate() and GraphedDecoder on KV caches."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import blockwise as bw
from conftest import rel_err
from oracle import c_oracle, fastmax_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-4, torch.bfloat16: 8e-3, torch.float16: 2e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _kv(B, H, D, max_len, dt, **kw):
    from fastmax_experiments_amd.decode import FastmaxKVDecodeState
    return FastmaxKVDecodeState(B, H, D, "cuda", max_len, dt, **kw)


def _chunk():
    from fastmax_experiments_amd import _lib
    return _lib.KV_CHUNK


def _row_err(got, ref):
    """worst over the rows (last axis = D) of max|got - ref| / max|ref| of that row"""
    got = np.asarray(got, np.float64).reshape(-1, ref.shape[-1])
    ref = np.asarray(ref, np.float64).reshape(-1, ref.shape[-1])
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-6)).max())


def _run(st, q, k, v, T):
    """prefill over the first T tokens, then one step per remaining token -> (prefill o, stacked step outputs (B,H,S,D))"""
    o = st.prefill(q[:, :, :T], k[:, :, :T], v[:, :, :T])
    steps = [st.step(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1]) for t in range(T, q.shape[2])]
    return o, torch.cat(steps, dim=2)


def _steps(st, q, k, v, a, b):
    return torch.cat([st.step(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1]) for t in range(a, b)], dim=2)


def _qkv(B, H, Hkv, N, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, N, D, generator=g).to(dt)
    k, v = (torch.randn(B, Hkv, N, D, generator=g).to(dt) for _ in range(2))
    return q, k, v


def _oracle(q, k, v, p=2):
    r = q.shape[1] // k.shape[1]
    ke, ve = (t.repeat_interleave(r, dim=1) for t in (k, v))
    ref, _ = c_oracle.fwd(q.float().numpy(), ke.float().numpy(), ve.float().numpy(), mask=True, p=p)
    return ref


# ---- 1. prefill + steps -----------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, -3, 64), (1, 2, 70, 32), (1, 2, 130, 128), (1, 2, 77, 40), (1, 2, 61, 80), (1, 2, 90, 256)]      # T < 0: CHUNK + T


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,T,D", SHAPES)
def test_prefill_and_steps_match_masked_forward(B, H, T, D, dt):
    T = T if T > 0 else _chunk() + T          # CHUNK - 3: the steps cross a chunk boundary, so two partials are combined
    q, k, v = _qkv(B, H, H, T + 6, D, dt, T + D)
    ref = _oracle(q, k, v)
    st = _kv(B, H, D, T + 6, dt)
    o, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    assert o.shape == (B, H, T, D) and steps.shape == (B, H, 6, D) and steps.dtype == dt
    assert rel_err(o.float().cpu().numpy(), ref[:, :, :T]) < TOL[dt]
    err = _row_err(steps.float().cpu().numpy(), ref[:, :, T:])
    print(f"kv decode ({B},{H},{T},{D}) {dt}: worst step row {err:.3e}")
    assert err < TOL[dt]
    assert st.count == T + 6 and st.header.tolist()[:2] == [T + 6, 0]


# ---- 2. first order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_first_order(dt):
    B, H, T, D = 1, 2, 70, 64
    q, k, v = _qkv(B, H, H, T + 6, D, dt, 101)
    ref = _oracle(q, k, v, p=1)
    st = _kv(B, H, D, T + 6, dt, p=1)
    o, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    assert rel_err(o.float().cpu().numpy(), ref[:, :, :T]) < TOL[dt]
    err = _row_err(steps.float().cpu().numpy(), ref[:, :, T:])
    print(f"kv decode p=1 {dt}: worst step row {err:.3e}")
    assert err < TOL[dt] and st.count == T + 6


# ---- 3. rows that are not whole 16-byte pieces -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_head_size_without_whole_16_byte_rows(dt):
    """D = 33: the caches' rows are not whole 16-byte pieces, every load and copy goes element by element"""
    B, H, T, D = 1, 2, 95, 33
    q, k, v = _qkv(B, H, H, T + 3, D, dt, 33)
    ref = _oracle(q, k, v)
    _, steps = _run(_kv(B, H, D, 200, dt), q.cuda(), k.cuda(), v.cuda(), T)
    assert _row_err(steps.float().cpu().numpy(), ref[:, :, T:]) < TOL[dt]


# ---- 4. grouped queries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv,D", [(2, 64), (1, 64), (1, 256)])
def test_grouped_query_heads(Hkv, D):
    B, H, T, S = 2, 8, 150, 5
    q, k, v = _qkv(B, H, Hkv, T + S, D, torch.float32, Hkv + D)
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    ref = _oracle(q, k, v)
    st = _kv(B, H, D, T + S, torch.float32, n_query_groups=Hkv)
    o, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    assert rel_err(o.cpu().numpy(), ref[:, :, :T]) < TOL[torch.float32]
    assert _row_err(steps.cpu().numpy(), ref[:, :, T:]) < TOL[torch.float32]
    # the same sequence through a cache with one K/V copy per query head over the expanded K, V
    full = _kv(B, H, D, T + S, torch.float32)
    o_f, steps_f = _run(full, q.cuda(), ke.cuda(), ve.cuda(), T)
    assert full.state.numel() > st.state.numel()
    assert _row_err(steps.cpu().numpy(), steps_f.cpu().numpy()) < 1e-5
    assert _row_err(o.cpu().numpy(), o_f.cpu().numpy()) < 1e-5


# ---- 5. steps after a long prefill ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 256])
def test_steps_after_long_prefill_blockwise(D):
    B, H, T, S = 1, 2, 4096, 64
    q, k, v = _qkv(B, H, H, T + S, D, torch.bfloat16, T + D)
    nt = orc.effective_normalize_term(D)
    st = _kv(B, H, D, T + S, torch.bfloat16)
    _, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    for h in range(H):
        ro, _ = bw.dense_rows(*(t[0, h].double().numpy() for t in (q, k, v)), nt=nt, p=2, mask=True)
        err, r0, _, scale = bw.worst_block(steps[0, h].double().cpu().numpy(), ro[T:], block=1)
        print(f"kv decode after {T} tokens, D={D}, head {h}: worst step row {err:.3e} (step {r0}, max|ref| {scale:.3e})")
        assert err <= TOL[torch.bfloat16], (h, r0, err)


# ---- 6. extend = single steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,Hkv", [(torch.bfloat16, 64, 2), (torch.float32, 40, 4), (torch.float16, 256, 1)])
def test_extend_is_bitwise_the_single_steps(dt, D, Hkv):
    B, H, T0 = 2, 4, 50
    N = T0 + 7 + 1 + 1
    q, k, v = (t.cuda() for t in _qkv(B, H, Hkv, N, D, dt, D + Hkv))
    ref = _oracle(q.cpu(), k.cpu(), v.cpu())
    a, b = (_kv(B, H, D, 200, dt, n_query_groups=Hkv) for _ in range(2))
    a.prefill(q[:, :, :T0], k[:, :, :T0], v[:, :, :T0])
    b.prefill(q[:, :, :T0], k[:, :, :T0], v[:, :, :T0])
    outs = [a.extend(q[:, :, T0:T0 + 7], k[:, :, T0:T0 + 7], v[:, :, T0:T0 + 7]),
            a.extend(q[:, :, T0 + 7:T0 + 8], k[:, :, T0 + 7:T0 + 8], v[:, :, T0 + 7:T0 + 8]),
            a.step(q[:, :, T0 + 8:], k[:, :, T0 + 8:], v[:, :, T0 + 8:])]
    got = torch.cat(outs, dim=2)
    assert got.shape == (B, H, 9, D) and got.dtype == dt
    assert _row_err(got.float().cpu().numpy(), ref[:, :, T0:]) < TOL[dt]
    single = _steps(b, q, k, v, T0, N)
    assert torch.equal(got, single) and torch.equal(a.state, b.state)
    assert a.count == b.count == N and a.header.tolist()[:2] == [N, 0]


def test_extend_onto_an_empty_cache_and_over_several_slices():
    """20 tokens at once (three slices of the kernel's token loop, the first chunk only) onto an empty cache"""
    B, H, Hkv, D, N = 1, 4, 2, 64, 20
    q, k, v = (t.cuda() for t in _qkv(B, H, Hkv, N, D, torch.float32, 20))
    ref = _oracle(q.cpu(), k.cpu(), v.cpu())
    a, b = (_kv(B, H, D, 64, torch.float32, n_query_groups=Hkv) for _ in range(2))
    got = a.extend(q, k, v)
    assert _row_err(got.cpu().numpy(), ref) < TOL[torch.float32]
    assert torch.equal(got, _steps(b, q, k, v, 0, N)) and torch.equal(a.state, b.state)


# ---- 7. what the bits do not depend on --------------------------------------------------------------------------------------------
def test_strided_inputs_bit_identical_to_contiguous():
    B, H, Hkv, T, S, D = 2, 4, 2, 90, 4, 64
    g = torch.Generator().manual_seed(7)
    packed = torch.randn(B, T + S, H + 2 * Hkv, D, generator=g).to(torch.bfloat16).cuda()      # (B, N, heads, D) storage
    q, k, v = (packed[:, :, a:b].transpose(1, 2) for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv)))
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    s1, s2 = (_kv(B, H, D, 128, torch.bfloat16, n_query_groups=Hkv) for _ in range(2))
    o1, st1 = _run(s1, q, k, v, T)
    o2, st2 = _run(s2, q.contiguous(), k.contiguous(), v.contiguous(), T)
    assert torch.equal(st1, st2) and torch.equal(o1, o2)
    assert torch.equal(s1.state, s2.state)


def test_bitwise_reproducible():
    B, H, Hkv, T, S, D = 1, 8, 2, 300, 5, 128
    q, k, v = (t.cuda() for t in _qkv(B, H, Hkv, T + S, D, torch.bfloat16, 11))
    runs = []
    for _ in range(2):
        st = _kv(B, H, D, T + S, torch.bfloat16, n_query_groups=Hkv)
        o, steps = _run(st, q, k, v, T)
        torch.cuda.synchronize()
        runs.append((o, steps, st.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt,D", [(torch.bfloat16, 64), (torch.float32, 80)])
def test_a_row_does_not_depend_on_the_batch_or_on_max_len(dt, D):
    B, H, Hkv, T, S = 3, 4, 2, 140, 4
    q, k, v = (t.cuda() for t in _qkv(B, H, Hkv, T + S, D, dt, 13))
    whole = _kv(B, H, D, 300, dt, n_query_groups=Hkv)
    whole.prefill(q[:, :, :T], k[:, :, :T], v[:, :, :T])
    steps = _steps(whole, q, k, v, T, T + S)
    for row in (0, 2):                                    # the same sequence alone, at either end of the batch
        one = _kv(1, H, D, 300, dt, n_query_groups=Hkv)
        sl = slice(row, row + 1)
        one.prefill(q[sl, :, :T], k[sl, :, :T], v[sl, :, :T])
        assert torch.equal(_steps(one, q[sl], k[sl], v[sl], T, T + S), steps[sl]), row
    roomy = _kv(B, H, D, 1000, dt, n_query_groups=Hkv)    # more chunks in the grid and in the workspace, the same live ones
    roomy.prefill(q[:, :, :T], k[:, :, :T], v[:, :, :T])
    assert torch.equal(_steps(roomy, q, k, v, T, T + S), steps)
    assert roomy.state.numel() > whole.state.numel()


# ---- 8. truncation ----------------------------------------------------------------------------------------------------------------
def test_lowering_count_truncates_the_cache():
    B, H, Hkv, D, dt = 2, 4, 2, 64, torch.bfloat16
    q, k, v = (t.cuda() for t in _qkv(B, H, Hkv, 45, D, dt, 17))
    st = _kv(B, H, D, 64, dt, n_query_groups=Hkv)
    st.extend(q[:, :, :40], k[:, :, :40], v[:, :, :40])
    with pytest.raises(ValueError, match="only be lowered"):
        st.count = 41
    st.count = 25
    assert st.count == 25 and st.header.tolist()[:2] == [25, 0]
    tail = st.extend(q[:, :, 40:], k[:, :, 40:], v[:, :, 40:])
    fresh = _kv(B, H, D, 64, dt, n_query_groups=Hkv)
    fresh.extend(q[:, :, :25], k[:, :, :25], v[:, :, :25])
    want = fresh.extend(q[:, :, 40:], k[:, :, 40:], v[:, :, 40:])
    assert torch.equal(tail, want) and st.count == fresh.count == 30
    assert st.header.tolist()[:2] == fresh.header.tolist()[:2] == [30, 0]
    rows = st.state[16:].clone()
    st.reset()                                            # the header only: the rows stay where they are
    assert st.count == 0 and st.header.tolist() == [0] * 16 and torch.equal(st.state[16:], rows)


# ---- 9. the guard -----------------------------------------------------------------------------------------------------------------
def test_a_full_cache_refuses_on_the_host_and_on_the_device():
    from fastmax_experiments_amd import _lib, ops
    B, H, D, dt = 2, 2, 64, torch.float32
    q, k, v = (t.cuda() for t in _qkv(B, H, H, 6, D, dt, 19))
    st = _kv(B, H, D, 5, dt)
    st.prefill(q[:, :, :5], k[:, :, :5], v[:, :, :5])
    torch.cuda.synchronize()
    before = st.state.clone()
    with pytest.raises(ValueError, match="do not fit"):
        st.step(q[:, :, 5:], k[:, :, 5:], v[:, :, 5:])
    with pytest.raises(ValueError, match="do not fit"):
        st.extend(q[:, :, 4:], k[:, :, 4:], v[:, :, 4:])
    assert st.count == 5 and torch.equal(st.state, before)          # nothing was launched
    # the entry point itself, as a graph replay too many would call it
    o = torch.ones(B, H, 1, D, dtype=dt, device="cuda")
    qd, kd, vd = (t[:, :, 5:].contiguous() for t in (q, k, v))
    need = _lib.lib().fastmax_hip_kv_decode_workspace(B, H, H, 1, D, 5)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().fastmax_hip_kv_decode_append_attend(*ops._qkv(qd, kd, vd), st.state.data_ptr(), o.data_ptr(), B, H, H, 1, D, 5,
                                                        _lib.F32, 2, 1.0 / st.nt, ws.data_ptr(), need,
                                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK
    torch.cuda.synchronize()
    assert st.header.tolist()[:2] == [5, 1]
    after = st.state.clone()
    after[:16].view(torch.int32)[_lib.KV_OVERFLOW] = 0
    assert torch.equal(after, before)                               # the rows and the length are where they were
    assert bool((o == 0).all())


# ---- 10. through the blocks -------------------------------------------------------------------------------------------------------
VOCAB = 96


def _stack(head_size, dt):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    torch.manual_seed(head_size)
    stack = BlockStack([Block(n_embd=64, n_head=2, n_query_groups=1, head_size=head_size, intermediate_size=128)
                        for _ in range(2)]).to("cuda", dt).eval()
    head = NextTokenHead(64, VOCAB).to("cuda", dt).eval()
    wte = torch.randn(VOCAB, 64).to(dt).cuda()
    cos, sin = build_rope_cache(32, stack.blocks[0].attn.rope_n_elem, device="cuda")
    return dict(stack=stack, head=head, wte=wte, cos=cos, sin=sin, hs=head_size, dt=dt)


def _kv_states(m, B, max_len):
    from fastmax_experiments_amd.decode import FastmaxKVDecodeState
    return [FastmaxKVDecodeState.for_attention(b.attn, B, max_len, "cuda", m["dt"]) for b in m["stack"].blocks]


def _rope64(x, cos, sin):
    half = x.shape[-1] // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * sin


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_block_attention_at_head_size_256_matches_float64(dt):
    """five tokens through attend_cached (a call of 3, two single tokens) against masked p=2 fastmax over the five positions fed
    the block's own QKV projection, de-interleaved and rotated in float64"""
    m = _stack(256, dt)
    blk = m["stack"].blocks[0].attn
    B, H, G, hs, qpk, N = 2, 2, 1, 256, 2, 5
    calls = [(0, 3), (3, 4), (4, 5)]
    x = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(6)).to(dt).cuda()
    cos, sin = m["cos"][:N], m["sin"][:N]
    with torch.no_grad():
        qkv = torch.cat([blk.attn(x[:, a:b]) for a, b in calls], dim=1)
    qkv = qkv.double().cpu().view(B, N, G, qpk + 2, hs)
    c64, s64 = cos.double().cpu(), sin.double().cpu()
    q = _rope64(qkv[:, :, :, :qpk].permute(0, 2, 3, 1, 4).reshape(B, H, N, hs), c64, s64)
    k = _rope64(qkv[:, :, :, qpk].permute(0, 2, 1, 3), c64, s64).repeat_interleave(qpk, dim=1)
    v = qkv[:, :, :, qpk + 1].permute(0, 2, 1, 3).repeat_interleave(qpk, dim=1)
    ref, _ = c_oracle.fwd(q.numpy(), k.numpy(), v.numpy(), mask=True, p=2)
    st = _kv_states(m, B, 8)[0]
    assert (st.H, st.Hkv, st.D, st.p, st.max_len) == (H, G, hs, 2, 8)
    with torch.no_grad():
        outs = [blk.attend_cached(x[:, a:b], cos[a:b], sin[a:b], st) for a, b in calls]
    for (a, b), o in zip(calls, outs):
        assert o.shape == (B, H, b - a, hs) and o.dtype == dt
    got = torch.cat(outs, dim=2).float().cpu().numpy()
    err = _row_err(got, ref)
    print(f"attend_cached on a KV cache, head size 256, {dt}: worst row {err:.3e} (bound {TOL[dt]:.0e})")
    assert err < TOL[dt] and st.count == N


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_stack_logits_on_kv_caches_match_the_second_order_state(dt):
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    m = _stack(64, dt)
    B, N = 2, 5
    x = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(8)).to(dt).cuda()
    kv = _kv_states(m, B, 8)
    p2 = [FastmaxDecodeState(B, 2, 64, "cuda", p=2, n_query_groups=1) for _ in range(2)]
    worst = 0.0
    with torch.no_grad():
        for a, b in [(0, 3), (3, 4), (4, 5)]:
            pos = torch.arange(a, b, device="cuda")
            la, lb = (m["head"].logits(m["stack"](x[:, a:b], m["cos"][a:b], m["sin"][a:b], pos, s)) for s in (kv, p2))
            assert la.shape == (B, VOCAB)
            worst = max(worst, _row_err(la.float().cpu().numpy(), lb.float().cpu().numpy()))
    print(f"two blocks, head size 64, {dt}: logits on KV caches against the p=2 state, worst row {worst:.3e}")
    assert worst < 2 * TOL[dt] and all(s.count == N for s in kv + p2)


# ---- 11. generation ---------------------------------------------------------------------------------------------------------------
PROMPT, NEW = 5, 12


@functools.lru_cache(maxsize=None)
def _gen_model():
    m = _stack(256, torch.float32)
    g = torch.Generator().manual_seed(4)
    m["prompt"] = torch.randint(0, VOCAB, (2, PROMPT), generator=g).cuda()
    return m


def _eager(m, states, n, **kw):
    from fastmax_experiments_amd.generate import generate
    return generate(m["wte"], m["stack"], m["head"], states, m["prompt"], n, cos=m["cos"], sin=m["sin"], **kw)


def test_generate_at_head_size_256():
    from fastmax_experiments_amd.generate import Sampler
    m = _gen_model()
    total = PROMPT + NEW
    states = _kv_states(m, 2, total - 1)
    out = _eager(m, states, total, temperature=0.0, sampler=Sampler(1))
    assert out.shape == (2, total) and out.dtype == torch.int64 and torch.equal(out[:, :PROMPT], m["prompt"])
    assert int(out.min()) >= 0 and int(out.max()) < VOCAB
    assert all(s.count == total - 1 and s.header.tolist()[:2] == [total - 1, 0] for s in states)
    with pytest.raises(ValueError, match="holds at most"):
        _eager(m, _kv_states(m, 2, total - 2), total, temperature=0.0)


def _common_eos(tokens):
    """the token every row has produced soonest, and the length at which the eager loop then stops; (None, full length) if none"""
    best = (None, tokens.shape[1])
    for e in sorted(set(tokens[:, PROMPT:].flatten().tolist())):
        first = [(row[PROMPT:] == e).nonzero().flatten()[:1].tolist() for row in tokens]
        if all(first):
            n = PROMPT + max(f[0] for f in first) + 1
            if n < best[1]:
                best = (e, n)
    return best


@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
def test_graphed_generate_on_kv_caches_equals_the_eager_loop(with_eos):
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler
    m = _gen_model()
    total = PROMPT + NEW
    kw = dict(temperature=0.8, top_k=5)
    eos, seed, room = None, 21, total + 1                 # room for the two tokens fed after the loop
    if with_eos:
        # a seed under which both rows produce some token early, so that the replays run past the end and the caches are cut back
        for seed in range(21, 61):
            full = _eager(m, _kv_states(m, 2, room), total, sampler=Sampler(seed), **kw)
            eos, stop = _common_eos(full)
            if eos is not None and stop <= total - 2:
                break
        if eos is None:                                   # no token shared by both rows: the first one of row 0, the loop runs on
            eos = int(full[0, PROMPT])
        kw["eos_id"] = eos
    eager_states, states = _kv_states(m, 2, room), _kv_states(m, 2, room)
    want = _eager(m, eager_states, total, sampler=Sampler(seed), **kw)
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], states, cos=m["cos"], sin=m["sin"], max_len=total, **kw)
    decoder.poll = 4
    got = decoder.generate(m["prompt"], total, Sampler(seed))
    n = want.shape[1]
    print(f"graphed generate on KV caches: seed {seed}, eos {eos}, {n} of {total} tokens, {decoder.replays} replays")
    assert got.shape == want.shape and torch.equal(got, want)
    assert decoder.captures == 1 and not decoder.cursor.read()["overflow"]
    for a, b in zip(states, eager_states):
        assert a.count == b.count == n - 1
        assert a.header.tolist()[:2] == b.header.tolist()[:2] == [n - 1, 0]
    # both routes continue from the same place
    q, k, v = (t.cuda() for t in _qkv(2, 2, 1, 2, 256, torch.float32, 23))
    for a, b in zip(states, eager_states):
        assert torch.equal(a.extend(q, k, v), b.extend(q, k, v))
        assert a.header.tolist()[:2] == b.header.tolist()[:2] == [n + 1, 0]
    with pytest.raises(ValueError, match="holds at most"):
        GraphedDecoder(m["wte"], m["stack"], m["head"], _kv_states(m, 2, total - 2), cos=m["cos"], sin=m["sin"], max_len=total)


def test_recording_on_a_cache_with_no_room_for_its_warm_up_steps():
    """a cache of exactly the tokens fed: the recording's three steps do not fit behind the prompt, so it runs them on a cache
    taken back by as many tokens and puts everything back"""
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler
    m = _gen_model()
    total = PROMPT + 3
    eager_states, states = _kv_states(m, 2, total - 1), _kv_states(m, 2, total - 1)
    want = _eager(m, eager_states, total, temperature=0.0, sampler=Sampler(3))
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], states, cos=m["cos"], sin=m["sin"], max_len=total, temperature=0.0)
    got = decoder.generate(m["prompt"], total, Sampler(3))
    assert torch.equal(got, want) and decoder.captures == 1 and decoder.replays == 2
    for a, b in zip(states, eager_states):
        assert a.count == b.count == total - 1 and torch.equal(a.state, b.state)
