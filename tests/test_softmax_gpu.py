"""Softmax attention on the GPU against the float64 reference of tests/softmax_ref.py (prefill, running maximum, decode, extend =
steps bit for bit, truncation, blocks and loops, refusals).  Measured fractions of the allowance: profiles/r28_softmax.md."""
import pytest
import torch

import softmax_ref as sr

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _state(B, H, Hkv, D, dt, max_len=200, **kw):
    from fastmax_experiments_amd.decode import SoftmaxKVDecodeState
    return SoftmaxKVDecodeState(B, H, D, "cuda", max_len, dt, n_query_groups=Hkv, **kw)


def _inside(what, o, lse, ref, rows=slice(None)):
    fo, fl = sr.fractions(o, lse, ref, rows)
    print(f"{what}: largest fraction of the allowance o {fo:.3f}, lse {fl:.3f}")
    assert fo <= 1.0 and fl <= 1.0


@DTYPES
@pytest.mark.parametrize("H, Hkv", [(2, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128, 256, 80])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 257])
def test_prefill_matches_the_reference(N, D, H, Hkv, dt):
    from fastmax_experiments_amd import ops
    q, k, v = sr.inputs(2, H, Hkv, N, D, dt, N + D)
    ref = sr.reference(q, k, v)
    kd, vd = k.cuda(), v.cuda()
    if Hkv != H:          # the block's group views: stride 0 over the group's query heads
        kd, vd = (t.expand(2, H, N, D) for t in (kd, vd))
    o, lse = ops.softmax_attention(q.cuda(), kd, vd, lse=True)
    assert o.dtype == dt and o.shape == q.shape and lse.dtype == torch.float32
    _inside(f"prefill N={N} D={D} H={H}/{Hkv} {dt}", o, lse, ref)
    assert torch.equal(o, ops.softmax_attention(q.cuda(), k.cuda(), v.cuda()))          # KV heads by stride or by view: the same bits


def _pattern(name, N):
    j = torch.arange(N, dtype=torch.float32)
    return {"rising": 200 * j / (N - 1), "falling": 200 - 200 * j / (N - 1), "spike": torch.where(j == 3, 200.0, -100.0),
            "equal": torch.full((N,), 50.0)}[name]


@DTYPES
@pytest.mark.parametrize("name", ["rising", "falling", "spike", "equal"])
def test_running_maximum(name, dt):
    from fastmax_experiments_amd import ops
    N, D = 200, 64
    q, k, v = sr.inputs(1, 2, 2, N, D, dt, 5)
    q.zero_(), k.zero_()
    q[..., 0] = 8.0
    k[..., 0] = (_pattern(name, N) / 8).to(dt)          # q_i . k_j = the pattern's score of key j (rounded to the dtype), scale 1
    o, lse = ops.softmax_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, lse=True)
    _inside(f"running maximum, {name}, {dt}", o, lse, sr.reference(q, k, v, scale=1.0))


@DTYPES
@pytest.mark.parametrize("H, Hkv", [(4, 4), (8, 1), (32, 4)])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_decode_across_the_chunk_boundary(D, H, Hkv, dt):
    from fastmax_experiments_amd import _lib
    T, S = _lib.KV_CHUNK - 3, 6
    q, k, v = sr.inputs(1, H, Hkv, T + S, D, dt, D + H)
    ref = sr.reference(q, k, v)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    st = _state(1, H, Hkv, D, dt)
    _inside("prefill rows", st.prefill(qd[:, :, :T], kd[:, :, :T], vd[:, :, :T]), None, ref, slice(0, T))
    outs = [st.step(qd[:, :, i:i + 1], kd[:, :, i:i + 1], vd[:, :, i:i + 1], lse=True) for i in range(T, T + S)]
    _inside(f"decode D={D} H={H}/{Hkv} {dt}", torch.cat([o for o, _ in outs], 2), torch.cat([l for _, l in outs], 2), ref, slice(T, T + S))
    assert st.count == T + S and st.header.tolist()[:2] == [T + S, 0]


def _steps(st, q, k, v, a, b):
    return torch.cat([st.step(q[:, :, i:i + 1], k[:, :, i:i + 1], v[:, :, i:i + 1]) for i in range(a, b)], 2)


@pytest.mark.parametrize("T", [7, 11])          # 11: more than one slice of new tokens
@pytest.mark.parametrize("count", [0, 5])
def test_extend_is_bitwise_the_single_steps(count, T):
    dt, H, Hkv, D, N = torch.bfloat16, 8, 2, 64, count + T
    q, k, v = (t.cuda() for t in sr.inputs(1, H, Hkv, N, D, dt, 9))
    ref = sr.reference(q, k, v)

    def run(B=1, row=0, max_len=200, strided=False, single=False):
        qq, kk, vv = q, k, v
        if B > 1:          # the sequence as row `row` of a batch of other sequences
            other = [t.cuda() for t in sr.inputs(B, H, Hkv, N, D, dt, 10)]
            for o_, t in zip(other, (q, k, v)):
                o_[row] = t[0]
            qq, kk, vv = other
        if strided:        # rows inside a wider buffer, heads and tokens swapped in memory
            qq, kk, vv = (torch.cat((t, t), -1).transpose(1, 2).contiguous().transpose(1, 2)[..., :D] for t in (qq, kk, vv))
        st = _state(B, H, Hkv, D, dt, max_len)
        if count:
            st.extend(qq[:, :, :count], kk[:, :, :count], vv[:, :, :count])
        o = _steps(st, qq, kk, vv, count, N) if single else st.extend(qq[:, :, count:], kk[:, :, count:], vv[:, :, count:])
        assert st.count == N
        return o[row:row + 1]

    want = run(single=True)
    _inside(f"steps from {count}", want, None, ref, slice(count, N))
    for kw in (dict(), dict(B=3, row=2), dict(max_len=1000), dict(strided=True), dict(B=3, row=1, single=True)):
        assert torch.equal(run(**kw), want), kw


def test_truncation_over_nan_rows():
    dt, H, Hkv, D, N = torch.float16, 8, 2, 64, 140
    q, k, v = (t.cuda() for t in sr.inputs(1, H, Hkv, N, D, dt, 11))
    dirty, fresh = _state(1, H, Hkv, D, dt), _state(1, H, Hkv, D, dt)
    kn, vn = k.clone(), v.clone()
    kn[:, :, 3:], vn[:, :, 3:] = float("nan"), float("nan")
    dirty.extend(q, kn, vn)
    dirty.count = 3
    fresh.extend(q[:, :, :3], k[:, :, :3], v[:, :, :3])
    for st in (dirty, fresh):
        st.out = torch.cat((_steps(st, q, k, v, 3, 8), st.extend(q[:, :, 8:20], k[:, :, 8:20], v[:, :, 8:20])), 2)
    assert torch.isfinite(dirty.out).all() and torch.equal(dirty.out, fresh.out) and dirty.header.tolist()[:2] == [20, 0]


VOCAB, PROMPT, NEW = 96, 9, 12


def _model():
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.decode import SoftmaxKVDecodeState
    from fastmax_experiments_amd.generate import NextTokenHead
    torch.manual_seed(3)
    dt = torch.bfloat16
    stack = BlockStack([Block(n_embd=64, n_head=4, n_query_groups=1, head_size=64, intermediate_size=128, attn_alg="quadratic")
                        for _ in range(2)]).to("cuda", dt).eval()
    cos, sin = build_rope_cache(32, 64, device="cuda")
    m = dict(stack=stack, head=NextTokenHead(64, VOCAB).to("cuda", dt).eval(), wte=torch.randn(VOCAB, 64).to(dt).cuda(), cos=cos, sin=sin)
    m["states"] = lambda B, n: [SoftmaxKVDecodeState.for_attention(b.attn, B, n, "cuda", dt) for b in stack.blocks]
    return m


def test_block_on_the_cache_matches_the_forward_over_the_prompt():
    """forward(x, cos, sin) against a prefill of 6 tokens and three single tokens on the cache; behind ``proj`` the tolerance is that
    of the same comparison on the fastmax KV route (tests/test_kv_decode_gpu.py: 2 x 8e-3 of a row's largest entry in bf16)"""
    m = _model()
    attn = m["stack"].blocks[0].attn
    x = torch.randn(2, PROMPT, 64, generator=torch.Generator().manual_seed(8)).bfloat16().cuda()
    st = m["states"](2, 16)[0]
    with torch.no_grad():
        want = attn(x, m["cos"][:PROMPT], m["sin"][:PROMPT]).float()
        got = torch.cat([attn(x[:, a:b], m["cos"][a:b], m["sin"][a:b], torch.arange(a, b, device="cuda"), st)
                         for a, b in [(0, 6), (6, 7), (7, 8), (8, 9)]], 1).float()
    err = ((got - want).abs().amax(-1) / want.abs().amax(-1)).max().item()
    print(f"quadratic attention sub-layer, bf16: cached rows against the forward over the prompt, worst row {err:.3e}")
    assert want.abs().amax(-1).min() > 0 and err < 2 * 8e-3 and st.count == PROMPT


def test_graphed_decoder_produces_the_eager_tokens():
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler, generate
    m = _model()
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(4)).cuda()
    total, kw = PROMPT + NEW, dict(temperature=0.8, top_k=5)
    want = generate(m["wte"], m["stack"], m["head"], m["states"](2, total), prompt, total, cos=m["cos"], sin=m["sin"],
                    sampler=Sampler(21), **kw)
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], m["states"](2, total), cos=m["cos"], sin=m["sin"], max_len=total, **kw)
    got = decoder.generate(prompt, total, Sampler(21))
    assert got.shape == (2, total) and torch.equal(got, want) and decoder.captures == 1


def test_refusals():
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.attention_block import CausalSelfAttention
    from fastmax_experiments_amd.decode import FastmaxKVDecodeState
    q, k, v = (t.cuda() for t in sr.inputs(1, 2, 2, 4, 64, torch.bfloat16, 1))
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.softmax_attention(q.float(), k.float(), v.float())
    for D in (12, 264):
        with pytest.raises(NotImplementedError, match=f"head size {D}"):
            ops.softmax_attention(*(torch.zeros(1, 2, 4, D, dtype=torch.bfloat16, device="cuda") for _ in range(3)))
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.softmax_attention(q.clone().requires_grad_(True), k, v)
    attn = CausalSelfAttention(n_embd=64, n_head=2, head_size=64, attn_alg="quadratic").to("cuda", torch.bfloat16)
    x, cos = torch.zeros(1, 1, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 64, device="cuda")
    with pytest.raises(TypeError, match="SoftmaxKVDecodeState"):
        attn.attend_cached(x, cos, cos, FastmaxKVDecodeState(1, 2, 64, "cuda", 8, torch.bfloat16))
    st = _state(1, 2, 2, 64, torch.bfloat16, max_len=5)
    st.extend(q, k, v)
    with pytest.raises(ValueError, match="do not fit"):          # the host refuses first
        st.extend(q[:, :, :2], k[:, :, :2], v[:, :, :2])
    st._count = 3                                                # the host's mirror is wrong: the device guard fires
    before = st.state.clone()
    o = st.extend(q[:, :, :2], k[:, :, :2], v[:, :, :2])
    assert not o.any() and st.header.tolist()[:2] == [4, 1]
    before[1] = st.state[1]
    assert torch.equal(before.view(torch.int32), st.state.view(torch.int32))          # nothing but the sticky flag was written
