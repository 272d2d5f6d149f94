"""`SoftmaxKVDecodeState.extend_block` (csrc/softmax_kv_block.hip) against the float64 reference of tests/softmax_ref.py under its
allowance, and the route's bit contract: a row's bits depend on its q row and the cache prefix alone."""
import pytest
import torch

import softmax_ref as sr
from fastmax_experiments_amd import _lib
from test_softmax_gpu import DTYPES, PROMPT, _inside, _model, _need_gpu, _pattern, _state          # _need_gpu: the skip without a device

pytestmark = pytest.mark.gpu
C, R, S = _lib.KV_CHUNK, _lib.KV_BLOCK_ROWS, _lib.KV_BLOCK_SPAN
# new tokens per q_per_kv from count = C - 3: the rows cross the chunk boundary inside the first tile, T * q_per_kv passes R with a
# ragged last tile (q_per_kv = 3: a token's heads straddle two tiles), and q_per_kv = 1 takes more than KV_BLOCK_TOKENS tokens
NEW = {1: _lib.KV_BLOCK_TOKENS + 6, 3: R // 3 + 2, 8: R // 8 + 3}
CASES = [(H, Hkv, D, C - 3, NEW[H // Hkv]) for H, Hkv in [(4, 4), (8, 1), (6, 2), (32, 4)] for D in (32, 64, 80, 128, 256)]
CASES += [(4, 4, 64, S * C - 2, 6), (4, 4, 64, 0, 9), (8, 1, 64, C - 3, 1), (8, 1, 64, 0, 1)]          # a span boundary; empty; T = 1


def _cut(t, a, b):
    return t[:, :, a:b]


@DTYPES
@pytest.mark.parametrize("H, Hkv, D, count, T", CASES)
def test_extend_block_matches_the_reference(H, Hkv, D, count, T, dt):
    N = count + T
    q, k, v = sr.inputs(1, H, Hkv, N, D, dt, D + H + T)
    ref = sr.reference(q, k, v)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    st = _state(1, H, Hkv, D, dt, max_len=N + 5)
    if count:
        st.prefill(_cut(q, 0, count), _cut(k, 0, count), _cut(v, 0, count))
    o, lse = st.extend_block(_cut(q, count, N), _cut(k, count, N), _cut(v, count, N), lse=True)
    _inside(f"extend_block D={D} H={H}/{Hkv} {count}+{T} {dt}", o, lse, ref, slice(count, N))
    assert o.shape == (1, H, T, D) and o.dtype == dt and lse.dtype == torch.float32 and st.count == N and st.header.tolist()[:2] == [N, 0]


@DTYPES
@pytest.mark.parametrize("name", ["rising", "falling", "spike", "equal"])
def test_running_maximum_inside_a_span(name, dt):
    N, D = 3 * C + 16, 64          # the last rows see four chunks of span 0: the rescale path
    assert S >= 4
    q, k, v = sr.inputs(1, 2, 2, N, D, dt, 5)
    q.zero_(), k.zero_()
    q[..., 0] = 8.0
    k[..., 0] = (_pattern(name, N) / 8).to(dt)          # q_i . k_j = the pattern's score of key j (rounded to the dtype), scale 1
    o, lse = _state(1, 2, 2, D, dt, max_len=N, scale=1.0).extend_block(q.cuda(), k.cuda(), v.cuda(), lse=True)
    _inside(f"running maximum inside a span, {name}, {dt}", o, lse, sr.reference(q, k, v, scale=1.0))


def test_bits_depend_on_the_row_and_the_prefix_alone():
    dt, H, Hkv, D, count, T = torch.bfloat16, 8, 2, 64, 5, 11
    N = count + T
    q, k, v = (t.cuda() for t in sr.inputs(1, H, Hkv, N, D, dt, 9))

    def run(cuts=(count, N), B=1, row=0, max_len=200, strided=False, graphed=False):
        qq, kk, vv = q, k, v
        if B > 1:          # the sequence as row `row` of a batch of other sequences
            other = [t.cuda() for t in sr.inputs(B, H, Hkv, N, D, dt, 10)]
            for o_, t in zip(other, (q, k, v)):
                o_[row] = t[0]
            qq, kk, vv = other
        if strided:        # rows inside a wider buffer, heads and tokens swapped in memory
            qq, kk, vv = (torch.cat((t, t), -1).transpose(1, 2).contiguous().transpose(1, 2)[..., :D] for t in (qq, kk, vv))
        st = _state(B, H, Hkv, D, dt, max_len)
        outs = []
        for a, b in zip((0,) + cuts, cuts):
            snap = st.state.clone() if graphed else None
            outs.append(st.extend_block(_cut(qq, a, b), _cut(kk, a, b), _cut(vv, a, b)))
        if graphed:        # the last call again, recorded: several replays from the state before it
            st._count, graph = a, torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                rec = st.extend_block(_cut(qq, a, b), _cut(kk, a, b), _cut(vv, a, b))
            for _ in range(3):
                st.state.copy_(snap)
                rec.zero_()
                graph.replay()
                assert torch.equal(rec, outs[-1]) and st.header.tolist()[:2] == [N, 0]
        assert st.count == N
        return torch.cat(outs[1:], 2)[row:row + 1]

    want = run()
    _inside("extend_block 5 + 11", want, None, sr.reference(q, k, v), slice(count, N))
    for kw in (dict(cuts=(count, 10, N)), dict(cuts=tuple(range(count, N + 1))), dict(B=3, row=2), dict(max_len=1000), dict(strided=True),
               dict(graphed=True)):
        assert torch.equal(run(**kw), want), kw


def test_truncation_over_nan_rows():
    dt, H, Hkv, D, N = torch.float16, 8, 2, 64, 140
    q, k, v = (t.cuda() for t in sr.inputs(1, H, Hkv, N, D, dt, 11))
    dirty, fresh = _state(1, H, Hkv, D, dt), _state(1, H, Hkv, D, dt)
    kn, vn = k.clone(), v.clone()
    kn[:, :, 3:], vn[:, :, 3:] = float("nan"), float("nan")
    dirty.extend_block(q, kn, vn)
    dirty.count = 3
    fresh.extend_block(_cut(q, 0, 3), _cut(k, 0, 3), _cut(v, 0, 3))
    a, b = (st.extend_block(_cut(q, 3, 20), _cut(k, 3, 20), _cut(v, 3, 20)) for st in (dirty, fresh))
    assert torch.isfinite(a).all() and torch.equal(a, b) and dirty.header.tolist()[:2] == [20, 0]


def test_device_guard():
    q, k, v = (t.cuda() for t in sr.inputs(1, 2, 2, 4, 64, torch.bfloat16, 1))
    st = _state(1, 2, 2, 64, torch.bfloat16, max_len=5)
    st.extend_block(q, k, v)
    st._count = 3                                                # the header's length is above the host's mirror: the device guard fires
    before = st.state.clone()
    o, lse = st.extend_block(_cut(q, 0, 2), _cut(k, 0, 2), _cut(v, 0, 2), lse=True)
    assert not o.any() and not lse.any() and st.header.tolist()[:2] == [4, 1]
    before[1] = st.state[1]
    assert torch.equal(before.view(torch.int32), st.state.view(torch.int32))          # nothing but the sticky flag was written


@pytest.mark.parametrize("adapted", [False, True])
def test_block_with_block_extend_matches_the_forward_over_the_prompt(adapted):
    """test_softmax_gpu's comparison and tolerance (2 x 8e-3 of a row's largest entry, bf16) with the second piece on extend_block"""
    from fastmax_experiments_amd import adapter
    m = _model()
    attn = m["stack"].blocks[0].attn
    if adapted:
        assert adapter.adapt([attn], adapter_start_layer=0) == 1
        for p in (p for p in attn.parameters() if p.requires_grad):
            torch.nn.init.normal_(p, std=0.2)
    x = torch.randn(2, PROMPT, 64, generator=torch.Generator().manual_seed(8)).bfloat16().cuda()
    st = m["states"](2, 16)[0]
    st.block_extend = True
    with torch.no_grad():
        want = attn(x, m["cos"][:PROMPT], m["sin"][:PROMPT]).float()
        got = torch.cat([attn(x[:, a:b], m["cos"][a:b], m["sin"][a:b], torch.arange(a, b, device="cuda"), st)
                         for a, b in [(0, 6), (6, 9)]], 1).float()
    err = ((got - want).abs().amax(-1) / want.abs().amax(-1)).max().item()
    print(f"quadratic attention sub-layer on extend_block, adapted={adapted}: worst row {err:.3e}")
    assert want.abs().amax(-1).min() > 0 and err < 2 * 8e-3 and st.count == PROMPT and (st.prefix is not None) == adapted
