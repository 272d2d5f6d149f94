"""The fp8 softmax KV cache on the GPU (csrc/softmax_kv_fp8.hip): the stored bytes against the torch restatement of the format, bit
for bit; o and lse against the float64 reference on the dequantised cache (tests/kv_fp8_ref.py), per element; a row's bits under
T, batch row, max_len and graph replay; truncation and the full cache; an adapted stack through generate() and GraphedDecoder."""
import itertools

import pytest
import torch

import kv_fp8_ref as fr
import softmax_ref as sr

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _state(B, H, Hkv, D, dt, max_len=200):
    from fastmax_experiments_amd.decode import SoftmaxFP8KVDecodeState
    return SoftmaxFP8KVDecodeState(B, H, D, "cuda", max_len, dt, n_query_groups=Hkv)


def _cut(ts, a, b):
    return tuple(t[:, :, a:b] for t in ts)


@DTYPES
def test_stored_bytes(dt):
    """prefill 5, step, extend 3: after each, codes() is the restatement of the format on the rows fed so far.  Positions 1 .. 3 and
    5 .. 7 hold an all-zero row, a row whose amax is exactly 448 * 2^-6 = 7 and a row one ulp above it; k and v are strided."""
    B, H, Hkv, D, N = 2, 4, 2, 64, 9
    q, k, v = sr.inputs(B, H, Hkv, N, D, dt, 1)
    above = (torch.tensor(7.0, dtype=dt).view(torch.int16) + 1).view(dt)
    for t in (k, v):
        for base in (1, 5):
            t[:, :, base] = 0
            t[:, :, base + 1:base + 3].clamp_(-6, 6)
            t[:, :, base + 1, 3], t[:, :, base + 2, 60] = -7.0, above
    qd, kd, vd = (torch.cat((t, t), -1).cuda().transpose(1, 2).contiguous().transpose(1, 2)[..., :D] for t in (q, k, v))
    assert not kd.is_contiguous()
    st = _state(B, H, Hkv, D, dt)
    for n, feed in ((5, st.prefill), (6, st.step), (9, st.extend)):
        feed(*_cut((qd, kd, vd), st.count, n))
        kc, vc, ks, vs = st.codes()
        for got, scale, rows in ((kc, ks, k), (vc, vs, v)):
            want, want_scale = fr.quantise(rows[:, :, :n])
            assert got.shape == (B, Hkv, n, D) and got.dtype == torch.uint8 and scale.dtype == torch.float32
            assert torch.equal(got.cpu(), want) and torch.equal(scale.cpu(), want_scale), n
    assert ks[0, 0, 1:4].tolist() == [1.0, 2.0 ** -6, 2.0 ** -5] and st.header.tolist()[:2] == [9, 0]


CASES = [(1, *c, 200) for c in itertools.product((16, 64, 256), ((4, 4), (8, 2), (20, 1)), (torch.bfloat16, torch.float16), (0, 127), (1, 3))]
CASES.append((2, 64, (8, 2), torch.bfloat16, 300, 3, 400))


@pytest.mark.parametrize("B, D, heads, dt, count, T, max_len", CASES)
def test_values_against_the_dequantised_cache(B, D, heads, dt, count, T, max_len):
    (H, Hkv), N = heads, count + T
    q, k, v = sr.inputs(B, H, Hkv, N, D, dt, D + H + count)
    dev = tuple(t.cuda() for t in (q, k, v))
    st = _state(B, H, Hkv, D, dt, max_len)
    if count:
        st.prefill(*_cut(dev, 0, count))
    o, lse = st.extend(*_cut(dev, count, N), lse=True) if T > 1 else st.step(*_cut(dev, count, N), lse=True)
    assert o.dtype == dt and o.shape == (B, H, T, D) and lse.shape == (B, H, T) and st.count == N
    fo, fl = sr.fractions(o, lse, fr.reference(q, st.codes()), slice(count, N))
    print(f"fp8 decode B={B} D={D} H={H}/{Hkv} {dt} count={count} T={T}: largest fraction of the allowance o {fo:.3f}, lse {fl:.3f}")
    assert fo <= 1.0 and fl <= 1.0


def test_a_token_has_the_same_bits_however_it_is_fed():
    dt, H, Hkv, D, count, N = torch.bfloat16, 8, 2, 64, 126, 131          # the last tokens sit in the second chunk
    q, k, v = (t.cuda() for t in sr.inputs(1, H, Hkv, N, D, dt, 9))

    def run(B=1, row=0, max_len=200, single=False, graph=False):
        qkv = (q, k, v)
        if B > 1:          # the sequence as row `row` of a batch of other sequences
            qkv = tuple(t.cuda() for t in sr.inputs(B, H, Hkv, N, D, dt, 10))
            for o_, t in zip(qkv, (q, k, v)):
                o_[row] = t[0]
        st = _state(B, H, Hkv, D, dt, max_len)
        st.extend(*_cut(qkv, 0, count))
        if not single:
            return st.extend(*_cut(qkv, count, N))[row:row + 1]
        outs = []
        for i in range(count, N):
            tok = _cut(qkv, i, i + 1)
            if graph:          # the step recorded after a warm-up step and a truncation, then replayed
                st.step(*tok)
                st.count = i
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    o = st.step(*tok)
                st.count = i
                g.replay()
                st._replayed(1)
                outs.append(o.clone())
            else:
                outs.append(st.step(*tok))
        return torch.cat(outs, 2)[row:row + 1]

    want = run(single=True)
    for kw in (dict(), dict(B=3, row=2), dict(max_len=1000), dict(B=3, row=1, single=True), dict(single=True, graph=True)):
        assert torch.equal(run(**kw), want), kw


def test_truncation_and_the_full_cache():
    dt, H, Hkv, D, N = torch.float16, 8, 2, 64, 140
    qkv = tuple(t.cuda() for t in sr.inputs(1, H, Hkv, N + 1, D, dt, 11))
    dirty, fresh = _state(1, H, Hkv, D, dt, N), _state(1, H, Hkv, D, dt, N)
    dirty.extend(*_cut(qkv, 0, N))
    dirty.count = 130
    fresh.prefill(*_cut(qkv, 0, 130))
    assert torch.equal(dirty.step(*_cut(qkv, 130, 131)), fresh.step(*_cut(qkv, 130, 131))) and dirty.header.tolist()[:2] == [131, 0]
    fresh.extend(*_cut(qkv, 131, N))
    before = fresh.state.clone()
    with pytest.raises(ValueError, match="do not fit"):          # raised on the host, before anything is launched
        fresh.step(*_cut(qkv, N, N + 1))
    assert torch.equal(before.view(torch.int32), fresh.state.view(torch.int32)) and fresh.count == N


def test_an_adapted_stack_generates_the_same_tokens_eager_and_graphed():
    from fastmax_experiments_amd import adapter
    from fastmax_experiments_amd.decode import SoftmaxFP8KVDecodeState
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler, generate
    from test_softmax_gpu import PROMPT, VOCAB, _model
    m = _model()
    assert adapter.adapt(m["stack"], adapter_start_layer=1) == 1
    torch.nn.init.normal_(m["stack"].blocks[1].attn.gating_factor, std=2.0)
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(4)).cuda()
    total, kw = PROMPT + 8, dict(temperature=0.0)

    def states():
        return [SoftmaxFP8KVDecodeState.for_attention(b.attn, 2, total, "cuda", torch.bfloat16) for b in m["stack"].blocks]

    want = generate(m["wte"], m["stack"], m["head"], states(), prompt, total, cos=m["cos"], sin=m["sin"], sampler=Sampler(21), **kw)
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], states(), cos=m["cos"], sin=m["sin"], max_len=total, **kw)
    got = decoder.generate(prompt, total, Sampler(21))
    assert got.shape == (2, total) and torch.equal(got, want) and decoder.captures == 1
