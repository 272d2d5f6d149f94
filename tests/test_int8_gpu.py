"""The int8 linear on an MI355X through the C ABI: quantisers and decode bit for bit against tests/int8_ref.py, the product inside
the allowance of its float64 reference, guarded buffers; then the module, a graph replayed on another outlier set, generation."""
import functools

import numpy as np
import pytest
import torch

import int8_ref as R
from fastmax_experiments_amd import _lib
from qlora_ref import F32, Guarded2D, padded

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, _lib.BF16), "fp16": (torch.float16, _lib.F16), "fp32": (torch.float32, _lib.F32)}
THR, PATTERNS = 6.0, ["none", "one", "edges", "every", "equal"]
_np = lambda t: t.detach().float().cpu().numpy()          # noqa: E731


def raw(rows, nbytes, dtype):
    """a guarded buffer of rows x nbytes of NaN bit patterns, and its payload seen as `dtype`"""
    g = Guarded2D(rows, nbytes // 4, dtype=F32)
    return g, g.t.view(dtype)


@functools.lru_cache(maxsize=None)
def weight(N, K, dt):
    # -> (dense weight on the device, the reference's codes, scales); one all-zero row, one row whose maximum is negative
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.05
    w[3], w[N - 2, K // 2] = 0.0, -0.9
    w = w.to(DT[dt][0]).cuda()
    return (w,) + R.quantize_weight(_np(w))


def activations(M, K, dt, pattern, pad):
    """x (M, K) in dt with row stride K + pad: |x| <= 5.5 except on the pattern's outlier columns; row M // 2 all zero"""
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(7 * M + K)) * 1.5).clamp(-5.5, 5.5)
    x[M // 2], x[0, 5] = 0.0, 5.96875                     # 5.96875: just under the threshold, stays an ordinary column
    cols = {"none": [], "one": [K // 3], "edges": [0, K - 1, K - 64 + 9, K - 64 + 41], "every": range(K), "equal": [17]}[pattern]
    for i, c in enumerate(cols):
        x[(3 * i) % M, c] = THR if pattern == "equal" else (-1) ** i * (8.0 + i % 5)
    return padded(x.to(DT[dt][0]), pad)


def call_linear(x, cb, scb, bias, dt, N):
    M, K = x.shape
    nb = _lib.lib().fastmax_hip_int8_linear_workspace(M, K)
    y, ws = Guarded2D(M, N, N + 8, dtype=DT[dt][0]), Guarded2D(1, nb // 4, dtype=F32)
    rc = _lib.lib().fastmax_hip_int8_linear(x.data_ptr(), x.stride(0), cb.data_ptr(), scb.data_ptr(), None if bias is None else bias.data_ptr(),
                                            y.ptr(), N + 8, M, N, K, DT[dt][1], THR, ws.ptr(), nb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    y.check("y"), ws.check("workspace", payload_written=False)
    return y.t


@pytest.mark.parametrize("src", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N, K", [(16, 64), (80, 192), (272, 512)])
def test_weight_quantiser_and_decode_bit_exact(N, K, src):
    w, cb_ref, scb_ref = weight(N, K, src)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    (gc, cb), scb = raw(N, K, torch.int8), Guarded2D(1, N, dtype=F32)
    assert L.fastmax_hip_int8_quantize_weight(w.data_ptr(), K, DT[src][1], cb.data_ptr(), scb.ptr(), N, K, stream) == 0
    assert np.array_equal(cb.cpu().numpy(), cb_ref) and np.array_equal(_np(scb.t)[0], scb_ref)
    gc.check("codes", payload_written=False), scb.check("SCB")
    assert scb_ref[3] == 0 and not cb_ref[3].any() and cb_ref[N - 2].min() == -127
    for out in DT:
        d = Guarded2D(N, K, K + 8, dtype=DT[out][0])
        assert L.fastmax_hip_int8_dequantize_weight(cb.data_ptr(), scb.ptr(), d.ptr(), K + 8, DT[out][1], N, K, stream) == 0
        d.check(out)
        assert np.array_equal(d.t.double().cpu().numpy(), R.round_once(R.dequantize_weight(cb_ref, scb_ref), out))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("K", [64, 192, 512])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 129])
def test_activation_pass_bit_exact(M, K, dt):
    for i, pattern in enumerate(p for p in PATTERNS if p != "every" or K == 64):
        x = activations(M, K, dt, pattern, pad=8 * (i % 2))
        ca_ref, sca_ref, flags_ref, cols_ref = R.quantize_rows(_np(x), THR)
        (gca, ca), sca, (gf, flags) = raw(M, K, torch.int8), Guarded2D(1, M, dtype=F32), raw(1, K, torch.uint8)
        (gl, lst), (gn, cnt) = raw(1, 4 * K, torch.int32), raw(1, 4, torch.int32)
        assert _lib.lib().fastmax_hip_int8_quantize_rows(x.data_ptr(), x.stride(0), DT[dt][1], THR, ca.data_ptr(), sca.ptr(), flags.data_ptr(),
                                                         lst.data_ptr(), cnt.data_ptr(), M, K, torch.cuda.current_stream().cuda_stream) == 0
        assert (n := int(cnt.item())) == len(cols_ref) and np.array_equal(lst.cpu().numpy()[0, :n], cols_ref), pattern
        assert np.array_equal(flags.cpu().numpy()[0], flags_ref) and (M == 1 or sca_ref[M // 2] == 0), pattern
        assert np.array_equal(ca.cpu().numpy(), ca_ref) and np.array_equal(_np(sca.t)[0], sca_ref), pattern
        [g.check(pattern, payload_written=g is sca) for g in (gca, gf, gl, gn, sca)]
        assert gl.t[0, n:].isnan().all(), "the list is written past its count"


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("K, N", [(64, 16), (192, 80), (512, 272)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 129, 200])
def test_linear_within_the_allowance(M, K, N, dt, bias):
    _, cb_ref, scb_ref = weight(N, K, "fp32")
    cb, scb = torch.from_numpy(cb_ref).cuda(), torch.from_numpy(scb_ref).cuda()
    b = torch.linspace(-2.0, 2.0, N).cuda() if bias else None
    for i, pattern in enumerate(p for p in PATTERNS if p != "every" or K == 64):
        x = activations(M, K, dt, pattern, pad=8 * (i % 2))
        y = _np(call_linear(x, cb, scb, b, dt, N)).astype(np.float64)
        ref, S, n_out = R.linear(_np(x), cb_ref, scb_ref, None if b is None else _np(b), THR)
        ratio = np.abs(y - ref) / R.allowance(ref, S, n_out, dt)
        print(f"{pattern}: n_out {n_out}, worst |err| / allowance {ratio.max():.3f}")
        assert ratio.max() <= 1.0, (pattern, np.unravel_index(np.argmax(ratio), ratio.shape))


@pytest.mark.parametrize("shape", [(5, 192), (2, 9, 192)])
def test_module_equals_the_c_abi(shape):
    from fastmax_experiments_amd.lora import Int8Linear
    torch.manual_seed(1)
    q = Int8Linear.from_linear(torch.nn.Linear(192, 80).cuda().to(torch.bfloat16), threshold=THR)
    x = activations(int(np.prod(shape[:-1])), 192, "bf16", "edges", 0).reshape(shape)
    want = call_linear(x.reshape(-1, 192), q.weight.data, q.SCB, q.bias.data, "bf16", 80)
    assert q(x).shape == shape[:-1] + (80,) and torch.equal(q(x).reshape(-1, 80), want)
    assert torch.equal(q(activations(x.numel() // 192, 192, "bf16", "edges", 8)), want)          # a padded row stride goes in as ldx
    with pytest.raises(NotImplementedError, match="bnb.int8-training"):
        q(x.clone().requires_grad_())


def test_lora_on_an_int8_base_and_merge():
    from fastmax_experiments_amd.lora import Int8Linear, LoRALinear
    torch.manual_seed(2)
    lin = LoRALinear(192, 80, r=8, lora_alpha=16).cuda().to(torch.bfloat16).quantize_base(mode="bnb.int8")
    x = activations(5, 192, "bf16", "one", 0)
    assert isinstance(lin.linear, Int8Linear) and lin.plan(x).route == lin.plan(x).lora == "tensor_ops"
    with torch.no_grad():
        lin.lora_B.normal_(std=0.05)
        assert torch.equal(lin(x), lin.linear(x) + ((x @ lin.lora_A.t()) @ lin.lora_B.t()) * lin.scaling)
        codes = lin.linear.weight.clone()
        lin.merge()
        assert isinstance(lin.linear, Int8Linear) and not torch.equal(lin.linear.weight, codes) and torch.equal(lin(x), lin.linear(x))


def test_graph_replay_with_another_outlier_set():
    from fastmax_experiments_amd.lora import Int8Linear
    q = Int8Linear.from_linear(torch.nn.Linear(512, 272).cuda().to(torch.bfloat16))
    static = activations(1, 512, "bf16", "none", 0).clone()
    q(static)                                                                    # the library is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = q(static)
    for pattern in ("edges", "none", "one"):
        x = activations(1, 512, "bf16", pattern, 0)
        static.copy_(x)
        graph.replay()
        assert torch.equal(out, q(x)), pattern


def test_generation_through_int8_blocks():
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    from fastmax_experiments_amd.generate import GraphedDecoder, NextTokenHead, generate
    torch.manual_seed(3)
    dt, total = torch.bfloat16, 5 + 4
    stack = BlockStack([Block.from_config("pythia-14m", attn_alg="fastmax").quantize_base(mode="bnb.int8") for _ in range(2)]).to("cuda", dt).eval()
    assert sum(type(m).__name__ == "Int8Linear" for m in stack.modules()) == 10
    head, wte = NextTokenHead(128, 515).to("cuda", dt).eval(), torch.randn(515, 128).to(dt).cuda()
    cos, sin = build_rope_cache(total, stack.blocks[0].attn.rope_n_elem, device="cuda")
    prompt = torch.randint(0, 515, (2, 5), generator=torch.Generator().manual_seed(4)).cuda()
    states = [[FastmaxDecodeState(2, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)] for _ in range(2)]
    kw = dict(cos=cos, sin=sin, temperature=1.0, top_k=1)
    want = generate(wte, stack, head, states[0], prompt, total, **kw)
    got = GraphedDecoder(wte, stack, head, states[1], max_len=total, **kw).generate(prompt, total)
    assert got.shape == (2, total) and torch.equal(got, want)
