"""LLaMA-Adapter's gated prefix attention (csrc/prefix_attention.hip) against the float64 reference of prefix_ref, per element."""
import pytest
import torch

import prefix_ref as pr
from test_softmax_gpu import _need_gpu, _state  # noqa: F401  (the module-wide skip fixture)

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
N2 = 2 * 512 + 1          # the smallest N with two whole backward chunks (FASTMAX_PREFIX_BWD_CHUNK rows) and a remainder


def _run(y, q, ak, av, gate, dO):
    from fastmax_experiments_amd import ops
    leaves = [t.detach().cuda().requires_grad_(True) for t in (y, q, ak, av, gate)]
    out = ops.prefix_attention_add(*leaves)
    gy, dq, dak, dav, dgate = torch.autograd.grad(out, leaves, dO.cuda())
    assert torch.equal(gy, dO.cuda())
    return dict(out=out.detach(), dq=dq, dak=dak, dav=dav, dgate=dgate)


@DTYPES
@pytest.mark.parametrize("N", [1, 33, N2])
@pytest.mark.parametrize("aT", [1, 10, 32])
@pytest.mark.parametrize("D", [40, 64, 128])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (8, 2)])
def test_parity_per_element(H, Hkv, D, aT, N, dt):
    z = H - 1          # the head whose gate is exactly 0
    args = pr.inputs(2, H, Hkv, N, D, aT, dt, N + D + aT, zero_head=z)
    ref = pr.reference(*args)
    got, again = _run(*args), _run(*args)
    for key in pr.KEYS:
        assert torch.equal(got[key], again[key]), key          # one summation order, no atomics
    fr = pr.fractions(got, ref)
    print(f"H {H}/{Hkv} D {D} aT {aT} N {N} {dt}: largest fraction of the allowance " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert all(v <= 1.0 for v in fr.values()), fr
    assert torch.equal(got["out"][:, z], args[0][:, z].cuda()) and not got["dq"][:, z].any()


@DTYPES
def test_forward_at_head_size_256(dt):
    from fastmax_experiments_amd import ops
    y, q, ak, av, gate, dO = pr.inputs(2, 8, 1, 161, 256, 10, dt, 3)
    out = ops.prefix_attention_add(*(t.cuda() for t in (y, q, ak, av, gate)))
    fr = pr.fractions(dict(out=out), pr.reference(y, q, ak, av, gate, dO))
    print(f"D 256 {dt}: largest fraction of the allowance out {fr['out']:.3f}")
    assert fr["out"] <= 1.0


def test_refusals():
    from fastmax_experiments_amd import ops
    z = torch.zeros(1, 2, 4, 136, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    a, gate = torch.zeros(2, 33, 136, dtype=torch.bfloat16, device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(NotImplementedError, match="128"):
        ops.prefix_attention_add(z, z, a[:, :10], a[:, :10], gate)
    with pytest.raises(ValueError, match="32"):
        ops.prefix_attention_add(z.detach(), z.detach(), a, a, gate)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.prefix_attention_add(*(t.detach().float() for t in (z, z, a[:, :10], a[:, :10])), gate)


def test_rows_do_not_depend_on_the_call():
    from fastmax_experiments_amd import ops
    y, q, ak, av, gate, _ = (t.cuda() for t in pr.inputs(2, 8, 2, 300, 64, 10, torch.bfloat16, 7))
    whole = ops.prefix_attention_add(y, q, ak, av, gate)
    for i in (0, 31, 128, 255, 256, 299):
        one = ops.prefix_attention_add(y[1:, :, i:i + 1].contiguous(), q[1:, :, i:i + 1].contiguous(), ak, av, gate)
        assert torch.equal(one, whole[1:, :, i:i + 1]), i


def test_decode_state_with_a_prefix():
    """prefill + 3 steps on a cache whose prefix is set: the bits of the same cache without one (whose prefill rows are the
    operator's on the whole sequence; a step's are the decode kernel's own) followed by prefix_attention_add on the whole sequence"""
    import softmax_ref as sr
    from fastmax_experiments_amd import ops
    dt, H, D, T = torch.bfloat16, 4, 64, 70
    q, k, v = (t.cuda() for t in sr.inputs(1, H, 1, T, D, dt, 13))
    _, _, ak, av, gate, _ = (t.cuda() for t in pr.inputs(1, H, 1, 1, D, 10, dt, 14))

    def rows(prefix):
        st = _state(1, H, 1, D, dt)
        st.prefix = prefix
        got = [st.prefill(q[:, :, :T - 3], k[:, :, :T - 3], v[:, :, :T - 3])]
        return torch.cat(got + [st.step(q[:, :, i:i + 1], k[:, :, i:i + 1], v[:, :, i:i + 1]) for i in range(T - 3, T)], 2)

    plain = rows(None)
    assert torch.equal(plain[:, :, :T - 3], ops.softmax_attention(q, k, v)[:, :, :T - 3])
    want = ops.prefix_attention_add(plain, q, ak, av, gate)
    assert not torch.equal(want, plain) and torch.equal(rows((ak, av, gate)), want)


def test_adapted_block():
    """gradients against the same module with the term on float32 tensor ops; the HIP term may err twice what the bf16 tensor-op
    term errs on the same inputs, per tensor, relative to the tensor's largest entry.  A fresh adapted block is the block itself."""
    from fastmax_experiments_amd import adapter
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    torch.manual_seed(6)
    attn = CausalSelfAttention(n_embd=64, n_head=4, n_query_groups=1, head_size=64, attn_alg="quadratic").to("cuda", torch.bfloat16)
    x = torch.randn(2, 70, 64, device="cuda").bfloat16().requires_grad_(True)
    cos, sin = build_rope_cache(70, 64, device="cuda")
    dy = torch.randn(2, 70, 64, device="cuda").bfloat16()
    plain = attn(x, cos, sin).detach()
    assert adapter.adapt([attn], adapter_start_layer=0) == 1
    assert torch.equal(attn(x, cos, sin).detach(), plain)
    names, trainable = zip(*((n, p) for n, p in attn.named_parameters() if p.requires_grad))
    assert {"adapter_wte.weight", "gating_factor"} <= set(names)
    for p in trainable:
        torch.nn.init.normal_(p, std=0.2)

    def run(dtype):          # None: the module as it is; else the term on tensor ops in ``dtype``
        def term(y, q, ak, av):
            return adapter.prefix_attention_tensor_ops(y, q, ak, av, attn.gating_factor, dtype).to(q.dtype)
        attn.__dict__.update({} if dtype is None else {"_prefix": term})
        got = torch.autograd.grad(attn(x, cos, sin), (x, *trainable), dy)
        attn.__dict__.pop("_prefix", None)
        return got

    for name, g, w, s in zip(("x", *names), run(None), run(torch.float32), run(torch.bfloat16)):
        err, base = ((t.float() - w.float()).abs().max().item() / w.float().abs().max().item() for t in (g, s))
        print(f"adapted block gradient {name}: HIP {err:.3e}, bf16 tensor ops {base:.3e} of the largest entry")
        assert err <= 2 * base, name


def test_graphed_decoder_runs_an_adapted_stack():
    """generate() on an adapted stack: the prefix term is recorded into the replayed step and changes the tokens"""
    from fastmax_experiments_amd import adapter
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler, generate
    from test_softmax_gpu import NEW, PROMPT, VOCAB, _model
    m = _model()
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(4)).cuda()
    total, kw = PROMPT + NEW, dict(temperature=0.8, top_k=5)

    def eager():
        return generate(m["wte"], m["stack"], m["head"], m["states"](2, total), prompt, total, cos=m["cos"], sin=m["sin"],
                        sampler=Sampler(21), **kw)

    plain = eager()
    assert adapter.adapt(m["stack"], adapter_start_layer=1) == 1 and torch.equal(eager(), plain)          # gates still zero
    torch.nn.init.normal_(m["stack"].blocks[1].attn.gating_factor, std=2.0)
    want = eager()
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], m["states"](2, total), cos=m["cos"], sin=m["sin"], max_len=total, **kw)
    got = decoder.generate(prompt, total, Sampler(21))
    assert torch.equal(got, want) and decoder.captures == 1 and not torch.equal(want, plain)
