"""Softmax attention's backward on the GPU against the float64 reference of tests/softmax_bwd_ref.py (parity per element, KV heads by
stride and by view, equal bits, peaked scores, the block against a float32 restatement, refusals).  Measured fractions of the
allowance: profiles/r29_softmax_backward.md."""
import pytest
import torch
import torch.nn.functional as F

import softmax_bwd_ref as br
from test_softmax_gpu import DTYPES, _need_gpu, _pattern  # noqa: F401  (the autouse fixture skips the module without a device)

pytestmark = pytest.mark.gpu


def _grads(q, k, v, dO, scale=None, views=False):
    """dO is a transposed view, as the block hands it back; ``views``: K/V as per-head stride-0 views, their gradients summed"""
    from fastmax_experiments_amd import ops
    (B, H, N, D), Hkv = q.shape, k.shape[1]
    q, k, v = (t.cuda().requires_grad_(True) for t in (q, k, v))
    dO = dO.cuda().transpose(1, 2).contiguous().transpose(1, 2)
    assert N == 1 or not dO.is_contiguous()
    if not views:
        return torch.autograd.grad(ops.softmax_attention_with_grad(q, k, v, scale), (q, k, v), dO)
    kv, vv = (t.view(B * Hkv, 1, N, D).expand(B * Hkv, H // Hkv, N, D) for t in (k, v))          # (batch, group) as the batch axis
    o = ops.softmax_attention_with_grad(q.view(B * Hkv, H // Hkv, N, D), kv, vv, scale).view(B, H, N, D)
    dq, dk, dv = torch.autograd.grad(o, (q, kv, vv), dO)
    return dq, dk.double().sum(1).view(B, Hkv, N, D), dv.double().sum(1).view(B, Hkv, N, D)


def _inside(what, grads, ref):
    fr = br.fractions(grads, ref)
    print(f"{what}: largest fraction of the allowance dq {fr[0]:.3f}, dk {fr[1]:.3f}, dv {fr[2]:.3f}")
    assert max(fr) <= 1.0


@DTYPES
@pytest.mark.parametrize("H, Hkv", [(2, 2), (8, 2)])
@pytest.mark.parametrize("D", [40, 64, 128])
@pytest.mark.parametrize("N", [1, 63, 65, 129, 300])
def test_backward_matches_the_reference(N, D, H, Hkv, dt):
    q, k, v, dO = br.inputs(2, H, Hkv, N, D, dt, N + D)
    ref = br.reference(q, k, v, dO)
    got = _grads(q, k, v, dO)
    assert got[0].shape == q.shape and got[1].shape == got[2].shape == k.shape and got[1].shape[1] == Hkv and got[1].dtype == dt
    _inside(f"backward N={N} D={D} H={H}/{Hkv} {dt}", got, ref)
    _inside("  K/V as per-head stride-0 views", _grads(q, k, v, dO, views=True), ref)
    assert all(torch.equal(a, b) for a, b in zip(got, _grads(q, k, v, dO)))          # two calls: the same bits


@DTYPES
@pytest.mark.parametrize("name", ["rising", "spike"])
def test_large_and_peaked_scores(name, dt):
    q, k, v, dO = br.inputs(1, 2, 2, 200, 64, dt, 5)
    q.zero_(), k.zero_()
    q[..., 0] = 8.0
    k[..., 0] = (_pattern(name, 200) / 8).to(dt)          # q_i . k_j = the pattern's score of key j, scale 1: up to 200
    _inside(f"peaked scores, {name}, {dt}", _grads(q, k, v, dO, scale=1.0), br.reference(q, k, v, dO, scale=1.0))


def test_block_trains_through_the_hip_backward():
    """against the same module on a float32 restatement of the operator; the HIP route may err twice what the bf16
    F.scaled_dot_product_attention route errs on the same inputs, per tensor, relative to the tensor's largest entry"""
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    torch.manual_seed(6)
    attn = CausalSelfAttention(n_embd=64, n_head=4, n_query_groups=1, head_size=64, attn_alg="quadratic").to("cuda", torch.bfloat16)
    names, trainable = zip(*((n, p) for n, p in attn.named_parameters() if p.requires_grad))
    for p in trainable:
        torch.nn.init.normal_(p, std=0.2)
    x = torch.randn(2, 70, 64, device="cuda").bfloat16().requires_grad_(True)
    cos, sin = build_rope_cache(70, 64, device="cuda")
    dy = torch.randn(2, 70, 64, device="cuda").bfloat16()
    assert attn.plan(x)[:2] == ("hip_pass", ops.KV_GROUPS)

    def run(cast):          # None: the module as it is; else the operator swapped for F.scaled_dot_product_attention on cast(q, k, v)
        def operator(q, k, v, *_):
            k, v = (t.repeat_interleave(q.shape[1] // t.shape[1], 1) for t in (k, v))
            return F.scaled_dot_product_attention(cast(q), cast(k), cast(v), is_causal=True).to(q.dtype)
        attn.__dict__.update({} if cast is None else {"_attend": operator})
        got = torch.autograd.grad(attn(x, cos, sin), (x, *trainable), dy)
        attn.__dict__.pop("_attend", None)
        return got

    for name, g, w, s in zip(("x", *names), run(None), run(torch.Tensor.float), run(lambda t: t)):
        err, base = ((t.float() - w.float()).abs().max().item() / w.float().abs().max().item() for t in (g, s))
        print(f"block gradient {name}: HIP {err:.3e}, bf16 SDPA {base:.3e} of the largest entry")
        assert err <= 2 * base, name


def test_refusals():
    from fastmax_experiments_amd import ops
    z = torch.zeros(1, 2, 4, 136, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="128"):
        ops.softmax_attention_with_grad(z, z, z)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.softmax_attention_with_grad(*(z[..., :64].float() for _ in range(3)))
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.softmax_attention(z[..., :64], z[..., :64], z[..., :64])
    q = torch.randn(1, 2, 9, 136, device="cuda").bfloat16()          # no gradient needed: softmax_attention's bits, at its head sizes
    assert torch.equal(ops.softmax_attention_with_grad(q, q, q), ops.softmax_attention(q, q, q))
