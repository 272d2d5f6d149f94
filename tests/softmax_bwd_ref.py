"""Float64 reference of the gradients of causal softmax attention (autograd over the float64 formula on the exact 16-bit inputs) and
the first-order allowance its tests grant, per element: the formulas of DESIGN.md 4.6b, doubled.  u is the unit roundoff, 2^-8
for bf16 (softmax_ref's 2^-9 understates it by a factor of 2; a_ic, the forward's allowance of o_ic, is evaluated with this u),
``tiny`` the half spacing below the dtype's normal range, where P, dS and the gradients round absolutely, not relatively."""
import torch

import softmax_ref

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
EPS = 2.0 ** -24


def inputs(B, H, Hkv, N, D, dt, seed):
    q, k, v = softmax_ref.inputs(B, H, Hkv, N, D, dt, seed)
    return q, k, v, torch.randn(B, H, N, D, generator=torch.Generator().manual_seed(seed + 1)).to(dt)


def reference(q, k, v, dO, scale=None):
    """16-bit q, dO (B,H,N,D), k, v (B,Hkv,N,D) -> dict(dq, dk, dv, allow_dq, allow_dk, allow_dv), float64, the allowances doubled"""
    u, tiny, (B, H, N, D), Hkv = U[q.dtype], TINY[q.dtype], q.shape, k.shape[1]
    r, scale = H // Hkv, D ** -0.5 if scale is None else scale
    q, k, v, dO = (t.double().cpu() for t in (q, k, v, dO))
    keep = torch.ones(N, N, dtype=torch.bool).tril()

    def attention(q, k, v):
        kx, vx = (t.repeat_interleave(r, dim=1) for t in (k, v))
        p = (scale * q @ kx.transpose(-1, -2)).masked_fill(~keep, float("-inf")).softmax(-1)
        return p, p @ vx

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    dq, dk, dv = torch.autograd.grad(attention(*leaves)[1], leaves, dO)
    kx, vx = (t.repeat_interleave(r, dim=1) for t in (k, v))
    p, o = attention(q, k, v)
    dS = p * (dO @ vx.transpose(-1, -2) - (dO * o).sum(-1, keepdim=True))

    def group(t):          # per query head (B,H,N,D) -> summed over each KV head's group
        return t.view(B, Hkv, r, N, D).sum(2)

    n = torch.arange(1, N + 1, dtype=torch.float64)[:, None]
    m = r * torch.arange(N, 0, -1, dtype=torch.float64)[:, None]
    delta = (D + 2) * EPS * scale * (q.abs() @ kx.abs().transpose(-1, -2)).masked_fill(~keep, 0.0).max(-1, keepdim=True).values
    eps = 2 * delta + (n + 12) * EPS
    a = u * o.abs() + (u + (n + D + 8) * EPS + 2 * delta) * (p @ vx.abs())
    derr = (dO.abs() * a).sum(-1, keepdim=True) + (D + 2) * EPS * (dO * o).abs().sum(-1, keepdim=True)
    E = (eps + u + 2 * EPS) * dS.abs() + tiny * keep + p * ((D + 2) * EPS * dO.abs() @ vx.abs().transpose(-1, -2) + derr)
    Et, dSt, pt = (t.transpose(-1, -2) for t in (E, dS.abs(), p))
    allow = dict(dq=u * dq.abs() + tiny + scale * (E @ kx.abs() + (n + 2) * EPS * (dS.abs() @ kx.abs())),
                 dk=u * dk.abs() + tiny + scale * (group(Et @ q.abs()) + (m + 2) * EPS * group(dSt @ q.abs())),
                 dv=u * dv.abs() + tiny + group(((eps + u) * p + tiny * keep).transpose(-1, -2) @ dO.abs()) + (m + 2) * EPS * group(pt @ dO.abs()))
    return dict(dq=dq, dk=dk, dv=dv, **{"allow_" + key: 2 * val for key, val in allow.items()})


def fractions(grads, ref):
    """the largest |error| / allowance of each of dq, dk, dv; finite gradients only"""
    assert all(torch.isfinite(g.float()).all() for g in grads)
    return [((g.double().cpu() - ref[key]).abs() / ref["allow_" + key]).max().item() for g, key in zip(grads, ("dq", "dk", "dv"))]
