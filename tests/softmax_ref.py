"""Float64 reference of causal softmax attention and the allowance its tests grant, per element.

Inputs are generated in the kernel's dtype, so the reference sees exactly the rounded values.  With A_ic = sum_j p_ij |v_jc|, u the
dtype's unit roundoff, n_i the number of keys of row i and
    delta_i = (D + 2) 2^-24 scale max_j sum_d |q_id k_jd|                                   (the error of a float32 score)
the first-order bound of an output element is
    u |o_ic| + (u + (n_i + D + 8) 2^-24 + 2 delta_i) A_ic
(output rounding; P rounded once to 16 bits; the float32 sums of the row and of P V; the scores), and of lse_i
    (n_i + 8) 2^-24 + delta_i.
The tests allow twice that."""
import torch

U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
EPS = 2.0 ** -24


def inputs(B, H, Hkv, N, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, N, D, generator=g).to(dt)
    k, v = (torch.randn(B, Hkv, N, D, generator=g).to(dt) for _ in range(2))
    return q, k, v


def reference(q, k, v, scale=None):
    """q (B,H,N,D), k, v (B,Hkv,N,D) in a 16-bit dtype -> dict(o, lse, allow_o, allow_lse), float64, the allowances doubled"""
    u, (B, H, N, D) = U[q.dtype], q.shape
    scale = D ** -0.5 if scale is None else scale
    q, k, v = (t.double().cpu() for t in (q, k, v))
    k, v = (t.repeat_interleave(H // t.shape[1], dim=1) for t in (k, v))
    keep = torch.ones(N, N, dtype=torch.bool).tril()
    s = (scale * q @ k.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    p = e / l
    n = torch.arange(1, N + 1, dtype=torch.float64)
    delta = (D + 2) * EPS * scale * (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~keep, 0.0).max(-1).values
    o, A = p @ v, p @ v.abs()
    allow_o = u * o.abs() + (u + (n + D + 8) * EPS + 2 * delta)[..., None] * A
    return dict(o=o, lse=(m + l.log())[..., 0], allow_o=2 * allow_o, allow_lse=2 * ((n + 8) * EPS + delta))


def fractions(o, lse, ref, rows=slice(None)):
    """the largest |error| / allowance of o (and of lse unless None) over ``rows`` of the reference; finite outputs only"""
    assert torch.isfinite(o.float()).all()
    fo = ((o.double().cpu() - ref["o"][:, :, rows]).abs() / ref["allow_o"][:, :, rows]).max().item()
    fl = 0.0 if lse is None else ((lse.double().cpu() - ref["lse"][:, :, rows]).abs() / ref["allow_lse"][:, :, rows]).max().item()
    return fo, fl
