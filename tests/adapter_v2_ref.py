"""Restatement of what csrc/adapter_v2.hip computes (include/fastmax_hip_adapter.h), with every rounding point explicit, and the
allowance for its two sums; shared by test_adapter_v2_cpu.py and test_adapter_v2_gpu.py.  Torch tensor ops on whatever device
the inputs are on: elementwise float32 operations and casts are the same bits everywhere, the sums are float64.

    same parameter dtype:   t = round(z + bias),  y = round(scale * t)
    float32 parameters:     t = float(z) + bias,  y = scale * t        (float32)
    dz = round(dy * scale)
    dscale = sum_m dy t,  dbias = sum_m dy scale                        (the terms formed from the rounded inputs, t with its rounding)

y and dz are compared bit for bit.  A sum of M float32 terms, whatever its order, differs from the exact sum of the same terms
by at most (M - 1) u sum|term| to first order, u = 2^-24; each term is itself a float32 product rounded once (u |term|), and the
terms of the partial sums are added again (another rounding per level, well inside the two spare units): the allowance is
(M + 2) 2^-24 sum_m |term_m|.  Derived, not measured."""
import torch

U = 2.0 ** -24


def restate(z, scale, bias, dy=None):
    """-> dict: t, y (y's dtype), and with dy: dz (z's dtype), dscale64 / dbias64 (float64 sums over the rows) and their
    allowances allow_scale / allow_bias (float64, per column).  z, dy: (M, N); scale, bias: (N,)"""
    same = scale.dtype == z.dtype
    zf, sf, bf = z.float(), scale.float(), bias.float()
    t = (zf + bf).to(z.dtype).float() if same else zf + bf
    y = (sf * t).to(z.dtype if same else torch.float32)
    out = {"t": t, "y": y}
    if dy is not None:
        M = z.shape[0]
        dyf = dy.float()
        out["dz"] = (dyf * sf).to(z.dtype)
        ts, tb = dyf.double() * t.double(), dyf.double() * sf.double()
        out["dscale64"], out["dbias64"] = ts.sum(0), tb.sum(0)
        out["allow_scale"], out["allow_bias"] = (M + 2) * U * ts.abs().sum(0), (M + 2) * U * tb.abs().sum(0)
    return out


def within(got, want64, allow) -> bool:
    """|got - want64| <= allow, entry by entry"""
    return bool(((got.double() - want64).abs() <= allow).all())


def worst(got, want64, allow) -> float:
    """the largest |got - want64| / allow (0 where both are 0): printed next to a failed assertion"""
    err = (got.double() - want64).abs()
    beyond = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    return float(torch.where(allow > 0, err / allow.clamp_min(1e-300), beyond).max())


def tensor_op(z, scale, bias, dy):
    """the reference's expression in tensor ops with autograd: -> (y, dz, dscale, dbias) as torch computes them"""
    z, scale, bias = (t.detach().clone().requires_grad_(True) for t in (z, scale, bias))
    y = scale * (z + bias)
    y.backward(dy)
    return y.detach(), z.grad, scale.grad, bias.grad
