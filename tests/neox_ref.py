"""float64 numpy restatements of the NeoX block's neighbours of the attention sub-layer, with the reference's rounding points:
LayerNorm (torch.nn.LayerNorm: float32 statistics, ONE rounding of the normalised, scaled and shifted row), the residual stream
of the parallel-residual block (mlp + h + x, two rounded adds, left to right) and the exact GELU of GptNeoxMLP.  Built on
block_ref.round_to / ulp / act_ref32.  Shared by test_neox_cpu.py (which proves the restatements on the fixtures) and
test_neox_gpu.py."""
import numpy as np

import block_ref as br


def stream_ref(x, r1=None, r2=None, dt="f32"):
    """x, round(x + r1), or round(round(r1 + r2) + x): Block.forward's `self.mlp(n_2) + h + x` with r1 = mlp, r2 = h"""
    x = np.asarray(x, np.float64)
    if r1 is None:
        return x
    if r2 is None:
        return br.round_to(x + np.asarray(r1, np.float64), dt)
    return br.round_to(br.round_to(np.asarray(r1, np.float64) + np.asarray(r2, np.float64), dt) + x, dt)


def layernorm_ref(s, w, b, eps, dt, exact=False):
    """-> (y, mean, rstd) in float64; y rounded once to `dt` (not at all with `exact`)"""
    s = np.asarray(s, np.float64)
    mean = s.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((s - mean) ** 2).mean(-1, keepdims=True) + eps)
    y = (s - mean) * rstd * np.asarray(w, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
    return (y if exact else br.round_to(y, dt)), mean[..., 0], rstd[..., 0]


def gelu_ref(a, dt):
    """round(gelu(a)), gelu evaluated with a float32 rounding after every operation as the reference does"""
    return br.round_to(br.act_ref32(a, "gelu"), dt)


def gelu_floor(a):
    """the float32 cancellation of 1 + erf in exact GELU: block_ref.gated_floor with b = 1, i.e. 2^-23 |a|"""
    return br.gated_floor(a, 1.0, "gelu")


def gelu_interval(a, dt):
    """(lo, hi) of round(gelu(a)) over the float32 cancellation error of 1 + erf: block_ref.gated_interval with b = 1"""
    return br.gated_interval(a, np.ones_like(np.asarray(a, np.float64)), "gelu", dt)
