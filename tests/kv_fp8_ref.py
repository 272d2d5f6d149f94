"""The fp8 KV cache's format restated in torch, and the float64 reference of a decode over the DEQUANTISED cache.

A row (D values of one K or V position) is stored as e4m3 codes x / s with s = 2^e the smallest power of two with
max |x| <= 448 s; `quantise` is include/fastmax_hip_kv_fp8.h's rule word for word.

`reference` is softmax_ref.reference on code * scale, with one more term in the allowance of o.  The kernel rounds p_j vs_j, not
p_j, to the 16-bit operand of the product with the V codes.  vs_j is a power of two, so while p_j vs_j stays a normal number of
the dtype the rounding has the relative error u that softmax_ref already charges for P (u A_ic, with A taken over |code| vs).
Below the dtype's smallest normal number the error is absolute instead: at most half the subnormal spacing, h = 2^-25 in fp16
and 2^-134 in bf16, whatever p_j is.  Key j then adds at most h |code_jc| to the unnormalised numerator of its wave, which
reaches o_ic times exp2(m_wave - M) <= 1 and divided by l_i = sum_j exp(s_ij - max_j s_ij):
    extra_ic = h sum_{j <= n_i} |code_jc| / l_i
charged for every key (an upper bound: only keys whose p_j vs_j is subnormal incur it), doubled like the other terms."""
import torch

import softmax_ref as sr

HALF_SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def quantise(x):
    """rows x (..., D) in a 16-bit dtype -> (codes uint8 (..., D), scale float32 (...))"""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-126, 127)
    s = torch.ldexp(torch.ones_like(amax), torch.where(amax == 0, torch.zeros_like(e), e))
    return (xf / s[..., None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def reference(q, codes, scale=None):
    """q (B,H,N,D) 16-bit and `codes` = (k_codes, v_codes, k_scale, v_scale) of N cached positions -> softmax_ref.reference's dict"""
    kc, vc, ks, vs = (t.cpu() for t in codes)
    k, v = (c.view(torch.float8_e4m3fn).float().double() * s.double()[..., None] for c, s in ((kc, ks), (vc, vs)))
    ref = sr.reference(q, k, v, scale)
    (B, H, N, D), rep = q.shape, q.shape[1] // k.shape[1]
    s = ((D ** -0.5 if scale is None else scale) * q.double().cpu() @ k.repeat_interleave(rep, 1).transpose(-1, -2))
    s = s.masked_fill(~torch.ones(N, N, dtype=torch.bool).tril(), float("-inf"))
    l = (s - s.max(-1, keepdim=True).values).exp().sum(-1, keepdim=True)
    mass = vc.view(torch.float8_e4m3fn).float().double().abs().cumsum(2).repeat_interleave(rep, 1)
    ref["allow_o"] = ref["allow_o"] + 2 * HALF_SUBNORMAL[q.dtype] * mass / l
    return ref
