"""What the int8-linear tests share: the LLM.int8 codec of include/fastmax_hip_int8.h in numpy float32 (the kernels match it bit for
bit), the float64 reference of the product built from those codes, and the element-wise allowance

    |y - ref| <= u_out |ref| + 2 (n_out + 6) 2^-24 S,      S = |int term| + sum_{c outlier} |x| |Wdeq| + |bias|

acc = sum CA CB is exact; float32 leaves about five roundings on the integer term, n_out + 4 on the outlier term and two adds, and
the factor 2 is margin for another summation order; u_out = 2^-8 (bf16) or 2^-11 (fp16) for the one rounding of the result.  Below
the format's smallest normal number the correctly rounded result itself is up to half a subnormal step (2^-25 for fp16) away, so
the rounding term is max(u_out |ref|, that half step).  No constant is measured."""
import numpy as np

f32, f64 = np.float32, np.float64
U_OUT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
HALF_SUBNORMAL_STEP = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25}


def _inv(scale):
    with np.errstate(divide="ignore"):
        return np.where(scale > 0, f32(127.0) / scale, f32(0.0)).astype(f32)


def quantize_weight(w):
    """w (N, K) float32 -> (CB int8 (N, K), SCB float32 (N,))"""
    w = np.asarray(w, f32)
    scb = np.abs(w).max(axis=1)
    return np.rint(w * _inv(scb)[:, None]).astype(np.int8), scb


def dequantize_weight(cb, scb):
    return cb.astype(f64) * scb.astype(f64)[:, None] / 127.0


def round_once(q, dt):
    """float64 rounded once (half to even) to dt, as float64; bf16 (8 significant bits) by frexp / rint / ldexp, normal range only"""
    if dt != "bf16":
        return q.astype(f32 if dt == "fp32" else np.float16).astype(f64)
    m, e = np.frexp(q)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def quantize_rows(x, threshold):
    """x (M, K) float32 -> (CA int8, SCA float32 (M,), flags uint8 (K,), ascending outlier columns int32)"""
    x = np.asarray(x, f32)
    flags = (np.abs(x) >= f32(threshold)).any(axis=0)
    sca = np.where(flags[None, :], f32(0.0), np.abs(x)).max(axis=1)
    ca = np.where(flags[None, :], f32(0.0), np.rint(x * _inv(sca)[:, None])).astype(np.int8)
    return ca, sca, flags.astype(np.uint8), np.nonzero(flags)[0].astype(np.int32)


def linear(x, cb, scb, bias, threshold):
    """float64 reference of the int8 linear from the reference's own codes -> (ref, S, n_out)"""
    ca, sca, _, cols = quantize_rows(x, threshold)
    acc = ca.astype(np.int64) @ cb.astype(np.int64).T
    int_term = acc.astype(f64) * (sca.astype(f64)[:, None] * scb.astype(f64)[None, :]) / 16129.0
    xo, wo = np.asarray(x, f64)[:, cols], dequantize_weight(cb, scb)[:, cols]
    b = np.zeros(cb.shape[0], f64) if bias is None else np.asarray(bias, f64)
    return int_term + xo @ wo.T + b, np.abs(int_term) + np.abs(xo) @ np.abs(wo).T + np.abs(b), len(cols)


def allowance(ref, S, n_out, dt):
    return np.maximum(U_OUT[dt] * np.abs(ref), HALF_SUBNORMAL_STEP[dt]) + 2.0 * (n_out + 6) * 2.0 ** -24 * S
