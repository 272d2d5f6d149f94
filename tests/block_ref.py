"""float64 numpy restatements of RMSNorm (lit_gpt/rmsnorm.py:20-31) and of the gated MLP (lit_gpt/model.py:622-641) with the
reference's rounding points, and the unit-in-the-last-place measure the block tests use.  Shared by
test_block_neighbours_cpu.py (which proves the restatements on the fixtures) and test_block_neighbours_gpu.py."""
import math

import numpy as np

MANT = {"f32": 23, "bf16": 7, "f16": 10}                   # explicit mantissa bits
MIN_EXP = {"f32": -126, "bf16": -126, "f16": -14}          # exponent of the smallest normal number


def round_to(x, dt):
    """float64 array -> the nearest value of dtype `dt` (ties to even), as float64"""
    x = np.asarray(x, np.float64)
    if dt == "f32":
        return x.astype(np.float32).astype(np.float64)
    if dt == "f16":                                                        # arithmetic is float32, then one rounding to 16 bits
        with np.errstate(over="ignore"):
            return x.astype(np.float32).astype(np.float16).astype(np.float64)
    assert dt == "bf16"
    bits = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def ulp(ref, dt):
    """the unit in the last place of dtype `dt` at each value of `ref`"""
    a = np.abs(np.asarray(ref, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** MIN_EXP[dt])))
    return 2.0 ** (e - MANT[dt])


def ulp_err(got, ref, dt):
    """worst |got - ref| in units in the last place of `dt` at ref"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / ulp(ref, dt)).max())


def out_dtype(dt, wdt):
    return dt if wdt == dt else "f32"


def rmsnorm_ref(x, w, eps, add_unit_offset, dt, wdt, r=None, exact=False):
    """-> (s, y, rstd) in float64.  exact: no rounding anywhere (the mathematical function, for the gradient checks)"""
    rnd = (lambda v, d: np.asarray(v, np.float64)) if exact else round_to
    s = np.asarray(x, np.float64)
    if r is not None:
        s = rnd(s + np.asarray(r, np.float64), dt)
    rstd = 1.0 / np.sqrt((s * s).mean(-1, keepdims=True) + eps)
    n = rnd(s * rstd, dt)
    w = np.asarray(w, np.float64)
    weff = rnd(1.0 + w, wdt) if add_unit_offset else w
    return s, rnd(n * weff, out_dtype(dt, wdt)), rstd[..., 0]


_erf = np.vectorize(math.erf, otypes=[np.float64])


def act_ref(a, act):
    a = np.asarray(a, np.float64)
    if act == "silu":
        with np.errstate(over="ignore"):
            return a / (1.0 + np.exp(-a))
    return 0.5 * a * (1.0 + _erf(a / math.sqrt(2.0)))


def gated_floor(a, b, act):
    """absolute allowance beside the ulp bounds of act(a) * b.  Exact GELU is a (1 + erf(a / sqrt 2)) / 2, and every float32
    evaluation of it -- the reference's included -- forms 1 + erf near erf = -1, where float32 numbers are 2^-24 apart: two
    implementations of erf that differ by one or two of those steps differ by up to 4 * 2^-24 in the sum, however small the sum
    is, i.e. by |a| / 2 * 4 * 2^-24 in act(a) and |b| times that in the product.  Far in the negative tail the float32 result is
    exactly 0 where float64 still has 1e-8.  SiLU has no such cancellation: no allowance."""
    if act == "silu":
        return 0.0
    return 2.0 ** -23 * np.abs(np.asarray(a, np.float64) * np.asarray(b, np.float64))


def gated_interval(a, b, act, dt):
    """(lo, hi): the results round(round(act) * b) obtainable from any value of act(a) within the float32 cancellation error
    of exact GELU (|a| 2^-23, see gated_floor) around its float32 evaluation; for SiLU lo = hi.  The reference's own vector
    and scalar code paths of erf land on different sides of a 16-bit rounding boundary of act(a) where one lies that close."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    act0 = act_ref32(a64, act)
    e = 0.0 if act == "silu" else 2.0 ** -23 * np.abs(a64)
    cands = [round_to(round_to(act0 + d, dt) * b64, dt) for d in (-e, 0.0, e)]
    return np.minimum.reduce(cands), np.maximum.reduce(cands)


def act_ref32(a, act):
    """act with a float32 rounding after every operation, as the reference evaluates it on 16-bit and float32 tensors
    (x / (1 + exp(-x));  x * 0.5 * (1 + erf(x / sqrt 2))): what the 16-bit rounding of act(a) is taken from"""
    f = lambda v: round_to(v, "f32")
    a = np.asarray(a, np.float64)
    if act == "silu":
        with np.errstate(over="ignore"):
            return f(a / f(1.0 + f(np.exp(-a))))
    return f(f(a * 0.5) * f(1.0 + f(_erf(f(a * f(math.sqrt(0.5)))))))


def gated_ref(a, b, act, dt):
    """round(round(act(a)) * b)"""
    return round_to(round_to(act_ref32(a, act), dt) * np.asarray(b, np.float64), dt)


def linear_ref(x, w, bias, dt):
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return round_to(y, dt)
