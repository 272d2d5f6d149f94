"""float64 reference of the row-wise cross entropy (csrc/fastmax_ce.hip behind loss.py), the per-row and per-entry allowances
its tests hold the kernels to, and the one case table that the CPU and the GPU tests share.  numpy / torch-CPU only, no project
code: test_ce_ref_cpu.py proves the reference against torch's float64 cross_entropy and the allowances against a float32
emulation of the kernel's arithmetic and its mutants; test_loss_rows_gpu.py holds the kernels to them.

The allowances (`ce_bounds`), term by term.  u is the unit roundoff of the logits' dtype, `sub` its subnormal spacing.

  lse   = m + log s (m the row maximum, s = sum exp(z - m) >= 1) is one float32 per row:
            b_lse = (|lse| + K) 2^-22
          |lse| 2^-24 is the one rounding of m + log s; the rest is the error of log s itself, which is of the size of
          2^-24 times what went into s: the fast exp of up to 256 E-entry pieces per thread, the rescaling exp(m_piece - m)
          of every (max, sum) combine (per piece, 6 across the lanes of a wave, 3 across the waves of the 256-thread row) and
          the fast log.  None of these grows with the logits' offset, so they sit in the constant K (in units of 2^-22).
  loss  = log s + (m - z_t): m - z_t is exact or rounded once at its own size, log s as above, one float32 sum:
            b_loss = (|loss| + K) 2^-22          (the loss buffer is float32 whatever the logits' dtype)
  p     = exp(z - lse) carries the relative error
            relp = (|lse| + |z - lse| + K) 2^-22
          |lse| 2^-22 : the absolute error of lse above, and z - lse rounded once (2^-24 max(|z|, |lse|) <= 2^-23 |lse| + ...),
                        both become relative errors of p;
          |z - lse| 2^-22 : the fast exp is exp2(x log2 e) with the product rounded to float32, an absolute error of
                        |x| log2 e 2^-24 in the exponent, i.e. |x| 2^-24 relative in p, plus the rounding of x itself;
          K 2^-22 : lse's K and the error of exp2 (a unit in the last place or two).
  dz    = (p - onehot) g rounded to the dtype:
            b_dz = u |dz| + |g| (p relp + 2^-23 |p - onehot| + 2^-126) + sub
          u |dz| : the one rounding to the dtype (for float32 this and the next term are the same size);
          p relp : the error of p;  2^-23 |p - onehot| : the float32 subtraction and the one float32 product with g
          (g itself is gscale_i * grad_scale rounded once);  2^-126 |g| : the fast exp may flush float32 subnormals to zero;
          sub : half a subnormal step of the output dtype, and the slack of u |dz| being taken at the reference.

K = 16.  It may be raised only with a written reason for a term missing above, never above 64, and never fitted to what a
kernel gives; the mutants of test_ce_ref_cpu.py have to stay rejected at its value.

Unscored rows (t == ignore_index, t < 0, t >= V: loss.scored_rows) have loss 0 and dz 0 exactly; their lse is still the row's.
-inf logits (masked vocabulary) have p = 0 and dz = 0 exactly."""
import itertools
import zlib
from collections import namedtuple

import numpy as np
import torch

K = 16
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}            # unit roundoff
SUB = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}          # subnormal spacing
ITEM = {"f32": 4, "bf16": 2, "f16": 2}
IGNORE = -1                                                                  # every case's ignore_index


def piece(dt):
    """E: the entries of one 16-byte load; a 256-thread row covers 256 E entries per sweep"""
    return 16 // ITEM[dt]


def round_to(x, dt):
    """float64 array -> the nearest value of dtype `dt`, as float64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(TD[dt]).double().numpy()


def scored(t, V, ignore_index):
    t = np.asarray(t)
    return (t != ignore_index) & (t >= 0) & (t < V)


def ce_rows_ref(z, t, ignore_index, g):
    """-> loss (M,), lse (M,), p (M, V), dz (M, V) in float64.  g: (M,) d(total)/d(row loss), grad_loss_row * grad_scale."""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.int64)
    M, V = z.shape
    g = np.broadcast_to(np.asarray(g, np.float64), (M,))
    m = z.max(1)
    with np.errstate(under="ignore"):
        s = np.exp(z - m[:, None]).sum(1)
    lse = m + np.log(s)
    ok = scored(t, V, ignore_index)
    tt = np.where(ok, t, 0)
    rows = np.arange(M)
    loss = np.where(ok, np.log(s) + (m - z[rows, tt]), 0.0)
    with np.errstate(under="ignore"):
        p = np.exp(z - lse[:, None])
    onehot = np.zeros_like(z)
    onehot[rows[ok], tt[ok]] = 1.0
    dz = np.where(ok[:, None], (p - onehot) * g[:, None], 0.0)
    return loss, lse, p, dz


Bounds = namedtuple("Bounds", "b_loss b_lse b_dz")


def ce_bounds(z, t, g, dt, ignore_index=IGNORE):
    """the allowances of the module docstring around ce_rows_ref(z, t, ignore_index, g): b_loss (M,), b_lse (M,), b_dz (M, V)"""
    z = np.asarray(z, np.float64)
    M, V = z.shape
    g = np.broadcast_to(np.asarray(g, np.float64), (M,))
    loss, lse, p, dz = ce_rows_ref(z, t, ignore_index, g)
    ok = scored(t, V, ignore_index)
    onehot = np.zeros_like(z)
    rows = np.arange(M)
    onehot[rows[ok], np.asarray(t, np.int64)[ok]] = 1.0
    e22 = 2.0 ** -22
    b_lse = (np.abs(lse) + K) * e22
    b_loss = (np.abs(loss) + K) * e22
    dist = np.where(np.isfinite(z), np.abs(z - lse[:, None]), 0.0)          # -inf entries: p is 0 exactly, nothing to allow
    relp = (np.abs(lse)[:, None] + dist + K) * e22
    ga = np.abs(g)[:, None]
    b_dz = UNIT[dt] * np.abs(dz) + ga * (p * relp + 2.0 ** -23 * np.abs(p - onehot) + 2.0 ** -126) + SUB[dt]
    return Bounds(b_loss, b_lse, b_dz)


def worst_ratios(z, t, got_loss, got_lse, got_dz, ref, bounds, ignore_index=IGNORE):
    """worst error / allowance of each of loss, lse, dz; inf where something that has to be exact is not: a NaN or an
    infinity anywhere, a nonzero loss or dz entry of an unscored row, a nonzero dz at a -inf logit"""
    z = np.asarray(z, np.float64)
    loss, lse, _, dz = ref
    got_loss, got_lse, got_dz = (np.asarray(a, np.float64) for a in (got_loss, got_lse, got_dz))
    ok = scored(t, z.shape[1], ignore_index)
    out = {}
    with np.errstate(invalid="ignore"):
        out["lse"] = float((np.abs(got_lse - lse) / bounds.b_lse).max())
        r = np.abs(got_loss - loss) / bounds.b_loss
        r = np.where(~ok & (got_loss != 0), np.inf, r)
        out["loss"] = float(r.max())
        r = np.abs(got_dz - dz) / bounds.b_dz
        exact = ~ok[:, None] | np.isneginf(z)
        r = np.where(exact & (got_dz != 0), np.inf, r)
        out["dz"] = float(r.max())
    for k, a in (("loss", got_loss), ("lse", got_lse), ("dz", got_dz)):
        if not np.isfinite(a).all() or np.isnan(out[k]):
            out[k] = float("inf")
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "dt M V layout values grad")

VALUES = ("randn3", "minus100", "plus1000", "randn10", "equal", "peak_target", "peak_other", "masked", "f16_extremes")
# layouts.  Forward: how the logits lie; backward: where d(logits) goes.  `ragged` needs V % E != 0, `offset` V % E == 0.
#   contig    : logits (M, V) contiguous, output contiguous
#   ragged    : row stride rounded up to a multiple of E (16-byte rows, vector path, ragged last piece), output the same stride
#   offset    : a view one element into an aligned buffer (scalar path though V % E == 0), output aligned
#   outstride : output stride differs from the logits' (both 16-byte aligned where V allows: logits as in ragged / contig)
#   inplace   : the output is the logits buffer (logits as in ragged / contig)
LAYOUTS = ("contig", "ragged", "offset", "outstride", "inplace")
GRADS = ("none", "rows")                     # grad_loss None with grad_scale 1;  a per-row vector with grad_scale 0.125
GRAD_SCALE = {"none": 1.0, "rows": 0.125}


def mask_start(dt, V):
    """first masked column of the `masked` values"""
    return V - max(2 * piece(dt) + 3, V // 4)


def _shapes():
    for dt in ("f32", "bf16", "f16"):
        E = piece(dt)
        for V in (1, 2, E - 1, E, E + 1, 256 * E - 1, 256 * E, 256 * E + 1, 2 * 256 * E + E + 3, 4099):
            yield dt, 5, V


def _applies(dt, V, layout, values):
    E = piece(dt)
    if layout == "ragged" and V % E == 0:
        return False
    if layout == "offset" and V % E != 0:
        return False
    if values == "f16_extremes" and dt != "f16":
        return False
    if values == "masked" and mask_start(dt, V) < 8:      # room for two targets, three scattered -inf and something unmasked
        return False
    return True


CASES = [Case(dt, M, V, layout, values, grad)
         for (dt, M, V), values, grad, layout in itertools.product(_shapes(), VALUES, GRADS, LAYOUTS)
         if _applies(dt, V, layout, values)]
CASES.append(Case("bf16", 8, 32000, "contig", "randn3", "rows"))             # the production vocabulary, about 0.5 MB


def numeric_key(c):
    """cases that differ only in layout share inputs, reference and bounds"""
    return (c.dt, c.M, c.V, c.values, c.grad)


Inputs = namedtuple("Inputs", "z t ignore_index grad_rows grad_scale g")


def case_inputs(c):
    """z: (M, V) float64 holding values of dtype c.dt exactly;  t: (M,) int64;  grad_rows: (M,) float32 or None;
    g: (M,) float64 = grad_rows * grad_scale (ones where grad_rows is None)"""
    dt, M, V = c.dt, c.M, c.V
    rng = np.random.default_rng(zlib.crc32(repr(numeric_key(c)).encode()))
    base = rng.standard_normal((M, V))
    hi = V - 1
    if c.values == "masked":
        hi = mask_start(dt, V) - 1
    # targets: the last (unmasked) column, column 0, and per case one of the three kinds of unscored row; M = 8 has all three
    unscored = (IGNORE, -100, V + 7)
    t = rng.integers(0, hi + 1, size=M)
    t[0], t[1] = hi, 0
    if M >= 8:
        t[2], t[3], t[4] = unscored
    else:
        t[3] = unscored[(VALUES.index(c.values) + GRADS.index(c.grad)) % 3]
    ok = scored(t, V, IGNORE)
    rows = np.arange(M)
    if c.values in ("randn3", "masked", "f16_extremes"):
        z = base * 3
    elif c.values == "minus100":
        z = base * 3 - 100
    elif c.values == "plus1000":
        z = base * 3 + 1000
    elif c.values == "randn10":
        z = base * 10
    elif c.values == "equal":
        z = np.full((M, V), -3.25)
    else:
        z = round_to(base * 3, dt)
        col = np.where(ok, t, 0) if c.values == "peak_target" else np.where(ok, (t + 1) % V, V - 1)
        z[rows, col] = z.max(1) + 25
    if c.values == "masked":
        z[:, hi + 1:] = -np.inf
        for i in rows:
            free = np.setdiff1d(np.arange(hi + 1), t[ok])
            z[i, rng.choice(free, size=3, replace=False)] = -np.inf
    if c.values == "f16_extremes":
        keep = z[rows[ok], t[ok]].copy()
        z[rows, (7 * rows + 1) % V] = -60000.0
        z[rows, (V // 2 + rows) % V] = -60000.0
        z[rows[ok], t[ok]] = keep                                         # no target at -60000: the loss stays inside fp16
        z[0, t[0]] = 60000.0                                              # the extreme as the target,
        z[1, (t[1] + 1) % V] = 60000.0                                    # beside the target,
        z[2, t[2]] = 60000.0                                              # twice in a row
        z[2, (t[2] + V // 3) % V] = 60000.0
    z = round_to(z, dt)
    if c.grad == "none":
        return Inputs(z, t, IGNORE, None, 1.0, np.ones(M))
    gr = rng.uniform(0.5, 1.5, size=M).astype(np.float32)
    gr[M - 1], gr[1] = 0.0, -gr[1]                                         # one zero, one negative; both on scored rows
    return Inputs(z, t, IGNORE, gr, GRAD_SCALE["rows"], gr.astype(np.float64) * GRAD_SCALE["rows"])
