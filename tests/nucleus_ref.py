"""numpy restatement of top-p (nucleus) sampling (include/fastmax_hip_nucleus.h) on top of next_token_ref.py, float64 unless
stated: the order of a row, the candidates the top-k leaves, the cumulative mass C(j), the exact length n of the nucleus, the band
of lengths an evaluation of C with error eps may return, and the library's fixed-point evaluation restated with numpy's float32
exp.  Shared by test_nucleus_cpu.py and test_nucleus_gpu.py; nothing here touches the library."""
import math

import numpy as np

import next_token_ref as ref

MASS_BITS = 40          # q_i = floor(w_i 2^40)
MAX_V = 1 << 22


def epsilon(V):
    """The bound of the header on |C(j) as the library evaluates it - C(j)|, for a row of V entries.

    w_i = expf(x_i), x_i = fl(fl(logit_i - m) / T): two roundings, |dx_i| <= 2^-23 |x_i|, so w_i is off by the factor
    exp(dx_i) = 1 + 2^-23 |x_i|; expf itself by at most 2 ulp = 2^-22 relative (the device library documents 1 ulp); the
    truncation to a multiple of 2^-40 by less than 2^-40 absolute, where the total W >= 1 (the maximum has w = 1).  A partial sum
    S(j) = sum_{i <= j} w_i is therefore off by at most sum_i w_i (2^-23 |x_i| + 2^-22) + V 2^-40, and relative to W:
        sum_i P_i |x_i| 2^-23 + 2^-22 + V 2^-40 <= 2^-23 ln V + 2^-22 + V 2^-40,
    because x_i = ln w_i = ln P_i + ln W with W >= 1, so |x_i| <= -ln P_i and sum_i P_i (-ln P_i) is an entropy, at most ln V.
    C(j) = S(j) / W has that error in its numerator and, times C(j) <= 1, in its denominator: the factor 2.  The target
    ceil(total * top_p) adds 2^-40 / W and 2^-52, which 1.01 covers."""
    return 1.01 * 2.0 * (2.0 ** -23 * math.log(max(V, 2)) + 2.0 ** -22 + V * 2.0 ** -MASS_BITS)


def order(row):
    """indices of a row by key descending, index ascending among equal keys"""
    keys = ref.order_key(row).astype(np.int64)
    return np.lexsort((np.arange(len(keys)), -keys))


def cumulative(row, top_k, temperature):
    """-> (idx, C): the candidates in the order (the first top_k of it; all for None) and C[j - 1] = C(j), j = 1 .. |K|"""
    row = np.asarray(row, dtype=np.float32)
    idx = order(row)
    if top_k is not None:
        idx = idx[:min(int(top_k), len(idx))]
    z = row[idx].astype(np.float64) / float(np.float32(temperature))
    w = np.exp(z - z.max())
    return idx, np.cumsum(w) / w.sum()


def length(C, top_p):
    """n = min{ j >= 1 : C(j) >= top_p }, top_p as the float32 the library receives (C(|K|) may round below 1: then all)"""
    hit = np.nonzero(C >= float(np.float32(top_p)))[0]
    return int(hit[0]) + 1 if len(hit) else len(C)


def band(C, top_p, eps):
    """(lo, hi): every n with C(n) >= top_p - eps and C(n - 1) < top_p + eps, an interval since C does not decrease"""
    p = float(np.float32(top_p))
    ok_hi = np.concatenate(([0.0], C[:-1])) < p + eps           # C(n - 1) < p + eps, n = 1 ..
    ok_lo = C >= p - eps
    ok_lo[-1] = True                                            # all of K is what is left when nothing reaches top_p - eps
    n = np.nonzero(ok_lo & ok_hi)[0] + 1
    return int(n[0]), int(n[-1])


def keep_mask(logits, top_k, top_p, temperature):
    """bool (B, V): the exact nucleus of every row; top_p None or 1.0, or temperature 0: the top-k's mask"""
    logits = np.asarray(logits, dtype=np.float32)
    if top_p is None or float(top_p) == 1.0 or temperature == 0:
        return ref.keep_mask(logits, top_k)
    out = np.zeros(logits.shape, dtype=bool)
    for b, row in enumerate(logits):
        idx, C = cumulative(row, top_k, temperature)
        out[b, idx[:length(C, top_p)]] = True
    return out


def prefix_length(mask_row, idx):
    """the n for which mask_row is exactly the first n entries of idx (the candidates in the order), or None"""
    n = int(mask_row.sum())
    want = np.zeros(len(mask_row), dtype=bool)
    want[idx[:n]] = True
    return n if n <= len(idx) and np.array_equal(mask_row, want) else None


def fixed_point_length(row, top_k, top_p, temperature):
    """the library's evaluation with numpy's float32 arithmetic: w = exp32((logit - m) / T), q = floor(w 2^40) summed as
    integers, needed = ceil(total * top_p) in float64 clamped to [1, total] -> n"""
    row = np.asarray(row, dtype=np.float32)
    idx = order(row)
    if top_k is not None:
        idx = idx[:min(int(top_k), len(idx))]
    x = (row[idx] - row[idx[0]]) / np.float32(temperature)
    assert x.dtype == np.float32
    w = np.minimum(np.exp(x), np.float32(1.0))
    q = [int(math.floor(float(v) * 2.0 ** MASS_BITS)) for v in w]          # exact: float32 times a power of two, in float64
    total = sum(q)
    want = math.ceil(float(total) * float(np.float32(top_p)))
    needed = max(1, total if want >= float(total) else int(want))
    run = 0
    for n, v in enumerate(q, 1):
        run += v
        if run >= needed:
            return n
    raise AssertionError("the total does not reach the target")


def sample_in(mask, logits, temperature, seed, draw):
    """next_token_ref.sample over a given kept set -> (tokens, gap to the runner-up inside it)"""
    s = np.where(mask, ref.scores(logits, temperature, seed, draw), -np.inf)
    tokens = np.argmax(s, axis=1)
    if s.shape[1] == 1:
        return tokens, np.full(s.shape[0], np.inf)
    top2 = np.partition(s, s.shape[1] - 2, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gap = top2[:, 1] - top2[:, 0]
    return tokens, np.where(np.isnan(gap), 0.0, gap)


def rows(V, B=3):
    """test_next_token_gpu.test_keep_mask_on_random_rows' rows without its -inf column and its rows of zeros: from
    default_rng(V).normal(0, 3), B fine rows, then B rounded to multiples of 0.5 (many ties, +0.0 and -0.0 among them)"""
    g = np.random.default_rng(V)
    fine = g.normal(0, 3, (B, V))
    coarse = np.round(g.normal(0, 3, (B, V)) * 2) / 2
    return np.concatenate([fine, coarse]).astype(np.float32)


def tie_rows(V):
    """designed ties: few distinct values, V in {5, 8, 12}; no C(j) comes within 1e-3 of 0.3, 0.6 or 0.85 at temperature 1"""
    base = {5: [1.0, 1.0, 0.0, 1.0, 0.0], 8: [2.0, 0.0, 2.0, 0.0, -0.0, 2.0, 0.0, 1.0],
            12: [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -1.0, 0.5, 0.5, 0.5, 0.5, 0.5]}[V]
    a = np.array(base, dtype=np.float32)
    flat = np.full(V, -2.5, dtype=np.float32)                   # one value everywhere: C(j) = j / V
    if V == 5:
        flat[3] = -2.0                                          # j / 5 would meet 0.6
    return np.stack([a, a[::-1].copy(), flat, np.roll(a, 2)])
