"""Reference, a-priori allowance and case table of the float64 fastmax kernels (csrc/fastmax_f64.hip); numpy, no device.

Reference: ``oracle.fastmax_oracle`` in numpy float64 (``fastmax_fwd_dense`` / ``fastmax_bwd_dense``; linearmax through
``normalize_qk`` and the chain rule of ``blockwise.prologue_backward_fp64``).

Allowance: a first-order bound per element, built the way tests/qlora_ref.py builds its bound -- the formula of each result
evaluated on absolute values, times (number of roundings on the longest path) * 2^-53:

  forward    (Nk + D + 16) 2^-53 (sum_j |w_ij| |v_jd| / |g_i|  +  |o_id| sum_j |w_ij| / |g_i|)
  g          (Nk + D + 16) 2^-53  sum_j |w_ij|
  gradients  (Nq + Nk + 2 D + 32) 2^-53 times the absolute-value versions of
             c = rowdot(dO, o), dP = (dO V^T - c) / g, dS = f'(S) mask dP, dq = a dS K, dk = a dS^T Q, dv = (W / g)^T dO

A test allows TWICE the bound: the float64 reference carries the same error.  The bound is a condition on the inputs, not a
measurement of the kernels: tests/test_fp64_cpu.py checks that with the input recipe below it stays under 2^-34 of every
16-row block's largest |reference| (fp32 rounding is 2^-24: a looser allowance would begin to hide float intermediates) and
that a float32 intermediate anywhere in the chain falls outside it.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import fastmax_oracle as orc

U = 2.0 ** -53

# masked: (B, H, N, D); unmasked: (B, H, Nq, Nk, D); every shape with p = 1 and p = 2
MASKED_SHAPES = [(1, 2, 1, 8), (1, 2, 15, 4), (1, 2, 16, 4), (1, 2, 17, 1), (1, 2, 33, 3), (1, 2, 33, 6), (2, 4, 130, 64),
                 (1, 2, 33, 132), (1, 2, 33, 256), (1, 8, 520, 64)]
UNMASKED_SHAPES = [(1, 2, 5, 37, 8), (1, 2, 64, 300, 64), (1, 2, 1, 33, 6)]


class Case(NamedTuple):
    mask: bool
    p: int
    B: int
    H: int
    Nq: int
    Nk: int
    D: int

    @property
    def id(self):
        return f"{'masked' if self.mask else 'unmasked'}-p{self.p}-{self.B}x{self.H}x{self.Nq}x{self.Nk}x{self.D}"


CASES = ([Case(True, p, B, H, N, N, D) for (B, H, N, D) in MASKED_SHAPES for p in (1, 2)] +
         [Case(False, p, B, H, Nq, Nk, D) for (B, H, Nq, Nk, D) in UNMASKED_SHAPES for p in (1, 2)])
CASE_IDS = [c.id for c in CASES]
NAMES = ("o", "g", "dq", "dk", "dv")


def inputs(c: Case, seed=0):
    """seeded randn q, k, v, grad_o (float64); normalize_term stays at its default 8 sqrt(D)"""
    rng = np.random.default_rng(1000 + seed)
    q = rng.standard_normal((c.B, c.H, c.Nq, c.D))
    k = rng.standard_normal((c.B, c.H, c.Nk, c.D))
    v = rng.standard_normal((c.B, c.H, c.Nk, c.D))
    go = rng.standard_normal((c.B, c.H, c.Nq, c.D))
    return q, k, v, go


def _f(s, p):
    return 1.0 + s if p == 1 else 1.0 + s + 0.5 * s * s


def _fp(s, p):
    return np.ones_like(s) if p == 1 else 1.0 + s


def weights(q, k, mask, nt, p):
    """(w, f'(s) mask): the (B,H,Nq,Nk) weights f(s) mask and the masked derivative"""
    s = np.einsum("bhid,bhjd->bhij", q, k) / nt
    w, wp = _f(s, p), _fp(s, p)
    if mask:
        tri = np.tril(np.ones(s.shape[-2:]))
        w, wp = w * tri, wp * tri
    return w, wp


def bounds(q, k, v, go, o, g, mask, nt, p, magnitudes=False):
    """dict name -> the first-order bound per element (NOT yet doubled); with ``magnitudes`` the absolute-value evaluations
    themselves (bound = depth 2^-53 magnitude): the size of the terms a result is summed from, which stays positive where
    the result itself cancels to exactly zero"""
    Nq, Nk, D = q.shape[2], k.shape[2], q.shape[3]
    w, wp = weights(q, k, mask, nt, p)
    aw, awp, ag = np.abs(w), np.abs(wp), np.abs(g)
    sw = aw.sum(-1)
    fwd = 1.0 if magnitudes else (Nk + D + 16) * U
    out = {"o": fwd * (np.einsum("bhij,bhjd->bhid", aw, np.abs(v)) / ag[..., None] + np.abs(o) * (sw / ag)[..., None]),
           "g": fwd * sw}
    bwd = 1.0 if magnitudes else (Nq + Nk + 2 * D + 32) * U
    cabs = (np.abs(go) * np.abs(o)).sum(-1)
    dpabs = (np.einsum("bhid,bhjd->bhij", np.abs(go), np.abs(v)) + cabs[..., None]) / ag[..., None]
    dsabs = dpabs * awp
    out["dq"] = bwd * np.einsum("bhij,bhjd->bhid", dsabs, np.abs(k)) / nt
    out["dk"] = bwd * np.einsum("bhij,bhid->bhjd", dsabs, np.abs(q)) / nt
    out["dv"] = bwd * np.einsum("bhij,bhid->bhjd", aw / ag[..., None], np.abs(go))
    return out


class Reference(NamedTuple):
    q: np.ndarray
    k: np.ndarray
    v: np.ndarray
    go: np.ndarray
    nt: float
    ref: dict          # name -> float64 reference
    allow: dict        # name -> allowance per element = 2 x bound
    mag: dict          # name -> the absolute-value evaluation behind the bound


@functools.lru_cache(maxsize=None)
def reference(c: Case, g_const=None) -> Reference:
    """the case's inputs, oracle results and allowances, computed once and shared (treat the arrays as read-only);
    g_const: the unmasked denominator's constant term, default N_q (fastmax.py:269-271)"""
    q, k, v, go = inputs(c)
    nt = orc.effective_normalize_term(c.D)
    o, g = orc.fastmax_fwd_dense(q, k, v, mask=c.mask, nt=nt, p=c.p, g_const=g_const)
    dq, dk, dv = orc.fastmax_bwd_dense(q, k, v, go, mask=c.mask, nt=nt, p=c.p, g_const=g_const)
    ref = dict(o=o, g=g, dq=dq, dk=dk, dv=dv)
    allow = {n: 2.0 * b for n, b in bounds(q, k, v, go, o, g, c.mask, nt, c.p).items()}
    mag = bounds(q, k, v, go, o, g, c.mask, nt, c.p, magnitudes=True)
    for a in (q, k, v, go, *ref.values(), *allow.values(), *mag.values()):
        a.setflags(write=False)
    return Reference(q, k, v, go, nt, ref, allow, mag)


def outside(got, ref, allow):
    """number of elements of ``got`` further from ``ref`` than ``allow``, and the worst |err| / allow (NaN counts as outside)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= allow)
    ratio = np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))
    return int(bad.sum()), float(np.nan_to_num(ratio, nan=np.inf).max())


def assert_inside(what, got, ref, allow):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    n, worst = outside(got, ref, allow)
    assert n == 0, f"{what}: {n} of {ref.size} elements outside the allowance, worst |err| / allowance = {worst:.3g}"
    return worst


def abi_scale(nt):
    """1/nt as the C ABI carries it for a float64 problem: float(1/nt) + float(1/nt - float(1/nt)), about 48 bits"""
    a = float(np.float32(1.0 / nt))
    return a + float(np.float32(1.0 / nt - a))


# ---- linearmax: the prologue in front of the same function with nt = 1 ------------------------------------------------------
# (mask, p, (B, H, Nq, Nk, D)); inputs(Case, seed=1)
LINEARMAX_CASES = [(True, 1, (1, 2, 33, 33, 6)), (True, 2, (2, 4, 130, 130, 64)), (True, 1, (1, 2, 33, 33, 132)),
                   (False, 1, (1, 2, 5, 37, 8)), (False, 2, (1, 2, 64, 300, 64))]


def linearmax_reference(q, k, v, go, p, mask):
    """float64 linearmax (fastmax_hack.py:5-60): -> (ref dict o, dq, dk, dv wrt the RAW q, k; allow dict).  The allowance is that
    of the attention on the normalised q, k, pushed through the prologue's chain rule on absolute values (the prologue adds
    O(D) roundings to q, k of relative size 2^-53 each, which the depth's + 16 / + 32 cover)."""
    from blockwise import prologue_backward_fp64
    qn, kn = orc.normalize_qk(q, k)
    Nk = k.shape[2]
    pe, gc = (p, None) if mask else (1, Nk)
    o, g = orc.fastmax_fwd_dense(qn, kn, v, mask=mask, nt=1.0, p=pe, g_const=gc)
    assert np.abs(o - orc.linearmax_fwd(q, k, v, p=p, mask=mask)).max() <= 1e-12 * np.abs(o).max()
    dqn, dkn, dv = orc.fastmax_bwd_dense(qn, kn, v, go, mask=mask, nt=1.0, p=pe, g_const=gc)
    b = bounds(qn, kn, v, go, o, g, mask, 1.0, pe)
    B, H = q.shape[:2]
    dq, dk = np.empty_like(q), np.empty_like(k)
    for bi in range(B):
        for h in range(H):
            dq[bi, h] = prologue_backward_fp64(q[bi, h], dqn[bi, h].copy())
            dk[bi, h] = prologue_backward_fp64(k[bi, h], dkn[bi, h].copy())

    def through_prologue(x, bx, gy):
        # |d/dx| of y = xc / M on absolute values: every term of prologue_backward_fp64 taken positive, plus the prologue's
        # own roundings on the gradient it hands back
        xc = x - x.mean(-1, keepdims=True)
        nrm = np.sqrt((xc * xc).sum(-1))
        M = nrm.max(-1)[..., None, None]
        base = bx / M
        extra = (bx * np.abs(xc)).sum((-1, -2), keepdims=True) / (M * M) * np.abs(xc) / M
        depth = (x.shape[-1] + x.shape[-2] + 16) * U
        extra = extra + depth * (np.abs(gy) * np.abs(xc)).sum((-1, -2), keepdims=True) / (M * M) * np.abs(xc) / M
        t = base + depth * np.abs(gy) / M + np.where(nrm[..., None] == nrm.max(-1)[..., None, None], extra, 0.0)
        return t + t.mean(-1, keepdims=True)

    ref = dict(o=o, dq=dq, dk=dk, dv=dv)
    allow = dict(o=2.0 * b["o"], dq=2.0 * through_prologue(q, b["dq"], dqn), dk=2.0 * through_prologue(k, b["dk"], dkn), dv=2.0 * b["dv"])
    return ref, allow


# ---- the kernels' tile order, restated: 16-key tiles, four-key steps, optional float32 plants -----------------------------
PLANTS = ("score", "f", "denominator", "rowdot")


def _r32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def tiled(q, k, v, go, mask, nt, p, g_const=None, plant=None):
    """(o, g, dq, dk, dv) of (B,H,N,D) float64 inputs in the order the kernels sum in: the other sequence in 16-row tiles, inside a
    tile the four lane groups' partial sums (rows r4, r4 + 4, r4 + 8, r4 + 12) kept apart for the denominator, products over D
    and over a tile's rows in steps of four.  ``plant``: one intermediate rounded to float32 -- what a kernel with a float
    intermediate there would compute."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    a = 1.0 / nt
    gadd = 0.0 if mask else float(Nq if g_const is None else g_const) - Nk

    def steps4(x, y):
        """x @ y with the contraction taken four at a time, in order"""
        acc = np.zeros(x.shape[:-1] + y.shape[-1:])
        for s0 in range(0, x.shape[-1], 4):
            acc = acc + x[..., s0:s0 + 4] @ y[..., s0:s0 + 4, :]
        return acc

    def score(qt, kt):
        s = a * steps4(qt, np.swapaxes(kt, -1, -2))
        return _r32(s) if plant == "score" else s

    o, g = np.empty_like(q), np.empty((B, H, Nq))
    tiles_q, tiles_k = range(0, Nq, 16), range(0, Nk, 16)
    for i0 in tiles_q:
        i1 = min(Nq, i0 + 16)
        acc, lanes = np.zeros((B, H, i1 - i0, D)), np.zeros((B, H, i1 - i0, 4))
        for j0 in tiles_k:
            if mask and j0 > i0:
                break
            j1 = min(Nk, j0 + 16)
            w = _f(score(q[:, :, i0:i1], k[:, :, j0:j1]), p)
            if mask:
                w = w * (np.arange(j0, j1)[None, :] <= np.arange(i0, i1)[:, None])
            if plant == "f":
                w = _r32(w)
            for r in range(j1 - j0):
                lanes[..., r % 4] += w[..., r]
            acc = acc + steps4(w, v[:, :, j0:j1])
        gt = ((lanes[..., 0] + lanes[..., 1]) + (lanes[..., 2] + lanes[..., 3])) + gadd
        if plant == "denominator":
            gt = _r32(gt)
        g[:, :, i0:i1] = gt
        o[:, :, i0:i1] = acc / gt[..., None]

    c = np.zeros((B, H, Nq))
    for d in range(D):
        c = c + go[..., d] * o[..., d]
    if plant == "rowdot":
        c = _r32(c)
    dq, dk, dv = np.empty_like(q), np.empty_like(k), np.empty_like(v)
    for i0 in tiles_q:
        i1 = min(Nq, i0 + 16)
        acc = np.zeros((B, H, i1 - i0, D))
        for j0 in tiles_k:
            if mask and j0 > i0:
                break
            j1 = min(Nk, j0 + 16)
            s = score(q[:, :, i0:i1], k[:, :, j0:j1])
            dp = steps4(go[:, :, i0:i1], np.swapaxes(v[:, :, j0:j1], -1, -2))
            ds = _fp(s, p) * ((dp - c[:, :, i0:i1, None]) / g[:, :, i0:i1, None])
            if mask:
                ds = ds * (np.arange(j0, j1)[None, :] <= np.arange(i0, i1)[:, None])
            acc = acc + steps4(ds, k[:, :, j0:j1])
        dq[:, :, i0:i1] = a * acc
    for j0 in tiles_k:
        j1 = min(Nk, j0 + 16)
        acck, accv = np.zeros((B, H, j1 - j0, D)), np.zeros((B, H, j1 - j0, D))
        for i0 in tiles_q:
            i1 = min(Nq, i0 + 16)
            if mask and i1 <= j0:
                continue
            s = score(q[:, :, i0:i1], k[:, :, j0:j1])
            dp = steps4(go[:, :, i0:i1], np.swapaxes(v[:, :, j0:j1], -1, -2))
            w = _f(s, p)
            if plant == "f":
                w = _r32(w)
            w = w / g[:, :, i0:i1, None]
            ds = _fp(s, p) * ((dp - c[:, :, i0:i1, None]) / g[:, :, i0:i1, None])
            if mask:
                tri = np.arange(j0, j1)[None, :] <= np.arange(i0, i1)[:, None]
                w, ds = w * tri, ds * tri
            acck = acck + steps4(np.swapaxes(ds, -1, -2), q[:, :, i0:i1])
            accv = accv + steps4(np.swapaxes(w, -1, -2), go[:, :, i0:i1])
        dk[:, :, j0:j1] = a * acck
        dv[:, :, j0:j1] = accv
    return dict(o=o, g=g, dq=dq, dk=dk, dv=dv)
