"""Row-block error metric and float64 linear-time references for the long-sequence parity tests.

Why per block: ``conftest.rel_err`` divides by the largest |ref| of the whole tensor.  In causal attention row i is an
average over i value rows and shrinks like 1/sqrt(i), so at 16 k tokens that scale is set by the first rows and the second
half of the output -- where the linear-time kernels carry their D x D prefix state across chunks and sequence-split
segments -- can be wrong by a dropped chunk and still pass.  ``block_rel_err`` scales each row block by its own magnitude.

The references work on one head at a time, (N, D) arrays, in numpy float64 on the CPU:
  * causal p = 1: chunked scan with a carried state, linear in N (16 k x 128 in well under a second);
  * p = 2 and unmasked shapes: the dense operator evaluated over one block of query rows at a time.
They are checked against the dense oracle (``oracle.fastmax_oracle``) in tests/test_blockwise_cpu.py.
"""
import numpy as np

from oracle import fastmax_oracle as orc


# --------------------------------------------------------------------------------------
# metric
# --------------------------------------------------------------------------------------
def block_rel_err(x, ref, block=64, axis=-2, floor=1e-3):
    """Error per row block along ``axis``: max|x - ref| over the block / max(max|ref| over the block, floor * max|ref|).

    The floor only guards blocks that are exactly zero (dq of a one-token prefix).  Every block <= tol implies
    ``rel_err(x, ref) <= tol``: a block's scale never exceeds the tensor's.  Returns a float64 array, one entry per block.
    """
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    ref = np.moveaxis(np.asarray(ref, dtype=np.float64), axis, 0)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    n = ref.shape[0]
    nb = (n + block - 1) // block
    pad = nb * block - n
    err = np.abs(x - ref).reshape(n, -1)
    mag = np.abs(ref).reshape(n, -1)
    if pad:
        err = np.concatenate([err, np.zeros((pad, err.shape[1]))])
        mag = np.concatenate([mag, np.zeros((pad, mag.shape[1]))])
    err = err.reshape(nb, -1).max(1)
    mag = mag.reshape(nb, -1).max(1)
    return err / np.maximum(mag, floor * max(float(mag.max()), np.finfo(np.float64).tiny))


def worst_block(x, ref, block=64, axis=-2, floor=1e-3):
    """(error, row0, row1, scale) of the worst row block"""
    e = block_rel_err(x, ref, block, axis, floor)
    b = int(e.argmax())
    r = np.moveaxis(np.asarray(ref, dtype=np.float64), axis, 0)
    r0, r1 = b * block, min(r.shape[0], (b + 1) * block)
    return float(e[b]), r0, r1, float(np.abs(r[r0:r1]).max())


def assert_blockwise(x, ref, tol, what="", block=64, axis=-2, floor=1e-3):
    err, r0, r1, scale = worst_block(x, ref, block, axis, floor)
    assert err <= tol, f"{what}: rows {r0}:{r1} err {err:.3e} > {tol:.1e} (block max|ref| {scale:.3e})"
    return err


# --------------------------------------------------------------------------------------
# causal first order: linear-time scans (one head, (N, D))
# --------------------------------------------------------------------------------------
def p1_causal_fwd(q, k, v, nt, chunk=256, dtype=np.float64):
    """o_i = sum_{j<=i} (1 + q_i.k_j / nt) v_j / g_i,  g_i = sum_{j<=i} (1 + q_i.k_j / nt).  Returns (o, g).

    With V' = [V | 1]: a dense causal product inside each chunk plus the carried state S1 = sum v'_j, S2 = sum k_j v'_j^T
    of the earlier chunks."""
    q, k, v = (np.asarray(t, dtype=dtype) for t in (q, k, v))
    N, D = q.shape
    a = dtype(1.0) / dtype(nt)
    vp = np.concatenate([v, np.ones((N, 1), dtype)], 1)
    S1 = np.zeros(D + 1, dtype)
    S2 = np.zeros((D, D + 1), dtype)
    out = np.empty((N, D + 1), dtype)
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        qc, kc, vc = q[c0:c1], k[c0:c1], vp[c0:c1]
        P = np.tril(1 + a * (qc @ kc.T))
        out[c0:c1] = P @ vc + S1 + a * (qc @ S2)
        S1 = S1 + vc.sum(0)
        S2 = S2 + kc.T @ vc
    g = out[:, D].copy()
    return out[:, :D] / g[:, None], g


def p1_causal_bwd(q, k, v, go, nt, chunk=256, dtype=np.float64):
    """(dq, dk, dv) of the causal first-order operator.  With Gh_i = [G_i | -G_i.o_i] / g_i and v'_j = [v_j | 1]:
        dq_i = a sum_{j<=i} (Gh_i.v'_j) k_j     (forward scan, state S2 = sum k_j v'_j^T)
        dk_j = a sum_{i>=j} (Gh_i.v'_j) q_i     (reverse scan, state R2 = sum q_i Gh_i^T)
        dv_j = sum_{i>=j} (1 + a q_i.k_j) Gh_i[:D]   (reverse scan, states R1 = sum Gh_i and R2)"""
    q, k, v, go = (np.asarray(t, dtype=dtype) for t in (q, k, v, go))
    N, D = q.shape
    a = dtype(1.0) / dtype(nt)
    o, g = p1_causal_fwd(q, k, v, nt, chunk, dtype)
    Gh = np.concatenate([go, -(go * o).sum(1, keepdims=True)], 1) / g[:, None]
    vp = np.concatenate([v, np.ones((N, 1), dtype)], 1)
    dq, dk, dvp = np.empty((N, D), dtype), np.empty((N, D), dtype), np.empty((N, D + 1), dtype)
    S2 = np.zeros((D, D + 1), dtype)
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        kc, vc, gc = k[c0:c1], vp[c0:c1], Gh[c0:c1]
        dq[c0:c1] = a * (np.tril(gc @ vc.T) @ kc + gc @ S2.T)
        S2 = S2 + kc.T @ vc
    R1 = np.zeros(D + 1, dtype)
    R2 = np.zeros((D, D + 1), dtype)
    for c0 in reversed(range(0, N, chunk)):
        c1 = min(N, c0 + chunk)
        qc, kc, vc, gc = q[c0:c1], k[c0:c1], vp[c0:c1], Gh[c0:c1]
        dk[c0:c1] = a * (np.tril(gc @ vc.T).T @ qc + vc @ R2.T)
        dvp[c0:c1] = np.tril(1 + a * (qc @ kc.T)).T @ gc + R1 + a * (kc @ R2)
        R1 = R1 + gc.sum(0)
        R2 = R2 + qc.T @ gc
    return dq, dk, dvp[:, :D].copy()


# --------------------------------------------------------------------------------------
# linearmax: the prologue (fastmax_hack.py:38-43) around the first-order scan with nt = 1
# --------------------------------------------------------------------------------------
def prologue_backward_fp64(x, gy):
    """d/dx of y = (x - mean_D x) / max_n ||x_n - mean_D x_n|| (fastmax.py:326-334), one head (N,D), fp64: the chain rule
    through the oracle's normalize -- only the row that attains the max-norm carries the dL/dM term."""
    xc = x - x.mean(-1, keepdims=True)
    nrm = np.sqrt((xc * xc).sum(-1))
    ns = int(nrm.argmax())
    M = nrm[ns]
    gxc = gy / M
    gxc[ns] -= (gy * xc).sum() / (M * M) * xc[ns] / M
    return gxc - gxc.mean(-1, keepdims=True)


def linearmax_fwd(q, k, v, chunk=256):
    """masked first-order linearmax of one head -> (o, g)"""
    qn, kn = orc.normalize_qk(q, k)
    return p1_causal_fwd(qn, kn, v, 1.0, chunk)


def linearmax_bwd(q, k, v, go, chunk=256):
    """gradients of masked first-order linearmax wrt the raw q, k, v of one head"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    qn, kn = orc.normalize_qk(q, k)
    dqn, dkn, dv = p1_causal_bwd(qn, kn, v, go, 1.0, chunk)
    return prologue_backward_fp64(q, dqn), prologue_backward_fp64(k, dkn), dv


# --------------------------------------------------------------------------------------
# p = 2 and unmasked: the dense operator, one block of query rows at a time
# --------------------------------------------------------------------------------------
def dense_rows(q, k, v, go=None, nt=None, p=1, mask=True, g_const=None, rows=512):
    """The function of ``fastmax_fwd_dense`` / ``fastmax_bwd_dense`` (same f, f', constant term g_const, default N_q),
    evaluated over ``rows`` query rows at a time so that only a (rows, N_k) score block is ever held.
    Returns (o, g) without ``go``, else (o, g, dq, dk, dv)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    Nq, D = q.shape
    Nk = k.shape[0]
    nt = orc.effective_normalize_term(D) if nt is None else nt
    gc = Nq if g_const is None else g_const
    o, g = np.empty((Nq, v.shape[1])), np.empty(Nq)
    if go is not None:
        go = np.asarray(go, np.float64)
        dq, dk, dv = np.empty_like(q), np.zeros_like(k), np.zeros_like(v)
    for r0 in range(0, Nq, rows):
        r1 = min(Nq, r0 + rows)
        n = r1 if mask else Nk                              # keys any of these rows can see
        s = q[r0:r1] @ k[:n].T / nt
        P = orc._f(s, p)
        if mask:
            P = P * (np.arange(n)[None, :] <= np.arange(r0, r1)[:, None])
            gb = P.sum(1)
        else:
            gb = P.sum(1) - Nk + gc
        ob = P @ v[:n] / gb[:, None]
        o[r0:r1], g[r0:r1] = ob, gb
        if go is None:
            continue
        G = go[r0:r1]
        dS = (G @ v[:n].T - (G * ob).sum(1, keepdims=True)) / gb[:, None] * orc._fprime(s, p)
        if mask:
            dS = dS * (np.arange(n)[None, :] <= np.arange(r0, r1)[:, None])
        dq[r0:r1] = dS @ k[:n] / nt
        dk[:n] += dS.T @ q[r0:r1] / nt
        dv[:n] += (P / gb[:, None]).T @ G
    return (o, g) if go is None else (o, g, dq, dk, dv)


# --------------------------------------------------------------------------------------
# the tile kernels: a rounded model of a correct kernel (calibration) and exact results with one tile fault (power)
# --------------------------------------------------------------------------------------
def _rounder(dtype):
    """float64 array -> the same values rounded to ``dtype`` ("bf16" / "f16"), back in float64"""
    import torch
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    return lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(tdt).double().numpy()


def tile_model(q, k, v, go, nt, p, mask, dtype, g_const=None, tile_forward=True, unit=None):
    """(o, g, dq, dk, dv) of one head as a correct tile kernel of ``dtype`` ("f32", "bf16", "f16") delivers them.

    16-bit: float64 arithmetic (the kernels accumulate in fp32, far below the roundings kept here) with the roundings the
    sources name: q, k, v, go exact in ``dtype``; P = f(s) rounded to ``dtype`` before P @ V and P^T @ gt, while g sums the
    unrounded P (poly, fastmax_quad32_mfma.hip:138-165), so that o_0 = v_0 rd(P_00) / P_00 and not v_0; masked o stored in
    ``dtype`` (unmasked: float32) and read back by the backward for c_i = G_i . o_i (bwd_prep_kernel,
    fastmax_quad_mfma_bwd.hip:60); gt_i = G_i / g_i in ``dtype`` (fastmax_quad_mfma_bwd.hip:65, fastmax_quad32_bwd.hip:15);
    dS rounded to ``dtype`` before dS @ K and dS^T @ Q (pack_tile, fastmax_quad32_bwd.hip:55-70); dq, dk, dv stored in
    ``dtype``.  The first rows of dq and dk feel the two roundings of o most: dS_ij = G_i . (v_j - o_i) / g_i is a difference
    of nearly equal terms while o_i is still an average of a few value rows.
    ``tile_forward=False``: the forward is a scan or a vector-ALU kernel, whose o is the exact quotient rounded once.
    ``unit`` (default: what the 32-row tiles do, launch_quad32_u, fastmax_quad32_mfma.hip:402-408, and launch_bwd32,
    fastmax_quad32_bwd.hip:632-637): single-part bf16 operands are scaled by a = 1 / nt on load only when a is a power of
    two.  Otherwise the score chain carries u = 1/a + q . k and what is rounded to bf16 is the unscaled polynomial,
    P / e2 = u u + 1/a^2 (p = 2, e2 = a^2 / 2) or u (p = 1, e2 = a) (fastmax_quad32_mfma.hip:130-165), and the unscaled
    dS / e1 = U u (p = 2, e1 = a) (fastmax_quad32_bwd.hip:177-186); e1, e2 are applied in fp32 afterwards.  The same
    relative rounding of another number: rd(P_00 / e2) e2 / P_00 can lie on the other side of 1 than rd(P_00) / P_00, and
    then o_0 = rd(v_0 rd(P_00) / P_00) is one bf16 step away from v_0 in every element instead of equal to it.
    f32: the same operator evaluated in numpy float32 with no further rounding.  ``g_const`` as in ``dense_rows``."""
    f32 = dtype == "f32"
    if unit is None:
        unit = dtype != "bf16" or float(np.frexp(np.float32(1.0 / nt))[0]) == 0.5
    e2 = 1.0 if unit else ((1.0 / nt) if p == 1 else 0.5 / (nt * nt))
    e1 = 1.0 if unit or p == 1 else 1.0 / nt
    wt = np.float32 if f32 else np.float64
    rd = (lambda x: x) if f32 else _rounder(dtype)
    q, k, v, go = (np.asarray(t, wt) for t in (q, k, v, go))
    Nq, Nk = q.shape[0], k.shape[0]
    a = wt(1.0 / nt)
    s = (q @ k.T) * a
    keep = (np.arange(Nk)[None, :] <= np.arange(Nq)[:, None]) if mask else np.ones((Nq, Nk), bool)
    P = np.where(keep, orc._f(s, p), wt(0))
    g = P.sum(1) if mask else P.sum(1) - wt(Nk) + wt(Nq if g_const is None else g_const)
    Pr = rd(P / e2) * e2
    o = ((Pr if tile_forward else P) @ v) / g[:, None]
    o = rd(o) if mask else o.astype(np.float32).astype(wt)
    w = wt(1) / g
    gt = rd(go * w[:, None])
    cw = (go * o).sum(1) * w
    dS = rd(np.where(keep, (gt @ v.T - cw[:, None]) * orc._fprime(s, p), wt(0)) / e1) * e1
    dq, dk, dv = rd((dS @ k) * a), rd((dS.T @ q) * a), rd(Pr.T @ gt)
    return tuple(np.asarray(t, np.float64) for t in (o, g, dq, dk, dv))


TILE_FAULTS = ("last_key_tile_dk_zero", "last_key_tile_dv_zero", "last_query_tile_skips_first_key_tile",
               "mask_plus_one_in_last_tile", "first_key_tile_twice_in_last_query_tile", "low_part_lost_in_last_key_tile")
FAULT_TENSOR = dict(zip(TILE_FAULTS, ("dk", "dv", "o", "o", "dq", "dv")))


def emulate_tiles(q, k, v, go, nt, p, mask, tile, fault=None, g_const=None):
    """Exact float64 (o, g, dq, dk, dv) of one head, computed the way a kernel with ``tile``-row tiles would, with one
    fault; the last tile is the ragged one, rows ``tile * ((N - 1) // tile)`` to N.  ``fault``:
      "last_key_tile_dk_zero", "last_key_tile_dv_zero"  -- the last key tile of dk / dv is never written
      "last_query_tile_skips_first_key_tile"            -- o and g of the last query tile miss keys 0:tile
      "mask_plus_one_in_last_tile"                      -- the diagonal compare of the last query tile is off by one key
                                                           (key + 1 <= row): each of its rows loses its own key in o, g
      "first_key_tile_twice_in_last_query_tile"         -- dq of the last query tile adds keys 0:tile twice
      "low_part_lost_in_last_key_tile"                  -- dv of the last key tile from P rounded to bf16: the low half
                                                           of a split-bf16 operand is dropped
    No fault: equal to ``dense_rows``."""
    assert fault is None or fault in TILE_FAULTS, fault
    q, k, v, go = (np.asarray(t, np.float64) for t in (q, k, v, go))
    Nq, Nk = q.shape[0], k.shape[0]
    a = 1.0 / nt
    q0, k0 = tile * ((Nq - 1) // tile), tile * ((Nk - 1) // tile)
    s = (q @ k.T) * a
    keep = (np.arange(Nk)[None, :] <= np.arange(Nq)[:, None]) if mask else np.ones((Nq, Nk), bool)
    const = 0.0 if mask else (Nq if g_const is None else g_const) - Nk
    P = np.where(keep, orc._f(s, p), 0.0)
    g = P.sum(1) + const
    o = (P @ v) / g[:, None]
    # the gradients take the exact o and g: a backward fault is a fault of the backward alone
    dS = np.where(keep, (go @ v.T - (go * o).sum(1, keepdims=True)) / g[:, None] * orc._fprime(s, p), 0.0)
    dq, dk, dv = (dS @ k) * a, (dS.T @ q) * a, (P / g[:, None]).T @ go
    if fault in ("last_query_tile_skips_first_key_tile", "mask_plus_one_in_last_tile"):
        Pb = P.copy()
        if fault == "last_query_tile_skips_first_key_tile":
            Pb[q0:, :tile] = 0.0
        else:
            Pb[q0:] *= (np.arange(Nk)[None, :] + 1 <= np.arange(q0, Nq)[:, None])
        g = Pb.sum(1) + const
        o = (Pb @ v) / g[:, None]
    elif fault == "last_key_tile_dk_zero":
        dk[k0:] = 0.0
    elif fault == "last_key_tile_dv_zero":
        dv[k0:] = 0.0
    elif fault == "first_key_tile_twice_in_last_query_tile":
        dq[q0:] += (dS[q0:, :tile] @ k[:tile]) * a
    elif fault == "low_part_lost_in_last_key_tile":
        dv[k0:] = (_rounder("bf16")(P[:, k0:]) / g[:, None]).T @ go
    return o, g, dq, dk, dv
