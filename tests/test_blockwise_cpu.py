"""CPU checks of tests/blockwise.py: the float64 linear-time references equal the dense oracle; legitimately rounded results
pass the block-wise tolerances the GPU tests use (calibration); and the scan faults a long-sequence kernel can make are
rejected by the block-wise check while the old per-tensor ``rel_err`` accepts them (power)."""
import numpy as np
import pytest
import torch

import blockwise as bw
from conftest import rel_err
from oracle import fastmax_oracle as orc


def _close(x, ref):
    """max |x - ref| / max(max |ref|, 1): N = 1 gradients are exactly zero in the dense oracle and ~1e-17 here"""
    return float(np.abs(np.asarray(x) - ref).max() / max(float(np.abs(ref).max()), 1.0))


def _h(x):
    return np.asarray(x, np.float64)[None, None]


# --------------------------------------------------------------------------------------
# reference correctness
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
def test_linear_time_references_equal_the_dense_oracle(N, D):
    rng = np.random.default_rng(N * 1000 + D)
    q, k, v, go = (rng.standard_normal((N, D)) for _ in range(4))
    nt = orc.effective_normalize_term(D)
    ro, rg = orc.fastmax_fwd_dense(_h(q), _h(k), _h(v), nt=nt)
    rgrads = orc.fastmax_bwd_dense(_h(q), _h(k), _h(v), _h(go), nt=nt)
    for chunk in (64, 256):                  # the kernels' chunk, and the references' default
        o, g = bw.p1_causal_fwd(q, k, v, nt, chunk)
        assert _close(o, ro[0, 0]) <= 1e-12 and _close(g, rg[0, 0]) <= 1e-12
        for got, want in zip(bw.p1_causal_bwd(q, k, v, go, nt, chunk), rgrads):
            assert _close(got, want[0, 0]) <= 1e-12
    # linearmax: prologue + nt = 1
    o, _ = bw.linearmax_fwd(q, k, v, chunk=64)
    assert _close(o, orc.linearmax_fwd(_h(q), _h(k), _h(v))[0, 0]) <= 1e-12
    qn, kn = orc.normalize_qk(_h(q), _h(k))
    lq = torch.from_numpy(q).requires_grad_(True)
    lk = torch.from_numpy(k).requires_grad_(True)
    lv = torch.from_numpy(v).requires_grad_(True)
    nq = lq - lq.mean(-1, keepdim=True)
    nk = lk - lk.mean(-1, keepdim=True)
    nq, nk = nq / nq.norm(dim=-1).max(), nk / nk.norm(dim=-1).max()
    P = torch.tril(1 + nq @ nk.T)
    ((P @ lv) / P.sum(1, keepdim=True)).backward(torch.from_numpy(go))          # float64 autograd of the dense form
    for got, want in zip(bw.linearmax_bwd(q, k, v, go, chunk=64), (lq.grad, lk.grad, lv.grad)):
        assert _close(got, want.numpy()) <= 1e-12
    # p = 2 masked, and unmasked with N_q != N_k, through the row-blocked dense form
    ro2, rg2 = orc.fastmax_fwd_dense(_h(q), _h(k), _h(v), nt=nt, p=2)
    got = bw.dense_rows(q, k, v, go, nt=nt, p=2, rows=50)
    for x, want in zip(got, (ro2, rg2) + tuple(orc.fastmax_bwd_dense(_h(q), _h(k), _h(v), _h(go), nt=nt, p=2))):
        assert _close(x, want[0, 0]) <= 1e-12
    kk, vv = (rng.standard_normal((N + 37, D)) for _ in range(2))
    got = bw.dense_rows(q, kk, vv, go, nt=nt, p=1, mask=False, rows=50)
    want = orc.fastmax_fwd_dense(_h(q), _h(kk), _h(vv), mask=False, nt=nt) + \
        orc.fastmax_bwd_dense(_h(q), _h(kk), _h(vv), _h(go), mask=False, nt=nt)
    for x, w in zip(got, want):
        assert _close(x, w[0, 0]) <= 1e-12


def test_block_metric_bounds_the_per_tensor_metric():
    rng = np.random.default_rng(1)
    ref = rng.standard_normal((1, 2, 1000, 8)) / np.sqrt(np.arange(1, 1001))[:, None]
    x = ref + 1e-3 * rng.standard_normal(ref.shape)
    e = bw.block_rel_err(x, ref)
    assert e.shape == (16,) and rel_err(x, ref) <= e.max()
    # the worst block is reported with its rows
    x[..., 900, 3] += 1.0
    err, r0, r1, _ = bw.worst_block(x, ref)
    assert (r0, r1) == (896, 960) and err > 1
    with pytest.raises(AssertionError, match="rows 896:960"):
        bw.assert_blockwise(x, ref, 1e-2, "o")
    # an exactly-zero block is measured against floor * the tensor's scale
    z = np.zeros((130, 4))
    z[64:] = 1.0
    e = bw.block_rel_err(z + 1e-5, z)
    assert np.allclose(e, [1e-2, 1e-5, 1e-5])
    # the metric runs along any axis
    assert np.allclose(bw.block_rel_err(np.swapaxes(x, -1, -2), np.swapaxes(ref, -1, -2), axis=-1), bw.block_rel_err(x, ref))


# --------------------------------------------------------------------------------------
# the long cases of tests/test_blockwise_gpu.py, one head each
# --------------------------------------------------------------------------------------
def split_plan(BH, N, D):
    """rows per sequence-split segment of the p = 1 masked forward (split_plan, fastmax_mfma_split.hip): 64-row chunks"""
    target = 256 if D > 64 else 512
    nchunks = (N + 63) // 64
    if BH >= target * 3 // 4 or nchunks < 8:
        return N
    nseg = min((target + BH - 1) // BH, nchunks // 4, 32)
    if nseg < 2:
        return N
    return 64 * ((nchunks + nseg - 1) // nseg)


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).double().numpy()


def _round(x, dt):
    return torch.from_numpy(np.asarray(x, np.float64)).to(dt).double().numpy()


# name -> (B*H of the GPU case, N, D, linearmax?, bf16 tolerances (fwd, bwd) of the GPU case)
LONG = {
    "config5_linearmax": (32, 16384, 128, True, (8e-3, 2.5e-2)),
    "p1_16k_d64": (2, 16384, 64, False, (8e-3, 2.5e-2)),
}


def _inputs(name):
    BH, N, D, lin, _ = LONG[name]
    rng = np.random.default_rng(5)
    q, k, v, go = (_bf16(rng.standard_normal((N, D))) for _ in range(4))
    if lin:
        q, k = orc.normalize_qk(q, k)                       # the scan sees normalised q, k with nt = 1
        return q, k, v, go, 1.0
    return q, k, v, go, orc.effective_normalize_term(D)


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        q, k, v, go, nt = _inputs(name)
        _CACHE[name] = (q, k, v, go, nt, bw.p1_causal_fwd(q, k, v, nt)[0], bw.p1_causal_bwd(q, k, v, go, nt))
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(LONG))
def test_calibration_rounded_results_pass(name):
    """the exact result rounded to bf16 / fp16 / fp32, and a float32 evaluation of the same scan, pass every block-wise
    tolerance tests/test_blockwise_gpu.py applies for that dtype (bf16 8e-3 / 2.5e-2, fp16 2e-3 / 5e-3, fp32 2e-4 / 1e-3)"""
    q, k, v, go, nt, o, grads = _case(name)
    for dt, tf, tb in ((torch.bfloat16, 8e-3, 2.5e-2), (torch.float16, 2e-3, 5e-3), (torch.float32, 2e-4, 1e-3)):
        bw.assert_blockwise(_round(o, dt), o, tf, f"o {dt}")
        for x, n in zip(grads, ("dq", "dk", "dv")):
            bw.assert_blockwise(_round(x, dt), x, tb, f"{n} {dt}")
    o32, _ = bw.p1_causal_fwd(q, k, v, nt, chunk=64, dtype=np.float32)
    bw.assert_blockwise(o32, o, 2e-4, "o fp32 scan")
    for x, want, n in zip(bw.p1_causal_bwd(q, k, v, go, nt, chunk=64, dtype=np.float32), grads, ("dq", "dk", "dv")):
        bw.assert_blockwise(x, want, 1e-3, n + " fp32 scan")


# --------------------------------------------------------------------------------------
# power: a chunked float64 scan with the faults a split kernel can make
# --------------------------------------------------------------------------------------
def emulate_fwd(q, k, v, nt, seg_rows, fault=None, chunk=64):
    """The kernels' forward schedule: 64-row chunks, segments of ``seg_rows`` rows whose carried state starts from the
    exclusive prefix of the earlier segments' totals.  ``fault``:
      "drop_chunk"    -- the keys of one chunk (the 200th) never reach the carried state
      "state_bf16"    -- the carried state (and every segment prefix) is rounded to bf16 at every chunk boundary
      "stale_segment" -- the last segment s starts from the prefix of segments < s-1 instead of < s
      "mask_shift"    -- from the second segment on, the in-chunk causal mask lets row i see key i+1"""
    N, D = q.shape
    a = 1.0 / nt
    vp = np.concatenate([v, np.ones((N, 1))], 1)
    rnd = _bf16 if fault == "state_bf16" else (lambda x: x)
    totals = []
    for s0 in range(0, N, seg_rows):
        s1 = min(N, s0 + seg_rows)
        totals.append((vp[s0:s1].sum(0), k[s0:s1].T @ vp[s0:s1]))
        if fault == "drop_chunk" and s0 <= 200 * chunk < s1:
            c0 = 200 * chunk
            totals[-1] = (totals[-1][0] - vp[c0:c0 + chunk].sum(0), totals[-1][1] - k[c0:c0 + chunk].T @ vp[c0:c0 + chunk])
    out = np.empty((N, D + 1))
    for s, s0 in enumerate(range(0, N, seg_rows)):
        upto = s - 1 if (fault == "stale_segment" and s0 + seg_rows >= N) else s
        S1 = rnd(sum((t[0] for t in totals[:upto]), np.zeros(D + 1)))
        S2 = rnd(sum((t[1] for t in totals[:upto]), np.zeros((D, D + 1))))
        for c0 in range(s0, min(N, s0 + seg_rows), chunk):
            c1 = min(N, c0 + chunk)
            qc, kc, vc = q[c0:c1], k[c0:c1], vp[c0:c1]
            P = np.tril(1 + a * (qc @ kc.T), 1 if (fault == "mask_shift" and s > 0) else 0)
            if fault == "mask_shift" and s > 0 and c1 < N:
                P = np.concatenate([P, (1 + a * (qc @ k[c1:c1 + 1].T)) * (np.arange(c1 - c0) == c1 - c0 - 1)[:, None]], 1)
                vc = np.concatenate([vc, vp[c1:c1 + 1]])
            out[c0:c1] = P @ vc + S1 + a * (qc @ S2)
            if not (fault == "drop_chunk" and c0 == 200 * chunk):
                S1 = rnd(S1 + vp[c0:c1].sum(0))
                S2 = rnd(S2 + kc.T @ vp[c0:c1])
    return out[:, :D] / out[:, D:]


def emulate_bwd_drop_reverse_chunk(q, k, v, go, nt, chunk=64, drop=30):
    """dk, dv by the reverse scan, with chunk ``drop`` never added to the reverse state R1 = sum Gh_i, R2 = sum q_i Gh_i^T"""
    N, D = q.shape
    a = 1.0 / nt
    o, g = bw.p1_causal_fwd(q, k, v, nt)
    Gh = np.concatenate([go, -(go * o).sum(1, keepdims=True)], 1) / g[:, None]
    vp = np.concatenate([v, np.ones((N, 1))], 1)
    dk, dvp = np.empty((N, D)), np.empty((N, D + 1))
    R1, R2 = np.zeros(D + 1), np.zeros((D, D + 1))
    for c0 in reversed(range(0, N, chunk)):
        c1 = min(N, c0 + chunk)
        qc, kc, vc, gc = q[c0:c1], k[c0:c1], vp[c0:c1], Gh[c0:c1]
        dk[c0:c1] = a * (np.tril(gc @ vc.T).T @ qc + vc @ R2.T)
        dvp[c0:c1] = np.tril(1 + a * (qc @ kc.T)).T @ gc + R1 + a * (kc @ R2)
        if c0 != drop * chunk:
            R1, R2 = R1 + gc.sum(0), R2 + qc.T @ gc
    return dk, dvp[:, :D]


@pytest.mark.parametrize("fault", ["drop_chunk", "state_bf16", "stale_segment", "mask_shift"])
@pytest.mark.parametrize("name", sorted(LONG))
def test_power_forward_faults_are_rejected(name, fault):
    """Each forward fault at the GPU case's shape, segment plan and bf16 tolerance fails the block-wise check and passes the
    per-tensor one.  Measured (seed 5, one head), per-tensor rel_err vs the 8e-3 it would have to beat / worst block:
      config5_linearmax (8 x 2048-row segments): drop_chunk 8.6e-4 / 9.6e-2, state_bf16 4.2e-4 / 2.6e-2,
                                                 stale_segment 5.1e-3 / 5.9e-1, mask_shift 7.6e-4 / 3.5e-2
      p1_16k_d64 (32 x 512-row segments):        drop_chunk 6.4e-4 / 6.4e-2, state_bf16 3.3e-4 / 1.5e-2,
                                                 stale_segment 1.8e-3 / 2.0e-1, mask_shift 3.5e-3 / 6.7e-2"""
    BH, N, D, _, (tf, _) = LONG[name]
    q, k, v, go, nt, o, _ = _case(name)
    bad = emulate_fwd(q, k, v, nt, split_plan(BH, N, D), fault)
    assert rel_err(bad, o) < tf                               # the old metric accepts it ...
    assert bw.block_rel_err(bad, o).max() > tf                # ... the block-wise one does not
    assert rel_err(emulate_fwd(q, k, v, nt, split_plan(BH, N, D)), o) < 1e-12     # the emulator itself is exact


@pytest.mark.parametrize("name", sorted(LONG))
def test_power_backward_reverse_state_fault_is_rejected(name):
    """one chunk (rows 1920:1984) missing from the reverse state of dK / dV: per-tensor rel_err vs 2.5e-2 / worst block,
      config5_linearmax: dk 5.1e-3 / 2.2e-1, dv 3.8e-3 / 1.7e-1;  p1_16k_d64: dk 1.2e-2 / 2.4e-1, dv 3.5e-3 / 2.2e-1"""
    _, _, _, _, (_, tb) = LONG[name]
    q, k, v, go, nt, _, (_, dk, dv) = _case(name)
    bk, bv = emulate_bwd_drop_reverse_chunk(q, k, v, go, nt)
    for bad, want in ((bk, dk), (bv, dv)):
        assert rel_err(bad, want) < tb
        assert bw.block_rel_err(bad, want).max() > tb
