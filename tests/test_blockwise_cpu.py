"""CPU checks of tests/blockwise.py: the float64 linear-time references equal the dense oracle; legitimately rounded results
pass the block-wise tolerances the GPU tests use (calibration); and the scan faults a long-sequence kernel can make are
rejected by the block-wise check while the old per-tensor ``rel_err`` accepts them (power).  The same two for the tile
kernels at the shapes of tests/plan_cases.py: ``blockwise.tile_model`` on every GPU case that launches (calibration) and the
tile faults of ``blockwise.emulate_tiles`` (power)."""
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


def _pc():
    import plan_cases as pc
    return pc


def _launching():
    """one case per problem that launches on the GPU: layout variants and forced paths share tensors and references"""
    pc = _pc()
    seen = {}
    for c in pc.GPU_CASES:
        if c.rc == 0:
            seen.setdefault((c.shape, c.dtype, c.mask, c.p), c)
    return list(seen.values())


def _heads(c):
    """per (batch, head): the case's inputs as float64 (N, D) arrays"""
    B, H = c.shape[:2]
    t = [x.double().numpy() for x in _pc().host_inputs(c)]
    return [tuple(x[b, h] for x in t) for b in range(B) for h in range(H)]


def test_block_tolerances_are_those_of_the_long_sequence_tests():
    import test_blockwise_gpu as long
    pc = _pc()
    assert pc.BLOCK_TOL == {"bf16": long.TOL[torch.bfloat16], "f16": long.TOL[torch.float16], "f32": long.TOL[torch.float32]}
    per_tensor = {"f32": (2e-4, 1e-3), "bf16": (8e-3, 2.5e-2), "f16": (2e-3, 5e-3)}          # TOL of test_plan_kernels_gpu.py
    for c in pc.GPU_CASES:
        assert all(b <= t for b, t in zip(pc.block_tol(c), per_tensor[c.dtype])), c.id
    # the calibration below covers the tensors of every GPU case that launches
    covered = {(c.shape, c.dtype, c.mask, c.p) for c in _launching()}
    assert all((c.shape, c.dtype, c.mask, c.p) in covered for c in pc.GPU_CASES if c.rc == 0)


@pytest.mark.parametrize("c", _launching(), ids=lambda c: c.id)
def test_calibration_tile_model_passes_every_block(c):
    """``blockwise.tile_model`` -- a correct kernel with the roundings the tile sources name -- stays within the case's GPU
    tolerance in every 16-row block of o, g, dq, dk, dv, on the very inputs the GPU test uses, against the oracle results the
    GPU test compares with.  Worst block of the model over all cases (forward / gradients): bf16 5.1e-3 / 9.9e-3,
    fp16 6.0e-4 / 9.7e-4, fp32 1.2e-5 / 2.5e-5 (tolerances 8e-3 / 1e-2, 2e-3 / 2e-3, 2e-4 / 2e-4), but for dq of rows 0:16 in
    the two bf16 p = 2 N = 257 cases of plan_cases.BLOCK_TOL_BWD_CASE: 2.05e-2 and 1.18e-2, which the MI355X reproduces to
    three digits.  A problem with a scan or vector-ALU forward is modelled with that forward (``tile_forward=False``)."""
    pc = _pc()
    tf, tb = pc.block_tol(c)
    B, H, Nq, Nk, D = c.shape
    ref = [r.reshape((B * H,) + r.shape[2:]) for r in pc.oracle_fwd(c) + pc.oracle_bwd(c)]
    # the harsher forward if any layout variant or forced path of the problem takes the matrix-core tiles
    tile_forward = any(x.fwd in pc.TILE_FORWARDS for x in pc.GPU_CASES if (x.shape, x.dtype, x.mask, x.p) == (c.shape, c.dtype, c.mask, c.p))
    for bh, (q, k, v, go) in enumerate(_heads(c)):
        got = bw.tile_model(q, k, v, go, pc.nt(D), c.p, c.mask, c.dtype, tile_forward=tile_forward)
        exact = bw.dense_rows(q, k, v, go, nt=pc.nt(D), p=c.p, mask=c.mask)
        for x, e, r, n in zip(got, exact, ref, ("o", "g", "dq", "dk", "dv")):
            assert _close(e, r[bh]) <= 1e-12, n                      # dense_rows is the oracle the GPU test uses
            axis, tol = (-1, tf) if n == "g" else (-2, tf if n == "o" else tb)
            err = bw.assert_blockwise(x, r[bh], tol, f"{c.id} {n} h{bh}", block=pc.BLOCK, axis=axis)
            print(f"MODEL {c.id} {n} h{bh} worst {err:.3e} tol {tol:.1e}")


@pytest.mark.parametrize("test,shape,p,seed,model", [
    ("wide", (1, 5, 520, 32), 1, 520 + 520 + 32 + 1, 1.058e-2), ("wide", (1, 2, 300, 256), 2, 300 + 300 + 256 + 2, 2.104e-2),
    ("ne8", (1, 2, 700, 33), 2, 700 + 33, 1.336e-2)])
def test_sweep_cases_with_their_own_tolerance_follow_the_model(test, shape, p, seed, model):
    """BLOCK_TOL_BF16_BWD_CASE of tests/test_fastmax_gpu.py: 1.5 x the worst gradient block of tile_model on that test's
    own bf16 inputs, at most the per-tensor 2.5e-2, and only where the model is above the ordinary 1e-2"""
    import test_fastmax_gpu as sweeps
    pc = _pc()
    B, H, N, D = shape
    g = torch.Generator().manual_seed(seed)
    if test == "wide":          # test_wide_tile_kernels_forward_backward draws q, grad_o, then k, v
        q, go, k, v = (torch.randn(shape, generator=g).to(torch.bfloat16) for _ in range(4))
        key = ((B, H, N, N, D), p)
    else:                       # test_head_sizes_that_are_not_a_multiple_of_eight draws q, k, v, grad_o
        q, k, v, go = (torch.randn(shape, generator=g).to(torch.bfloat16) for _ in range(4))
        key = (shape, p)
    worst = 0.0
    for b in range(B):
        for h in range(H):
            a = [t[b, h].double().numpy() for t in (q, k, v, go)]
            exact = bw.dense_rows(*a, nt=pc.nt(D), p=p)
            got = bw.tile_model(*a, pc.nt(D), p, True, "bf16")
            worst = max(worst, *(bw.block_rel_err(got[i], exact[i], block=16).max() for i in (2, 3, 4)))
    assert abs(worst - model) <= 1e-5 and worst > pc.BLOCK_TOL["bf16"][1]
    assert abs(sweeps.BLOCK_TOL_BF16_BWD_CASE[key] - min(1.5 * model, 2.5e-2)) <= 1e-4


def _causal_130():
    return [c for c in _launching() if c.mask and c.shape[2] >= 130]


_FAULTY = {}


def _faulty(shape, dtype, p, tile_f, tile_b, fault):
    """per head: (exact, with the fault) for the fault's tensor, on the inputs of the plan cases of that shape and dtype"""
    pc = _pc()
    key = (shape, dtype, p, tile_f, tile_b, fault)
    if key not in _FAULTY:
        c = pc.Case("power", shape, dtype, p, True, "auto", "aligned", 0, None, None, False, True, None, None)
        i = ("o", "g", "dq", "dk", "dv").index(bw.FAULT_TENSOR[fault])
        tile = tile_f if bw.FAULT_TENSOR[fault] == "o" else tile_b
        out = []
        for q, k, v, go in _heads(c):
            exact = bw.dense_rows(q, k, v, go, nt=pc.nt(shape[4]), p=p)
            clean = bw.emulate_tiles(q, k, v, go, pc.nt(shape[4]), p, True, tile)
            assert all(_close(x, e) <= 1e-12 for x, e in zip(clean, exact))          # the emulator itself is exact
            out.append((exact[i], bw.emulate_tiles(q, k, v, go, pc.nt(shape[4]), p, True, tile, fault)[i]))
        _FAULTY[key] = out
    return _FAULTY[key]


@pytest.mark.parametrize("fault", bw.TILE_FAULTS)
@pytest.mark.parametrize("c", _causal_130(), ids=lambda c: c.id)
def test_power_tile_faults_are_rejected(c, fault):
    """every tile fault of ``blockwise.emulate_tiles``, at the tile height of the kernels the case names and on the case's
    inputs, exceeds the case's tolerance in some 16-row block of some head (the lost low part: the fp32 tolerance)"""
    pc = _pc()
    tf, tb = pc.BLOCK_TOL["f32"] if fault == "low_part_lost_in_last_key_tile" else pc.block_tol(c)
    tol = tf if bw.FAULT_TENSOR[fault] == "o" else tb
    for exact, bad in _faulty(c.shape, c.dtype, c.p, *pc.tile_rows(c), fault):
        assert bw.block_rel_err(bad, exact, block=pc.BLOCK).max() > tol


# N, p, tile height -> the faults the per-tensor bf16 tolerance (8e-3 forward, 2.5e-2 gradients) accepts
ACCEPTED_PER_TENSOR = {
    (130, 1, 16): ("last_key_tile_dk_zero", "last_key_tile_dv_zero"),
    (255, 2, 16): ("last_key_tile_dv_zero", "mask_plus_one_in_last_tile"),
    (256, 2, 32): ("last_key_tile_dv_zero",),
    (257, 2, 32): ("last_key_tile_dv_zero", "mask_plus_one_in_last_tile"),
    (300, 1, 32): ("last_key_tile_dk_zero", "last_key_tile_dv_zero", "mask_plus_one_in_last_tile"),
    (511, 1, 32): ("last_key_tile_dk_zero", "last_key_tile_dv_zero", "mask_plus_one_in_last_tile"),
    (520, 1, 32): ("last_key_tile_dk_zero", "last_key_tile_dv_zero", "mask_plus_one_in_last_tile"),
}


@pytest.mark.parametrize("N,p,tile", sorted(ACCEPTED_PER_TENSOR))
def test_power_tile_faults_pass_the_per_tensor_metric(N, p, tile):
    """What tests/test_plan_kernels_gpu.py could not see before it went block by block: (1, 2, N, 64) bf16 causal, the plan
    cases' inputs, the fault in both heads.  Per-tensor rel_err as that test computes it -> worst 16-row block:
      N, p, tile   dk of the last key tile 0   dv of the last key tile 0   mask off by one key in the last tile (o)
      130, 1, 16   2.0e-2 -> 1.0               1.0e-2 -> 1.0               8.9e-3 -> 9.8e-2
      255, 2, 16   2.6e-2 -> 1.0               1.2e-2 -> 1.0               4.5e-3 -> 7.4e-2
      256, 2, 32   4.7e-2 -> 1.0               2.1e-2 -> 1.0               8.6e-3 -> 1.3e-1
      257, 2, 32   3.0e-2 -> 1.0               3.2e-3 -> 1.0               3.3e-3 -> 7.5e-2
      300, 1, 32   2.1e-2 -> 1.0               1.0e-2 -> 1.0               3.2e-3 -> 6.6e-2
      511, 1, 32   1.2e-2 -> 1.0               9.6e-3 -> 1.0               2.8e-3 -> 7.9e-2
      520, 1, 32   1.2e-2 -> 1.0               3.9e-3 -> 1.0               2.7e-3 -> 5.6e-2
    The per-tensor bf16 tolerances (2.5e-2 gradients, 8e-3 forward) accept exactly the entries of ACCEPTED_PER_TENSOR, 16 of
    the 21 (at N = 257 the last row of grad_o is aligned with v, see plan_cases.host_inputs, which makes that row of dk large);
    the block tolerances (1e-2, 8e-3) reject all 21.  Swap block_rel_err for rel_err and this test fails."""
    pc = _pc()
    tf, tb = pc.BLOCK_TOL["bf16"]
    rows = []
    for fault in ("last_key_tile_dk_zero", "last_key_tile_dv_zero", "mask_plus_one_in_last_tile"):
        heads = _faulty((1, 2, N, N, 64), "bf16", p, tile, tile, fault)
        exact, bad = (np.stack(x) for x in zip(*heads))
        fwd = bw.FAULT_TENSOR[fault] == "o"
        old = rel_err(bad, exact) if fwd else rel_err(bad, exact, atol=2e-2)
        new = max(bw.block_rel_err(b, e, block=pc.BLOCK).max() for e, b in heads)
        print(f"POWER {N} p{p} {fault}: per tensor {old:.1e} -> worst block {new:.1e}")
        rows.append((fault, fwd, old, new))
    for fault, fwd, old, new in rows:
        assert new > (tf if fwd else tb), fault
        assert (old < (8e-3 if fwd else 2.5e-2)) == (fault in ACCEPTED_PER_TENSOR[(N, p, tile)]), fault


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
