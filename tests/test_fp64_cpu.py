"""float64 fastmax without a device: the input conditions the allowance of tests/fp64_ref.py rests on, proof that the allowance
tells a float intermediate from a double one, and the host side of the C ABI for FASTMAX_F64 problems (plan, path and workspace
queries on made-up addresses: nothing is read through them and nothing is launched)."""
import ctypes
import itertools

import numpy as np
import pytest

import fp64_ref as fr
from conftest import rel_err

ATOL = rel_err.__defaults__[0]          # conftest.rel_err's floor for exactly-zero gradients (N = 1 masked)
CAP = 2.0 ** -34


def _block_max(x, block=16):
    """largest |x| of every 16-row block along the sequence axis, broadcast back to x's shape"""
    a = np.abs(x if x.ndim == 4 else x[..., None])
    n = a.shape[2]
    out = np.empty_like(a)
    for r0 in range(0, n, block):
        out[:, :, r0:r0 + block] = a[:, :, r0:r0 + block].max(axis=(2, 3), keepdims=True)
    return out.reshape(x.shape)


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_input_conditions(case):
    """visible weights and denominators stay away from zero (no cancellation the first-order bound would miss), and the
    allowance is at most 2^-34 of every 16-row block's largest |reference|, floored with rel_err's atol.  A block whose
    reference is exactly zero (dq, dk of the N = 1 masked case: dP cancels) has no magnitude of its own and atol = 1e-6 is not
    one either -- an allowance of 1e-14 is 2^-26 of it whatever the kernels do -- so there the allowance is held to 2^-34 of
    the larger of atol and the terms the zero is summed from (the absolute-value evaluation behind the bound)."""
    R = fr.reference(case)
    w, _ = fr.weights(R.q, R.k, case.mask, R.nt, case.p)
    visible = np.tril(np.ones(w.shape[-2:], bool)) if case.mask else np.ones(w.shape[-2:], bool)
    assert w[..., visible].min() >= 0.25
    assert np.abs(R.ref["g"]).min() >= 0.25
    for name in fr.NAMES:
        scale = _block_max(R.ref[name])
        scale = np.maximum(np.where(scale == 0.0, _block_max(R.mag[name]), scale), ATOL)
        worst = float((R.allow[name] / scale).max())
        print(f"{case.id} {name}: allowance / block max <= 2^{np.log2(max(worst, 1e-300)):.1f}")
        assert worst <= CAP, (name, worst)


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_tile_order_restatement_is_inside(case):
    """float64 in the kernels' own summation order stays inside the allowance at every element"""
    R = fr.reference(case)
    got = fr.tiled(R.q, R.k, R.v, R.go, case.mask, R.nt, case.p)
    for name in fr.NAMES:
        fr.assert_inside(f"{case.id} {name}", got[name], R.ref[name], R.allow[name])


# shapes with enough rows and columns for every plant to reach every output: one masked, one unmasked, both p
PLANT_CASES = [c for c in fr.CASES if (c.Nq, c.D) in ((130, 64), (64, 64))]


@pytest.mark.parametrize("plant", fr.PLANTS)
@pytest.mark.parametrize("case", PLANT_CASES, ids=[c.id for c in PLANT_CASES])
def test_float32_intermediate_is_outside(case, plant):
    """one intermediate rounded to float32 -- the score, f(S), the denominator, rowdot -- leaves the allowance"""
    R = fr.reference(case)
    got = fr.tiled(R.q, R.k, R.v, R.go, case.mask, R.nt, case.p, plant=plant)
    hit = {"score": ("o", "g", "dq", "dk", "dv"), "f": ("o", "g", "dv"), "denominator": ("o", "g", "dq", "dk", "dv"),
           "rowdot": ("dq", "dk")}[plant]
    if case.p == 1 and plant == "score":
        hit = ("o", "g", "dv")          # f' = 1: the score reaches dq, dk only through o and g
    for name in hit:
        n, worst = fr.outside(got[name], R.ref[name], R.allow[name])
        print(f"{case.id} {plant} -> {name}: {n} elements outside, worst ratio {worst:.3g}")
        assert n > 0 and worst > 8.0, (name, n, worst)


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_abi_scale_stays_inside_half_the_allowance(case):
    """A float64 problem carries 1/nt across the C ABI as the sum of two floats (fr.abi_scale): relative 2^-48 = 32 units of
    2^-53 where nt is no power of two.  To first order that moves a result by 2^-48 (1 + max |s f'(s) / f(s)|) of the terms it is
    summed from (dq, dk carry the factor itself, everything else only through the scores), against an allowance of
    2 depth 2^-53 of the same terms: a share of 16 (1 + kappa) / depth, at most 1/2 for depth >= 50 and |s| <= 0.6.  Held here per
    element, so that a tighter allowance cannot silently collide with the ABI's 48 bits."""
    from oracle import fastmax_oracle as orc
    R = fr.reference(case)
    nt48 = 1.0 / fr.abi_scale(R.nt)
    o, g = orc.fastmax_fwd_dense(R.q, R.k, R.v, mask=case.mask, nt=nt48, p=case.p)
    dq, dk, dv = orc.fastmax_bwd_dense(R.q, R.k, R.v, R.go, mask=case.mask, nt=nt48, p=case.p)
    for name, got in zip(fr.NAMES, (o, g, dq, dk, dv)):
        n, worst = fr.outside(got, R.ref[name], 0.5 * R.allow[name])
        print(f"{case.id} {name}: 48-bit 1/nt moves the result by {worst / 2:.3g} of the allowance at the most")
        assert n == 0, (name, worst / 2)


@pytest.mark.parametrize("mask,p,shape", fr.LINEARMAX_CASES)
def test_linearmax_allowance_is_capped_and_discriminates(mask, p, shape):
    """the linearmax allowance (the attention's, pushed through the prologue's chain rule) is at most 2^-34 of every 16-row
    block's largest |reference|, and the normalised q rounded to float32 falls outside it in o, dq, dk and dv.  One row per
    head is held to a wider cap: the row n* that attains the max-norm receives -(sum_nd gy xc) xc[n*] / M^3, a signed sum over
    all N D entries of the head's gradient, which cancels like sqrt(N D) while the roundings of its terms add absolutely -- so
    there the allowance may reach 2^-34 sqrt(N D) of the reference (2^-27.5 at N D = 8320; float32 rounding is 2^-24, and the
    second half of this test shows that it still falls outside)."""
    from blockwise import prologue_backward_fp64
    from oracle import fastmax_oracle as orc
    c = fr.Case(mask, p, *shape)
    q, k, v, go = fr.inputs(c, seed=1)
    ref, allow = fr.linearmax_reference(q, k, v, go, p, mask)
    for name in ("o", "dq", "dk", "dv"):
        ratio = allow[name] / np.maximum(_block_max(ref[name]), ATOL)
        star = np.zeros(ratio.shape, bool)
        if name in ("dq", "dk"):
            x = q if name == "dq" else k
            xc = x - x.mean(-1, keepdims=True)
            nrm = np.sqrt((xc * xc).sum(-1))
            star[...] = (nrm == nrm.max(-1, keepdims=True))[..., None]
        worst, worst_star = float(ratio[~star].max()), float(ratio[star].max()) if star.any() else 0.0
        print(f"linearmax {c.id} {name}: allowance / block max <= 2^{np.log2(worst):.1f}" +
              (f", max-norm rows 2^{np.log2(worst_star):.1f}" if star.any() else ""))
        assert worst <= CAP, (name, worst)
        assert worst_star <= CAP * np.sqrt(x.shape[2] * x.shape[3]) if star.any() else True, (name, worst_star)
    qn, kn = orc.normalize_qk(q, k)
    qn = qn.astype(np.float32).astype(np.float64)
    pe, gc = (p, None) if mask else (1, c.Nk)
    o, _ = orc.fastmax_fwd_dense(qn, kn, v, mask=mask, nt=1.0, p=pe, g_const=gc)
    dqn, dkn, dv = orc.fastmax_bwd_dense(qn, kn, v, go, mask=mask, nt=1.0, p=pe, g_const=gc)
    dq, dk = np.empty_like(q), np.empty_like(k)
    for b in range(c.B):
        for h in range(c.H):
            dq[b, h] = prologue_backward_fp64(q[b, h], dqn[b, h].copy())
            dk[b, h] = prologue_backward_fp64(k[b, h], dkn[b, h].copy())
    for name, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        n, worst = fr.outside(got, ref[name], allow[name])
        print(f"linearmax {c.id} float32 q -> {name}: {n} elements outside, worst ratio {worst:.3g}")
        assert n > 0 and worst > 8.0, (name, n, worst)


# ---- host side of the ABI ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from fastmax_experiments_amd import _lib
    return _lib.lib()


def _problem(D=64, N=48, Nk=None, p=1, causal=1, in_dt=3, out_dt=3, path=0, B=1, H=2):
    from fastmax_experiments_amd import _lib
    return _lib.Problem(B, H, N, N if Nk is None else Nk, D, in_dt, out_dt, p, causal, 0.125, 0.0, float(N), path)


def _operands(prob, row=None, base=4096, off=None):
    """made-up addresses and strides of contiguous-like tensors with row stride ``row`` (default: D rounded up to even);
    off: {operand name: bytes added to its address}"""
    off = off or {}
    D = prob.D
    row = (D + 1) // 2 * 2 if row is None else row

    def strides(n):
        return (ctypes.c_int64 * 3)(prob.H * n * row, n * row, row)
    addr = {n: base * (i + 1) * 4096 + off.get(n, 0) for i, n in enumerate(("q", "k", "v", "o", "go", "dq", "dk", "dv"))}
    fwd = (addr["q"], strides(prob.Nq), addr["k"], strides(prob.Nk), addr["v"], strides(prob.Nk), addr["o"])
    bwd = (addr["go"], strides(prob.Nq), addr["dq"], addr["dk"], addr["dv"])
    return fwd, bwd


def _plan(L, prob, fwd, bwd=None):
    from fastmax_experiments_amd import _lib
    plan = _lib.Plan()
    rc = L.fastmax_hip_plan(ctypes.byref(prob), *fwd, *(bwd or (None,) * 5), ctypes.byref(plan))
    assert rc == plan.rc
    return plan


@pytest.mark.parametrize("D", [1, 3, 64, 132, 256])
@pytest.mark.parametrize("causal", [1, 0])
@pytest.mark.parametrize("p", [1, 2])
def test_f64_problems_are_planned(L, p, causal, D):
    from fastmax_experiments_amd import _lib
    assert _lib.F64 == 3
    prob = _problem(D=D, p=p, causal=causal, Nk=None if causal else 77)
    fwd, bwd = _operands(prob)
    for plan in (_plan(L, prob, fwd), _plan(L, prob, fwd, bwd)):
        assert plan.rc == 0 and plan.path == _lib.PATH_QUADRATIC_MFMA == 4
        assert _lib.FWD_KERNELS[plan.fwd_kernel] == "FWD_F64" and plan.fwd_kernel == 9
        assert plan.nseg == 1 and plan.state_bytes == 0
    assert plan.bwd_kernel == 6 and _lib.BWD_KERNELS[6] == "BWD_F64"
    assert _plan(L, prob, fwd).bwd_kernel == -1
    assert L.fastmax_hip_select_path(ctypes.byref(prob)) == 4
    assert L.fastmax_hip_forward_workspace(ctypes.byref(prob)) == 0
    assert L.fastmax_hip_forward_state_bytes(ctypes.byref(prob), *fwd) == 0
    assert L.fastmax_hip_backward_workspace(ctypes.byref(prob)) == 8 * prob.B * prob.H * prob.Nq          # rowdot, doubles


@pytest.mark.parametrize("in_dt,out_dt", [(i, o) for i, o in itertools.product(range(4), repeat=2) if (i == 3) != (o == 3)])
def test_mixed_dtypes_are_rejected(L, in_dt, out_dt):
    from fastmax_experiments_amd import _lib
    prob = _problem(in_dt=in_dt, out_dt=out_dt)
    fwd, bwd = _operands(prob)
    assert _plan(L, prob, fwd, bwd).rc == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_select_path(ctypes.byref(prob)) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_forward_workspace(ctypes.byref(prob)) == 0 and L.fastmax_hip_backward_workspace(ctypes.byref(prob)) == 0
    ws = ctypes.c_void_p(1 << 20)
    assert L.fastmax_hip_forward(ctypes.byref(prob), *fwd, None, ws, 1 << 20, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_backward(ctypes.byref(prob), *fwd, 1 << 24, *bwd, ws, 1 << 20, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_backward_with_states(ctypes.byref(prob), *fwd, 1 << 24, *bwd, ws, 1 << 20, None, 0, None) == _lib.E_BAD_DTYPE


@pytest.mark.parametrize("path", [1, 2, 3, 4])
def test_forced_path_is_rejected(L, path):
    from fastmax_experiments_amd import _lib
    prob = _problem(path=path)
    fwd, bwd = _operands(prob)
    plan = _plan(L, prob, fwd, bwd)
    assert plan.rc == _lib.E_BAD_SHAPE and plan.path == -1 and plan.fwd_kernel == -1
    assert L.fastmax_hip_select_path(ctypes.byref(prob)) == _lib.E_BAD_SHAPE
    ws = ctypes.c_void_p(1 << 20)
    assert L.fastmax_hip_forward(ctypes.byref(prob), *fwd, None, ws, 1 << 20, None) == _lib.E_BAD_SHAPE
    assert L.fastmax_hip_backward(ctypes.byref(prob), *fwd, 1 << 24, *bwd, ws, 1 << 20, None) == _lib.E_BAD_SHAPE


@pytest.mark.parametrize("operand", ["q", "k", "v", "o", "go", "dq", "dk", "dv"])
def test_eight_byte_offsets_are_rejected(L, operand):
    from fastmax_experiments_amd import _lib
    prob = _problem()
    fwd, bwd = _operands(prob, off={operand: 8})
    assert _plan(L, prob, fwd, bwd).rc == _lib.E_ALIGNMENT
    ws = ctypes.c_void_p(1 << 20)
    if operand in ("q", "k", "v", "o"):
        assert _plan(L, prob, fwd).rc == _lib.E_ALIGNMENT
        assert L.fastmax_hip_forward(ctypes.byref(prob), *fwd, None, ws, 1 << 20, None) == _lib.E_ALIGNMENT
    else:
        assert _plan(L, prob, fwd).rc == 0
    assert L.fastmax_hip_backward(ctypes.byref(prob), *fwd, 1 << 24, *bwd, ws, 1 << 20, None) == _lib.E_ALIGNMENT


def test_odd_row_stride_is_rejected(L):
    from fastmax_experiments_amd import _lib
    prob = _problem(D=3)
    fwd, bwd = _operands(prob, row=3)          # contiguous rows of three doubles: every other row starts at 8 mod 16
    assert _plan(L, prob, fwd, bwd).rc == _lib.E_ALIGNMENT
    fwd, bwd = _operands(prob, row=4)
    assert _plan(L, prob, fwd, bwd).rc == 0


def test_other_entry_points_keep_rejecting_float64(L):
    from fastmax_experiments_amd import _lib
    prob = _problem(D=64, N=256, p=1, causal=1)
    fwd, bwd = _operands(prob)
    ws, big = ctypes.c_void_p(1 << 20), 1 << 30
    st = (ctypes.c_int64 * 3)(64 * 256 * 2, 64 * 256, 64)
    assert L.fastmax_hip_normalize_cast(1 << 20, st, 3, 1 << 21, 1 << 22, 1, 2, 256, 64, ws, big, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_normalize_cast_expand(1 << 20, st, 3, 1 << 21, 1 << 22, 1, 2, 2, 256, 64, ws, big, None) == _lib.E_BAD_DTYPE
    inv = 1 << 23
    assert L.fastmax_hip_linearmax_forward(ctypes.byref(prob), *fwd[:6], inv, inv, fwd[6], None, ws, big, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_linearmax_forward_auto(ctypes.byref(prob), *fwd[:6], inv, inv, None, None, fwd[6], None, ws, big, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_linearmax_forward_auto_workspace(ctypes.byref(prob)) == 0
    assert L.fastmax_hip_linearmax_backward(ctypes.byref(prob), *fwd, 1 << 24, *bwd[:2], inv, inv, None, None, *bwd[2:], ws, big,
                                            None, 0, 0, None) == _lib.E_BAD_DTYPE
    assert L.fastmax_hip_linearmax_train_supported(ctypes.byref(prob)) == 0
