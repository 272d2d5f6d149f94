"""float64 fastmax on the device (csrc/fastmax_f64.hip): every element of o, g, dq, dk, dv against the numpy float64 oracle
within the a-priori allowance of tests/fp64_ref.py (2^-34 of a block's magnitude at the most: a float32 intermediate anywhere
falls outside, tests/test_fp64_cpu.py), through the C ABI shim (ops) and through the operators with autograd; gradcheck;
strided, grouped, offset and misaligned layouts bit for bit with guard bands; determinism; the A/B switch."""
import importlib

import numpy as np
import pytest
import torch

import fp64_ref as fr

pytestmark = pytest.mark.gpu

F64 = torch.float64
fm = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax")


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to("cuda") for a in arrays)          # a copy: the shared references are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _ops_run(q, k, v, go, p, mask, nt, g0):
    from fastmax_experiments_amd import ops
    q, k, v, go = (ops._prep(t, t.device) for t in (q, k, v, go))
    o, g = ops.forward(q, k, v, p, mask, nt, g0, F64)
    dq, dk, dv = ops.backward(q, k, v, o, g, go, p, mask, nt)
    return dict(o=o, g=g, dq=dq, dk=dk, dv=dv)


# ---- 1. the kernels through ops.forward / ops.backward, every case, every element -----------------------------------------------
@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_every_element_within_the_allowance(case):
    R = fr.reference(case)
    got = _ops_run(*_dev(R.q, R.k, R.v, R.go), case.p, case.mask, R.nt, float(case.Nq))
    worst = {}
    for name in fr.NAMES:
        assert got[name].dtype == F64
        worst[name] = fr.outside(_np(got[name]), R.ref[name], R.allow[name])
    print(case.id, {n: f"{w[1]:.3g}" for n, w in worst.items()})          # worst |err| / allowance per tensor
    for name in fr.NAMES:
        fr.assert_inside(f"{case.id} {name}", _np(got[name]), R.ref[name], R.allow[name])


# ---- 2. the operators with autograd ------------------------------------------------------------------------------------------
def _autograd(fn, R, device="cuda"):
    q, k, v = (torch.from_numpy(a.copy()).to(device).requires_grad_(True) for a in (R.q, R.k, R.v))
    o = fn(q, k, v)
    o.backward(torch.from_numpy(R.go.copy()).to(device))
    return o, q.grad, k.grad, v.grad


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_fastmax_operator(case):
    R = fr.reference(case)
    res = _autograd(lambda q, k, v: fm.fastmax(q, k, v, mask=case.mask, p=case.p), R)
    for name, t in zip(("o", "dq", "dk", "dv"), res):
        assert t.dtype == F64 and t.is_cuda
        fr.assert_inside(f"{case.id} {name}", _np(t), R.ref[name], R.allow[name])


def test_fastmax_operator_on_cpu_resident_inputs():
    case = fr.CASES[fr.CASE_IDS.index("masked-p2-1x2x33x33x6")]
    R = fr.reference(case)
    res = _autograd(lambda q, k, v: fm.fastmax(q, k, v, mask=True, p=2), R, device="cpu")
    for name, t in zip(("o", "dq", "dk", "dv"), res):
        assert t.dtype == F64 and t.device.type == "cpu"
        fr.assert_inside(name, _np(t), R.ref[name], R.allow[name])


@pytest.mark.parametrize("mask,p,shape", fr.LINEARMAX_CASES)
def test_linearmax_operator(mask, p, shape):
    from fastmax_experiments_amd.attention_mechanisms.fastmax_hack import fastmax_hack, linearmax_plan
    c = fr.Case(mask, p, *shape)
    q, k, v, go = fr.inputs(c, seed=1)
    ref, allow = fr.linearmax_reference(q, k, v, go, p, mask)
    plan = linearmax_plan(F64, c.B, c.H, c.Nq, c.Nk, c.D, p, mask, True, fp64_kernels=fm.FP64_KERNELS)
    assert (plan.operator, plan.prologue) == ("two_node" if mask else "unmasked", "tensor_ops")
    R = fr.Reference(q, k, v, go, 1.0, ref, allow, {})
    res = _autograd(lambda a, b, c_: fastmax_hack(a, b, c_, p=p, mask=mask), R)
    for name, t in zip(("o", "dq", "dk", "dv"), res):
        assert t.dtype == F64
        fr.assert_inside(f"linearmax {c.id} {name}", _np(t), ref[name], allow[name])


# ---- 3. gradcheck with torch's defaults ------------------------------------------------------------------------------------------
def _randn(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed)).to("cuda").requires_grad_(True)


@pytest.mark.parametrize("mask,p,B,H,Nq,Nk,D", [(True, 1, 1, 2, 19, 19, 8), (True, 2, 1, 2, 19, 19, 8), (True, 2, 1, 1, 17, 17, 6),
                                                 (False, 1, 1, 2, 5, 19, 8)])
def test_gradcheck_fastmax(mask, p, B, H, Nq, Nk, D):
    q, k, v = _randn(B, H, Nq, D, seed=1), _randn(B, H, Nk, D, seed=2), _randn(B, H, Nk, D, seed=3)
    assert torch.autograd.gradcheck(lambda a, b, c: fm.fastmax(a, b, c, mask=mask, p=p), (q, k, v), eps=1e-6, atol=1e-5, rtol=1e-3)


@pytest.mark.parametrize("mask,p", [(True, 1), (True, 2), (False, 1)])
def test_gradcheck_linearmax(mask, p):
    from fastmax_experiments_amd.attention_mechanisms.fastmax_hack import fastmax_hack
    q, k, v = _randn(1, 2, 19, 8, seed=4), _randn(1, 2, 19, 8, seed=5), _randn(1, 2, 19, 8, seed=6)
    assert torch.autograd.gradcheck(lambda a, b, c: fastmax_hack(a, b, c, p=p, mask=mask), (q, k, v), eps=1e-6, atol=1e-5, rtol=1e-3)


# ---- 4. layouts: bit-equal to the contiguous call, guard bands stay NaN ------------------------------------------------------------
GUARD = 64


def _guarded_empty(orig_empty):
    """torch.empty for float64 results with NaN guard bands before and after; the bands are kept for the check"""
    made = []

    def empty(shape, dtype=None, device=None, **kw):
        if dtype != F64:
            return orig_empty(shape, dtype=dtype, device=device, **kw)
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=F64, device=device)
        made.append((buf, n))
        return buf[GUARD:GUARD + n].view(*shape)
    return empty, made


def _run_guarded(monkeypatch, q, k, v, go, p, mask, nt):
    """ops.forward / ops.backward with o, g, dq, dk, dv allocated inside NaN guard bands -> results, after checking the bands"""
    from fastmax_experiments_amd import ops
    empty, made = _guarded_empty(torch.empty)
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        got = _ops_run(q, k, v, go, p, mask, nt, float(q.shape[2]))
        torch.cuda.synchronize()
    assert len(made) >= 5
    for buf, n in made:
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all()
    for t in got.values():
        assert not torch.isnan(t).any()
    return got


@pytest.mark.parametrize("p,mask", [(2, True), (1, False)])
def test_layouts_bit_equal_and_guarded(monkeypatch, p, mask):
    B, H, N, D, nt = 2, 4, 37, 12, 8 * 12 ** 0.5
    gen = torch.Generator().manual_seed(7)
    q, k, v, go = (torch.randn(B, H, N, D, dtype=F64, generator=gen).to("cuda") for _ in range(4))
    want = _run_guarded(monkeypatch, q, k, v, go, p, mask, nt)

    def same(got, what):
        for name in fr.NAMES:
            assert torch.equal(got[name], want[name]), (what, name)

    # (B,N,H,D) storage
    bnhd = [t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v, go)]
    assert bnhd[0].stride(1) == D
    same(_run_guarded(monkeypatch, *bnhd, p, mask, nt), "bnhd")
    # a base 16 bytes into a larger buffer
    off = []
    for t in (q, k, v, go):
        big = torch.full((t.numel() + 8,), float("nan"), dtype=F64, device="cuda")
        big[2:2 + t.numel()] = t.reshape(-1)
        off.append(big[2:2 + t.numel()].view(t.shape))
        assert off[-1].data_ptr() % 32 == 16
    same(_run_guarded(monkeypatch, *off, p, mask, nt), "offset")
    # grouped-query K, V: (B * G, rep, N, D) with head stride 0, as the attention block's group views hand them on, against
    # the materialised copies
    kg, vg = (t[:, ::2].contiguous() for t in (k, v))
    G, rep = H // 2, 2
    qv = q.view(B * G, rep, N, D)
    gov = go.view(B * G, rep, N, D)
    kview = kg.view(B * G, 1, N, D).expand(B * G, rep, N, D)
    vview = vg.view(B * G, 1, N, D).expand(B * G, rep, N, D)
    assert kview.stride(1) == 0
    grouped = _run_guarded(monkeypatch, qv, kview, vview, gov, p, mask, nt)
    copies = _run_guarded(monkeypatch, qv, kview.contiguous(), vview.contiguous(), gov, p, mask, nt)
    for name in fr.NAMES:
        assert torch.equal(grouped[name], copies[name]), ("grouped", name)


def test_misaligned_view_is_copied_by_the_shim():
    """rows that start 8 bytes off the 16-byte rule (an odd head size sliced out of wider rows): the shim copies, same bits"""
    B, H, N, D = 1, 2, 21, 5
    gen = torch.Generator().manual_seed(9)
    wide = [torch.randn(B, H, N, D + 2, dtype=F64, generator=gen).to("cuda") for _ in range(3)]
    views = [w[..., 1:1 + D] for w in wide]
    assert all(t.data_ptr() % 16 == 8 for t in views)

    def run(ts):
        ts = [t.detach().requires_grad_(True) for t in ts]
        o = fm.fastmax(*ts, mask=True, p=2)
        o.backward(torch.ones_like(o))
        return (o, *(t.grad for t in ts))
    for a, b in zip(run(views), run([t.contiguous() for t in views])):
        assert a.dtype == F64 and torch.equal(a, b)


# ---- 5. determinism and batch independence ------------------------------------------------------------------------------------
def test_deterministic_and_batch_independent():
    H, N, D, nt = 3, 70, 20, 8 * 20 ** 0.5
    gen = torch.Generator().manual_seed(3)
    q3, k3, v3, go3 = (torch.randn(3, H, N, D, dtype=F64, generator=gen).to("cuda") for _ in range(4))
    for p, mask in ((1, True), (2, True), (2, False)):
        a = _ops_run(q3, k3, v3, go3, p, mask, nt, float(N))
        b = _ops_run(q3, k3, v3, go3, p, mask, nt, float(N))
        one = _ops_run(*(t[2:3].contiguous() for t in (q3, k3, v3, go3)), p, mask, nt, float(N))
        for name in fr.NAMES:
            assert torch.equal(a[name], b[name]), (p, mask, name, "two runs")
            assert torch.equal(a[name][2:3], one[name]), (p, mask, name, "batch row 2 of 3 against B = 1")


# ---- 6. the A/B switch ---------------------------------------------------------------------------------------------------------
def test_switch_restores_the_float32_route(monkeypatch):
    gen = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, 2, 40, 16, dtype=F64, generator=gen).to("cuda") for _ in range(3))
    on = fm.fastmax(q, k, v, mask=True, p=2)
    monkeypatch.setattr(fm, "FP64_KERNELS", False)
    off = fm.fastmax(q, k, v, mask=True, p=2)
    assert off.dtype == F64 and torch.equal(off, fm.fastmax(q.float(), k.float(), v.float(), mask=True, p=2).double())
    # the two routes differ by float32 rounding and no more: inputs and every one of the N + D + 16 steps at 2^-24, on sums of
    # |w| |v| / g <= max |v|, both terms of o as in fp64_ref's forward bound
    assert not torch.equal(on, off)
    assert (on - off).abs().max() <= (40 + 16 + 16) * 2.0 ** -24 * 2 * v.abs().max()
