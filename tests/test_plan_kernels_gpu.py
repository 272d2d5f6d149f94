"""Every kernel fwd_plan / bwd_select can pick, once, against float64: for each GPU case of tests/plan_cases.py the plan
query on the real tensors has to name the expected kernels, then fastmax_hip_forward and fastmax_hip_backward_with_states run
through the C ABI directly (ops._prep would copy a misaligned operand to aligned storage and undo the case's layout), and
o, g, dq, dk, dv are compared with oracle.c_oracle on the upcast inputs at the suite's per-dtype tolerances.  Every output
lies between 64-element bands of NaN inside its own buffer: the bands must come back bit for bit and the outputs without a
NaN, so a 16-byte store or a ragged tail on an offset tensor cannot write outside it unseen.  Needs an MI355X."""
import ctypes

import pytest
import torch

import plan_cases as pc
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_FWD = 2e-4
TOL_BWD = 1e-3
# the suite's tolerances for these kernels (tests/test_fastmax_gpu.py): forward, gradients
TOL = {"f32": (TOL_FWD, TOL_BWD), "bf16": (8e-3, 2.5e-2), "f16": (2e-3, 5e-3)}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()


def _input(x, dtype, off8=False, rowpad=False):
    """x (float32, CPU) on the device in `dtype`, as a view into a larger buffer: 8 bytes past a 16-byte boundary, or with
    rows 8 bytes longer than D"""
    tdt = TORCH_DT[dtype]
    pad = 8 // pc.elem_bytes(dtype)
    if rowpad:
        buf = torch.zeros(x.shape[:3] + (x.shape[3] + pad,), dtype=tdt, device="cuda")
        view = buf[..., :x.shape[3]]
    else:
        off = pad if off8 else 0
        buf = torch.zeros(off + x.numel(), dtype=tdt, device="cuda")
        view = buf[off:].view(x.shape)
    view.copy_(x.to(tdt))
    assert view.data_ptr() % 16 == (8 if off8 else 0) and view.stride(3) == 1
    return view


class Guarded:
    """a contiguous output tensor of NaN between two bands of NaN in one buffer"""

    def __init__(self, shape, dtype, off8=False):
        n = 1
        for s in shape:
            n *= s
        self.lo = pc.GUARD + (8 // pc.elem_bytes(dtype) if off8 else 0)
        self.buf = torch.full((self.lo + n + pc.GUARD,), float("nan"), dtype=TORCH_DT[dtype], device="cuda")
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        self.before = self._bits().clone()
        assert self.t.data_ptr() % 16 == (8 if off8 else 0)

    def _bits(self):
        return self.buf.view(torch.int32 if self.buf.element_size() == 4 else torch.int16)

    def check(self, name):
        now, n = self._bits(), self.t.numel()
        assert torch.equal(now[:self.lo], self.before[:self.lo]), f"{name}: written before the tensor"
        assert torch.equal(now[self.lo + n:], self.before[self.lo + n:]), f"{name}: written past the tensor"
        assert not torch.isnan(self.t).any(), f"{name}: elements left unwritten or NaN"

    def untouched(self):
        return torch.equal(self._bits(), self.before)


def _run(c, L, ops):
    B, H, Nq, Nk, D = c.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    q, k, v, go = pc.host_inputs(c)
    dq_ = _input(q, c.dtype, off8=c.layout == "q_off8")
    dk_ = _input(k, c.dtype, rowpad=c.layout == "k_rowpad")
    dv_ = _input(v, c.dtype)
    dgo = _input(go, c.dtype, off8=c.layout == "go_off8")
    o = Guarded((B, H, Nq, D), pc.out_dtype(c), off8=c.layout == "o_off8")
    g = Guarded((B, H, Nq), "f32")
    gq = Guarded((B, H, Nq, D), c.dtype, off8=c.layout == "dq_off8")
    gk, gv = Guarded((B, H, Nk, D), c.dtype), Guarded((B, H, Nk, D), c.dtype)
    prob = pc.problem(c)
    pr = ctypes.byref(prob)
    qkv = ops._qkv(dq_, dk_, dv_)
    # the plan on the real tensors
    rc, plan = pc.query(L, prob, qkv + (o.t.data_ptr(),) + ops._qkv(dgo) + (gq.t.data_ptr(), gk.t.data_ptr(), gv.t.data_ptr()))
    assert rc == plan.rc and pc.answer(plan) == pc.expected(c)

    ws_bytes = L.fastmax_hip_forward_workspace(pr)
    wsb, wsp = ops._ws(ws_bytes, dev)
    rc = L.fastmax_hip_forward(pr, *qkv, o.t.data_ptr(), g.t.data_ptr(), wsp, ws_bytes, ops._stream(dev))
    torch.cuda.synchronize()
    assert rc == c.rc
    if c.rc:          # rejected before anything is launched: nothing is written
        assert o.untouched() and g.untouched()
        return
    o.check("o")
    g.check("g")
    tf, tb = TOL[c.dtype]
    ro, rg = pc.oracle_fwd(c)
    print(f"{c.id}: o {rel_err(o.t.float().cpu().numpy(), ro):.3e} g {rel_err(g.t.cpu().numpy(), rg):.3e}")
    assert rel_err(o.t.float().cpu().numpy(), ro) < tf
    assert rel_err(g.t.cpu().numpy(), rg) < tf
    o_bits = o.buf.clone()

    bws_bytes = L.fastmax_hip_backward_workspace(pr)
    runs = [(wsp, plan.state_bytes), (None, 0)] if c.split else [(None, 0)]          # with the forward's kept states, and without
    assert not c.split or c.fwd not in pc.SCANS or 0 < plan.state_bytes <= ws_bytes
    results = []
    for states, nbytes in runs:
        for t in (gq, gk, gv):
            t.buf.fill_(float("nan"))
        bwsb, bwsp = ops._ws(bws_bytes, dev)
        rc = L.fastmax_hip_backward_with_states(pr, *qkv, o.t.data_ptr(), g.t.data_ptr(), *ops._qkv(dgo), gq.t.data_ptr(), gk.t.data_ptr(),
                                                gv.t.data_ptr(), bwsp, bws_bytes, states, nbytes, ops._stream(dev))
        torch.cuda.synchronize()
        assert rc == 0
        for t, n, r in zip((gq, gk, gv), ("dq", "dk", "dv"), pc.oracle_bwd(c)):
            t.check(n)
            err = rel_err(t.t.float().cpu().numpy(), r, atol=2e-2)
            print(f"{c.id}: {n} {err:.3e}")
            assert err < tb, n
        results.append([t.t.clone() for t in (gq, gk, gv)])
        del bwsb
    if len(results) == 2:
        for a, b, n in zip(results[0], results[1], ("dq", "dk", "dv")):
            assert torch.equal(a, b), f"{n}: kept states and recomputed states give different bits"
    assert torch.equal(o.buf.view(torch.uint8), o_bits.view(torch.uint8)), "the backward wrote to o"
    del wsb


@pytest.mark.parametrize("c", pc.GPU_CASES, ids=[c.id for c in pc.GPU_CASES])
def test_planned_kernels_against_float64(c):
    from fastmax_experiments_amd import _lib, ops
    L = _lib.lib()
    with pc.tuned(L, c):
        _run(c, L, ops)


def test_python_face_of_the_plan_query():
    """ops.planned_kernels next to ops.selected_path: names, family, split, for tensors as the operator hands them over"""
    from fastmax_experiments_amd import _lib, ops
    q = torch.zeros(1, 2, 520, 64, device="cuda")
    plan = ops.planned_kernels(q, q, q, 1, True)
    assert (plan["fwd_kernel"], plan["bwd_kernel"], plan["nseg"] > 1, plan["path"]) == ("FWD_SCAN_V2", None, True, _lib.PATH_MFMA)
    assert plan["path"] == ops.selected_path(q, q, 1, True) and plan["state_bytes"] > 0
    plan = ops.planned_kernels(q, q, q, 1, True, o=torch.empty_like(q), grad_o=q)
    assert (plan["fwd_kernel"], plan["bwd_kernel"]) == ("FWD_SCAN_V2", "BWD_LIN")
    plan = ops.planned_kernels(q[:, :, :256], q[:, :, :256], q[:, :, :256], 2, True, grad_o=q[:, :, :256])
    assert (plan["fwd_kernel"], plan["bwd_kernel"], plan["nseg"]) == ("FWD_QUAD32", "BWD_QUAD32", 1)
