"""Every kernel fwd_plan / bwd_select can pick, once, against float64: for each GPU case of tests/plan_cases.py the plan
query on the real tensors has to name the expected kernels, then fastmax_hip_forward and fastmax_hip_backward_with_states run
through the C ABI directly (ops._prep would copy a misaligned operand to aligned storage and undo the case's layout), and
o, g, dq, dk, dv are compared with oracle.c_oracle on the upcast inputs at the suite's per-dtype tolerances.  Every output
lies between 64-element bands of NaN inside its own buffer: the bands must come back bit for bit and the outputs without a
NaN, so a 16-byte store or a ragged tail on an offset tensor cannot write outside it unseen.  Needs an MI355X.

Block by block: the last tile of a causal tensor is 20 to 300 times smaller than its first rows, and a wrong ragged tile stays
under the per-tensor tolerances (tests/test_blockwise_cpu.py, test_power_tile_faults_pass_the_per_tensor_metric).  So o and dq
(along the queries), dk and dv (along the keys) and g (along N_q) are also checked in 16-row blocks per head, each block
relative to its own magnitude, and one BLOCKWISE line per tensor gives the worst block.  16 is the tile height of the narrow
kernels and half that of the wide ones.  Tolerances per block (forward and g / gradients): TOL of tests/test_blockwise_gpu.py
through plan_cases.BLOCK_TOL -- bf16 8e-3 / 1e-2, fp16 2e-3 / 2e-3, fp32 2e-4 / 2e-4 -- none above the per-tensor value.
Worst block of blockwise.tile_model over the cases (tests/test_blockwise_cpu.py) next to the worst measured on the MI355X:
  bf16  model 5.1e-3 / 9.9e-3;  measured forward: 32-row tiles 5.2e-3, 16-row tiles 5.0e-3, vector-ALU tiles 3.1e-3, recurrence
        3.5e-3, scans 3.9e-3;  gradients: 16-row tiles 6.2e-3, vector-ALU tiles 3.7e-3, linear-time 9.4e-3, 32-row tiles 7.6e-3
        but for the two cases below
  fp16  model 6.0e-4 / 9.7e-4;  measured forward <= 4.6e-4 (every family), gradients <= 6.5e-4 (32-row tiles, dk)
  fp32  model 1.2e-5 / 2.5e-5;  measured forward <= 2.6e-5 (g of one query against 256 keys), gradients <= 5.9e-5 (same case)
Two cases exceed 1e-2 in dq and dk of rows 0:16 and keep their own gradient tolerance, plan_cases.BLOCK_TOL_BWD_CASE: bf16 p = 2
(1, 2, 257, 64), model 2.05e-2 and measured 2.05e-2, and (1, 8, 257, 64), model 1.18e-2 and measured 1.18e-2.  The 32-row
forward divides the bf16-rounded P by the sum of the unrounded P (fastmax_quad32_mfma.hip:138-165) and stores o in bf16; the
backward reads it back for c_i = G_i . o_i (fastmax_quad_mfma_bwd.hip:60), and dS_ij = G_i . (v_j - o_i) / g_i of the first
rows is a difference of nearly equal terms.  The tolerance is 1.5 x the model's worst block, at most the per-tensor 2.5e-2."""
import ctypes

import pytest
import torch

import blockwise as bw
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


def _blocks(c, name, got, ref, tol, failures):
    """every 16-row block of every head against the float64 result, relative to the block's own magnitude: one BLOCKWISE line
    with the worst block over the heads; a block above ``tol`` is recorded, and asserted once every tensor has been printed"""
    B, H = c.shape[:2]
    got, ref = (x.reshape((B * H,) + x.shape[2:]) for x in (got, ref))
    axis = -1 if name == "g" else -2
    worst = max((bw.worst_block(got[bh], ref[bh], block=pc.BLOCK, axis=axis) + (bh,) for bh in range(B * H)), key=lambda w: w[0])
    err, r0, r1, scale, bh = worst
    print(f"BLOCKWISE {c.id} {name} h{bh} worst {err:.3e} rows {r0}:{r1} tol {tol:.1e}")
    if not err <= tol:
        failures.append(f"{name} h{bh}: rows {r0}:{r1} err {err:.3e} > {tol:.1e} (block max|ref| {scale:.3e})")


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
    btf, btb = pc.block_tol(c)
    failures = []
    _blocks(c, "o", o.t.double().cpu().numpy(), ro, btf, failures)
    _blocks(c, "g", g.t.double().cpu().numpy(), rg, btf, failures)
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
            _blocks(c, n, t.t.double().cpu().numpy(), r, btb, failures)
        results.append([t.t.clone() for t in (gq, gk, gv)])
        del bwsb
    if len(results) == 2:
        for a, b, n in zip(results[0], results[1], ("dq", "dk", "dv")):
            assert torch.equal(a, b), f"{n}: kept states and recomputed states give different bits"
    assert torch.equal(o.buf.view(torch.uint8), o_bits.view(torch.uint8)), "the backward wrote to o"
    assert not failures, f"{c.id}: " + "; ".join(failures)
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
