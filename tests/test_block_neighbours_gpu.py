"""The decoder block's neighbours of the attention sub-layer on an MI355X (csrc/block_neighbours.hip, block.py):
RMSNorm forward (plain and with the residual add), its backward with the fixed-order dweight, the gated activation forward
and backward, the modules on the reference's fixtures, Block / BlockStack with the kernels on against the tensor-op
restatement, generation through the whole block on both state caches, and the captured fine-tune step.

Bounds.  fp32 against float64: 2e-6 of the largest reference magnitude (forward, rstd), 1e-5 (backward).  16-bit forward: one
unit in the last place of the output dtype (gated activation: two, act is rounded and the product again; exact GELU over
block_ref.gated_floor, the float32 cancellation of 1 + erf).  16-bit backward: twice the error the tensor-op restatement in
that dtype makes against the same float64 on the same inputs, floored at one unit in the last place of the largest magnitude."""
import numpy as np
import pytest
import torch

import block_ref as br
from conftest import golden_names, load_golden, rel_err

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAME = {v: k for k, v in TD.items()}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _rand(shape, seed, dt, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(TD[dt]).cuda()


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_fwd(got, want, dt, what, ulps=1.0, floor=0.0):
    if dt == "f32":
        e = rel_err(got, want)
        print(f"{what}: {e:.3e} (bound 2e-6)")
        assert e < 2e-6, what
    else:
        excess = np.abs(got - want) - floor
        worst = float((excess / br.ulp(want, dt)).max())
        print(f"{what}: {worst:.2f} ulp (bound {ulps})")
        assert worst <= ulps, what


# ---- RMSNorm forward ---------------------------------------------------------------------------------------------------------
def _inner_flip(x64, w64, rstd64, offset, dt, wdt):
    """allowance of the comparisons against the float64 restatement (not against the fixtures, which hold at one unit): the
    16-bit result has TWO rounding points, the normalised row and the product with the weight.  float32 statistics a few ulp
    from float64 can move the normalised row across a rounding boundary, which shifts the product by |w'| units of the row
    before the product's own rounding (the one unit in the last place of the bound)."""
    if dt == "f32":
        return 0.0
    weff = br.round_to(1.0 + w64, wdt) if offset else w64
    return np.abs(weff) * br.ulp(x64 * rstd64[:, None], dt)


@pytest.mark.parametrize("name", golden_names("rmsnorm_"))
def test_rmsnorm_forward_matches_fixture(name):
    from fastmax_experiments_amd.block import rms_norm_forward
    d, m = load_golden(name)
    dt, wdt = m["x_dtype"], m["weight_dtype"]
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda()
    w = torch.from_numpy(d["weight"]).to(TD[wdt]).cuda()
    _, y, rstd = rms_norm_forward(x, None, w, m["eps"], m["add_unit_offset"])
    assert y.dtype == TD[br.out_dtype(dt, wdt)] and y.shape == x.shape
    _check_fwd(_np(y), d["y"], dt, name)          # float32 weight: the rounding boundary is the 16-bit normalised row's
    _, _, rstd64 = br.rmsnorm_ref(d["x"], d["weight"], m["eps"], m["add_unit_offset"], dt, wdt)
    assert rel_err(_np(rstd), rstd64.reshape(-1)) < 2e-6


@pytest.mark.parametrize("dt,wdt", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32")])
@pytest.mark.parametrize("C", [1, 7, 72, 128, 2048, 4096, 5128])
def test_rmsnorm_forward_matches_float64(C, dt, wdt):
    """every launch shape: scalar (1, 7; 72 in 16 bits is whole pieces, in fp32 too), a wave per row, 1 / 2 / 4 / 8 pieces per
    thread, and rows at M = 1, 3, 130 (more than one workgroup, a last workgroup with idle waves)"""
    from fastmax_experiments_amd.block import rms_norm_forward
    for M, eps, offset in ((1, 1e-5, False), (3, 1e-6, True), (130, 1e-5, True)):
        x = _rand((M, C), 7 * C + M, dt, 1.5)
        w = _rand((C,), C + 1, wdt, 0.3) + (0.0 if offset else 1.0)
        _, y, rstd = rms_norm_forward(x, None, w, eps, offset)
        _, y64, rstd64 = br.rmsnorm_ref(_np(x), _np(w), eps, offset, dt, wdt)
        _check_fwd(_np(y), y64, dt, f"rmsnorm C={C} M={M} {dt}/{wdt}", floor=_inner_flip(_np(x), _np(w), rstd64, offset, dt, wdt))
        assert rel_err(_np(rstd), rstd64) < 2e-6


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_rmsnorm_forward_with_a_row_stride_larger_than_c(dt):
    from fastmax_experiments_amd.block import rms_norm_forward
    big = _rand((130, 2048 + 64), 5, dt)
    x = big[:, :2048]
    w = _rand((2048,), 6, dt, 0.3) + 1.0
    assert x.stride(0) == 2048 + 64
    _, y, rstd = rms_norm_forward(x, None, w, 1e-5, False)
    _, y2, rstd2 = rms_norm_forward(x.contiguous(), None, w, 1e-5, False)
    assert torch.equal(y, y2) and torch.equal(rstd, rstd2)
    odd = big[:, 1:2049]                                   # rows that do not start on a 16-byte boundary: the scalar path
    _, y3, _ = rms_norm_forward(odd, None, w, 1e-5, False)
    _, y64, rstd64 = br.rmsnorm_ref(_np(odd), _np(w), 1e-5, False, dt, dt)
    _check_fwd(_np(y3), y64, dt, f"misaligned rows {dt}", floor=_inner_flip(_np(odd), _np(w), rstd64, False, dt, dt))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [72, 2048])
def test_fused_add_norm_is_bitwise_the_add_then_the_norm(C, dt):
    from fastmax_experiments_amd.block import rms_norm_forward
    x, r = _rand((130, C), 11 + C, dt), _rand((130, C), 12 + C, dt, 2.0)
    w = _rand((C,), 13, dt, 0.3) + 1.0
    s, y, rstd = rms_norm_forward(x, r, w, 1e-5, False)
    s_ref = x + r
    _, y_ref, rstd_ref = rms_norm_forward(s_ref, None, w, 1e-5, False)
    assert torch.equal(s, s_ref) and torch.equal(y, y_ref) and torch.equal(rstd, rstd_ref)


# ---- RMSNorm backward ---------------------------------------------------------------------------------------------------------
def _norm_f64(x, w, eps, offset):
    xf = x.double()
    n = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return n * ((1 + w.double()) if offset else w.double())


def _eager_norm(x, w, eps, offset):
    xf = x.float()
    n = (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)).to(x.dtype)
    return n * ((1 + w) if offset else w)


def _bwd_bound(got, eager, ref, dt, what):
    """fp32: 1e-5 of the largest magnitude.  16 bits: twice the restatement's own error, floored at one unit in the last place"""
    scale = np.abs(ref).max()
    e_k = float(np.abs(got - ref).max())
    if dt == "f32":
        print(f"{what}: kernel {e_k / scale:.3e} (bound 1e-5)")
        assert e_k <= 1e-5 * scale, what
        return
    e_e = float(np.abs(eager - ref).max())
    bound = max(2 * e_e, float(br.ulp(scale, dt)))
    print(f"{what}: kernel {e_k:.3e}, restatement {e_e:.3e}, bound {bound:.3e} (scale {scale:.3e})")
    assert e_k <= bound, what


@pytest.mark.parametrize("dt,wdt", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16")])
@pytest.mark.parametrize("M,C", [(130, 72), (1000, 128), (3, 4096), (5, 2048)])     # (5, 2048): one piece per thread in 16 bits
def test_rmsnorm_backward_matches_float64_autograd(M, C, dt, wdt):
    from fastmax_experiments_amd.block import rms_norm_backward, rms_norm_forward
    eps, offset = 1e-5, (C == 128)
    x = _rand((M, C), 21 + C, dt, 1.5)
    w = _rand((C,), 22 + C, wdt, 0.3) + (0.0 if offset else 1.0)
    gy = _rand((M, C), 23 + C, br.out_dtype(dt, wdt))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    _norm_f64(x64, w64, eps, offset).backward(gy.double())
    xe, we = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    _eager_norm(xe, we, eps, offset).backward(gy)
    _, _, rstd = rms_norm_forward(x, None, w, eps, offset)
    ds, dw = rms_norm_backward(gy, x, w, rstd, None, offset, True)
    assert ds.dtype == x.dtype and dw.dtype == torch.float32 and dw.shape == (C,)
    _bwd_bound(_np(ds), _np(xe.grad), _np(x64.grad), dt, f"ds ({M},{C}) {dt}/{wdt}")
    _bwd_bound(_np(dw), _np(we.grad), _np(w64.grad), dt, f"dweight ({M},{C}) {dt}/{wdt}")
    ds2, dw2 = rms_norm_backward(gy, x, w, rstd, None, offset, True)
    assert torch.equal(dw, dw2) and torch.equal(ds, ds2)                      # fixed order: bitwise reproducible
    # the fused add's backward: ds_in is added, to one rounding of the dtype
    ds_in = _rand((M, C), 24 + C, dt)
    ds3, _ = rms_norm_backward(gy, x, w, rstd, ds_in, offset, False)
    want = _np(ds) + _np(ds_in)
    assert np.array_equal(_np(ds3), br.round_to(want, dt))                    # one rounding of the sum of the two, no more
    # dweight not requested: no workspace, ds unchanged
    from fastmax_experiments_amd.block import rms_norm_backward_workspace
    assert rms_norm_backward_workspace(M, C, TD[dt], False) == 0 and rms_norm_backward_workspace(M, C, TD[dt], True) > 0
    ds4, none = rms_norm_backward(gy, x, w, rstd, None, offset, False)
    assert none is None and torch.equal(ds4, ds)


def test_rmsnorm_backward_without_dweight_writes_nothing_else():
    """called through the C ABI with a null dweight and a null workspace: accepted, and a guard tensor next to ds is untouched"""
    from fastmax_experiments_amd import _lib, ops
    M, C = 33, 256
    x, gy = _rand((M, C), 31, "bf16"), _rand((M, C), 32, "bf16")
    w = _rand((C,), 33, "bf16", 0.3) + 1.0
    from fastmax_experiments_amd.block import rms_norm_forward
    _, _, rstd = rms_norm_forward(x, None, w, 1e-5, False)
    buf = torch.full((M + 2, C), 7.0, dtype=torch.bfloat16, device="cuda")
    ds = buf[1:M + 1]
    ws = ops._call("fastmax_hip_rmsnorm_backward", x.device,
                   (gy.data_ptr(), C, x.data_ptr(), C, w.data_ptr(), rstd.data_ptr(), None, 0, ds.data_ptr(), C, None, M, C, 0,
                    _lib.BF16, _lib.BF16), ws=0)
    assert ws is None                                   # accepted (a rejection raises), and no workspace was made
    torch.cuda.synchronize()
    assert bool((buf[0] == 7.0).all()) and bool((buf[M + 1] == 7.0).all()) and not bool((ds == 7.0).all())


def test_c_abi_rejections():
    from fastmax_experiments_amd import _lib
    L = _lib.lib()
    x = _rand((4, 64), 1, "f32")
    w = torch.ones(64, device="cuda")
    y = torch.empty_like(x)
    p = lambda t: t.data_ptr()
    fwd = L.fastmax_hip_rmsnorm_forward
    assert fwd(None, 64, None, 0, p(w), None, 0, p(y), 64, None, 4, 64, 1e-5, 0, _lib.F32, _lib.F32, None) == _lib.E_NULL
    assert fwd(p(x), 64, p(x), 64, p(w), None, 0, p(y), 64, None, 4, 64, 1e-5, 0, _lib.F32, _lib.F32, None) == _lib.E_NULL
    assert fwd(p(x), 64, None, 0, p(w), None, 0, p(y), 64, None, 4, 64, 1e-5, 0, 7, _lib.F32, None) == _lib.E_BAD_DTYPE
    assert fwd(p(x), 64, None, 0, p(w), None, 0, p(y), 64, None, 4, 64, 1e-5, 0, _lib.F32, _lib.BF16, None) == _lib.E_BAD_DTYPE
    assert fwd(p(x), 64, None, 0, p(w), None, 0, p(y), 64, None, 4, 0, 1e-5, 0, _lib.F32, _lib.F32, None) == _lib.E_BAD_SHAPE
    assert fwd(p(x), 32, None, 0, p(w), None, 0, p(y), 64, None, 4, 64, 1e-5, 0, _lib.F32, _lib.F32, None) == _lib.E_BAD_SHAPE
    assert fwd(p(x) + 2, 64, None, 0, p(w), None, 0, p(y), 64, None, 3, 64, 1e-5, 0, _lib.F32, _lib.F32, None) == _lib.E_ALIGNMENT
    g = L.fastmax_hip_gated_act_forward
    assert g(p(x), 64, None, 64, p(y), 64, 4, 64, 0, _lib.F32, None) == _lib.E_NULL
    assert g(p(x), 64, p(x), 64, p(y), 64, 4, 64, 2, _lib.F32, None) == _lib.E_BAD_SHAPE
    assert g(p(x), 64, p(x), 64, p(y), 64, 4, 64, 0, 5, None) == _lib.E_BAD_DTYPE


# ---- gated activation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("mlp_"))
def test_gated_act_forward_matches_fixture_activations(name):
    from fastmax_experiments_amd.block import gated_act_forward
    d, m = load_golden(name)
    dt = m["dtype"]
    a, b = (torch.from_numpy(d[k]).to(TD[dt]).cuda() for k in ("a", "b"))
    assert tuple(a.shape[-2:]) in ((3, 88), (2, 7))
    y = gated_act_forward(a, b, m["act"])
    _check_fwd(_np(y), d["g"], dt, name, ulps=2.0, floor=br.gated_floor(d["a"], d["b"], m["act"]))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("M,I", [(2, 7), (3, 88), (5, 5632)])
def test_gated_act_forward_matches_restatement_and_takes_buffer_halves(M, I, act, dt):
    """(5, 5632) has no fixture (it would be hundreds of KB): the restatement the CPU test proves on the fixtures stands in"""
    from fastmax_experiments_amd.block import gated_act_forward
    ab = _rand((M, 2 * I), 41 + I, dt, 2.0)
    a, b = ab[:, :I], ab[:, I:]
    y_halves = gated_act_forward(a, b, act)
    y_sep = gated_act_forward(a.contiguous(), b.contiguous(), act)
    assert torch.equal(y_halves, y_sep)
    _check_fwd(_np(y_sep), br.gated_ref(_np(a), _np(b), act, dt), dt, f"gated {act} ({M},{I}) {dt}", ulps=2.0,
               floor=br.gated_floor(_np(a), _np(b), act))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("M,I", [(2, 7), (3, 88), (5, 5632)])
def test_gated_act_backward_matches_float64_autograd(M, I, act, dt):
    import torch.nn.functional as F
    from fastmax_experiments_amd.block import gated_act_backward
    f = F.silu if act == "silu" else F.gelu
    a, b, gy = _rand((M, I), 51 + I, dt, 2.0), _rand((M, I), 52 + I, dt), _rand((M, I), 53 + I, dt)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    (f(a64) * b64).backward(gy.double())
    ae, be = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (f(ae) * be).backward(gy)
    da, db = gated_act_backward(a, b, gy, act)
    _bwd_bound(_np(da), _np(ae.grad), _np(a64.grad), dt, f"da {act} ({M},{I}) {dt}")
    _bwd_bound(_np(db), _np(be.grad), _np(b64.grad), dt, f"db {act} ({M},{I}) {dt}")


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("dt,big", [("f32", 60.0), ("f16", 30000.0)])
def test_gated_act_large_arguments_stay_finite(act, dt, big):
    from fastmax_experiments_amd.block import gated_act_backward, gated_act_forward
    a = torch.tensor([[big, -big, big, -big, 0.0, 1.0, -1.0, 0.5]], dtype=TD[dt], device="cuda")
    b = torch.ones_like(a)
    y = gated_act_forward(a, b, act)
    da, db = gated_act_backward(a, b, torch.ones_like(a), act)
    for t in (y, da, db):
        assert bool(torch.isfinite(t).all())
    assert float(y[0, 0]) == big and abs(float(y[0, 1])) < 1e-20 and float(da[0, 0]) == 1.0 and abs(float(da[0, 1])) < 1e-20


# ---- modules on the fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("rmsnorm_"))
def test_rmsnorm_module_reproduces_fixture_outputs_and_gradients(name):
    from fastmax_experiments_amd.block import RMSNorm
    d, m = load_golden(name)
    dt, wdt = m["x_dtype"], m["weight_dtype"]
    odt = br.out_dtype(dt, wdt)
    norm = RMSNorm(m["size"], eps=m["eps"], add_unit_offset=m["add_unit_offset"])
    norm.load_state_dict({"weight": torch.from_numpy(d["weight"])})
    norm.to("cuda", TD[wdt])
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda().requires_grad_(True)
    y = norm(x)
    y.backward(torch.from_numpy(d["gy"]).to(TD[odt]).cuda())
    _check_fwd(_np(y), d["y"], dt, name)
    # gradients: the fixture is the reference in that dtype, itself a few units from float64 -- twice its own error
    x64, w64 = torch.from_numpy(d["x"]).double().requires_grad_(True), torch.from_numpy(d["weight"]).double().requires_grad_(True)
    _norm_f64(x64, w64, m["eps"], m["add_unit_offset"]).backward(torch.from_numpy(d["gy"]).double())
    _bwd_bound(_np(x.grad), d["dx"], _np(x64.grad), dt, name + " dx")
    _bwd_bound(_np(norm.weight.grad), d["dweight"], _np(w64.grad), dt, name + " dweight")
    assert norm.weight.grad.dtype == TD[wdt]


@pytest.mark.parametrize("name", golden_names("mlp_"))
def test_mlp_modules_reproduce_fixture_outputs_and_gradients(name):
    """bounds of tests/test_reference_neighbours.py for LoRALinear on the device: fp32 rtol 1e-5 / atol 1e-6 -> here the
    tensor-scale 2e-5 (three linears deep), 16 bits 2e-2 of the largest magnitude forward and 3e-2 for the gradients"""
    from fastmax_experiments_amd import block
    d, m = load_golden(name)
    dt = m["dtype"]
    mlp = getattr(block, m["fn"])(m["n_embd"], m["intermediate_size"], bias=m["bias"])
    sd = {}
    for lin in ("fc_1", "fc_2", "proj"):
        sd[f"{lin}.linear.weight"] = torch.from_numpy(d[f"{lin}_weight"])
        if m["bias"]:
            sd[f"{lin}.linear.bias"] = torch.from_numpy(d[f"{lin}_bias"])
    mlp.load_state_dict(sd)
    mlp.to("cuda", TD[dt])
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda().requires_grad_(True)
    y = mlp(x)
    y.backward(torch.from_numpy(d["gy"]).to(TD[dt]).cuda())
    fwd_tol, bwd_tol = (2e-5, 2e-5) if dt == "f32" else (2e-2, 3e-2)
    assert rel_err(_np(y), d["y"]) <= fwd_tol
    assert rel_err(_np(x.grad), d["dx"]) <= bwd_tol
    for lin in ("fc_1", "fc_2", "proj"):
        assert rel_err(_np(getattr(mlp, lin).linear.weight.grad), d[f"d_{lin}_weight"]) <= bwd_tol, lin


# ---- Block -------------------------------------------------------------------------------------------------------------------
def _block(alg, dt, n_embd, seed=0, **kw):
    from fastmax_experiments_amd.block import Block
    torch.manual_seed(seed)
    blk = Block(n_embd=n_embd, n_head=4, n_query_groups=2, intermediate_size=176 if n_embd == 64 else 384, attn_alg=alg,
                to_mlp=True, to_projection=True, r=4, **kw)
    for n, p in blk.named_parameters():
        if n.endswith("lora_B"):
            torch.nn.init.normal_(p, std=0.05)
        if n.endswith("norm_1.weight") or n.endswith("norm_2.weight"):
            torch.nn.init.normal_(p, mean=1.0, std=0.2)
    return blk.to("cuda", dt)


@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
@pytest.mark.parametrize("dt,n_embd", [(torch.float32, 64), (torch.bfloat16, 128)])
def test_block_kernels_against_the_tensor_op_restatement(alg, dt, n_embd):
    """fp32: 2e-5; bf16: the bounds test_block_gpu.py uses for the attention sub-layer -- output 5e-3 and input gradient 1e-2
    (its fused_neighbours on / off test), LoRA parameter gradients 3e-2 (its grouped-route A/B test, the same quantity on the
    same kind of block; they are stored in bf16 here, two to four units of which are 1e-2 already)"""
    from fastmax_experiments_amd.attention_block import build_rope_cache
    blk = _block(alg, dt, n_embd)
    B, T = 2, 33
    x = _rand((B, T, n_embd), 61, NAME[dt])
    gy = _rand((B, T, n_embd), 62, NAME[dt])
    cos, sin = build_rope_cache(T, blk.attn.rope_n_elem, device="cuda")
    outs = []
    for fused in (True, False):
        blk.fused_neighbours = fused
        blk.zero_grad()
        xx = x.clone().requires_grad_(True)
        y = blk(xx, cos, sin)
        y.backward(gy)
        grads = {n: _np(p.grad) for n, p in blk.named_parameters() if "lora_" in n}
        assert len(grads) == 10 and all(np.abs(g).max() > 0 for g in grads.values())
        outs.append((_np(y), _np(xx.grad), grads))
    ft, gt, pt = (2e-5, 2e-5, 2e-5) if dt == torch.float32 else (5e-3, 1e-2, 3e-2)
    print(f"block {alg} {dt}: y {rel_err(outs[0][0], outs[1][0]):.3e}, dx {rel_err(outs[0][1], outs[1][1]):.3e}")
    assert rel_err(outs[0][0], outs[1][0]) < ft
    assert rel_err(outs[0][1], outs[1][1]) < gt
    for n in outs[0][2]:
        print(f"    {n}: {rel_err(outs[0][2][n], outs[1][2][n]):.3e}")
        assert rel_err(outs[0][2][n], outs[1][2][n]) < pt, n


@pytest.mark.parametrize("dt,n_embd", [(torch.float32, 64), (torch.bfloat16, 128)])
def test_block_stack_equals_two_block_calls_bitwise(dt, n_embd):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import BlockStack
    b0, b1 = _block("fastmax", dt, n_embd, seed=1), _block("linearmax", dt, n_embd, seed=2)
    stack = BlockStack([b0, b1])
    x = _rand((2, 33, n_embd), 71, NAME[dt])
    gy = _rand((2, 33, n_embd), 72, NAME[dt])
    cos, sin = build_rope_cache(33, b0.attn.rope_n_elem, device="cuda")
    res = []
    for run in (lambda v: stack(v, cos, sin), lambda v: b1(b0(v, cos, sin), cos, sin)):
        stack.zero_grad()
        xx = x.clone().requires_grad_(True)
        y = run(xx)
        y.backward(gy)
        res.append((y.detach(), xx.grad.clone(), [p.grad.clone() for n, p in stack.named_parameters() if "lora_" in n]))
    assert torch.equal(res[0][0], res[1][0])                   # forward: the fused hand-over is the add, then norm_1
    assert torch.equal(res[0][1], res[1][1])
    for g0, g1 in zip(res[0][2], res[1][2]):
        assert torch.equal(g0, g1)


# ---- generation ---------------------------------------------------------------------------------------------------------------
def _heads_side_by_side(blk, n_1, cos, sin, row, alg):
    """the attention of the state-free forward over n_1 (B, L, C) at token `row`, heads laid side by side (what the T = 1
    step's reshape gives; the no-transpose reshape of longer calls, quirk Q3, mixes tokens and is not comparable row by row)"""
    from attention_mechanisms.fastmax import fastmax
    from attention_mechanisms.fastmax_hack import fastmax_hack
    from fastmax_experiments_amd.attention_block import apply_rope
    at = blk.attn
    B, L, _ = n_1.shape
    G, hs = at.n_query_groups, at.head_size
    qpk = at.n_head // G
    qkv = at.attn(n_1).view(B, L, G, qpk + 2, hs)
    q = qkv[:, :, :, :qpk].permute(0, 2, 3, 1, 4).reshape(B, at.n_head, L, hs)
    k, v = (qkv[:, :, :, qpk + i].permute(0, 2, 1, 3).repeat_interleave(qpk, dim=1) for i in (0, 1))
    n = at.rope_n_elem
    q = torch.cat((apply_rope(q[..., :n], cos[:L], sin[:L]), q[..., n:]), dim=-1)
    k = torch.cat((apply_rope(k[..., :n], cos[:L], sin[:L]), k[..., n:]), dim=-1)
    y = fastmax(q, k, v, p=2, mask=True) if alg == "fastmax" else fastmax_hack(q.contiguous(), k.contiguous(), v.contiguous(), p=1, mask=True)
    return at.proj(y[:, :, row].reshape(B, 1, at.n_head * hs))


@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
def test_generation_through_the_whole_block_on_the_state_cache(alg):
    """a 9-token prompt, then three single tokens.  fastmax: each single token against its row of the state-free forward over
    all 12 tokens (masked: a row sees only its prefix).  linearmax: against the state-free forward over that prefix, because
    its rows see whole-sequence statistics.  Tolerance: test_block_generate_gpu.py's T = 1 test, fp32 2e-4 per row."""
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import rms_norm_add
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    from test_block_generate_gpu import _row_err
    blk = _block(alg, torch.float32, 64).eval()
    B, N = 2, 12
    x = _rand((B, N, 64), 81, "f32")
    cos, sin = build_rope_cache(N, blk.attn.rope_n_elem, device="cuda")
    st = (FastmaxDecodeState(B, 4, 16, "cuda", p=2, n_query_groups=2) if alg == "fastmax"
          else LinearmaxDecodeState(B, 4, 16, "cuda", n_query_groups=2))
    worst = 0.0
    with torch.no_grad():
        n_1 = blk.norm_1(x)
        outs = [blk(x[:, a:b], cos[a:b], sin[a:b], torch.arange(a, b, device="cuda"), st) for a, b in ((0, 9), (9, 10), (10, 11), (11, 12))]
        assert outs[0].shape == (B, 9, 64) and st.count == N
        for t, y in zip((9, 10, 11), outs[1:]):
            L = N if alg == "fastmax" else t + 1
            h = _heads_side_by_side(blk, n_1[:, :L], cos, sin, t, alg)
            s, n_2 = rms_norm_add(h, x[:, t:t + 1], blk.norm_2)
            ref = blk.mlp(n_2) + s
            assert y.shape == (B, 1, 64)
            worst = max(worst, _row_err(_np(y), _np(ref)))
    print(f"generation {alg}: worst row {worst:.3e} (bound 2e-4)")
    assert worst < 2e-4


# ---- the captured fine-tune step -----------------------------------------------------------------------------------------------
def test_full_block_step_replayed_as_hip_graph_matches_eager():
    from fastmax_experiments_amd import dp, finetune_step
    from fastmax_experiments_amd.attention_block import build_rope_cache
    dev = torch.device("cuda")
    mb, accum, T = 2, 2, 64
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2 * accum, mb, T, 128, device=dev, generator=g).to(torch.bfloat16)
    tgt = torch.randint(0, 512, (2 * accum, mb, T), device=dev, generator=g)
    finals, losses = [], []
    for graph in (False, True):
        torch.manual_seed(0)
        model = finetune_step.AttentionStack("pythia-14m", 2, "fastmax", vocab=512, lora_dropout=0.0, block="full").prepare(dev)
        assert model.blocks[0].norm_1.weight.dtype == torch.bfloat16 and model.blocks[0].fused_neighbours
        cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(T, model.rope_n_elem, device=dev))
        params = dp.trainable_lora_parameters(model)
        opt = torch.optim.AdamW(params, lr=1e-3)
        st = dp.DataParallelStepper(model, opt, dp.TrainArgs(global_batch_size=mb * accum, micro_batch_size=mb),
                                    lambda m, b: m.loss(b[0], b[1], cos, sin))
        if graph:
            st.capture((x[0], tgt[0]))
        ls = [float(st.micro_step((x[i], tgt[i]))) for i in range(2 * accum)]
        assert st.step_count == 2 and all(np.isfinite(ls))
        losses.append(ls)
        finals.append(torch.cat([p.detach().float().reshape(-1) for p in params]).clone())
    assert losses[0] == losses[1]
    assert torch.equal(finals[0], finals[1])
