"""The NeoX (pythia) block's neighbours of the attention sub-layer on an MI355X (csrc/neox_block.hip, neox_block.py):
LayerNorm forward (single, pair, with the residual adds), its backward with the fixed-order parameter gradients, the exact GELU
forward and backward, the modules on the fixtures, NeoXBlock / NeoXStack with the kernels on against the tensor-op
restatement, generation through the blocks on both state caches, and the fine-tune step.

Bounds are those of tests/test_block_neighbours_gpu.py.  fp32 against float64: 2e-6 of the largest reference magnitude (forward,
mean, rstd), 1e-5 (backward).  16-bit forward: one unit in the last place of the output dtype (exact GELU: beyond
block_ref.gated_floor with b = 1, the float32 cancellation of 1 + erf).  16-bit backward: twice the error the tensor-op
restatement in that dtype makes against the same float64 on the same inputs, floored at one unit in the last place of the
largest magnitude.

One allowance beside the unit of the LayerNorm forward, from the number formats alone (LN_FLOOR).  y = n w + b is evaluated in
float32 from float32 statistics, and where the two terms cancel, the sum keeps their ABSOLUTE float32 error however small it
gets; a bfloat16 output below 2^-15 of its terms has a unit smaller than that.  The terms: mean is a float32 sum of C values,
known to some 2^-24 of the magnitudes summed per level of the summation -- four such units, 2^-22 mean_c|s|, reach y as
|w| rstd times that; n = (s - mean) rstd carries three float32 roundings, the product with w a fourth, and rstd its own float32
error: 2^-21 |n w| in all; b's value enters the rounded sum at 2^-24 |b| at most.  The allowance is far under one unit of the
output wherever the terms do not cancel.  torch's own float32 kernel has the same property (on the CPU its bf16 / f32 result at
C = 2056 is 4 units off at an output of -1.25e-6 = -0.0525516 + 0.0525503), and the 1296-element fixtures never get there."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_ref as br
import neox_ref as nr
from conftest import golden_names, load_golden, rel_err

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAME = {v: k for k, v in TD.items()}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _rand(shape, seed, dt, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(TD[dt]).cuda()


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


def LN_FLOOR(s64, w64, b64, eps):
    """the float32 error of n w + b evaluated from float32 statistics (module docstring)"""
    s64, w64 = np.asarray(s64, np.float64), np.asarray(w64, np.float64)
    nw, _, rstd = nr.layernorm_ref(s64, w64, None, eps, "f32", exact=True)
    from_mean = np.abs(w64) * rstd[..., None] * 2.0 ** -22 * np.abs(s64).mean(-1, keepdims=True)
    return 2.0 ** -21 * np.abs(nw) + from_mean + 2.0 ** -24 * np.abs(0.0 if b64 is None else b64)


def _check_ln(y, mean, rstd, s, w, b, eps, dt, what):
    s64, w64, b64 = _np(s), _np(w), None if b is None else _np(b)
    y64, mean64, rstd64 = nr.layernorm_ref(s64, w64, b64, eps, dt)
    _check_fwd(_np(y), y64, dt, what, floor=LN_FLOOR(s64, w64, b64, eps))
    if mean is not None:
        assert rel_err(_np(mean), mean64.reshape(-1)) < 2e-6, what + " mean"
        assert rel_err(_np(rstd), rstd64.reshape(-1)) < 2e-6, what + " rstd"


def _params(C, seed, wdt):
    return _rand((C,), seed, wdt, 0.3, 1.0), _rand((C,), seed + 1, wdt, 0.2)


# ---- 1. LayerNorm forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("layernorm_"))
def test_layernorm_forward_matches_fixture(name):
    from fastmax_experiments_amd.neox_block import layer_norm_forward
    d, m = load_golden(name)
    dt, wdt = m["x_dtype"], m["weight_dtype"]
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda()
    w, b = (torch.from_numpy(d[k]).to(TD[wdt]).cuda() for k in ("weight", "bias"))
    s, y, y2, mean, rstd = layer_norm_forward(x, w, b, m["eps"])
    assert s is x and y2 is None and y.dtype == TD[dt] and y.shape == x.shape and mean.shape == rstd.shape == (18,)
    _check_fwd(_np(y), d["y"], dt, name, floor=LN_FLOOR(d["x"], d["weight"], d["bias"], m["eps"]))
    _check_ln(y, mean, rstd, x, w, b, m["eps"], dt, name + " float64")


# fp32 pieces hold 4 elements, 16-bit pieces 8: one wave per row up to 64 pieces (C <= 256 / 512), then 1, 2, 4 pieces per
# thread (C <= 1024 / 2048, 2048 / 4096, 4096 / 8192), then the scalar path
C_LIST = [1, 7, 72, 128, 260, 512, 520, 1028, 2048, 2052, 2056, 4100, 4104, 8200]


@pytest.mark.parametrize("dt,wdt", PAIRS)
@pytest.mark.parametrize("C", C_LIST)
def test_layernorm_forward_matches_float64(C, dt, wdt):
    """every launch shape: scalar (1, 7: no whole pieces; 4100 in fp32 and 8200 in 16 bits: more than 1024 pieces), a wave per
    row (72, 128; 512 in 16 bits), 1 / 2 / 4 pieces per thread and the first C past each step (fp32: 260, 1028, 2052, 4100;
    16 bits: 520, 2056, 4104, 8200), rows at M = 1, 3, 130 (more than one workgroup, a last workgroup with idle waves)"""
    from fastmax_experiments_amd.neox_block import layer_norm_forward
    for M, eps in ((1, 1e-5), (3, 1e-6), (130, 1e-5)):
        x = _rand((M, C), 7 * C + M, dt, 1.5, 0.4)
        w, b = _params(C, C + 1, wdt)
        _, y, _, mean, rstd = layer_norm_forward(x, w, b, eps)
        _check_ln(y, mean, rstd, x, w, b, eps, dt, f"layernorm C={C} M={M} {dt}/{wdt}")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_layernorm_forward_row_strides_misaligned_rows_and_null_outputs(dt):
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.neox_block import layer_norm_forward
    big = _rand((130, 2048 + 64), 5, dt, 1.0, -0.3)
    x = big[:, :2048]
    w, b = _params(2048, 6, dt)
    assert x.stride(0) == 2048 + 64
    _, y, _, mean, rstd = layer_norm_forward(x, w, b, 1e-5)
    _, y2, _, mean2, rstd2 = layer_norm_forward(x.contiguous(), w, b, 1e-5)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    odd = big[:, 1:2049]                                   # rows that do not start on a 16-byte boundary: the scalar path
    _, y3, _, mean3, rstd3 = layer_norm_forward(odd, w, b, 1e-5)
    _check_ln(y3, mean3, rstd3, odd, w, b, 1e-5, dt, f"misaligned rows {dt}")
    # b, mean and rstd may be NULL: the same y as with a zero bias
    _, y0, _, _, _ = layer_norm_forward(x, w, torch.zeros_like(w), 1e-5)
    _, yn, _, _, _ = layer_norm_forward(x, w, None, 1e-5)
    raw = torch.empty_like(y0)
    ops._call("fastmax_hip_layernorm_forward", x.device,
              (x.data_ptr(), x.stride(0), None, 0, None, 0, w.data_ptr(), None, None, None, None, 0, raw.data_ptr(), 2048, None, 0,
               None, None, 130, 2048, 1e-5, ops._DT[TD[dt]], ops._DT[TD[dt]]))
    assert torch.equal(yn, y0) and torch.equal(raw, y0)


# ---- 2. pair and residual forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,wdt", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16")])
@pytest.mark.parametrize("C", [7, 72, 2048])
@pytest.mark.parametrize("res", [0, 1, 2], ids=["no_residual", "r1", "r1_r2"])
def test_pair_and_residual_forms(res, C, dt, wdt):
    """s is bitwise torch's m + h + x (exact roundings); y1 of the pair is bitwise the single norm's y on that s, y2 likewise
    under its own parameters; both meet the forward bounds on s"""
    from fastmax_experiments_amd.neox_block import layer_norm_forward
    M = 130
    x, m, h = _rand((M, C), 11 + C, dt, 1.0, 0.2), _rand((M, C), 12 + C, dt, 2.0), _rand((M, C), 13 + C, dt, 0.7)
    w1, b1 = _params(C, 14, wdt)
    w2, b2 = _params(C, 16, wdt)
    r1, r2 = (m if res >= 1 else None), (h if res == 2 else None)
    s_ref = x if res == 0 else (x + m if res == 1 else m + h + x)
    s, y1, y2, mean, rstd = layer_norm_forward(x, w1, b1, 1e-5, r1, r2, w2, b2)
    assert torch.equal(s, s_ref) and (res > 0 or s is x)
    _, ya, none, mean_a, rstd_a = layer_norm_forward(s_ref, w1, b1, 1e-5)
    _, yb, _, _, _ = layer_norm_forward(s_ref, w2, b2, 1e-5)
    assert none is None
    assert torch.equal(y1, ya) and torch.equal(y2, yb) and torch.equal(mean, mean_a) and torch.equal(rstd, rstd_a)
    _check_ln(y1, mean, rstd, s_ref, w1, b1, 1e-5, dt, f"pair y1 C={C} {dt}/{wdt} res={res}")
    _check_ln(y2, None, None, s_ref, w2, b2, 1e-5, dt, f"pair y2 C={C} {dt}/{wdt} res={res}")
    assert np.array_equal(_np(s), nr.stream_ref(_np(x), None if r1 is None else _np(r1), None if r2 is None else _np(r2), dt))


# ---- 3. LayerNorm backward -------------------------------------------------------------------------------------------------------
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


def _eager_ln(x, w, b, eps):
    if w.dtype != x.dtype:                  # torch's device kernel wants one dtype: float32 arithmetic, one rounding
        return F.layer_norm(x.float(), x.shape[-1:], w, b, eps).to(x.dtype)
    return F.layer_norm(x, x.shape[-1:], w, b, eps)


@pytest.mark.parametrize("dt,wdt", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16")])
@pytest.mark.parametrize("M,C", [(1, 72), (3, 4104), (130, 72), (130, 7), (1000, 128), (5, 2048)])
def test_layernorm_backward_matches_float64_autograd(M, C, dt, wdt):
    """the pair with ds_in and the single norm without, at a wave per row (72, 128), the scalar path (7; 4104 in fp32), 1 and 4
    pieces per thread (2048, 4104 in 16 bits); M = 1000 spans 63 row blocks of the partial sums"""
    from fastmax_experiments_amd.neox_block import layer_norm_backward, layer_norm_backward_workspace, layer_norm_forward
    eps = 1e-5
    s = _rand((M, C), 21 + C, dt, 1.5, 0.4)
    (w1, b1), (w2, b2) = _params(C, 22 + C, wdt), _params(C, 24 + C, wdt)
    gy1, gy2, ds_in = (_rand((M, C), 26 + C + i, dt) for i in range(3))
    _, _, _, mean, rstd = layer_norm_forward(s, w1, b1, eps)
    for pair in (True, False):
        p64 = [t.double().requires_grad_(True) for t in ((s, w1, b1, w2, b2) if pair else (s, w1, b1))]
        pe = [t.clone().requires_grad_(True) for t in ((s, w1, b1, w2, b2) if pair else (s, w1, b1))]
        for ts, gs, ln in ((p64, [g.double() for g in (gy1, gy2)], lambda x, w, b: F.layer_norm(x, (C,), w, b, eps)),
                           (pe, [gy1, gy2], lambda x, w, b: _eager_ln(x, w, b, eps))):
            outs = [ln(ts[0], ts[1], ts[2])] + ([ln(ts[0], ts[3], ts[4])] if pair else [])
            torch.autograd.backward(outs, gs[:len(outs)])
        want = (True,) * (4 if pair else 2) + (False,) * (0 if pair else 2)
        got = layer_norm_backward(gy1, s, w1, mean, rstd, gy2 if pair else None, w2 if pair else None, ds_in if pair else None, want)
        ds_ref, ds_eager = _np(p64[0].grad), pe[0].grad
        if pair:
            ds_ref, ds_eager = ds_ref + _np(ds_in), ds_eager + ds_in
        tag = f"({M},{C}) {dt}/{wdt} {'pair' if pair else 'single'}"
        assert got[0].dtype == s.dtype and got[0].shape == s.shape
        _bwd_bound(_np(got[0]), _np(ds_eager), ds_ref, dt, "ds " + tag)
        for k, nm in enumerate(("dw1", "db1", "dw2", "db2")[:len(p64) - 1]):
            assert got[1 + k].dtype == torch.float32 and got[1 + k].shape == (C,)
            _bwd_bound(_np(got[1 + k]), _np(pe[1 + k].grad), _np(p64[1 + k].grad), dt, f"{nm} {tag}")
        assert got[3] is None or pair
        again = layer_norm_backward(gy1, s, w1, mean, rstd, gy2 if pair else None, w2 if pair else None, ds_in if pair else None, want)
        for a, b in zip(got, again):
            assert (a is None and b is None) or torch.equal(a, b)                 # fixed order: bitwise reproducible
        # no parameter gradient wanted: no workspace, ds unchanged; only some wanted: those unchanged
        assert layer_norm_backward_workspace(M, C, TD[dt], pair, False) == 0 and layer_norm_backward_workspace(M, C, TD[dt], pair, True) > 0
        bare = layer_norm_backward(gy1, s, w1, mean, rstd, gy2 if pair else None, w2 if pair else None, ds_in if pair else None)
        assert torch.equal(bare[0], got[0]) and all(g is None for g in bare[1:])
        some = layer_norm_backward(gy1, s, w1, mean, rstd, gy2 if pair else None, w2 if pair else None, None, (False, True, False, pair))
        assert some[1] is None and some[3] is None and torch.equal(some[2], got[2]) and (not pair or torch.equal(some[4], got[4]))
        if pair:                                     # ds_in is added to the rounded result: one rounding of the sum of the two
            assert np.array_equal(_np(got[0]), br.round_to(_np(some[0]) + _np(ds_in), dt))


def test_layernorm_backward_without_parameter_gradients_writes_nothing_else():
    """called through the C ABI with null gradients and a null workspace: accepted, and guard rows next to ds are untouched"""
    from fastmax_experiments_amd import _lib, ops
    from fastmax_experiments_amd.neox_block import layer_norm_forward
    M, C = 33, 256
    s, gy1, gy2 = _rand((M, C), 31, "bf16"), _rand((M, C), 32, "bf16"), _rand((M, C), 33, "bf16")
    (w1, b1), (w2, _) = _params(C, 34, "bf16"), _params(C, 36, "bf16")
    _, _, _, mean, rstd = layer_norm_forward(s, w1, b1, 1e-5)
    buf = torch.full((M + 2, C), 7.0, dtype=torch.bfloat16, device="cuda")
    ds = buf[1:M + 1]
    ws = ops._call("fastmax_hip_layernorm_backward", s.device,
                   (gy1.data_ptr(), C, gy2.data_ptr(), C, s.data_ptr(), C, w1.data_ptr(), w2.data_ptr(), mean.data_ptr(),
                    rstd.data_ptr(), None, 0, ds.data_ptr(), C, None, None, None, None, M, C, _lib.BF16, _lib.BF16), ws=0)
    assert ws is None                                   # accepted (a rejection raises), and no workspace was made
    torch.cuda.synchronize()
    assert bool((buf[0] == 7.0).all()) and bool((buf[M + 1] == 7.0).all()) and not bool((ds == 7.0).all())


# ---- 4. GELU ----------------------------------------------------------------------------------------------------------------------
def _gelu_inputs(M, I, dt, seed):
    """the whole range [-12, 12], the negative tail included, in a seeded order, with both ends present"""
    g = torch.Generator().manual_seed(seed)
    a = torch.linspace(-12.0, 12.0, M * 2 * I)[torch.randperm(M * 2 * I, generator=g)].view(M, 2 * I)
    a[0, 0], a[-1, I - 1] = -12.0, 12.0
    return a.to(TD[dt]).cuda()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("I", [1, 7, 88, 2048])
def test_gelu_forward_and_backward(I, dt):
    """a is the left half of an (M, 2 I) buffer (a row stride that is not the row length; at I = 1, 7 rows off the 16-byte
    grid); the contiguous copy gives the same bits"""
    from fastmax_experiments_amd.neox_block import gelu_backward, gelu_forward
    M = 5
    a = _gelu_inputs(M, I, dt, 41 + I)[:, :I]
    assert a.stride(0) == 2 * I and float(a.min()) == -12.0 and float(a.max()) == 12.0
    y = gelu_forward(a)
    assert torch.equal(y, gelu_forward(a.contiguous())) and y.dtype == a.dtype and y.shape == a.shape
    _check_fwd(_np(y), nr.gelu_ref(_np(a), dt), dt, f"gelu ({M},{I}) {dt}", ulps=1.0, floor=nr.gelu_floor(_np(a)))
    gy = _rand((M, 2 * I), 43 + I, dt)[:, I:]
    a64 = a.double().requires_grad_(True)
    F.gelu(a64).backward(gy.double())
    ae = a.clone().requires_grad_(True)
    F.gelu(ae).backward(gy)
    da = gelu_backward(a, gy)
    assert torch.equal(da, gelu_backward(a.contiguous(), gy.contiguous()))
    _bwd_bound(_np(da), _np(ae.grad), _np(a64.grad), dt, f"gelu backward ({M},{I}) {dt}")


@pytest.mark.parametrize("dt,big", [("f32", 60.0), ("f16", 30000.0)])
def test_gelu_large_arguments_stay_finite(dt, big):
    from fastmax_experiments_amd.neox_block import gelu_backward, gelu_forward
    a = torch.tensor([[big, -big, big, -big, 0.0, 1.0, -1.0, 0.5]], dtype=TD[dt], device="cuda")
    y, da = gelu_forward(a), gelu_backward(a, torch.ones_like(a))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(da).all())
    assert float(y[0, 0]) == big and abs(float(y[0, 1])) < 1e-20 and float(da[0, 0]) == 1.0 and abs(float(da[0, 1])) < 1e-20


# ---- 5. modules on the fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("layernorm_"))
def test_layernorm_module_reproduces_fixture_outputs_and_gradients(name):
    from fastmax_experiments_amd.neox_block import LayerNorm
    d, m = load_golden(name)
    dt, wdt = m["x_dtype"], m["weight_dtype"]
    norm = LayerNorm(m["size"], eps=m["eps"])
    norm.load_state_dict({"weight": torch.from_numpy(d["weight"]), "bias": torch.from_numpy(d["bias"])})
    norm.to("cuda", TD[wdt])
    norm.fused_neighbours = True
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda().requires_grad_(True)
    y = norm(x)
    y.backward(torch.from_numpy(d["gy"]).to(TD[dt]).cuda())
    _check_fwd(_np(y), d["y"], dt, name, floor=LN_FLOOR(d["x"], d["weight"], d["bias"], m["eps"]))
    # gradients: the fixture is the reference in that dtype, itself a few units from float64 -- twice its own error
    t64 = [torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("x", "weight", "bias")]
    F.layer_norm(t64[0], (m["size"],), t64[1], t64[2], m["eps"]).backward(torch.from_numpy(d["gy"]).double())
    _bwd_bound(_np(x.grad), d["dx"], _np(t64[0].grad), dt, name + " dx")
    _bwd_bound(_np(norm.weight.grad), d["dweight"], _np(t64[1].grad), dt, name + " dweight")
    _bwd_bound(_np(norm.bias.grad), d["dbias"], _np(t64[2].grad), dt, name + " dbias")
    assert norm.weight.grad.dtype == TD[wdt] and norm.bias.grad.dtype == TD[wdt]


@pytest.mark.parametrize("name", golden_names("neox_mlp_"))
def test_neox_mlp_reproduces_fixture_outputs_and_gradients(name):
    """bounds of test_block_neighbours_gpu.py for the gated MLPs (LoRALinear on the device): fp32 the tensor-scale 2e-5, 16 bits
    2e-2 of the largest magnitude forward and 3e-2 for the gradients; the activation alone at the forward bounds of test 4"""
    from fastmax_experiments_amd.neox_block import GptNeoxMLP, gelu_forward
    d, m = load_golden(name)
    dt = m["dtype"]
    a = torch.from_numpy(d["a"]).to(TD[dt]).cuda()
    _check_fwd(_np(gelu_forward(a)), nr.gelu_ref(d["a"], dt), dt, name + " gelu", floor=nr.gelu_floor(d["a"]))
    mlp = GptNeoxMLP(m["n_embd"], m["intermediate_size"], bias=m["bias"])
    sd = {}
    for lin in ("fc", "proj"):
        sd[f"{lin}.linear.weight"] = torch.from_numpy(d[f"{lin}_weight"])
        if m["bias"]:
            sd[f"{lin}.linear.bias"] = torch.from_numpy(d[f"{lin}_bias"])
    mlp.load_state_dict(sd)
    mlp.to("cuda", TD[dt])
    mlp.fused_neighbours = True
    x = torch.from_numpy(d["x"]).to(TD[dt]).cuda().requires_grad_(True)
    y = mlp(x)
    y.backward(torch.from_numpy(d["gy"]).to(TD[dt]).cuda())
    fwd_tol, bwd_tol = (2e-5, 2e-5) if dt == "f32" else (2e-2, 3e-2)
    assert rel_err(_np(y), d["y"]) <= fwd_tol
    assert rel_err(_np(x.grad), d["dx"]) <= bwd_tol
    for lin in ("fc", "proj"):
        assert rel_err(_np(getattr(mlp, lin).linear.weight.grad), d[f"d_{lin}_weight"]) <= bwd_tol, lin
        if m["bias"]:
            assert rel_err(_np(getattr(mlp, lin).linear.bias.grad), d[f"d_{lin}_bias"]) <= bwd_tol, lin


# ---- 6. NeoXBlock and NeoXStack ----------------------------------------------------------------------------------------------------
def _block(alg, dt, seed=0, **kw):
    from fastmax_experiments_amd.neox_block import NeoXBlock
    torch.manual_seed(seed)
    blk = NeoXBlock.from_config("pythia-14m", attn_alg=alg, to_mlp=True, to_projection=True, r=4, **kw)
    for n, p in blk.named_parameters():
        if n.endswith("lora_B"):
            torch.nn.init.normal_(p, std=0.05)
        if n.startswith("norm_") and n.endswith("weight"):
            torch.nn.init.normal_(p, mean=1.0, std=0.2)
        if n.startswith("norm_") and n.endswith("bias"):
            torch.nn.init.normal_(p, mean=0.0, std=0.2)
    blk.fused_neighbours = True             # the kernels are opt-in
    return blk.to("cuda", dt)


def _trained(module):
    return {n: p for n, p in module.named_parameters() if "lora_" in n or "norm_" in n}


@pytest.mark.parametrize("shared", [False, True], ids=["two_norms", "shared_norm"])
@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
def test_neox_block_kernels_against_the_tensor_op_restatement(alg, shared):
    """pythia-14m, bf16, T = 33.  The bounds test_block_neighbours_gpu.py uses for Block against its restatement in bf16: output
    5e-3, input gradient 1e-2, parameter gradients (LoRA and, here, the norms') 3e-2"""
    from fastmax_experiments_amd.attention_block import build_rope_cache
    blk = _block(alg, torch.bfloat16, shared_attention_norm=shared)
    B, T, C = 2, 33, 128
    x, gy = _rand((B, T, C), 61, "bf16"), _rand((B, T, C), 62, "bf16")
    cos, sin = build_rope_cache(T, blk.attn.rope_n_elem, device="cuda")
    outs = []
    for fused in (True, False):
        blk.fused_neighbours = fused
        blk.zero_grad()
        xx = x.clone().requires_grad_(True)
        y = blk(xx, cos, sin)
        y.backward(gy)
        grads = {n: _np(p.grad) for n, p in _trained(blk).items()}
        assert len(grads) == 8 + (2 if shared else 4) and all(np.abs(g).max() > 0 for g in grads.values())
        outs.append((_np(y), _np(xx.grad), grads))
    print(f"neox block {alg}: y {rel_err(outs[0][0], outs[1][0]):.3e}, dx {rel_err(outs[0][1], outs[1][1]):.3e}")
    assert rel_err(outs[0][0], outs[1][0]) < 5e-3
    assert rel_err(outs[0][1], outs[1][1]) < 1e-2
    for n in outs[0][2]:
        print(f"    {n}: {rel_err(outs[0][2][n], outs[1][2][n]):.3e}")
        assert rel_err(outs[0][2][n], outs[1][2][n]) < 3e-2, n


def test_neox_stack_equals_block_by_block_bitwise_and_meets_the_restatement():
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.neox_block import NeoXStack
    dt = torch.bfloat16
    blocks = [_block("fastmax", dt, seed=1), _block("linearmax", dt, seed=2, shared_attention_norm=True), _block("fastmax", dt, seed=3)]
    stack = NeoXStack(blocks)
    x, gy = _rand((2, 33, 128), 71, "bf16"), _rand((2, 33, 128), 72, "bf16")
    cos, sin = build_rope_cache(33, blocks[0].attn.rope_n_elem, device="cuda")

    def by_block(v):
        for b in blocks:
            v = b(v, cos, sin)
        return v

    res = []
    for fused, run in ((True, lambda v: stack(v, cos, sin)), (True, by_block), (False, lambda v: stack(v, cos, sin))):
        for b in blocks:
            b.fused_neighbours = fused
        stack.zero_grad()
        xx = x.clone().requires_grad_(True)
        y = run(xx)
        y.backward(gy)
        res.append((y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in _trained(stack).items()}))
    assert torch.equal(res[0][0], res[1][0])                   # forward: the fused hand-over is the two adds, then both norms
    assert torch.equal(res[0][1], res[1][1])                   # and its backward the accumulation autograd would do
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n
    assert rel_err(_np(res[0][0]), _np(res[2][0])) < 5e-3 and rel_err(_np(res[0][1]), _np(res[2][1])) < 1e-2
    for n in res[0][2]:
        assert rel_err(_np(res[0][2][n]), _np(res[2][2][n])) < 3e-2, n


# ---- 7. generation ------------------------------------------------------------------------------------------------------------------
def _states(alg, B, n):
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    if alg == "fastmax":
        return [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(n)]
    return [LinearmaxDecodeState(B, 4, 32, "cuda", n_query_groups=4) for _ in range(n)]


@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
def test_generation_through_two_neox_blocks_on_the_state_cache(alg):
    """a 9-token prompt, then five single tokens, through two pythia-14m blocks.  Each block's single-token rows against the
    whole-sequence forward over the tokens that block was fed, exactly as test_block_neighbours_gpu.py does for Block: the
    state-free attention over all 14 tokens (masked: a row sees only its prefix; linearmax: over that prefix, because its rows
    see whole-sequence statistics), heads laid side by side, then both norms, the MLP and the three-way add in tensor ops.
    Tolerance: test_block_generate_gpu.py's, fp32 2e-4 per row.  The stack on fresh caches gives the same bits."""
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.neox_block import NeoXStack
    from test_block_generate_gpu import TOL, _row_err
    from test_block_neighbours_gpu import _heads_side_by_side
    blocks = [_block(alg, torch.float32, seed=4).eval(), _block(alg, torch.float32, seed=5).eval()]
    B, N, C = 2, 14, 128
    x = _rand((B, N, C), 81, "f32")
    cos, sin = build_rope_cache(N, blocks[0].attn.rope_n_elem, device="cuda")
    calls = [(0, 9)] + [(t, t + 1) for t in range(9, N)]
    states = _states(alg, B, 2)
    worst = 0.0
    with torch.no_grad():
        fed = [[], []]                       # what each block was fed, call by call
        outs = []
        for a, b in calls:
            v = x[:, a:b]
            for i, blk in enumerate(blocks):
                fed[i].append(v)
                v = blk(v, cos[a:b], sin[a:b], torch.arange(a, b, device="cuda"), states[i])
            outs.append(v)
        assert outs[0].shape == (B, 9, C) and all(st.count == N for st in states)
        for i, blk in enumerate(blocks):
            xi = torch.cat(fed[i], dim=1)
            blk.fused_neighbours = False
            n_1 = blk.norm_1(xi)
            for t in range(9, N):
                L = N if alg == "fastmax" else t + 1
                h = _heads_side_by_side(blk, n_1[:, :L], cos, sin, t, alg)
                xt = xi[:, t:t + 1]
                ref = blk.mlp(blk.norm_2(xt)) + h + xt
                got = fed[i + 1][t - 8] if i == 0 else outs[t - 8]
                assert got.shape == (B, 1, C)
                worst = max(worst, _row_err(_np(got), _np(ref)))
            blk.fused_neighbours = True
        fresh = _states(alg, B, 2)
        stack = NeoXStack(blocks)
        for (a, b), want in zip(calls, outs):
            assert torch.equal(stack(x[:, a:b], cos[a:b], sin[a:b], torch.arange(a, b, device="cuda"), fresh), want)
    print(f"neox generation {alg}: worst row {worst:.3e} (bound {TOL[torch.float32]:.0e})")
    assert worst < TOL[torch.float32]


@pytest.mark.parametrize("alg", ["fastmax", "linearmax"])
def test_generate_through_a_neox_stack_with_a_layernorm_head_is_greedy(alg):
    """temperature 0: every token generate() returns is the argmax of the logits the tensor-op head (LayerNorm, then the whole
    lm_head) gives for the same sequence fed through the blocks on fresh caches in the same calls.  A tie within the float32
    error of the two heads (1e-5 of the largest logit) may go either way."""
    from fastmax_experiments_amd import generate
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.neox_block import LayerNorm, NeoXStack
    stack = NeoXStack([_block(alg, torch.float32, seed=6).eval(), _block(alg, torch.float32, seed=7).eval()])
    B, T, n_max, V, C = 2, 9, 14, 515, 128
    torch.manual_seed(8)
    head = generate.NextTokenHead(C, V, norm_class="LayerNorm").to("cuda").eval()
    assert isinstance(head.ln_f, LayerNorm)
    with torch.no_grad():
        head.ln_f.weight.normal_(1.0, 0.2)
        head.ln_f.bias.normal_(0.0, 0.2)
    wte = _rand((V, C), 91, "f32")
    prompt = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(92)).cuda()
    cos, sin = build_rope_cache(n_max, stack.blocks[0].attn.rope_n_elem, device="cuda")
    tokens = generate.generate(wte, stack, head, _states(alg, B, 2), prompt, n_max, cos=cos, sin=sin, temperature=0.0)
    assert tokens.shape == (B, n_max) and torch.equal(tokens[:, :T], prompt)
    as_list = generate.generate(wte, list(stack.blocks), head, _states(alg, B, 2), prompt, n_max, cos=cos, sin=sin, temperature=0.0)
    assert torch.equal(as_list, tokens)
    fresh = _states(alg, B, 2)
    pos = torch.arange(n_max, device="cuda")
    with torch.no_grad():
        for a, b in [(0, T)] + [(t, t + 1) for t in range(T, n_max - 1)]:
            hidden = stack(F.embedding(tokens[:, a:b], wte), cos[a:b], sin[a:b], pos[a:b], fresh)
            fused = head.logits(hidden)
            head.fused = False
            eager = head.logits(hidden)
            head.fused = True
            assert rel_err(_np(fused), _np(eager)) < 1e-5
            chosen = eager.gather(1, tokens[:, b:b + 1])[:, 0]
            assert bool((chosen >= eager.max(dim=1).values - 1e-5 * eager.abs().max()).all()), (a, b)


# ---- 8. the fine-tune step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["kernels_on", "kernels_off"])
def test_finetune_step_with_neox_blocks_runs_and_reproduces(fused, monkeypatch):
    """two optimizer steps without dropout: the loss is finite and bitwise the same in a second run.  The step builds its own
    model, so the kernels (opt-in) are switched on through the modules' default"""
    from fastmax_experiments_amd import finetune_step, neox_block
    monkeypatch.setattr(neox_block, "FUSED_NEIGHBOURS_DEFAULT", fused)
    losses = []
    for _ in range(2):
        torch.manual_seed(0)
        r = finetune_step.run("pythia-14m", 2, "fastmax", seq=64, micro_batch=2, accum=1, steps=2, warmup=0,
                              device=torch.device("cuda"), lora_dropout=0.0, block="neox")
        assert r["optimizer_steps"] == 2 and np.isfinite(r["last_loss"])
        losses.append(r["last_loss"])
    assert losses[0] == losses[1]
