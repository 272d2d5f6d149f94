"""The NeoX (pythia) block's neighbours of the attention sub-layer, everything that needs no device
(include/fastmax_hip_neox.h, csrc/neox_block.hip, fastmax_experiments_amd/neox_block.py, tests/golden/layernorm_*.npz and
neox_mlp_*.npz):

1. the source in the build's list, the workspace query (the binding table against this header: test_binding_cpu);
2. every rejection the header lists, returned on made-up aligned addresses before any launch;
3. the float64 restatements in neox_ref.py reproduce every fixture: 16-bit forward to one unit in the last place (GELU: beyond
   the float32 cancellation allowance 2^-23 |a|), fp32 below 2e-6, the fp32 fixtures' gradients against float64 autograd below
   1e-5.  The GPU tests lean on these restatements at the shapes the fixtures do not have;
4. with fused_neighbours = False the modules reproduce the fixtures on the CPU bit for bit;
5. state-dict keys are the reference's; error paths: ValueError for malformed shapes, "no CPU path" for CPU tensors through the
   kernel wrappers, NotImplementedError for the tanh GELU; AttentionStack(block="neox") builds NeoXBlocks."""

import numpy as np
import pytest
import torch

import block_ref as br
import neox_ref as nr
from conftest import golden_names, load_golden, rel_err
from fastmax_experiments_amd import _lib

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ---- 1. the build, the workspace query (the binding itself: test_binding_cpu) ---------------------------------------------------
def test_the_build_compiles_the_source():
    from fastmax_experiments_amd import build
    assert "neox_block.hip" in build.SOURCES


def test_workspace_query_needs_no_device():
    q = _lib.lib().fastmax_hip_layernorm_backward_workspace
    assert q(1000, 128, _lib.BF16, 1, 0) == 0 and q(0, 128, _lib.F32, 1, 1) == 0 and q(5, 128, 7, 1, 1) == 0
    assert q(1000, 128, _lib.BF16, 1, 1) == ((1000 + 15) // 16) * 4 * 128 * 4    # dw1, db1, dw2, db2: a float32 row each per 16 rows
    assert q(1000, 128, _lib.BF16, 0, 1) == ((1000 + 15) // 16) * 2 * 128 * 4
    assert q(3, 4096, _lib.F32, 0, 1) == 2 * 4096 * 4


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _fwd(**over):
    a = dict(x=A, xs=72, r1=A, r1s=72, r2=A, r2s=72, w1=A, b1=A, w2=A, b2=A, s=A, ss=72, y1=A, y1s=72, y2=A, y2s=72, mean=A, rstd=A,
             M=4, C=72, eps=1e-5, dtype=_lib.BF16, wdtype=_lib.BF16, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_layernorm_forward(*a.values())


def _bwd(**over):
    a = dict(dy1=A, dy1s=72, dy2=A, dy2s=72, s=A, ss=72, w1=A, w2=A, mean=A, rstd=A, di=A, dis=72, ds=A, dss=72, dw1=A, db1=A, dw2=A,
             db2=A, M=4, C=72, dtype=_lib.BF16, wdtype=_lib.BF16, ws=A, wsb=1 << 20, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_layernorm_backward(*a.values())


def _act(bwd=False, **over):
    a = dict(a=A, as_=88, dy=A, dys=88, out=A, os=88, M=3, I=88, act=_lib.NEOX_ACT_GELU, dtype=_lib.F16, stream=None)
    a.update(over)
    if not bwd:
        a.pop("dy"), a.pop("dys")
    fn = _lib.lib().fastmax_hip_act_backward if bwd else _lib.lib().fastmax_hip_act_forward
    return fn(*a.values())


def test_layernorm_forward_rejects_bad_calls_before_any_launch():
    for missing in ("x", "w1", "y1"):
        assert _fwd(**{missing: None}) == _lib.E_NULL, missing
    assert _fwd(r1=None) == _lib.E_NULL                      # r2 without r1
    assert _fwd(s=None) == _lib.E_NULL                       # a residual without s_out
    assert _fwd(y2=None) == _lib.E_NULL                      # w2 without y2
    assert _fwd(w2=None) == _lib.E_NULL                      # b2 without w2
    for dt in (-1, 3):
        assert _fwd(dtype=dt, wdtype=_lib.F32) == _lib.E_BAD_DTYPE
    assert _fwd(dtype=_lib.BF16, wdtype=_lib.F16) == _lib.E_BAD_DTYPE and _fwd(dtype=_lib.F32, wdtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(M=0), dict(C=0), dict(M=-2), dict(xs=71), dict(r1s=71), dict(r2s=8), dict(ss=71), dict(y1s=71), dict(y2s=0)):
        assert _fwd(**bad) == _lib.E_BAD_SHAPE, bad
    for odd in ("x", "r1", "r2", "w1", "b1", "w2", "b2", "s", "y1", "y2"):
        assert _fwd(**{odd: A + 1}) == _lib.E_ALIGNMENT, odd
    assert _fwd(mean=A + 2) == _lib.E_ALIGNMENT and _fwd(rstd=A + 1) == _lib.E_ALIGNMENT
    assert _fwd(dtype=_lib.F32, wdtype=_lib.F32, x=A + 2) == _lib.E_ALIGNMENT
    assert _fwd(wdtype=_lib.F32, w1=A + 2) == _lib.E_ALIGNMENT


def test_layernorm_backward_rejects_bad_calls_before_any_launch():
    for missing in ("dy1", "s", "w1", "mean", "rstd", "ds"):
        assert _bwd(**{missing: None}) == _lib.E_NULL, missing
    assert _bwd(dy2=None) == _lib.E_NULL and _bwd(w2=None) == _lib.E_NULL        # dy2 and w2 come together
    assert _bwd(dy2=None, w2=None, db2=None) == _lib.E_NULL                       # a gradient of a norm that is not there
    assert _bwd(ws=None) == _lib.E_NULL                                           # parameter gradients without a workspace
    for dt in (-1, 3):
        assert _bwd(dtype=dt, wdtype=_lib.F32) == _lib.E_BAD_DTYPE
    assert _bwd(dtype=_lib.F16, wdtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(M=0), dict(C=-1), dict(dy1s=71), dict(dy2s=71), dict(ss=1), dict(dis=71), dict(dss=71)):
        assert _bwd(**bad) == _lib.E_BAD_SHAPE, bad
    for odd in ("dy1", "dy2", "s", "w1", "w2", "di", "ds"):
        assert _bwd(**{odd: A + 1}) == _lib.E_ALIGNMENT, odd
    for odd in ("mean", "rstd", "dw1", "db1", "dw2", "db2"):
        assert _bwd(**{odd: A + 2}) == _lib.E_ALIGNMENT, odd
    assert _bwd(ws=A + 8) == _lib.E_ALIGNMENT
    need = _lib.lib().fastmax_hip_layernorm_backward_workspace(4, 72, _lib.BF16, 1, 1)
    assert need == 4 * 72 * 4 and _bwd(wsb=need - 1) == _lib.E_WORKSPACE


def test_act_rejects_bad_calls_before_any_launch():
    for bwd in (False, True):
        for missing in ("a", "out") + (("dy",) if bwd else ()):
            assert _act(bwd, **{missing: None}) == _lib.E_NULL, missing
        for dt in (-1, 3):
            assert _act(bwd, dtype=dt) == _lib.E_BAD_DTYPE
        for bad in (dict(M=0), dict(I=0), dict(I=-4), dict(as_=87), dict(os=87), dict(act=1), dict(act=-1),
                    dict(M=2 ** 31 - 1, I=2 ** 20, as_=2 ** 20, os=2 ** 20, dys=2 ** 20, dtype=_lib.F32)):
            assert _act(bwd, **bad) == _lib.E_BAD_SHAPE, bad
        assert _act(bwd, a=A + 1) == _lib.E_ALIGNMENT and _act(bwd, out=A + 1) == _lib.E_ALIGNMENT
        assert _act(bwd, dtype=_lib.F32, a=A + 2) == _lib.E_ALIGNMENT
    assert _act(True, dys=87) == _lib.E_BAD_SHAPE and _act(True, dy=A + 1) == _lib.E_ALIGNMENT


# ---- 3. the restatements reproduce the fixtures ---------------------------------------------------------------------------------
LN = golden_names("layernorm_")
MLP = golden_names("neox_mlp_")


def _check(got, want, dt, what, floor=0.0):
    if dt == "f32":
        assert rel_err(got, want) < 2e-6, what
    else:
        worst = float(((np.abs(got - want) - floor) / br.ulp(want, dt)).max())
        assert worst <= 1.0, f"{what}: {worst} ulp"


def test_fixture_grid_is_complete():
    metas = [load_golden(n)[1] for n in LN]
    assert {(m["x_dtype"], m["weight_dtype"]) for m in metas} == {("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"),
                                                                  ("f16", "f32")}
    assert {m["eps"] for m in metas} == {1e-5} and {m["size"] for m in metas} == {72}
    assert all(load_golden(n)[0]["x"].shape == (2, 9, 72) for n in LN)
    metas = [load_golden(n)[1] for n in MLP]
    assert {m["fn"] for m in metas} == {"GptNeoxMLP"}
    assert {(m["dtype"], m["rows"], m["intermediate_size"]) for m in metas} >= {(d, 3, 88) for d in ("f32", "bf16", "f16")}
    assert any(m["bias"] and m["intermediate_size"] == 7 for m in metas)


@pytest.mark.parametrize("name", LN)
def test_layernorm_restatement_reproduces_fixture(name):
    d, m = load_golden(name)
    dt = m["x_dtype"]
    assert m["out_dtype"] == str(TD[dt])                     # torch's rule: y has x's dtype whatever the parameters' is
    y, _, _ = nr.layernorm_ref(d["x"], d["weight"], d["bias"], m["eps"], dt)
    _check(y, d["y"], dt, name)


@pytest.mark.parametrize("name", MLP)
def test_neox_mlp_restatement_reproduces_fixture(name):
    """piece by piece on the activations the fixture caught inside the module, so that one rounding flip in a linear does not
    travel: fc from x; GELU from the fixture's a; proj from the fixture's g"""
    d, m = load_golden(name)
    dt, I = m["dtype"], m["intermediate_size"]
    bias = (lambda k: d.get(k + "_bias")) if m["bias"] else (lambda k: None)
    x = d["x"].reshape(-1, m["n_embd"])
    a = br.linear_ref(x, d["fc_weight"], bias("fc"), dt)
    if dt == "f32":
        assert rel_err(a, d["a"].reshape(a.shape)) < 2e-6
    else:
        assert float(np.abs(a - d["a"].reshape(a.shape)).max()) <= float(br.ulp(np.abs(d["a"]).max(), dt))
    if dt == "f32":
        assert rel_err(nr.gelu_ref(d["a"], dt), d["g"]) < 2e-6
    else:
        # one unit in the last place of what the restatement can give, as test_block_neighbours_cpu.py does for the gated GELU:
        # gelu(a) is known to the reference's own float32 evaluation only within the cancellation error of 1 + erf (2^-23 |a|),
        # so where a 16-bit rounding boundary lies inside that error both roundings are the restatement's (neox_ref.gelu_interval)
        lo, hi = nr.gelu_interval(d["a"], dt)
        u = br.ulp(d["g"], dt)
        assert ((d["g"] >= lo - u) & (d["g"] <= hi + u)).all(), name
    y = br.linear_ref(d["g"].reshape(-1, I), d["proj_weight"], bias("proj"), dt)
    if dt == "f32":
        assert rel_err(y, d["y"].reshape(y.shape)) < 2e-6
    else:
        # a sum of I products rounded once: one unit in the last place at the size of the LARGEST output (cancellation leaves
        # small outputs with the float32 accumulation error of the large terms)
        assert float(np.abs(y - d["y"].reshape(y.shape)).max()) <= float(br.ulp(np.abs(d["y"]).max(), dt))


def test_stream_restatement_is_torchs_two_rounded_adds():
    g = torch.Generator().manual_seed(3)
    for dt, tdt in TD.items():
        m, h, x = (torch.randn(5, 33, generator=g).to(tdt) * s for s in (1.0, 3.0, 0.5))
        want = (m + h + x).double().numpy()
        assert np.array_equal(nr.stream_ref(x.double().numpy(), m.double().numpy(), h.double().numpy(), dt), want), dt
        assert np.array_equal(nr.stream_ref(x.double().numpy(), m.double().numpy(), None, dt), (x + m).double().numpy()), dt


def test_fp32_fixture_gradients_match_float64_autograd():
    import torch.nn.functional as F
    for name in LN:
        d, m = load_golden(name)
        if m["x_dtype"] != "f32":
            continue
        x, w, b = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("x", "weight", "bias"))
        F.layer_norm(x, (m["size"],), w, b, m["eps"]).backward(torch.from_numpy(d["gy"]).double())
        for got, want in ((x.grad, d["dx"]), (w.grad, d["dweight"]), (b.grad, d["dbias"])):
            assert rel_err(got.numpy(), want) < 1e-5, name
    for name in MLP:
        d, m = load_golden(name)
        if m["dtype"] != "f32":
            continue
        t = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("x", "fc_weight", "proj_weight")}
        bias = {k: (torch.from_numpy(d[k + "_bias"]).double() if m["bias"] else None) for k in ("fc", "proj")}
        F.linear(F.gelu(F.linear(t["x"], t["fc_weight"], bias["fc"])), t["proj_weight"], bias["proj"]).backward(
            torch.from_numpy(d["gy"]).double())
        assert rel_err(t["x"].grad.numpy(), d["dx"]) < 1e-5, name
        for k in ("fc", "proj"):
            assert rel_err(t[k + "_weight"].grad.numpy(), d[f"d_{k}_weight"]) < 1e-5, (name, k)


# ---- 4. the modules' tensor-op restatement on the CPU -----------------------------------------------------------------------------
def test_eager_modules_run_on_the_cpu_and_reproduce_the_fixtures():
    from fastmax_experiments_amd.neox_block import GptNeoxMLP, LayerNorm, layer_norm_pair
    torch.set_num_threads(4)
    for name in LN:
        d, m = load_golden(name)
        norm = LayerNorm(m["size"], eps=m["eps"])
        norm.fused_neighbours = False
        norm.load_state_dict({"weight": torch.from_numpy(d["weight"]), "bias": torch.from_numpy(d["bias"])})
        norm.to(TD[m["weight_dtype"]])
        x = torch.from_numpy(d["x"]).to(TD[m["x_dtype"]])
        assert torch.equal(norm(x).float(), torch.from_numpy(d["y"])), name
        s, y1, y2 = layer_norm_pair(x, norm, None)
        assert s is x and y2 is y1 and torch.equal(y1.float(), torch.from_numpy(d["y"]))
    for name in MLP:
        d, m = load_golden(name)
        mlp = GptNeoxMLP(m["n_embd"], m["intermediate_size"], bias=m["bias"])
        mlp.fused_neighbours = False
        sd = {}
        for lin in ("fc", "proj"):
            sd[f"{lin}.linear.weight"] = torch.from_numpy(d[f"{lin}_weight"])
            if m["bias"]:
                sd[f"{lin}.linear.bias"] = torch.from_numpy(d[f"{lin}_bias"])
        mlp.load_state_dict(sd)
        mlp.to(TD[m["dtype"]])
        x = torch.from_numpy(d["x"]).to(TD[m["dtype"]]).requires_grad_(True)
        y = mlp(x)
        y.backward(torch.from_numpy(d["gy"]).to(TD[m["dtype"]]))
        assert torch.equal(y.detach().float(), torch.from_numpy(d["y"])), name
        assert torch.equal(x.grad.float(), torch.from_numpy(d["dx"])), name


def test_eager_pair_is_the_reference_block_arithmetic():
    """x = mlp + h + x left to right, both norms on that sum; a parallel-residual block in tensor ops equals the formula"""
    from fastmax_experiments_amd.neox_block import LayerNorm, layer_norm_pair
    torch.manual_seed(0)
    n1, n2 = LayerNorm(24), LayerNorm(24)
    for n in (n1, n2):
        n.fused_neighbours = False
        torch.nn.init.normal_(n.weight, 1.0, 0.2)
        torch.nn.init.normal_(n.bias, 0.0, 0.2)
        n.to(torch.bfloat16)
    m, h, x = (torch.randn(2, 5, 24).to(torch.bfloat16) for _ in range(3))
    s, y1, y2 = layer_norm_pair(x, n1, n2, m, h)
    assert torch.equal(s, m + h + x)
    assert torch.equal(y1, torch.nn.functional.layer_norm(s, (24,), n1.weight, n1.bias, 1e-5))
    assert torch.equal(y2, torch.nn.functional.layer_norm(s, (24,), n2.weight, n2.bias, 1e-5))
    s1, _, _ = layer_norm_pair(x, n1, n2, m)
    assert torch.equal(s1, x + m)


# ---- 5. keys and error paths ---------------------------------------------------------------------------------------------------
SMALL = dict(n_embd=64, n_head=4, n_query_groups=4, intermediate_size=256)


def test_state_dict_keys_are_the_references():
    from fastmax_experiments_amd import generate
    from fastmax_experiments_amd.neox_block import NeoXBlock, NeoXStack
    attn = {"attn.attn.linear.weight", "attn.attn.linear.bias", "attn.attn.lora_A", "attn.attn.lora_B",
            "attn.proj.linear.weight", "attn.proj.linear.bias", "attn.proj.lora_A", "attn.proj.lora_B"}
    mlp = {"mlp.fc.linear.weight", "mlp.fc.linear.bias", "mlp.fc.lora_A", "mlp.fc.lora_B",
           "mlp.proj.linear.weight", "mlp.proj.linear.bias", "mlp.proj.lora_A", "mlp.proj.lora_B"}
    blk = NeoXBlock(to_mlp=True, to_projection=True, r=4, **SMALL)
    assert set(blk.state_dict()) == attn | mlp | {"norm_1.weight", "norm_1.bias", "norm_2.weight", "norm_2.bias"}
    shared = NeoXBlock(to_mlp=True, to_projection=True, r=4, shared_attention_norm=True, **SMALL)
    assert shared.norm_2 is None and set(shared.state_dict()) == attn | mlp | {"norm_1.weight", "norm_1.bias"}
    plain = NeoXBlock(**SMALL)                                  # to_mlp off: r = 0, no LoRA parameters on the MLP
    assert not [k for k in plain.state_dict() if k.startswith("mlp.") and "lora" in k]
    assert blk.mlp.fc.linear.weight.shape == (256, 64) and blk.mlp.proj.linear.weight.shape == (64, 256)
    assert set(NeoXStack([plain]).state_dict()) == {"blocks.0." + k for k in plain.state_dict()}
    from fastmax_experiments_amd import neox_block
    assert neox_block.FUSED_NEIGHBOURS_DEFAULT is False          # opt-in: profiles/r13_neox_block.md
    for b in (blk, shared):
        assert not (b.fused_neighbours or b.norm_1.fused_neighbours or b.mlp.fused_neighbours)
        b.fused_neighbours = True
        assert b.norm_1.fused_neighbours and b.mlp.fused_neighbours and (b.norm_2 is None or b.norm_2.fused_neighbours)
        b.fused_neighbours = False
        assert not (b.norm_1.fused_neighbours or b.mlp.fused_neighbours or (b.norm_2 is not None and b.norm_2.fused_neighbours))
    stack = NeoXStack([blk, shared])
    stack.fused_neighbours = True
    assert blk.fused_neighbours and shared.fused_neighbours and stack.fused_neighbours
    p70 = NeoXBlock.from_config("pythia-70m")
    assert p70.mlp.fc.linear.weight.shape == (2048, 512) and p70.attn.rope_n_elem == 16 and p70.attn.attn.linear.bias is not None
    head = generate.NextTokenHead(16, 40, norm_class="LayerNorm")
    assert list(head.state_dict()) == ["ln_f.weight", "ln_f.bias", "lm_head.weight"]
    assert list(generate.NextTokenHead(16, 40).state_dict()) == ["ln_f.weight", "lm_head.weight"]
    with pytest.raises(ValueError):
        generate.NextTokenHead(16, 40, norm_class="BatchNorm")
    head.fused = False                                          # the tensor-op restatement runs anywhere
    assert head.logits(torch.zeros(2, 3, 16)).shape == (2, 40)


def _on(module):
    module.fused_neighbours = True          # the kernels are opt-in
    return module


def test_malformed_arguments_raise_value_error():
    from fastmax_experiments_amd import neox_block
    from fastmax_experiments_amd.neox_block import gelu_backward, gelu_forward, layer_norm_backward, layer_norm_forward, layer_norm_pair
    LayerNorm = lambda *a, **kw: _on(neox_block.LayerNorm(*a, **kw))
    x = torch.randn(3, 8)
    with pytest.raises(ValueError, match="weight"):
        layer_norm_forward(x, torch.ones(7))
    with pytest.raises(ValueError, match="bias"):
        layer_norm_forward(x, torch.ones(8), torch.zeros(9))
    with pytest.raises(ValueError, match="weight"):
        LayerNorm(9)(x)
    with pytest.raises(ValueError, match="C = 0"):
        layer_norm_forward(torch.randn(3, 0), torch.ones(0))
    with pytest.raises(ValueError, match="r1 should match"):
        layer_norm_pair(x, LayerNorm(8), LayerNorm(8), torch.randn(2, 8))
    with pytest.raises(ValueError, match="r2 should match"):
        layer_norm_pair(x, LayerNorm(8), LayerNorm(8), x, torch.randn(3, 8).half())
    with pytest.raises(ValueError, match="r2 needs r1"):
        layer_norm_pair(x, LayerNorm(8), LayerNorm(8), None, x)
    with pytest.raises(ValueError, match="eps"):
        layer_norm_pair(x, LayerNorm(8), LayerNorm(8, eps=1e-6))
    with pytest.raises(ValueError, match="share"):
        layer_norm_forward(x.half(), torch.ones(8), torch.zeros(8).half())
    with pytest.raises(ValueError, match="share"):
        layer_norm_forward(x, torch.ones(8).half())
    with pytest.raises(ValueError, match="come together"):
        layer_norm_backward(x, x, torch.ones(8), torch.zeros(3), torch.ones(3), dy2=x)
    with pytest.raises(ValueError, match="empty"):
        gelu_forward(torch.randn(0, 8))
    with pytest.raises(ValueError, match="agree"):
        gelu_backward(x, torch.randn(3, 9))
    with pytest.raises(ValueError, match="agree"):
        gelu_backward(x, x.half())


def test_cpu_tensor_meets_the_no_cpu_path_error():
    from fastmax_experiments_amd import neox_block
    from fastmax_experiments_amd.neox_block import (NeoXBlock, gelu, gelu_backward, gelu_forward, layer_norm_backward,
                                                    layer_norm_forward, layer_norm_pair)
    LayerNorm = lambda *a, **kw: _on(neox_block.LayerNorm(*a, **kw))
    GptNeoxMLP = lambda *a, **kw: _on(neox_block.GptNeoxMLP(*a, **kw))
    x = torch.randn(3, 8)
    one, zero = torch.ones(8), torch.zeros(8)
    for call in (lambda: LayerNorm(8)(x), lambda: layer_norm_pair(x, LayerNorm(8), LayerNorm(8), x, x),
                 lambda: layer_norm_forward(x, one, zero), lambda: layer_norm_backward(x, x, one, torch.zeros(3), torch.ones(3)),
                 lambda: gelu(x), lambda: gelu_forward(x), lambda: gelu_backward(x, x), lambda: GptNeoxMLP(8, 16)(x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    blk = _on(NeoXBlock(**SMALL))
    with pytest.raises(RuntimeError, match="no CPU path"):
        blk(torch.randn(1, 4, 64), torch.zeros(4, 4), torch.zeros(4, 4))


def test_what_is_not_built_raises_not_implemented():
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.neox_block import GptNeoxMLP, NeoXBlock
    with pytest.raises(NotImplementedError, match="tanh"):
        GptNeoxMLP(8, 16, gelu_approximate="tanh")
    with pytest.raises(NotImplementedError, match="tanh"):
        NeoXBlock(gelu_approximate="tanh", **SMALL)
    with pytest.raises(ValueError, match="intermediate_size"):
        NeoXBlock(n_embd=64, n_head=4)
    with pytest.raises(NotImplementedError, match="parallel_residual"):       # Block is no front door for the new form
        Block(parallel_residual=True, n_embd=64, n_head=4, intermediate_size=176)


def test_attention_stack_builds_neox_blocks_and_generate_refuses_a_mix():
    from fastmax_experiments_amd import finetune_step, generate
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.neox_block import NeoXBlock
    a = finetune_step.AttentionStack("pythia-14m", 2, "fastmax", vocab=64)
    n = finetune_step.AttentionStack("pythia-14m", 2, "linearmax", vocab=64, block="neox")
    assert all(type(b) is NeoXBlock for b in n.blocks) and n.block == "neox" and n.rope_n_elem == a.rope_n_elem
    assert n.blocks[0].mlp.fc.linear.weight.shape == (512, 128) and n.blocks[0].attn.attn_alg == "linearmax"
    assert float(n.blocks[0].attn.attn.lora_B.detach().abs().max()) > 0              # a non-zero branch, as for the other block kinds
    with pytest.raises(ValueError):
        finetune_step.AttentionStack("pythia-14m", 1, "fastmax", block="mlp")
    head = generate.NextTokenHead(64, 40, norm_class="LayerNorm")
    mix = [NeoXBlock(**SMALL), Block(n_embd=64, n_head=4, intermediate_size=176)]
    with pytest.raises(ValueError, match="mix"):
        generate.generate(torch.zeros(40, 64), mix, head, [None, None], torch.zeros(2, 3, dtype=torch.int64), 6,
                          cos=torch.zeros(8, 4), sin=torch.zeros(8, 4))


def test_the_two_block_forms_share_a_base_and_name_their_runner():
    from fastmax_experiments_amd import block, neox_block
    from fastmax_experiments_amd.block import Block, DecoderBlock
    from fastmax_experiments_amd.neox_block import NeoXBlock
    assert issubclass(Block, DecoderBlock) and issubclass(NeoXBlock, DecoderBlock)
    assert Block.run_sequence is block.run_blocks and NeoXBlock.run_sequence is neox_block.run_neox_blocks
    for name in ("from_config", "quantize_base", "fused_neighbours"):      # held once, by the base
        assert name in vars(DecoderBlock) and name not in vars(Block) and name not in vars(NeoXBlock)
    b = Block(n_embd=64, n_head=4, intermediate_size=176)
    assert b.fused_neighbours is True and b.run_sequence is block.run_blocks
    n = NeoXBlock(shared_attention_norm=True, **SMALL)
    assert n.norm_2 is None and n.fused_neighbours is neox_block.FUSED_NEIGHBOURS_DEFAULT
    for on in (True, False):
        n.fused_neighbours = on                                            # walks norm_1 and mlp; the absent norm_2 is passed over
        assert n.fused_neighbours is on and n.norm_1.fused_neighbours is on and n.mlp.fused_neighbours is on
        b.fused_neighbours = on
        assert b.norm_1.fused_neighbours is on and b.norm_2.fused_neighbours is on and b.mlp.fused_neighbours is on
