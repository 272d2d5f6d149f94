"""The decoder block's neighbours of the attention sub-layer, everything that needs no device
(include/fastmax_hip_block.h, fastmax_experiments_amd/block.py, tests/golden/rmsnorm_*.npz and mlp_*.npz):

1. the library exports every name of the header and binds it as its row of _lib.ABI says (the rows against the prototypes, the
   FASTMAX_ACT_* enum and the pin over the whole table: test_binding_cpu.py);
2. the float64 restatements in block_ref.py (RMSNorm, the gated MLP) reproduce every fixture the reference's own code produced:
   fp32 fixtures to 1e-6 relative, 16-bit fixtures to one unit in the last place of their dtype.  The GPU tests lean on these
   restatements at the shapes the fixtures do not have;
3. error paths: what is not built raises NotImplementedError and names it, malformed arguments raise ValueError, a CPU tensor
   meets the "no CPU path" error;
4. Block's state dict carries the reference's key names."""
import ctypes

import numpy as np
import pytest
import torch

import block_ref as br
from conftest import golden_names, load_golden, rel_err
from fastmax_experiments_amd import _lib


# ---- 1. binding ------------------------------------------------------------------------------------------------------------
BLOCK_ENTRY_POINTS = ["fastmax_hip_rmsnorm_forward", "fastmax_hip_rmsnorm_backward_workspace", "fastmax_hip_rmsnorm_backward",
                      "fastmax_hip_gated_act_forward", "fastmax_hip_gated_act_backward"]


def test_library_exports_every_name():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in BLOCK_ENTRY_POINTS:
        assert hasattr(L, name), name
    bound = _lib.lib()          # binds the whole table or raises
    for name in BLOCK_ENTRY_POINTS:
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib.ABI[name][0], _lib.ABI[name][1]), name
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9


def test_workspace_query_needs_no_device():
    q = _lib.lib().fastmax_hip_rmsnorm_backward_workspace
    assert q(1000, 128, _lib.BF16, 0) == 0 and q(0, 128, _lib.F32, 1) == 0
    assert q(1000, 128, _lib.BF16, 1) == ((1000 + 15) // 16) * 128 * 4          # one float32 row of partials per 16 rows
    assert q(3, 4096, _lib.F32, 1) == 4096 * 4


# ---- 2. the restatements reproduce the fixtures ---------------------------------------------------------------------------------
def _check(got, want, dt, what):
    if dt == "f32":
        assert rel_err(got, want) < 1e-6, what
    else:
        assert br.ulp_err(got, want, dt) <= 1.0, f"{what}: {br.ulp_err(got, want, dt)} ulp"


RMS = golden_names("rmsnorm_")
MLP = golden_names("mlp_")


def test_fixture_grid_is_complete():
    metas = [load_golden(n)[1] for n in RMS]
    assert {m["x_dtype"] for m in metas} == {"f32", "bf16", "f16"}
    assert {m["eps"] for m in metas} == {1e-5, 1e-6}
    assert {m["add_unit_offset"] for m in metas} == {True, False}
    assert {(m["x_dtype"], m["weight_dtype"]) for m in metas} >= {("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32")}
    metas = [load_golden(n)[1] for n in MLP]
    assert {(m["fn"], m["dtype"]) for m in metas} == {(f, d) for f in ("LLaMAMLP", "GemmaMLP") for d in ("f32", "bf16", "f16")}
    assert {(m["rows"], m["intermediate_size"]) for m in metas} == {(3, 88), (2, 7)}


@pytest.mark.parametrize("name", RMS)
def test_rmsnorm_restatement_reproduces_fixture(name):
    d, m = load_golden(name)
    dt, wdt = m["x_dtype"], m["weight_dtype"]
    _, y, _ = br.rmsnorm_ref(d["x"], d["weight"], m["eps"], m["add_unit_offset"], dt, wdt)
    assert m["out_dtype"] == {"f32": "torch.float32", "bf16": "torch.bfloat16", "f16": "torch.float16"}[br.out_dtype(dt, wdt)]
    _check(y, d["y"], br.out_dtype(dt, wdt), name)


@pytest.mark.parametrize("name", MLP)
def test_gated_mlp_restatement_reproduces_fixture(name):
    """piece by piece on the activations the fixture caught inside the module, so that one rounding flip in a linear does not
    travel: fc_1, fc_2 from x; the gated activation from the fixture's a, b; proj from the fixture's g"""
    d, m = load_golden(name)
    dt = m["dtype"]
    x = d["x"].reshape(-1, m["n_embd"])
    bias = (lambda k: d.get(k + "_bias")) if m["bias"] else (lambda k: None)
    _check(br.linear_ref(x, d["fc_1_weight"], bias("fc_1"), dt), d["a"].reshape(-1, m["intermediate_size"]), dt, name + " fc_1")
    _check(br.linear_ref(x, d["fc_2_weight"], bias("fc_2"), dt), d["b"].reshape(-1, m["intermediate_size"]), dt, name + " fc_2")
    g = br.gated_ref(d["a"], d["b"], m["act"], dt)
    if dt == "f32":
        assert rel_err(g, d["g"]) < 1e-6
    else:
        # one unit in the last place of what the restatement can give: act(a) of exact GELU is known to the reference's own
        # float32 evaluation only within the cancellation error of 1 + erf, so where a 16-bit rounding boundary of act(a) lies
        # inside that error both roundings are the restatement's (block_ref.gated_interval; SiLU: a single value)
        lo, hi = br.gated_interval(d["a"], d["b"], m["act"], dt)
        u = br.ulp(d["g"], dt)
        assert ((d["g"] >= lo - u) & (d["g"] <= hi + u)).all(), name
    y = br.linear_ref(d["g"].reshape(-1, m["intermediate_size"]), d["proj_weight"], bias("proj"), dt)
    if dt == "f32":
        assert rel_err(y, d["y"].reshape(y.shape)) < 1e-6
    else:
        # a sum of 88 products rounded once: one unit in the last place at the size of the LARGEST output of the row's sum
        # (cancellation leaves small outputs with the float32 accumulation error of the large terms)
        assert float(np.abs(y - d["y"].reshape(y.shape)).max()) <= float(br.ulp(np.abs(d["y"]).max(), dt))


def test_fp32_fixture_gradients_match_float64_autograd():
    """the gradients the fixtures store (backward() on the seeded cotangent), fp32 fixtures against float64 autograd of the same
    function: 1e-5 of the largest magnitude"""
    import torch.nn.functional as F
    for name in RMS:
        d, m = load_golden(name)
        if m["x_dtype"] != "f32":
            continue
        x, w = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("x", "weight"))
        n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + m["eps"])
        (n * ((1 + w) if m["add_unit_offset"] else w)).backward(torch.from_numpy(d["gy"]).double())
        assert rel_err(x.grad.numpy(), d["dx"]) < 1e-5 and rel_err(w.grad.numpy(), d["dweight"]) < 1e-5, name
    for name in MLP:
        d, m = load_golden(name)
        if m["dtype"] != "f32":
            continue
        t = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("x", "fc_1_weight", "fc_2_weight", "proj_weight")}
        bias = {k: (torch.from_numpy(d[k + "_bias"]).double() if m["bias"] else None) for k in ("fc_1", "fc_2", "proj")}
        act = F.silu if m["act"] == "silu" else F.gelu
        h = act(F.linear(t["x"], t["fc_1_weight"], bias["fc_1"])) * F.linear(t["x"], t["fc_2_weight"], bias["fc_2"])
        F.linear(h, t["proj_weight"], bias["proj"]).backward(torch.from_numpy(d["gy"]).double())
        assert rel_err(t["x"].grad.numpy(), d["dx"]) < 1e-5, name
        for k in ("fc_1", "fc_2", "proj"):
            assert rel_err(t[k + "_weight"].grad.numpy(), d[f"d_{k}_weight"]) < 1e-5, (name, k)


def test_round_to_matches_torch():
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3
    for dt, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
        want = x.float().to(tdt).double().numpy()
        assert np.array_equal(br.round_to(x.numpy(), dt), want), dt
    assert br.ulp(1.0, "bf16") == 2.0 ** -7 and br.ulp(1.5, "f16") == 2.0 ** -10 and br.ulp(0.75, "bf16") == 2.0 ** -8


# ---- 3. error paths -----------------------------------------------------------------------------------------------------------
SMALL = dict(n_embd=64, n_head=4, n_query_groups=2, intermediate_size=176)


def test_block_refuses_what_is_not_built():
    from fastmax_experiments_amd.block import Block
    with pytest.raises(NotImplementedError, match="parallel_residual"):
        Block(parallel_residual=True, **SMALL)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        Block(norm_class=torch.nn.LayerNorm, **SMALL)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        Block(norm_class="LayerNorm", **SMALL)
    with pytest.raises(NotImplementedError, match="GptNeoxMLP"):
        Block(mlp_class="GptNeoxMLP", **SMALL)


def test_malformed_arguments_raise_value_error():
    from fastmax_experiments_amd.block import RMSNorm, rms_norm_add, rms_norm_forward
    x = torch.randn(3, 8)
    with pytest.raises(ValueError, match="weight"):
        rms_norm_forward(x, None, torch.ones(7), 1e-5, False)
    with pytest.raises(ValueError, match="weight"):
        RMSNorm(9)(x)
    with pytest.raises(ValueError, match="C = 0"):
        rms_norm_forward(torch.randn(3, 0), None, torch.ones(0), 1e-5, False)
    with pytest.raises(ValueError, match="r should match"):
        rms_norm_add(x, torch.randn(2, 8), RMSNorm(8))
    with pytest.raises(ValueError, match="r should match"):
        rms_norm_add(x, torch.randn(3, 8).half(), RMSNorm(8))


def test_cpu_tensor_meets_the_no_cpu_path_error():
    from fastmax_experiments_amd.block import GemmaMLP, LLaMAMLP, RMSNorm, gated_act, rms_norm_add
    x = torch.randn(3, 8)
    for call in (lambda: RMSNorm(8)(x), lambda: rms_norm_add(x, x, RMSNorm(8)), lambda: gated_act(x, x, "silu"),
                 lambda: LLaMAMLP(8, 16)(x), lambda: GemmaMLP(8, 16)(x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_eager_restatement_runs_on_the_cpu_and_matches_the_fixtures():
    """fused_neighbours = False is plain tensor ops: the module with a fixture's parameters reproduces the fixture on the CPU"""
    from fastmax_experiments_amd.block import RMSNorm
    TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    for name in RMS:
        d, m = load_golden(name)
        norm = RMSNorm(m["size"], eps=m["eps"], add_unit_offset=m["add_unit_offset"])
        norm.fused_neighbours = False
        norm.weight.data = torch.from_numpy(d["weight"]).to(TD[m["weight_dtype"]])
        y = norm(torch.from_numpy(d["x"]).to(TD[m["x_dtype"]]))
        assert torch.equal(y.float(), torch.from_numpy(d["y"])), name


# ---- 4. state dict --------------------------------------------------------------------------------------------------------------
def test_block_state_dict_has_the_reference_key_names():
    from fastmax_experiments_amd.block import Block, BlockStack
    blk = Block(to_mlp=True, to_projection=True, r=4, **SMALL)
    keys = set(blk.state_dict())
    assert keys == {"norm_1.weight", "norm_2.weight",
                    "attn.attn.linear.weight", "attn.attn.lora_A", "attn.attn.lora_B",
                    "attn.proj.linear.weight", "attn.proj.lora_A", "attn.proj.lora_B",
                    "mlp.fc_1.linear.weight", "mlp.fc_1.lora_A", "mlp.fc_1.lora_B",
                    "mlp.fc_2.linear.weight", "mlp.fc_2.lora_A", "mlp.fc_2.lora_B",
                    "mlp.proj.linear.weight", "mlp.proj.lora_A", "mlp.proj.lora_B"}
    plain = Block(**SMALL)                                      # to_mlp off: r = 0, no LoRA parameters on the MLP
    assert not [k for k in plain.state_dict() if k.startswith("mlp.") and "lora" in k]
    assert blk.mlp.fc_1.linear.weight.shape == (176, 64) and blk.mlp.proj.linear.weight.shape == (64, 176)
    assert set(BlockStack([plain]).state_dict()) == {"blocks.0." + k for k in plain.state_dict()}
    blk.fused_neighbours = False
    assert not (blk.norm_1.fused_neighbours or blk.norm_2.fused_neighbours or blk.mlp.fused_neighbours)


def test_attention_stack_default_is_unchanged_and_full_takes_the_config_mlp():
    from fastmax_experiments_amd import finetune_step
    from fastmax_experiments_amd.attention_block import CausalSelfAttention
    from fastmax_experiments_amd.block import Block
    a = finetune_step.AttentionStack("pythia-14m", 2, "fastmax", vocab=64)
    assert all(type(b) is CausalSelfAttention for b in a.blocks) and a.block == "attention"
    f = finetune_step.AttentionStack("pythia-14m", 2, "linearmax", vocab=64, block="full")
    assert all(type(b) is Block for b in f.blocks)
    assert f.blocks[0].mlp.fc_1.linear.weight.shape == (512, 128) and f.rope_n_elem == a.rope_n_elem
    with pytest.raises(ValueError):
        finetune_step.AttentionStack("pythia-14m", 1, "fastmax", block="mlp")
