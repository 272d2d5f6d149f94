"""Adapter-v2 fine-tuning, everything that needs no device (include/fastmax_hip_adapter.h, csrc/adapter_v2.hip,
fastmax_experiments_amd/adapter_v2.py, tests/golden/adapterv2_*.npz):

1. the source in the build's list; the workspace formula and ROWS_PER_BLOCK against the header (the header's rows of _lib.ABI
   are checked where every header's are, in test_binding_cpu.py);
2. every rejection the header lists, returned on made-up aligned addresses before any launch;
3. the restatement of adapter_v2_ref.py reproduces every fixture: bits for y and dz, the allowance for the float32-parameter
   gradients against both the float64 sums and the stored gradient;
4. with fused = False the module reproduces the fixtures on the CPU bit for bit;
5. state-dict keys, adapter_filter against the recorded answers, mark_only_adapter_v2_as_trainable on a Block and a NeoXBlock
   plus head, adapt's refusals and count, the checkpoint round trip, AttentionStack(method=...)."""
import re

import pytest
import torch
import torch.nn as nn

import adapter_v2_ref as ar
from conftest import golden_names, load_golden
from fastmax_experiments_amd import _lib, adapter_v2 as av2, build
from test_binding_cpu import header_text

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = [n for n in golden_names("adapterv2_") if n != "adapterv2_filter"]
SMALL = dict(n_embd=64, n_head=4, intermediate_size=88)


def tensors(d, m):
    """the fixture's arrays as torch tensors in the dtypes they were computed in"""
    dt, pdt, ydt = TD[m["dtype"]], TD[m["param_dtype"]], torch.promote_types(TD[m["dtype"]], TD[m["param_dtype"]])
    kind = dict(x=dt, weight=dt, bias=dt, z=dt, dz=dt, adapter_scale=pdt, adapter_bias=pdt, dscale=pdt, dbias=pdt, y=ydt, dy=ydt)
    return {k: torch.from_numpy(v).to(kind[k]) for k, v in d.items()}


# ---- 1. the build and the binding ------------------------------------------------------------------------------------------------
def test_the_build_compiles_the_source_and_watches_the_header():
    assert "adapter_v2.hip" in build.SOURCES


def test_workspace_formula_and_rows_per_block_match_the_header():
    R = int(re.search(r"#define FASTMAX_ADAPTER_ROWS_PER_BLOCK (\d+)", header_text("fastmax_hip_adapter.h")).group(1))
    assert R == _lib.ADAPTER_ROWS_PER_BLOCK == av2.ROWS_PER_BLOCK
    q = _lib.lib().fastmax_hip_adapter_backward_workspace
    for M, N in ((1, 1), (R - 1, 7), (R, 24), (R + 1, 24), (9 * R + 1, 2056), (16384, 11008)):
        assert q(M, N, _lib.BF16, 1) == -(-M // R) * 2 * N * 4, (M, N)
        assert q(M, N, _lib.F32, 0) == 0
    assert q(0, 8, _lib.F32, 1) == 0 and q(8, 0, _lib.F32, 1) == 0 and q(8, 8, 3, 1) == 0 and q(8, 8, -1, 1) == 0
    assert av2.adapter_backward_workspace(R + 1, 24, torch.float16, True) == 2 * 2 * 24 * 4
    assert av2.FUSED_DEFAULT in (False, True) and av2.AdapterV2Linear(4, 4).fused is av2.FUSED_DEFAULT


# ---- 2. rejections ------------------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _fwd(**over):
    a = dict(z=A, zs=24, scale=A, bias=A, y=A, ys=24, M=4, N=24, dtype=_lib.BF16, pdtype=_lib.BF16, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_adapter_forward(*a.values())


def _bwd(**over):
    a = dict(dy=A, dys=24, z=A, zs=24, scale=A, bias=A, dz=A, dzs=24, dscale=A, dbias=A, M=4, N=24, dtype=_lib.BF16,
             pdtype=_lib.BF16, ws=A, wsb=1 << 20, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_adapter_backward(*a.values())


def test_forward_rejects_bad_calls_before_any_launch():
    for missing in ("z", "scale", "bias", "y"):
        assert _fwd(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _fwd(dtype=dt, pdtype=_lib.F32) == _lib.E_BAD_DTYPE
    assert _fwd(dtype=_lib.BF16, pdtype=_lib.F16) == _lib.E_BAD_DTYPE and _fwd(dtype=_lib.F32, pdtype=_lib.BF16) == _lib.E_BAD_DTYPE
    assert _fwd(pdtype=3) == _lib.E_BAD_DTYPE
    for bad in (dict(M=0), dict(N=0), dict(M=-2), dict(zs=23), dict(ys=23), dict(ys=0)):
        assert _fwd(**bad) == _lib.E_BAD_SHAPE, bad
    big = 2 ** 31 - 1
    assert _fwd(M=big, N=big, zs=big, ys=big) == _lib.E_BAD_SHAPE                # the grid does not fit
    for odd in ("z", "scale", "bias", "y"):
        assert _fwd(**{odd: A + 1}) == _lib.E_ALIGNMENT, odd
    assert _fwd(dtype=_lib.F32, pdtype=_lib.F32, z=A + 2) == _lib.E_ALIGNMENT
    assert _fwd(pdtype=_lib.F32, scale=A + 2) == _lib.E_ALIGNMENT and _fwd(pdtype=_lib.F32, y=A + 2) == _lib.E_ALIGNMENT


def test_backward_rejects_bad_calls_before_any_launch():
    for missing in ("dy", "z", "scale", "bias"):
        assert _bwd(**{missing: None}) == _lib.E_NULL, missing
    assert _bwd(dscale=None) == _lib.E_NULL and _bwd(dbias=None) == _lib.E_NULL   # the two sums come together
    assert _bwd(dz=None, dscale=None, dbias=None) == _lib.E_NULL                  # a call that asks for nothing
    assert _bwd(ws=None) == _lib.E_NULL                                           # the sums without a workspace
    for dt in (-1, 3):
        assert _bwd(dtype=dt, pdtype=_lib.F32) == _lib.E_BAD_DTYPE
    assert _bwd(dtype=_lib.F16, pdtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(M=0), dict(N=-1), dict(dys=23), dict(zs=1), dict(dzs=23)):
        assert _bwd(**bad) == _lib.E_BAD_SHAPE, bad
    big = 2 ** 31 - 1
    assert _bwd(M=big, N=big, dys=big, zs=big, dz=None, dscale=None, dbias=None) == _lib.E_NULL
    assert _bwd(M=big, N=big, dys=big, zs=big, dzs=big, dscale=None, dbias=None) == _lib.E_BAD_SHAPE
    for odd in ("dy", "z", "scale", "bias", "dz"):
        assert _bwd(**{odd: A + 1}) == _lib.E_ALIGNMENT, odd
    for odd in ("dscale", "dbias"):
        assert _bwd(**{odd: A + 2}) == _lib.E_ALIGNMENT, odd
    assert _bwd(pdtype=_lib.F32, dy=A + 2) == _lib.E_ALIGNMENT
    assert _bwd(ws=A + 8) == _lib.E_ALIGNMENT
    need = _lib.lib().fastmax_hip_adapter_backward_workspace(4, 24, _lib.BF16, 1)
    assert need == 2 * 24 * 4 and _bwd(wsb=need - 1) == _lib.E_WORKSPACE
    assert _bwd(dscale=None, dbias=None, ws=None, wsb=0, M=0) == _lib.E_BAD_SHAPE  # no sums: no workspace is asked for


# ---- 3. the restatement against the fixtures ---------------------------------------------------------------------------------
def test_fixture_grid_is_complete():
    assert len(CASES) == 20
    seen = set()
    for name in CASES:
        d, m = load_golden(name)
        seen.add((m["dtype"], m["param_dtype"], m["rows"], m["out_features"], m["bias"]))
        assert ("bias" in d) == m["bias"]
        assert float(d["adapter_scale"][m["zero_scale_column"]]) == 0.0
        assert d["z"].shape == d["y"].shape == d["dy"].shape == d["dz"].shape == (m["rows"], m["out_features"])
    pairs = {("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32")}
    assert seen == {(dt, pdt, M, N, b) for dt, pdt in pairs for M, N in ((5, 24), (3, 7)) for b in (True, False)}


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(name):
    d, m = load_golden(name)
    t = tensors(d, m)
    r = ar.restate(t["z"], t["adapter_scale"], t["adapter_bias"], t["dy"])
    assert r["y"].dtype == t["y"].dtype and torch.equal(r["y"], t["y"]), name
    assert r["dz"].dtype == t["dz"].dtype and torch.equal(r["dz"], t["dz"]), name
    if m["param_dtype"] == "f32":
        # torch's own float32 column sums are one more summation order of the same terms
        for got, want, allow in ((t["dscale"], r["dscale64"], r["allow_scale"]), (t["dbias"], r["dbias64"], r["allow_bias"])):
            assert ar.within(got, want, allow), (name, ar.worst(got, want, allow))
        # and a float32 sum of the restated terms, in row order, meets both
        dyf = t["dy"].float()
        mine = (dyf * r["t"]).sum(0), (dyf * t["adapter_scale"].float()).sum(0)
        for got, stored, want, allow in ((mine[0], t["dscale"], r["dscale64"], r["allow_scale"]),
                                         (mine[1], t["dbias"], r["dbias64"], r["allow_bias"])):
            assert ar.within(got, want, allow) and ar.within(got, stored.double(), 2 * allow), name


# ---- 4. the module's tensor-op form on the CPU -----------------------------------------------------------------------------------
def test_unfused_module_runs_on_the_cpu_and_reproduces_the_fixtures():
    torch.set_num_threads(4)
    for name in CASES:
        d, m = load_golden(name)
        t = tensors(d, m)
        lin = av2.AdapterV2Linear(m["in_features"], m["out_features"], bias=m["bias"])
        lin.fused = False
        lin.to(TD[m["dtype"]])
        sd = {"linear.weight": t["weight"], "adapter_scale": t["adapter_scale"], "adapter_bias": t["adapter_bias"]}
        if m["bias"]:
            sd["linear.bias"] = t["bias"]
        lin.adapter_scale.data, lin.adapter_bias.data = (p.data.to(TD[m["param_dtype"]]) for p in (lin.adapter_scale, lin.adapter_bias))
        lin.load_state_dict(sd)
        lin.adapter_scale.requires_grad_(True), lin.adapter_bias.requires_grad_(True)
        caught = {}

        def hook(mod, inp, out, caught=caught):
            out.retain_grad()
            caught["z"] = out

        lin.linear.register_forward_hook(hook)
        y = lin(t["x"])
        y.backward(t["dy"])
        assert torch.equal(caught["z"].detach(), t["z"]), name
        assert y.dtype == t["y"].dtype and torch.equal(y.detach(), t["y"]), name
        assert torch.equal(caught["z"].grad, t["dz"]), name
        assert torch.equal(lin.adapter_scale.grad, t["dscale"]) and torch.equal(lin.adapter_bias.grad, t["dbias"]), name


def test_cpu_tensors_do_not_reach_the_kernels():
    lin = av2.AdapterV2Linear(8, 5)
    lin.fused = True
    x = torch.randn(3, 8)
    for call in (lambda: lin(x), lambda: av2.adapter_forward(x[:, :5], lin.adapter_scale, lin.adapter_bias),
                 lambda: av2.adapter_backward(x[:, :5], x[:, :5], lin.adapter_scale, lin.adapter_bias)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="5 elements"):
        av2.adapter_forward(x[:, :5], torch.ones(4), torch.zeros(5))
    with pytest.raises(ValueError, match="float32"):
        av2.adapter_forward(x[:, :5], torch.ones(5, dtype=torch.bfloat16), torch.zeros(5, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="N >= 1"):
        av2.adapter_forward(torch.zeros(3, 0), torch.ones(0), torch.zeros(0))


# ---- 5. names, filters, adapt, checkpoints, the step ------------------------------------------------------------------------------
def test_state_dict_keys_and_creation_are_the_references():
    lin = av2.AdapterV2Linear(8, 5, bias=True)
    assert list(lin.state_dict()) == ["adapter_bias", "adapter_scale", "linear.weight", "linear.bias"]
    assert not lin.adapter_bias.requires_grad and not lin.adapter_scale.requires_grad
    assert torch.equal(lin.adapter_bias, torch.zeros(5)) and torch.equal(lin.adapter_scale, torch.ones(5))
    with torch.no_grad():
        lin.adapter_bias.add_(1.0), lin.adapter_scale.mul_(3.0)
    lin.reset_parameters()
    assert torch.equal(lin.adapter_bias, torch.zeros(5)) and torch.equal(lin.adapter_scale, torch.ones(5))
    base = nn.Linear(8, 5).to(torch.bfloat16)
    wrapped = av2.AdapterV2Linear.from_linear(base)
    assert wrapped.linear is base and wrapped.adapter_scale.dtype == torch.bfloat16 and not wrapped.adapter_scale.requires_grad
    from fastmax_experiments_amd.lora import NF4Linear
    q = av2.AdapterV2Linear(128, 64, bias=False).quantize_base()
    assert isinstance(q.linear, NF4Linear) and q.quantize_base().linear is q.linear
    assert [k for k in q.state_dict() if "adapter" in k] == ["adapter_bias", "adapter_scale"]


def test_adapter_filter_gives_the_recorded_answers():
    d, m = load_golden("adapterv2_filter")
    assert len(m["keys"]) == len(d["answers"]) and 0 < int(d["answers"].sum()) < len(m["keys"])
    for key, want in zip(m["keys"], d["answers"]):
        assert av2.adapter_filter(key, None) == bool(want), key


def _model():
    from fastmax_experiments_amd.block import Block
    from fastmax_experiments_amd.generate import NextTokenHead
    from fastmax_experiments_amd.neox_block import NeoXBlock
    return nn.ModuleDict(dict(block=Block(r=0, **SMALL), neox=NeoXBlock(r=0, bias=True, **SMALL),
                              head=NextTokenHead(64, 48, 40, lm_head_bias=True)))


def test_adapt_counts_and_marks_exactly_the_adapter_parameters_and_the_norms():
    model = _model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    bases = {n: m.linear for n, m in model.named_modules() if hasattr(m, "linear")}
    bases["head.lm_head"] = model["head"].lm_head
    assert av2.adapt(model) == 5 + 4 + 1            # attn, proj, fc_1, fc_2, proj; attn, proj, fc, proj; lm_head
    assert av2.adapt(model) == 0
    adapted = {n: m for n, m in model.named_modules() if isinstance(m, av2.AdapterV2Linear)}
    assert set(adapted) == set(bases) and len(adapted) == 10
    for n, m in adapted.items():
        assert m.linear is bases[n], n                # the same base layer, not a copy
    assert adapted["head.lm_head"].linear.weight.shape == (48, 64)
    for k, v in before.items():                       # every old key is still there, one level down for the head
        k2 = k.replace("head.lm_head.", "head.lm_head.linear.")
        assert torch.equal(model.state_dict()[k2], v), k
    av2.mark_only_adapter_v2_as_trainable(model)
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    want = {f"{n}.{p}" for n in adapted for p in ("adapter_scale", "adapter_bias")}
    want |= {"block.norm_1.weight", "block.norm_2.weight", "neox.norm_1.weight", "neox.norm_1.bias", "neox.norm_2.weight",
             "neox.norm_2.bias", "head.ln_f.weight"}
    assert trainable == want


def test_adapt_refuses_a_live_branch_and_the_mixture_of_experts():
    from fastmax_experiments_amd.block import Block
    live = nn.ModuleList([Block(r=4, **SMALL)])
    with pytest.raises(ValueError, match=r"0\.attn\.attn"):
        av2.adapt(live)
    assert not any(isinstance(m, av2.AdapterV2Linear) for m in live.modules())      # nothing was replaced on the way
    live[0].attn.attn.merge()
    assert av2.adapt(live) == 5                                                     # a merged branch is absent
    moe = nn.ModuleList([Block(r=0, mlp_class="LLaMAMoE", n_expert=4, n_expert_per_token=2, **SMALL)])
    with pytest.raises(NotImplementedError, match="LLaMAMoE"):
        av2.adapt(moe)
    from fastmax_experiments_amd.lora import LoRALinear
    with pytest.raises(ValueError, match="holds the layer"):
        av2.adapt(LoRALinear(8, 8))


def test_checkpoint_round_trip_and_the_tolerated_keys(tmp_path):
    model = _model()
    av2.adapt(model)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if av2.adapter_filter(n, p):
                p.add_(torch.randn(p.shape, generator=g))
    path = tmp_path / "adapter.pth"
    av2.save_adapter_checkpoint(model, path)
    saved = torch.load(str(path), weights_only=True)["model"]
    assert set(saved) == {k for k in model.state_dict() if av2.adapter_filter(k, None)} and not any("linear" in k for k in saved)
    fresh = _model()
    av2.adapt(fresh)
    fresh.load_state_dict({k: v for k, v in model.state_dict().items() if k not in saved}, strict=False)
    av2.load_adapter_checkpoint(fresh, path)
    for (k, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), k
    # a reference checkpoint also carries adapter v1's parameters: inert here, skipped
    v1 = dict(saved)
    v1["block.attn.adapter_wte.weight"] = torch.zeros(10, 64)
    v1["block.attn.gating_factor"] = torch.zeros(1, 1, 4, 1)
    torch.save({"model": v1}, str(path))
    av2.load_adapter_checkpoint(fresh, path)
    v1["block.attn.attn.lora_A"] = torch.zeros(4, 64)
    torch.save({"model": v1}, str(path))
    with pytest.raises(KeyError, match="lora_A"):
        av2.load_adapter_checkpoint(fresh, path)


def test_attention_stack_builds_both_methods():
    from fastmax_experiments_amd import finetune_step
    lora = finetune_step.AttentionStack("pythia-14m", 2, "fastmax", vocab=64)
    names = [n for n, _ in lora.named_parameters()]
    assert names[:7] == ["lm_head", "blocks.0.attn.lora_A", "blocks.0.attn.lora_B", "blocks.0.attn.linear.weight",
                         "blocks.0.attn.linear.bias", "blocks.0.proj.linear.weight", "blocks.0.proj.linear.bias"]
    assert lora.method == "lora" and not any("adapter" in n for n in names)
    assert float(lora.blocks[0].attn.lora_B.detach().abs().max()) > 0
    for block, per_block in (("attention", 2), ("full", 5), ("neox", 4)):
        m = finetune_step.AttentionStack("pythia-14m", 2, "linearmax", vocab=64, block=block, method="adapter_v2")
        layers = [x for x in m.modules() if isinstance(x, av2.AdapterV2Linear)]
        assert len(layers) == 2 * per_block and not any("lora_" in n for n, _ in m.named_parameters())
        trainable = {n for n, p in m.named_parameters() if p.requires_grad}
        assert trainable == {n for n, _ in m.named_parameters() if av2.adapter_filter(n, None)} and "lm_head" not in trainable
        for x in layers:                                   # away from scale 1 and bias 0: every gradient is exercised
            assert float((x.adapter_scale.detach() - 1).abs().min()) > 0 and float(x.adapter_bias.detach().abs().min()) > 0
    with pytest.raises(ValueError, match="method"):
        finetune_step.AttentionStack("pythia-14m", 1, "fastmax", method="adapter")
