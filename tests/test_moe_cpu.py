"""The mixture-of-experts MLP (include/fastmax_hip_moe.h, csrc/moe.hip, fastmax_experiments_amd/moe.py), everything that needs
no device:

1. the size limits against the header, the source in the build's list (the binding table against this header:
   test_binding_cpu);
2. every rejection of the C ABI, returned before any launch (null streams, made-up addresses);
3. the restatement moe_ref.py on every fixture of tests/golden/make_golden_moe.py: float32 to 1e-6 of the tensor's scale, 16-bit to
   one unit in the last place;
4. ``LLaMAMoE(fused_neighbours=False)`` on CPU, loaded from a fixture's parameters: y, dx and every parameter gradient to the same
   bounds, the experts without tokens with zero gradients;
5. the host contract: state-dict keys, ``Block(mlp_class="LLaMAMoE")``, the size limits, the fused route's CPU-tensor error."""

import numpy as np
import pytest
import torch

import moe_ref
from block_ref import ulp_err
from conftest import golden_names, load_golden, rel_err
from fastmax_experiments_amd import _lib, build
from test_binding_cpu import header_text

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FIXTURES = golden_names("moe_")


# ---- 1. limits, build ------------------------------------------------------------------------------------------------------------
def test_the_limits_are_the_headers():
    text = header_text("fastmax_hip_moe.h")
    assert f"#define FASTMAX_MOE_MAX_EXPERTS {_lib.MOE_MAX_EXPERTS}" in text
    assert f"#define FASTMAX_MOE_MAX_PER_TOKEN {_lib.MOE_MAX_PER_TOKEN}" in text


def test_the_build_lists_the_source_and_the_header():
    assert "moe.hip" in build.SOURCES and "row_kernels.h" in build.HEADERS


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _call(name, defaults, over):
    a = dict(defaults)
    a.update(over)
    return getattr(_lib.lib(), name)(*a.values())


def _route(**over):
    return _call("fastmax_hip_moe_route", dict(router=A, rs=8, expert=A, prob=A, prob32=A, offsets=A, row_of=A, slot_of=A, M=5, E=8,
                                               k=2, dtype=_lib.BF16, ws=A, wsb=1 << 20, stream=None), over)


def _gather(**over):
    return _call("fastmax_hip_moe_gather", dict(x=A, xs_=64, row_of=A, xs=A, xss=64, M=5, S=10, C=64, dtype=_lib.BF16, stream=None),
                 over)


def _combine(**over):
    return _call("fastmax_hip_moe_combine", dict(ys=A, yss=64, prob=A, slot_of=A, y=A, ys_=64, M=5, k=2, C=64, dtype=_lib.BF16,
                                                 stream=None), over)


def _combine_bwd(**over):
    return _call("fastmax_hip_moe_combine_backward", dict(dy=A, dys_=64, ys=A, yss=64, prob=A, slot_of=A, dys=A, dyss=64, dprob=A,
                                                          M=5, k=2, C=64, dtype=_lib.BF16, stream=None), over)


def _gather_bwd(**over):
    return _call("fastmax_hip_moe_gather_backward", dict(dxs=A, dxss=64, slot_of=A, dx=A, dxs_=64, M=5, k=2, C=64, dtype=_lib.BF16,
                                                         stream=None), over)


def _route_bwd(**over):
    return _call("fastmax_hip_moe_route_backward", dict(dprob=A, prob32=A, expert=A, drouter=A, drs=8, M=5, E=8, k=2,
                                                        dtype=_lib.BF16, stream=None), over)


POINTERS = {_route: ("router", "expert", "prob", "prob32", "offsets", "row_of", "slot_of", "ws"), _gather: ("x", "row_of", "xs"),
            _combine: ("ys", "prob", "slot_of", "y"), _combine_bwd: ("dy", "ys", "prob", "slot_of", "dys", "dprob"),
            _gather_bwd: ("dxs", "slot_of", "dx"), _route_bwd: ("dprob", "prob32", "expert", "drouter")}
INT_POINTERS = {"expert", "prob32", "offsets", "row_of", "slot_of", "ws"}        # 4-byte elements whatever dtype is
STRIDES = {_route: ("rs",), _gather: ("xs_", "xss"), _combine: ("yss", "ys_"), _combine_bwd: ("dys_", "yss", "dyss"),
           _gather_bwd: ("dxss", "dxs_"), _route_bwd: ("drs",)}


def test_the_entry_points_reject_bad_calls_before_any_launch():
    for call, names in POINTERS.items():
        for n in names:
            assert call(**{n: None}) == _lib.E_NULL, (call.__name__, n)
            off = 2 if n in INT_POINTERS else 1                         # off a 4-byte element / off a bf16 element
            assert call(**{n: A + off}) == _lib.E_ALIGNMENT, (call.__name__, n)
        for d in (-1, 3):
            assert call(dtype=d) == _lib.E_BAD_DTYPE, (call.__name__, d)
        assert call(M=0) == _lib.E_BAD_SHAPE, call.__name__
        for s in STRIDES[call]:
            short = 7 if call in (_route, _route_bwd) else 63
            assert call(**{s: short}) == _lib.E_BAD_SHAPE, (call.__name__, s)
    for call in (_route, _route_bwd):
        for bad in (dict(k=0), dict(k=9, E=16), dict(k=3, E=2), dict(E=65, rs=65, drs=65), dict(M=1 << 30, k=2)):
            bad = {n: v for n, v in bad.items() if n != ("drs" if call is _route else "rs")}
            assert call(**bad) == _lib.E_BAD_SHAPE, (call.__name__, bad)
    for call in (_combine, _combine_bwd, _gather_bwd):
        for bad in (dict(k=0), dict(k=9), dict(C=0), dict(M=1 << 30, k=2)):
            assert call(**bad) == _lib.E_BAD_SHAPE, (call.__name__, bad)
    for bad in (dict(S=4), dict(S=11), dict(S=45), dict(C=0)):
        assert _gather(**bad) == _lib.E_BAD_SHAPE, bad
    assert _route(wsb=0) == _lib.E_WORKSPACE
    ws = _lib.lib().fastmax_hip_moe_route_workspace
    assert ws(5, 8) == 8 * 4 and ws(257, 8) == 2 * 8 * 4 and ws(1031, 64) == 5 * 64 * 4 and ws(0, 8) == 0 and ws(5, 65) == 0


# ---- 3. the restatement on the fixtures ---------------------------------------------------------------------------------------
def _experts(d, E):
    return [tuple(d[f"experts_{e}_{n}_weight"] for n in ("fc_1", "fc_2", "proj")) for e in range(E)]


def _module(d, m, dtype=None):
    from fastmax_experiments_amd.moe import LLaMAMoE
    moe = LLaMAMoE(m["n_embd"], m["intermediate_size"], m["n_expert"], m["n_expert_per_token"])
    state = {"gate.linear.weight": torch.from_numpy(d["gate_weight"])}
    for e in range(m["n_expert"]):
        for n in ("fc_1", "fc_2", "proj"):
            state[f"experts.{e}.{n}.linear.weight"] = torch.from_numpy(d[f"experts_{e}_{n}_weight"])
    moe.load_state_dict(state)
    return moe.to(dtype or DT[m["dtype"]])


def _close(got, ref, dt, what):
    if dt == "f32":
        assert rel_err(got, ref) <= 1e-6, what
    else:
        assert ulp_err(got, ref, dt) <= 1.0, what


def test_the_fixtures_are_the_cases_of_the_generator():
    assert FIXTURES == sorted(f"moe_{dt}_m{M}_e{E}_k{k}" for dt, M, E, k in
                              [(dt, 37, 8, 2) for dt in ("f32", "bf16", "f16")] + [(dt, 33, 6, 3) for dt in ("f32", "bf16")] +
                              [(dt, 5, 8, 2) for dt in ("f32", "bf16")])
    for name in FIXTURES:
        d, m = load_golden(name)
        assert m["min_kth_gap_ulp"] >= 4.0 and m["seed"] >= 1
        if m["rows"] == 5:
            assert len(m["experts_used"]) < m["n_expert"]
            idle = sorted(set(range(m["n_expert"])) - set(m["experts_used"]))
            assert all(not d[f"d_experts_{e}_{n}_weight"].any() for e in idle for n in ("fc_1", "fc_2", "proj"))


@pytest.mark.parametrize("name", FIXTURES)
def test_moe_ref_reproduces_the_routing_of_the_fixture(name):
    """selection and probabilities against torch.topk / softmax on the stored router; the dispatch arrays against torch.where"""
    d, m = load_golden(name)
    dt, k, E = m["dtype"], m["n_expert_per_token"], m["n_expert"]
    router = torch.from_numpy(d["router"]).to(DT[dt])
    r = moe_ref.route(d["router"], k, dt)
    top, chosen = torch.topk(router, k)
    prob = top.softmax(dim=1, dtype=torch.float).to(DT[dt])
    order = chosen.argsort(dim=1)
    assert np.array_equal(r["expert"], chosen.gather(1, order).numpy())
    _close(r["prob"], prob.gather(1, order).float().numpy(), dt, "prob")
    assert r["offsets"][0] == 0 and r["offsets"][-1] == m["rows"] * k
    for e in range(E):
        t, j = torch.where(chosen == e)
        lo, hi = r["offsets"][e], r["offsets"][e + 1]
        assert np.array_equal(r["row_of"][lo:hi], t.numpy()), e
    rows = np.arange(m["rows"])[:, None]
    assert np.array_equal(r["row_of"][r["slot_of"]], np.broadcast_to(rows, r["slot_of"].shape))
    slots_e = np.searchsorted(r["offsets"], r["slot_of"], side="right") - 1
    assert np.array_equal(slots_e, r["expert"])


@pytest.mark.parametrize("name", FIXTURES)
def test_moe_ref_reproduces_the_output_of_the_fixture(name):
    """the combine with its rounding points, fed the experts' outputs as torch computes them on the dispatched rows"""
    d, m = load_golden(name)
    dt, k = m["dtype"], m["n_expert_per_token"]
    moe = _module(d, m)
    moe.fused_neighbours = False
    r = moe_ref.route(d["router"], k, dt)
    x = torch.from_numpy(d["x"]).to(DT[dt]).view(-1, m["n_embd"])
    xs = x[torch.from_numpy(r["row_of"]).long()]
    with torch.no_grad():
        ys = torch.cat([moe.experts[e](xs[r["offsets"][e]:r["offsets"][e + 1]]) for e in range(m["n_expert"])])
    y = moe_ref.combine(ys.float().numpy(), r["prob"], r["slot_of"], dt)
    _close(y, d["y"].reshape(y.shape), dt, "y")
    # the all-float64 restatement of the whole layer: float32 to the same bound
    if dt == "f32":
        y64, _, _ = moe_ref.moe_forward(d["x"].reshape(y.shape), d["router"], _experts(d, m["n_expert"]), k, dt)
        assert rel_err(y64, d["y"].reshape(y.shape)) <= 1e-6


@pytest.mark.parametrize("name", [n for n in FIXTURES if "_f32_" in n])
def test_moe_ref_exact_gradients_are_the_float32_fixture_gradients(name):
    d, m = load_golden(name)
    M, C = m["rows"], m["n_embd"]
    dx, dgate, grads = moe_ref.moe_backward(d["x"].reshape(M, C), d["gate_weight"], _experts(d, m["n_expert"]),
                                            m["n_expert_per_token"], d["gy"].reshape(M, C))
    assert rel_err(dx, d["dx"].reshape(M, C)) <= 1e-5
    assert rel_err(dgate, d["d_gate_weight"]) <= 1e-5
    for e, g3 in enumerate(grads):
        for n, g in zip(("fc_1", "fc_2", "proj"), g3):
            assert rel_err(g, d[f"d_experts_{e}_{n}_weight"]) <= 1e-5, (e, n)


# ---- 4. the tensor-op route on CPU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_the_tensor_op_route_reproduces_the_fixture_on_cpu(name):
    d, m = load_golden(name)
    dt = m["dtype"]
    moe = _module(d, m)
    moe.fused_neighbours = False
    x = torch.from_numpy(d["x"]).to(DT[dt]).requires_grad_(True)
    y = moe(x)
    assert y.shape == x.shape and y.dtype == x.dtype
    y.backward(torch.from_numpy(d["gy"]).to(DT[dt]))
    _close(y.detach().float().numpy(), d["y"], dt, "y")
    _close(x.grad.float().numpy(), d["dx"], dt, "dx")
    _close(moe.gate.linear.weight.grad.float().numpy(), d["d_gate_weight"], dt, "d gate")
    for e in range(m["n_expert"]):
        for n in ("fc_1", "fc_2", "proj"):
            g = getattr(moe.experts[e], n).linear.weight.grad
            if e not in m["experts_used"]:                                 # an idle expert is not called: no gradient, the
                assert g is None and not d[f"d_experts_{e}_{n}_weight"].any()      # fixture's is zero
                continue
            _close(g.float().numpy(), d[f"d_experts_{e}_{n}_weight"], dt, (e, n))


# ---- 5. the host contract ---------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_s():
    from fastmax_experiments_amd.moe import LLaMAMoE
    moe = LLaMAMoE(16, 24, 4, 2)
    keys = list(moe.state_dict())
    assert keys == ["gate.linear.weight"] + [f"experts.{e}.{n}.linear.weight" for e in range(4) for n in ("fc_1", "fc_2", "proj")]
    lora = LLaMAMoE(16, 24, 4, 2, r=4, alpha=8, to_mlp=True)
    assert {"gate.lora_A", "gate.lora_B", "experts.3.proj.lora_A", "experts.3.fc_1.lora_B"} <= set(lora.state_dict())
    assert LLaMAMoE(16, 24, 4, 2, r=4, alpha=8, to_mlp=False).gate.r == 0


def test_block_builds_the_moe_and_still_refuses_the_neox_mlp(monkeypatch):
    from fastmax_experiments_amd.block import CONFIG_INTERMEDIATE, CONFIG_MOE, Block
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES
    from fastmax_experiments_amd.moe import LLaMAMoE
    small = dict(n_embd=64, n_head=4, intermediate_size=96)
    blk = Block(mlp_class="LLaMAMoE", n_expert=4, n_expert_per_token=2, **small)
    assert isinstance(blk.mlp, LLaMAMoE) and len(blk.mlp.experts) == 4 and blk.mlp.n_expert_per_token == 2
    assert "mlp.experts.3.fc_2.linear.weight" in blk.state_dict() and "mlp.gate.linear.weight" in blk.state_dict()
    blk.fused_neighbours = False
    assert not blk.mlp.fused_neighbours and not blk.mlp.experts[0].fused_neighbours
    with pytest.raises(NotImplementedError, match="GptNeoxMLP"):
        Block(mlp_class="GptNeoxMLP", **small)
    with pytest.raises(ValueError, match="n_expert_per_token"):
        Block(mlp_class="LLaMAMoE", **small)                                # the sizes are required
    name = "Mixtral-8x7B-v0.1"
    assert CONFIG_SHAPES[name] == dict(n_embd=4096, n_head=32, n_query_groups=8, head_size=128, rotary_percentage=1.0, bias=False)
    assert CONFIG_INTERMEDIATE[name] == 14336
    assert CONFIG_MOE[name] == dict(mlp_class="LLaMAMoE", n_expert=8, n_expert_per_token=2)
    assert not {"n_expert", "n_expert_per_token"} & set(CONFIG_SHAPES[name])
    # from_config merges CONFIG_MOE in (at a width that can be built here), and the caller's arguments still win
    monkeypatch.setitem(CONFIG_SHAPES, "tiny-moe", dict(n_embd=64, n_head=4, n_query_groups=2, head_size=16))
    monkeypatch.setitem(CONFIG_INTERMEDIATE, "tiny-moe", 96)
    monkeypatch.setitem(CONFIG_MOE, "tiny-moe", CONFIG_MOE[name])
    tiny = Block.from_config("tiny-moe")
    assert len(tiny.mlp.experts) == 8 and tiny.mlp.n_expert_per_token == 2 and tiny.mlp.experts[7].fc_1.linear.weight.shape == (96, 64)
    assert len(Block.from_config("tiny-moe", n_expert=4).mlp.experts) == 4
    monkeypatch.delitem(CONFIG_MOE, "tiny-moe")
    assert not isinstance(Block.from_config("tiny-moe").mlp, LLaMAMoE)


@pytest.mark.parametrize("E, k, word", [(4, 5, "exceeds"), (65, 2, "n_expert"), (16, 9, "n_expert_per_token"), (4, 0, "n_expert_per_token")])
def test_sizes_outside_the_limits_raise_value_error(E, k, word):
    from fastmax_experiments_amd import moe
    with pytest.raises(ValueError, match=word):
        moe.LLaMAMoE(16, 24, E, k)
    with pytest.raises(ValueError, match=word):
        moe.route(torch.zeros(3, E), k)                                     # before the device check


def test_the_fused_route_has_no_cpu_path():
    from fastmax_experiments_amd import moe
    layer = moe.LLaMAMoE(16, 24, 4, 2)
    assert layer.fused_neighbours
    x = torch.randn(2, 3, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(x)
    ints = torch.zeros(3, 2, dtype=torch.int32)
    for call in (lambda: moe.route(torch.zeros(3, 4), 2), lambda: moe.gather(x[0], ints.view(-1)),
                 lambda: moe.combine(torch.zeros(6, 16), torch.zeros(3, 2), ints),
                 lambda: moe.combine_backward(x[0], torch.zeros(6, 16), torch.zeros(3, 2), ints),
                 lambda: moe.gather_backward(torch.zeros(6, 16), ints),
                 lambda: moe.route_backward(torch.zeros(3, 2), torch.zeros(3, 2), ints, 4)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    layer.fused_neighbours = False
    assert layer(x).shape == x.shape
