"""LLaMA-Adapter without a GPU: the new header's rows of the binding table against its prototypes, the C ABI's host-side refusals
and workspace sizes, adapt / filter / checkpoints, the fine-tune stack's method, and the reference module's own output."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import prefix_ref
from fastmax_experiments_amd import _lib, adapter, build, ops
from fastmax_experiments_amd.attention_block import CausalSelfAttention
from test_binding_cpu import ctypes_kind, header_prototypes

HEADER = "fastmax_hip_prefix.h"
P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host


def test_rows_match_the_header_and_the_library():
    protos = header_prototypes(HEADER)
    assert [n for n, _, _ in protos] == list(_lib.ABI_EXT3), "names in the header's order"
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, ret, kinds in protos:
        restype, argtypes = _lib.ABI_EXT3[name]
        assert ctypes_kind(restype) == ret and [ctypes_kind(t) for t in argtypes] == kinds, name
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert _lib.HEADERS_EXT3 == (HEADER,) and not set(_lib.ABI_EXT3) & (set(_lib.ABI) | set(_lib.ABI_EXT) | set(_lib.ABI_EXT2))
    assert os.path.join("..", "..", "include", HEADER) in build.HEADERS and "prefix_attention.hip" in build.SOURCES
    assert build.FILE_FLAGS["prefix_attention.hip"] == build.FILE_FLAGS["softmax_attention_bwd.hip"]
    assert bound.fastmax_hip_abi_version() == _lib.ABI_VERSION == 9
    ws = bound.fastmax_hip_prefix_backward_workspace
    assert ws(2, 8, 512, 64) == 2 * 8 * (2 * 32 * 64 + 1) * 4 and ws(2, 8, 513, 64) == 2 * ws(2, 8, 1, 64)
    assert ws(1, 2, 4, 12) == 0 and ws(1, 2, 4, 136) == 0 and ws(1, 2, 0, 64) == 0
    assert (_lib.PREFIX_MAX_ROWS, _lib.PREFIX_BWD_CHUNK) == (32, 512)


def _call(fn, kw):
    a = {**dict(q=P, y=P, ak=P, gate=P, out=P, B=1, H=2, Hkv=1, N=3, D=64, aT=10, dtype=_lib.BF16, ws_bytes=1 << 30, st=(640, 640, 64)),
         **kw}
    s = (ctypes.c_int64 * 3)(*a["st"])
    tail = (a["B"], a["H"], a["Hkv"], a["N"], a["D"], a["aT"], a["dtype"], 0.125)
    if fn == "forward":
        return _lib.lib().fastmax_hip_prefix_forward(a["q"], s, a["y"], s, a["ak"], P, a["gate"], a["out"], *tail, None)
    return _lib.lib().fastmax_hip_prefix_backward(a["q"], s, a["y"], s, a["ak"], P, a["gate"], a["out"], P, P, P, *tail, P, a["ws_bytes"], None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
@pytest.mark.parametrize("kw, code", [
    (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(D=12), _lib.E_BAD_SHAPE), (dict(D=264), _lib.E_BAD_SHAPE),
    (dict(N=0), _lib.E_BAD_SHAPE), (dict(Hkv=3), _lib.E_BAD_SHAPE), (dict(aT=0), _lib.E_BAD_SHAPE), (dict(aT=33), _lib.E_BAD_SHAPE),
    (dict(q=None), _lib.E_NULL), (dict(gate=None), _lib.E_NULL), (dict(out=None), _lib.E_NULL), (dict(q=None, dtype=_lib.F32), _lib.E_NULL),
    (dict(ak=P + 2), _lib.E_ALIGNMENT), (dict(st=(640, 640, 68)), _lib.E_ALIGNMENT), (dict(D=12, y=P + 2), _lib.E_BAD_SHAPE)])
def test_host_side_refusals(fn, kw, code):
    assert _call(fn, kw) == code


def test_backward_head_sizes_and_a_short_workspace():
    assert _call("backward", dict(D=136)) == _lib.E_BAD_SHAPE and _call("backward", dict(ws_bytes=64)) == _lib.E_WORKSPACE
    z = torch.zeros(1, 2, 4, 136, dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(NotImplementedError, match="128"):
        ops.prefix_attention_add(z, z, z[0, :, :, :], z[0], torch.zeros(2))


def _stack(alg="quadratic", n=3):
    from fastmax_experiments_amd.block import Block, BlockStack
    return BlockStack([Block(n_embd=64, n_head=4, n_query_groups=2, head_size=16, intermediate_size=32, attn_alg=alg, r=0) for _ in range(n)])


def test_adapt_filter_trainable_and_checkpoints(tmp_path):
    model = _stack()
    assert adapter.adapt(model, adapter_prompt_length=10, adapter_start_layer=1) == 2
    keys = {k for k in model.state_dict() if adapter.adapter_filter(k, None)}
    assert keys == {f"blocks.{i}.attn.{n}" for i in (1, 2) for n in ("adapter_wte.weight", "gating_factor")}
    a = model.blocks[1].attn
    assert isinstance(a, adapter.AdapterCausalSelfAttention) and type(model.blocks[0].attn) is CausalSelfAttention
    assert a.adapter_wte.weight.shape == (10, 64) and a.gating_factor.shape == (1, 1, 4, 1) and not a.gating_factor.any()
    adapter.mark_only_adapter_as_trainable(model)
    assert {n for n, p in model.named_parameters() if p.requires_grad} == keys
    with pytest.raises(ValueError, match="quadratic"):
        adapter.adapt(_stack("fastmax"))
    with pytest.raises(ValueError, match="32"):
        adapter.adapt(_stack(), adapter_prompt_length=33)
    # (ak, av): the K and V slots of the layer's own projection of the prompt, at their KV heads; cached only without gradients
    ak, av = a.adapter_kv(torch.float32)
    want = a.attn(a.adapter_wte.weight).view(10, 2, 4, 16)
    assert ak.shape == (2, 10, 16) and torch.equal(ak, want[:, :, 2].transpose(0, 1)) and torch.equal(av, want[:, :, 3].transpose(0, 1))
    assert ak.requires_grad and a._adapter_kv is None
    with torch.no_grad():
        assert a.adapter_kv(torch.float32)[0] is a.adapter_kv(torch.float32)[0]
    a.train()
    assert a._adapter_kv is None
    # round trip, and the old (1, n_head, 1, 1) gate layout
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k in keys:
                v.copy_(torch.randn(v.shape))
    path = tmp_path / "adapter.pth"
    adapter.save_adapter_checkpoint(model, path)
    saved = torch.load(str(path), weights_only=True)["model"]
    assert set(saved) == keys
    fresh = _stack()
    adapter.adapt(fresh, adapter_start_layer=1)
    adapter.load_adapter_checkpoint(fresh, path)
    assert all(torch.equal(fresh.state_dict()[k], saved[k]) for k in keys)
    old = {k: (v.permute(0, 2, 1, 3) if "gating" in k else v) for k, v in saved.items()}
    torch.save({"model": old}, str(path))
    fresh.blocks[2].attn.gating_factor.data.zero_()
    adapter.load_adapter_checkpoint(fresh, path)
    assert torch.equal(fresh.blocks[2].attn.gating_factor, saved["blocks.2.attn.gating_factor"])
    torch.save({"model": {**saved, "blocks.0.attn.gating_factor": torch.zeros(1, 1, 4, 1)}}, str(path))
    with pytest.raises(KeyError, match="blocks.0"):
        adapter.load_adapter_checkpoint(fresh, path)


def test_attention_stack_builds_the_adapter_method():
    from fastmax_experiments_amd import finetune_step
    m = finetune_step.AttentionStack("pythia-14m", 2, "quadratic", vocab=64, method="adapter")
    trainable = {n: p for n, p in m.named_parameters() if p.requires_grad}
    assert set(trainable) == {f"blocks.{i}.{n}" for i in (0, 1) for n in ("adapter_wte.weight", "gating_factor")}
    assert all(p.dtype == torch.float32 for p in trainable.values()) and not any("lora_" in n for n, _ in m.named_parameters())
    assert all(float(b.gating_factor.detach().abs().min()) >= 0.25 for b in m.blocks)
    with pytest.raises(ValueError, match="method"):
        finetune_step.AttentionStack("pythia-14m", 1, "linearmax", method="adapter")


def test_the_reference_modules_output():
    """lit_gpt.adapter.CausalSelfAttention's own forward (float32, tests/golden/make_golden_adapter_v1.py) against prefix_ref's
    formula wired as adapter.py wires it: the prompt through the QKV linear, slot split, no RoPE on the prompt, one gate per head"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adapter_v1_gqa.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    t = {k: torch.from_numpy(g[k]).double() for k in g.files if k != "meta"}
    H, G, hs, aT = meta["n_head"], meta["n_query_groups"], meta["head_size"], meta["adapter_prompt_length"]
    B, T, _ = t["x"].shape

    def qkv(x):
        return (x @ t["attn.weight"].T + t["attn.bias"]).view(*x.shape[:-1], G, H // G + 2, hs)

    q, k, v = ops.eager_rope_qkv_split(qkv(t["x"]), t["cos"], t["sin"], meta["rope_n_elem"])
    k, v = (x.repeat_interleave(H // G, dim=1) for x in (k, v))
    y = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    prompt = qkv(t["adapter_wte.weight"])
    ak, av = (prompt[:, :, H // G + s].transpose(0, 1) for s in (0, 1))
    out = prefix_ref.formula(y, q, ak, av, t["gating_factor"], hs ** -0.5)[2]
    got = out.transpose(1, 2).reshape(B, T, H * hs) @ t["proj.weight"].T + t["proj.bias"]
    assert t["gating_factor"].abs().min() > 0 and (got - t["y"]).abs().max() < 1e-5 * t["y"].abs().max()
