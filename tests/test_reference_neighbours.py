"""The operator's neighbours against OUTPUTS OF THE REFERENCE'S OWN CODE (tests/golden/make_golden_neighbours.py: apply_rope /
build_rope_cache of lit_gpt/model.py:677-708, chunked_cross_entropy of lit_gpt/utils.py:228-272, LoRALinear / LoRAQKVLinear of
lit_gpt/lora.py:64-433, executed from the reference files in the build container).  Only the .npz files are read here."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
DT = {"torch.float32": torch.float32, "torch.bfloat16": torch.bfloat16, "torch.float16": torch.float16}


def load(name):
    d = np.load(os.path.join(GOLD, name + ".npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    return {k: d[k] for k in d.files if k != "meta"}, meta


def t(a, dtype=None):
    x = torch.from_numpy(np.asarray(a))
    return x.to(dtype) if dtype is not None else x


LORA_CASES = ["lora_linear_r4", "lora_qkv_mha_qv", "lora_qkv_mha_qkv", "lora_qkv_mha_k", "lora_qkv_gqa_qv", "lora_qkv_gqa_qkv",
              "lora_qkv_gqa_v", "lora_qkv_mqa_qv", "lora_qkv_mqa_qk"]


def build_layer(d, meta):
    from fastmax_experiments_amd import lora
    if meta["fn"] == "LoRALinear":
        layer = lora.LoRALinear(meta["in_features"], meta["out_features"], r=meta["r"], lora_alpha=meta["lora_alpha"], bias=meta["bias"])
    else:
        layer = lora.LoRAQKVLinear(meta["in_features"], meta["out_features"], n_head=meta["n_head"], n_query_groups=meta["n_query_groups"],
                                   r=meta["r"], lora_alpha=meta["lora_alpha"], enable_lora=tuple(meta["enable_lora"]), bias=meta["bias"])
    with torch.no_grad():
        layer.linear.weight.copy_(t(d["weight"]))
        if meta["bias"]:
            layer.linear.bias.copy_(t(d["bias"]))
        assert layer.lora_A.shape == d["lora_A"].shape and layer.lora_B.shape == d["lora_B"].shape
        layer.lora_A.copy_(t(d["lora_A"]))
        layer.lora_B.copy_(t(d["lora_B"]))
    return layer


@pytest.mark.parametrize("name", LORA_CASES)
def test_lora_layers_match_the_reference_classes_on_cpu(name):
    """same parameters in, same y, dx, dA, dB, lora_ind, get_lora_AB and merged weight out (float32 tensor-op route of the host
    classes: the formulation of zero_pad / conv1d / lora_ind here is the build's own, the numbers are the reference's)"""
    d, meta = load(name)
    layer = build_layer(d, meta).eval()
    if "lora_ind" in d:
        assert list(layer.lora_ind) == [int(i) for i in d["lora_ind"]]
    x = t(d["x"]).requires_grad_(True)
    y = layer(x)
    assert torch.allclose(y, t(d["y"]), rtol=1e-5, atol=1e-6)
    y.backward(t(d["gy"]))
    # The gradients meet the reference's through a float64 evaluation of the same layer on the same numbers.  A float32
    # evaluation differs from the reference's float32 results by its rounding plus theirs, and on the few elements that cancel
    # (|dA| ~ 2e-4 out of terms ~ 1e-1) that sum exceeds the element-wise tolerance wherever the host BLAS sums in another
    # order than the machine the reference ran on.  The float32 route is held to the float64 one at the tensor's scale.
    layer64 = build_layer(d, meta).double().eval()
    x64 = t(d["x"]).double().requires_grad_(True)
    layer64(x64).backward(t(d["gy"]).double())
    for got, exact, want in ((x.grad, x64.grad, d["dx"]), (layer.lora_A.grad, layer64.lora_A.grad, d["d_lora_A"]),
                             (layer.lora_B.grad, layer64.lora_B.grad, d["d_lora_B"])):
        assert torch.allclose(exact, t(want).double(), rtol=1e-4, atol=1e-6)
        assert got.dtype == torch.float32 and rel_err(got.numpy(), exact.numpy()) < 2e-6
    assert torch.allclose(layer.get_lora_AB(), t(d["lora_AB"]), rtol=1e-5, atol=1e-7)
    layer.merge()
    assert layer.merged and torch.allclose(layer.linear.weight, t(d["merged_weight"]), rtol=1e-5, atol=1e-7)
    assert torch.allclose(layer(t(d["x"])), t(d["y_merged"]), rtol=1e-5, atol=1e-6)


def test_fixture_inventory():
    """every fixture the generator writes is present and carries its call arguments"""
    for n in LORA_CASES + ["rope_f32_hs64_full", "rope_bf16_hs64_cache_f32", "rope_bf16_hs64_cache_bf16", "rope_bf16_hs128_cache_bf16",
                           "rope_bf16_hs32_partial8", "rope_f16_hs64_partial32", "ce_plain", "ce_ignore", "ce_all_ignored", "ce_ignore_index_5"]:
        _, meta = load(n)
        assert meta["fn"] in ("LoRALinear", "LoRAQKVLinear", "apply_rope", "chunked_cross_entropy")


# ---- GPU: the HIP kernels behind the same interfaces ---------------------------------------------------------------------
ROPE_CASES = ["rope_f32_hs64_full", "rope_bf16_hs64_cache_f32", "rope_bf16_hs64_cache_bf16", "rope_bf16_hs128_cache_bf16",
              "rope_bf16_hs32_partial8", "rope_f16_hs64_partial32"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROPE_CASES)
def test_fused_neighbours_kernel_against_reference_apply_rope(name):
    """fastmax_rope.hip (QKV de-interleave + RoPE) reproduces the reference's apply_rope BIT FOR BIT, fp32 and 16-bit rope
    caches, full and partial rotation: q and k heads of the fixture's x come back as its y, v comes back untouched"""
    from fastmax_experiments_amd import ops
    d, meta = load(name)
    xdt, cdt = DT[meta["x_dtype"]], DT[meta["cache_dtype"]]
    B, H, T, hs, n = meta["B"], meta["H"], meta["T"], meta["hs"], meta["rope_n_elem"]
    if not ops.rope_qkv_supported(xdt, hs, n):
        pytest.skip("piece alignment of the kernel")
    x = t(d["x"], xdt).cuda()                                             # (B, H, T, hs)
    want = t(d["y"], DT[meta["out_dtype"]]).cuda()
    cos, sin = t(d["cos"], cdt).cuda(), t(d["sin"], cdt).cuda()
    # one query head per group: qkv (B, T, G = H, 1 + 2, hs) with q = k = v = x
    qkv = x.permute(0, 2, 1, 3).unsqueeze(3).expand(B, T, H, 3, hs).contiguous()
    q, k, v = ops.RopeQKVSplit.apply(qkv, cos, sin, n)
    assert q.dtype == want.dtype
    assert torch.equal(q, want) and torch.equal(k.reshape(B, H, T, hs), want) and torch.equal(v.reshape(B, H, T, hs), x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ce_plain", "ce_ignore", "ce_all_ignored", "ce_ignore_index_5"])
def test_chunked_cross_entropy_against_the_reference(name):
    """every branch of lit_gpt/utils.py:228-272 (tensor / list of chunks, chunk_size 0 / 16 / 128, ignore_index, nothing scored
    -> 0 in the chunked branches and NaN where the reference takes cross_entropy's own mean): losses and d(logits)"""
    from fastmax_experiments_amd.loss import chunked_cross_entropy
    d, meta = load(name)
    logits, targets = t(d["logits"]).cuda(), t(d["targets"]).cuda()
    for tag, split, cs in [("tensor_chunk128", 0, 128), ("tensor_chunk16", 0, 16), ("tensor_chunk0", 0, 0), ("list16_chunk128", 16, 128),
                           ("list8_chunk0", 8, 0)]:
        lg = logits.clone().requires_grad_(True)
        arg = list(lg.split(split, dim=1)) if split else lg
        loss = chunked_cross_entropy(arg, targets, chunk_size=cs, ignore_index=meta["ignore_index"])
        want = float(d["loss_" + tag])
        if np.isnan(want):
            assert torch.isnan(loss), tag
            continue
        assert abs(float(loss) - want) <= 2e-6 * max(1.0, abs(want)), tag
        if "dlogits_" + tag in d:
            loss.backward()
            assert torch.allclose(lg.grad.cpu(), t(d["dlogits_" + tag]), rtol=1e-4, atol=1e-7), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", LORA_CASES)
def test_lora_layers_on_the_device_against_the_reference(name):
    """the same fixtures through the device route of the host classes (bf16 tensors: results within bf16 rounding of the
    reference's float32 numbers)"""
    d, meta = load(name)
    layer = build_layer(d, meta).eval().to(torch.bfloat16).cuda()
    x = t(d["x"], torch.bfloat16).cuda().requires_grad_(True)
    y = layer(x)
    y.backward(t(d["gy"], torch.bfloat16).cuda())
    scale = lambda a: float(np.abs(a).max())
    assert float((y.float().cpu() - t(d["y"])).abs().max()) <= 2e-2 * scale(d["y"])
    assert float((x.grad.float().cpu() - t(d["dx"])).abs().max()) <= 3e-2 * scale(d["dx"])
    assert float((layer.lora_A.grad.float().cpu() - t(d["d_lora_A"])).abs().max()) <= 3e-2 * scale(d["d_lora_A"])
    assert float((layer.lora_B.grad.float().cpu() - t(d["d_lora_B"])).abs().max()) <= 3e-2 * scale(d["d_lora_B"])
