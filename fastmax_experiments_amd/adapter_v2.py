"""Adapter-v2 fine-tuning for MI355X: a trainable per-column scale and bias behind every linear, in HIP.

Mirrors the reference's ``lit_gpt/adapter_v2.py``:
  AdapterV2Linear                      adapter_v2.py:50-62   y = adapter_scale * (linear(x) + adapter_bias)
  adapter_filter                       adapter_v2.py:34-47   the adapter parameters and the norms
  mark_only_adapter_v2_as_trainable    adapter_v2.py:221-224
Adapter v2 does not depend on the attention operator, which is why it is the adapter method built here: the adaption prompt of
adapter v1 lives inside scaled_dot_product_attention, which a ``fastmax`` / ``linearmax`` block never calls.  The base
``linear`` may be dense or an ``NF4Linear`` (``finetune/adapter_v2.py --quantize bnb.nf4``).

What runs in csrc/adapter_v2.hip (C ABI and rounding points: include/fastmax_hip_adapter.h, bound by ``_lib.ABI``):
    adapter_forward     z -> y, one read and one write
    adapter_backward    (dy, z) -> dz and both parameter gradients in one pass, the sums in a fixed order
There is no CPU path through the kernels; ``AdapterV2Linear.fused = False`` selects the reference's expression in tensor ops
(A/B runs, parity tests).  ``adapt(module)`` turns a model built from this package's blocks into its adapter-v2 form.
"""
from typing import Any

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .lora import LoRALinear, NF4Linear

# Whether a new AdapterV2Linear runs the kernels: measured ahead of the tensor-op form at every training shape by far more than
# the spread between runs (profiles/r22_adapter_v2.md).  One decode-size call in an eager loop costs the host more than the two
# torch operators do; a graphed loop does not see it
FUSED_DEFAULT = True
ROWS_PER_BLOCK = _lib.ADAPTER_ROWS_PER_BLOCK


# ---- kernel calls -------------------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor, N: int) -> torch.Tensor:
    """(..., N) -> (M, N) with unit stride along the row (a view whenever the layout allows)"""
    t2 = t.reshape(-1, N)
    return t2 if t2.stride(1) == 1 and t2.stride(0) >= N else t2.contiguous()


def _operands(what: str, z: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor):
    """checks, then (N, y's dtype, scale, bias) with the parameters contiguous"""
    N = z.shape[-1] if z.dim() else 0
    if N == 0:
        raise ValueError(f"{what}: z should be (..., N) with N >= 1, got shape {tuple(z.shape)}")
    for name, p in (("scale", scale), ("bias", bias)):
        if p.dim() != 1 or p.shape[0] != N:
            raise ValueError(f"{what}: {name} should have {N} elements, got shape {tuple(p.shape)}")
    if scale.dtype != bias.dtype or (scale.dtype != z.dtype and scale.dtype != torch.float32):
        raise ValueError(f"{what}: scale and bias should both be {z.dtype} or float32, got {scale.dtype} and {bias.dtype}")
    if z.device.type != "cuda":
        ops._device()                         # no device at all: the package's one message
        raise RuntimeError(f"{what} runs on an MI355X only; there is no CPU path through the kernels "
                           "(fused = False selects the tensor-op restatement)")
    if z.dtype not in ops._DT:
        raise TypeError(f"{what}: dtype {z.dtype} is not float32, bfloat16 or float16")
    if scale.device != z.device or bias.device != z.device:
        raise ValueError(f"{what}: z is on {z.device}, scale on {scale.device}, bias on {bias.device}")
    return N, torch.promote_types(z.dtype, scale.dtype), scale.detach().contiguous(), bias.detach().contiguous()


def adapter_forward(z: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """scale * (z + bias) over the last dimension of z (..., N); scale, bias (N,) in z's dtype or float32.  The sum is rounded
    to z's dtype before the product when the parameters have it; with float32 parameters the result is float32."""
    N, ydt, sc, bi = _operands("adapter_forward", z, scale, bias)
    if z.numel() == 0:
        return torch.empty(z.shape, dtype=ydt, device=z.device)
    z2 = _rows(z, N)
    M = z2.shape[0]
    y = torch.empty((M, N), dtype=ydt, device=z.device)
    ops._call("fastmax_hip_adapter_forward", z.device,
              (z2.data_ptr(), z2.stride(0), sc.data_ptr(), bi.data_ptr(), y.data_ptr(), y.stride(0), M, N, ops._DT[z.dtype],
               ops._DT[sc.dtype]))
    return y.view(z.shape)


def adapter_backward_workspace(M: int, N: int, dtype, want_param_grads: bool) -> int:
    return int(_lib.lib().fastmax_hip_adapter_backward_workspace(M, N, ops._DT[dtype], int(bool(want_param_grads))))


def adapter_backward(dy, z, scale, bias, want_dz: bool = True, want_param_grads: bool = True):
    """-> (dz, dscale, dbias), each None unless asked for: dz in z's dtype; dscale, dbias (N,) float32, bitwise reproducible.
    One pass over dy and z."""
    N, ydt, sc, bi = _operands("adapter_backward", z, scale, bias)
    if dy.shape != z.shape:
        raise ValueError(f"adapter_backward: dy should have z's shape {tuple(z.shape)}, got {tuple(dy.shape)}")
    if not (want_dz or want_param_grads):
        return None, None, None
    dev = z.device
    dsc, dbi = ((torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2)) if want_param_grads else (None, None))
    if z.numel() == 0:
        return (torch.empty_like(z) if want_dz else None,) + ((dsc.zero_(), dbi.zero_()) if want_param_grads else (None, None))
    z2 = _rows(z, N)
    dy2 = _rows(dy if dy.dtype == ydt else dy.to(ydt), N)
    M = z2.shape[0]
    dz = torch.empty((M, N), dtype=z.dtype, device=dev) if want_dz else None
    ws = adapter_backward_workspace(M, N, z.dtype, want_param_grads)
    ops._call("fastmax_hip_adapter_backward", dev,
              (dy2.data_ptr(), dy2.stride(0), z2.data_ptr(), z2.stride(0), sc.data_ptr(), bi.data_ptr(), ops._ptr(dz),
               0 if dz is None else dz.stride(0), ops._ptr(dsc), ops._ptr(dbi), M, N, ops._DT[z.dtype], ops._DT[sc.dtype]), ws=ws)
    return (None if dz is None else dz.view(z.shape)), dsc, dbi


# ---- autograd -------------------------------------------------------------------------------------------------------------------
class _AdapterV2Fn(torch.autograd.Function):
    """(z, scale, bias) -> y.  dz only when z asks for it, the sums only when a parameter does."""

    @staticmethod
    def forward(ctx, z, scale, bias):
        ctx.save_for_backward(z, scale, bias)
        return adapter_forward(z, scale, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        z, scale, bias = ctx.saved_tensors
        want = ctx.needs_input_grad
        dz, dsc, dbi = adapter_backward(dy, z, scale, bias, want_dz=want[0], want_param_grads=want[1] or want[2])
        return dz, (dsc.to(scale.dtype) if want[1] else None), (dbi.to(bias.dtype) if want[2] else None)


def adapter_v2(z: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """scale * (z + bias) through the kernels, differentiable once; under ``no_grad``, or when nothing asks for a gradient,
    the forward kernel alone (nothing is saved)"""
    if torch.is_grad_enabled() and (z.requires_grad or scale.requires_grad or bias.requires_grad):
        return _AdapterV2Fn.apply(z, scale, bias)
    return adapter_forward(z, scale, bias)


# ---- the layer ------------------------------------------------------------------------------------------------------------------
class AdapterV2Linear(nn.Module):
    """lit_gpt/adapter_v2.py:50-62: same constructor, same state-dict keys (``linear.weight``, ``linear.bias``,
    ``adapter_bias``, ``adapter_scale``), both adapter parameters created frozen as there."""

    def __init__(self, in_features: int, out_features: int, **kwargs: Any) -> None:
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, **kwargs)
        self._init_adapter(out_features, self.linear.weight.device)

    def _init_adapter(self, out_features: int, device) -> None:
        self.adapter_bias = nn.Parameter(torch.zeros(out_features, device=device), requires_grad=False)
        self.adapter_scale = nn.Parameter(torch.ones(out_features, device=device), requires_grad=False)
        self.fused = FUSED_DEFAULT            # False: the tensor-op restatement in forward
        # True: float32 adapter parameters beside 16-bit activations are cast to the activations' dtype on the way in (master
        # weights, as the LoRA matrices are used), so y keeps that dtype; False is torch's promotion, as in the reference
        self.cast_params = False

    @classmethod
    def from_linear(cls, lin: nn.Module) -> "AdapterV2Linear":
        """around an existing ``nn.Linear`` / ``NF4Linear``, which is kept, not copied; the adapter parameters take the dtype of
        the dense weight, or the one the NF4 codes were quantised from, so a "bf16-true" model stays in one dtype"""
        if not isinstance(lin, (nn.Linear, NF4Linear)):
            raise TypeError(f"AdapterV2Linear.from_linear: expected nn.Linear or NF4Linear, got {type(lin).__name__}")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.linear = lin
        self._init_adapter(lin.out_features, lin.weight.device)
        dtype = lin.weight.quant_state[2] if isinstance(lin, NF4Linear) else lin.weight.dtype
        self.adapter_bias.data = self.adapter_bias.data.to(dtype)
        self.adapter_scale.data = self.adapter_scale.data.to(dtype)
        return self

    def reset_parameters(self) -> None:
        nn.init.zeros_(self.adapter_bias)
        nn.init.ones_(self.adapter_scale)

    def quantize_base(self, double_quant: bool = False) -> "AdapterV2Linear":
        """swap the dense frozen layer for its NF4 version, as ``LoRALinear.quantize_base`` does"""
        if not isinstance(self.linear, NF4Linear):
            self.linear = NF4Linear.from_linear(self.linear, double_quant=double_quant)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        z, scale, bias = self.linear(x), self.adapter_scale, self.adapter_bias
        if self.cast_params and scale.dtype != z.dtype:
            scale, bias = scale.to(z.dtype), bias.to(z.dtype)
        if not self.fused:
            return scale * (z + bias)
        return adapter_v2(z, scale, bias)


# ---- a model's adapter-v2 form ---------------------------------------------------------------------------------------------
def adapt(module: nn.Module) -> int:
    """Replace, in place, every ``LoRALinear`` / ``LoRAQKVLinear`` of ``module`` whose LoRA branch is absent (r == 0, or merged)
    by an ``AdapterV2Linear`` around the same ``linear`` (dense or NF4), and a ``NextTokenHead``'s ``lm_head`` likewise.
    -> the number of layers replaced.  A live LoRA branch raises ValueError naming the module; anything inside a
    ``moe.LLaMAMoE`` raises NotImplementedError (its decode route reads ``LoRALinear`` internals)."""
    from .generate import NextTokenHead
    from .moe import LLaMAMoE
    todo = []
    for name, m in module.named_modules():
        if isinstance(m, LLaMAMoE):
            raise NotImplementedError(f"adapt: {name or type(m).__name__} is a LLaMAMoE; adapter v2 on its experts is not built")
        for child_name, child in m.named_children():
            full = f"{name}.{child_name}" if name else child_name
            if isinstance(child, LoRALinear):
                if child._lora_enabled():
                    raise ValueError(f"adapt: {full} has a live LoRA branch (r = {child.r}); merge it or build the model with r=0")
                todo.append((m, child_name, child.linear))
            elif isinstance(m, NextTokenHead) and child_name == "lm_head" and not isinstance(child, AdapterV2Linear):
                todo.append((m, child_name, child))
    if isinstance(module, LoRALinear):
        raise ValueError("adapt: pass the module that holds the layer; a bare LoRALinear cannot be replaced in place")
    for parent, child_name, lin in todo:
        new = AdapterV2Linear.from_linear(lin)
        new.train(parent.training)
        setattr(parent, child_name, new)
    return len(todo)


def adapter_filter(key: str, value: Any) -> bool:
    """lit_gpt/adapter_v2.py:34-47 (the adapter-v1 names stay in the list, as there)"""
    return any(s in key for s in ("adapter_wte", "gating_factor", "adapter_scale", "adapter_bias", "norm_1", "norm_2", "ln_f"))


def mark_only_adapter_v2_as_trainable(model: nn.Module) -> None:
    """lit_gpt/adapter_v2.py:221-224: the adapter parameters and the norms train, nothing else"""
    for name, param in model.named_parameters():
        param.requires_grad = adapter_filter(name, param)


# adapter-v1 parameters of a reference checkpoint: inert for these attention operators, skipped on load
_V1_KEYS = ("adapter_wte", "gating_factor")


def save_adapter_checkpoint(model: nn.Module, file_path) -> None:
    """finetune/adapter_v2.py: only what ``adapter_filter`` names goes to disk (``filter={"model": adapter_filter}``)"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if adapter_filter(k, v)}
    torch.save({"model": sd}, str(file_path))


def load_adapter_checkpoint(model: nn.Module, file_path) -> None:
    """adapter weights and norms on top of the already-loaded base model (strict=False).  Keys of adapter v1 are skipped; any
    other key the model does not have raises."""
    ckpt = torch.load(str(file_path), map_location="cpu", weights_only=True)
    sd = ckpt.get("model", ckpt)
    sd = {k: v for k, v in sd.items() if not any(s in k for s in _V1_KEYS)}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if unexpected:
        raise KeyError(f"unexpected keys in adapter-v2 checkpoint: {unexpected}")
