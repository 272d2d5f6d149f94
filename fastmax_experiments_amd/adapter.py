"""LLaMA-Adapter (adapter v1) fine-tuning for MI355X: a gated attention over a learned prompt behind every softmax block, in HIP.

Mirrors the reference's ``lit_gpt/adapter.py``:
  AdapterCausalSelfAttention           adapter.py:104-158   y + gating_factor * softmax(q ak^T / sqrt(hs)) av, where (ak, av) are
                                                            the K and V slots of the layer's own QKV projection of
                                                            ``adapter_wte.weight`` (no RoPE, no mask)
  adapter_filter                       adapter.py:167-168
  mark_only_adapter_as_trainable       adapter.py:161-164
The term lives inside scaled_dot_product_attention, which only ``attn_alg="quadratic"`` blocks call: adapting a ``fastmax`` /
``linearmax`` layer raises.  What runs in csrc/prefix_attention.hip (C ABI and rounding points: include/fastmax_hip_prefix.h,
bound by ``_lib.ABI_EXT3``): the forward as one launch behind the causal kernel, the backward as one tile kernel and an
ordered reduce (``ops.prefix_attention_add``).  ``ak`` and ``av`` stay at their KV heads: the kernels index the group.

One deliberate deviation: the reference caches (ak, av) on first use even while training, so a second training step would run
on the first step's prompt.  Here the cache is filled and used only when no gradient is needed, and ``train()`` drops it.
``prefix_fused = False`` selects the reference's expression in tensor ops (A/B runs, parity tests).
"""
import math
from typing import Any

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .attention_block import CausalSelfAttention


def prefix_attention_tensor_ops(y, q, ak, av, gate, dtype=None):
    """adapter.py:146-149 restated: a second attention call with the all-ones mask, a multiply and an add.  y, q (B,H,T,hs);
    ak, av (Hkv,aT,hs), repeated per query head as there; gate (1,1,H,1).  ``dtype``: compute in it (float32 for a parity
    reference) and return it."""
    dt = dtype or q.dtype
    r = q.shape[1] // ak.shape[0]
    ak, av = (t.to(dt).repeat_interleave(r, dim=0).unsqueeze(0) for t in (ak, av))
    amask = torch.ones(q.shape[2], ak.shape[2], dtype=torch.bool, device=q.device)
    ay = F.scaled_dot_product_attention(q.to(dt), ak, av, attn_mask=amask, dropout_p=0.0, scale=1.0 / math.sqrt(q.shape[3]))
    return y.to(dt) + gate.to(dt).reshape(1, -1, 1, 1) * ay


class AdapterCausalSelfAttention(CausalSelfAttention):
    """A ``CausalSelfAttention`` (``attn_alg="quadratic"``) with the adaption prompt: ``adapter_wte`` (``nn.Embedding(aT,
    n_embd)``) and ``gating_factor`` (zeros, (1, 1, n_head, 1)), under the reference's state-dict keys.  Made by ``adapt``."""

    prefix_fused = True          # False: the tensor-op restatement (settable per instance)
    _adapter_kv = None

    @classmethod
    def from_attention(cls, attn: CausalSelfAttention, adapter_prompt_length: int = 10) -> "AdapterCausalSelfAttention":
        """the same module object, converted in place (its linears are kept, not copied)"""
        if attn.attn_alg != "quadratic":
            raise ValueError(f"adapter v1 lives inside softmax attention: attn_alg={attn.attn_alg!r} has no adaption prompt "
                             "(build the block with attn_alg='quadratic', or use adapter_v2)")
        if not 1 <= adapter_prompt_length <= ops.PREFIX_MAX_ROWS:
            raise ValueError(f"adapter_prompt_length should be 1 .. {ops.PREFIX_MAX_ROWS}, got {adapter_prompt_length}")
        if isinstance(attn, cls):
            raise ValueError("the attention is adapted already")
        lin = getattr(attn.attn, "linear", attn.attn)
        w = lin.weight
        dtype = w.quant_state[2] if hasattr(w, "quant_state") else w.dtype if w.dtype.is_floating_point else torch.bfloat16
        attn.__class__ = cls
        attn.adapter_wte = nn.Embedding(adapter_prompt_length, lin.in_features, device=w.device, dtype=dtype)
        attn.gating_factor = nn.Parameter(torch.zeros(1, 1, attn.n_head, 1, device=w.device, dtype=dtype))
        attn._adapter_kv = None
        return attn

    @property
    def adapter_prompt_length(self) -> int:
        return self.adapter_wte.num_embeddings

    def reset_parameters(self) -> None:
        nn.init.zeros_(self.gating_factor)

    def train(self, mode: bool = True):
        self._adapter_kv = None
        return super().train(mode)

    def adapter_kv(self, dtype):
        """(ak, av), each (n_query_groups, aT, head_size) in ``dtype``: the prompt through the QKV linear, K and V slots of each
        group, no RoPE.  Cached only when nothing needs a gradient."""
        need_grad = torch.is_grad_enabled() and (self.adapter_wte.weight.requires_grad or
                                                 any(p.requires_grad for p in self.attn.parameters()))
        if not need_grad and self._adapter_kv is not None and self._adapter_kv[0].dtype == dtype:
            return self._adapter_kv
        G, hs, aT = self.n_query_groups, self.head_size, self.adapter_prompt_length
        q_per_kv = self.n_head // G
        aqkv = self.attn(self.adapter_wte.weight.to(dtype).unsqueeze(0)).view(aT, G, q_per_kv + 2, hs)
        ak, av = (aqkv[:, :, q_per_kv + s].transpose(0, 1).contiguous() for s in (0, 1))
        if not need_grad:
            self._adapter_kv = (ak, av)
        return ak, av

    def _attend(self, q, k, v, operator, mask, q_per_kv):
        y = super()._attend(q, k, v, operator, mask, q_per_kv)          # group views: (B * G, q_per_kv, T, hs), head-major
        T, hs = q.shape[2], q.shape[3]
        out = self._prefix(y.reshape(-1, self.n_head, T, hs), q.reshape(-1, self.n_head, T, hs), *self.adapter_kv(q.dtype))
        return out.reshape(y.shape)

    def _prefix(self, y, q, ak, av):
        if not self.prefix_fused:
            return prefix_attention_tensor_ops(y, q, ak, av, self.gating_factor)
        return ops.prefix_attention_add(y, q, ak, av, self.gating_factor)

    def attend_cached(self, x, cos, sin, state):
        with torch.no_grad():
            state.prefix = (*self.adapter_kv(x.dtype), self.gating_factor)
        return super().attend_cached(x, cos, sin, state)

    def _load_from_state_dict(self, state_dict, prefix, *args: Any, **kwargs: Any) -> None:
        """adapter.py:154-158: older checkpoints keep the gate as (1, n_head, 1, 1)"""
        key = prefix + "gating_factor"
        if key in state_dict and state_dict[key].dim() == 4 and state_dict[key].size(1) == self.n_head:
            state_dict[key] = state_dict[key].permute(0, 2, 1, 3)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


def _blocks_of(model):
    blocks = getattr(model, "blocks", model)
    if isinstance(blocks, (nn.ModuleList, list, tuple)):
        return list(blocks)
    raise TypeError(f"adapt: expected a BlockStack, a NeoXStack or a list of blocks, got {type(model).__name__}")


def adapt(model, adapter_prompt_length: int = 10, adapter_start_layer: int = 2) -> int:
    """Convert, in place, the attention of every block from index ``adapter_start_layer`` on (adapter.py:110) of a ``BlockStack``
    / ``NeoXStack`` / list of blocks or of bare ``CausalSelfAttention`` layers.  -> the number of layers adapted.  A layer whose
    ``attn_alg`` is not "quadratic" raises ValueError, before anything is changed."""
    todo = []
    for i, blk in enumerate(_blocks_of(model)):
        attn = blk if isinstance(blk, CausalSelfAttention) else getattr(blk, "attn", None)
        if not isinstance(attn, CausalSelfAttention):
            raise TypeError(f"adapt: block {i} ({type(blk).__name__}) has no CausalSelfAttention")
        if i >= adapter_start_layer:
            if attn.attn_alg != "quadratic":
                raise ValueError(f"adapt: block {i} has attn_alg={attn.attn_alg!r}; adapter v1 needs 'quadratic' (softmax) attention")
            todo.append(attn)
    for attn in todo:
        AdapterCausalSelfAttention.from_attention(attn, adapter_prompt_length)
    return len(todo)


def adapter_filter(key: str, value: Any) -> bool:
    """lit_gpt/adapter.py:167-168"""
    return "adapter_wte" in key or "gating_factor" in key


def mark_only_adapter_as_trainable(model: nn.Module) -> None:
    """lit_gpt/adapter.py:161-164"""
    for name, param in model.named_parameters():
        param.requires_grad = adapter_filter(name, param)


def save_adapter_checkpoint(model: nn.Module, file_path) -> None:
    """finetune/adapter.py: only what ``adapter_filter`` names goes to disk"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if adapter_filter(k, v)}
    torch.save({"model": sd}, str(file_path))


def load_adapter_checkpoint(model: nn.Module, file_path) -> None:
    """the prompts and gates on top of the already-loaded base model (strict=False); a gate in the old (1, n_head, 1, 1) layout
    is permuted.  A key the model does not have raises."""
    ckpt = torch.load(str(file_path), map_location="cpu", weights_only=True)
    sd = dict(ckpt.get("model", ckpt))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if unexpected:
        raise KeyError(f"unexpected keys in adapter checkpoint: {unexpected}")
