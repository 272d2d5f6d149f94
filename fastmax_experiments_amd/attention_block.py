"""The caller of the hot path, as a host for parity tests and the data-parallel fine-tune step.

Reproduces the CALL CONTRACT of the reference's ``CausalSelfAttention.forward`` with LoRA / QLoRA layers
(lit_gpt/model.py:380-458 with the ``attn_alg`` dispatch at 432-451, LoRA wiring lit_gpt/lora.py:565-604):
    qkv = attn(x)                      LoRAQKVLinear (4-bit NF4 base when quantised)          model.py:392
    view / permute / split / GQA expand / reshape to (B, n_head, T, head_size)               model.py:397-420
    RoPE on the first rope_n_elem dims (apply_rope, model.py:702-708)                       model.py:422-425
    y = fastmax(q,k,v,p=2,mask) | fastmax_hack(q,k,v,p=1,mask)  -- on the DEVICE tensors     model.py:460-487
    y.reshape(B, T, head_size * n_head)   (no transpose on these branches: quirk Q3)        model.py:453-455
    proj(y)                            LoRALinear                                            model.py:458
It is deliberately NOT a port of lit-gpt's GPT: no config registry, KV cache, MLP or norms -- only the
attention sub-layer that hands tensors to the operator.  Everything outside the two LoRA linears and the
attention operator is stock tensor plumbing.

Generation: ``forward(x, cos, sin, input_pos, state=FastmaxDecodeState(p=2, ...))`` runs the ``fastmax`` block on the
second-order decode state cache (decode.py) in place of the reference's zero-padded KV cache (model.py:427-430): masked p=2
fastmax over everything the state has seen plus the T new tokens, at a fixed cost per token.  ``linearmax`` blocks generate
on a ``LinearmaxDecodeState(B, n_head, head_size, device, n_query_groups=...)``: their prologue's two statistics (the largest
centred-row norms Mq, Mk over the whole sequence) leave the bilinear sums as the one scalar a = 1 / (Mq Mk),
o_i = (S1 + a qc_i^T S2) / (count + a qc_i . ksum) over sums of the centred, UNSCALED rows, so the carried state never needs
rescaling and only two running maxima move (decode.py).  Each of the T rows sees the statistics of everything up to the last
new token, as the masked forward over that sequence would compute them.
"""
import torch
import torch.nn as nn

from . import lora, ops
from .attention_mechanisms.fastmax import fastmax
from .attention_mechanisms.fastmax_hack import fastmax_hack, fastmax_hack_grouped, grouped_route_supported
from .decode import FastmaxDecodeState, LinearmaxDecodeState
from .lora import LoRALinear, LoRAQKVLinear
from .ops import apply_rope, build_rope_cache  # noqa: F401  (re-exported: the public RoPE formula lives beside its kernels)


class CausalSelfAttention(nn.Module):
    gemm_rope = True          # qkv projection + de-interleave + RoPE as one kernel where it applies (settable per instance: A/B)

    def __init__(self, n_embd: int, n_head: int, n_query_groups: int = None, head_size: int = None, bias: bool = False,
                 rotary_percentage: float = 1.0, attn_alg: str = "fastmax", r: int = 8, alpha: int = 16,
                 dropout: float = 0.0, to_query: bool = True, to_key: bool = False, to_value: bool = True,
                 to_projection: bool = False):
        super().__init__()
        self.n_head = n_head
        self.n_query_groups = n_query_groups or n_head
        self.head_size = head_size or n_embd // n_head
        self.rope_n_elem = int(rotary_percentage * self.head_size)
        if attn_alg not in ("fastmax", "linearmax"):
            raise ValueError(f"Attention algorithm {attn_alg} not supported")          # model.py:450-451
        self.attn_alg = attn_alg
        self.fused_neighbours = True          # False: tensor-op slicing instead of the one-pass HIP kernel (A/B, parity tests)
        self.group_views = True               # grouped-query heads: K, V never copied per query head (False: the reference's expand)
        shape = (n_head + 2 * self.n_query_groups) * self.head_size
        self.attn = LoRAQKVLinear(n_embd, shape, n_head=n_head, n_query_groups=self.n_query_groups, r=r, lora_alpha=alpha,
                                  lora_dropout=dropout, enable_lora=(to_query, to_key, to_value), bias=bias)
        self.proj = LoRALinear(self.head_size * n_head, n_embd, r=(r if to_projection else 0), lora_alpha=alpha,
                               lora_dropout=dropout, bias=bias)

    def quantize_base(self, double_quant: bool = False):
        """QLoRA: both frozen linears become 4-bit NF4 (what the bnb precision plugin does in the reference);
        ``double_quant`` = the "bnb.nf4-dq" mode (finetune/lora.py:38)."""
        self.attn.quantize_base(double_quant)
        self.proj.quantize_base(double_quant)
        return self

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, input_pos=None, state=None) -> torch.Tensor:
        """``state`` (a ``FastmaxDecodeState(B, n_head, head_size, p=2, n_query_groups=...)``; for a ``linearmax`` block a
        ``LinearmaxDecodeState(B, n_head, head_size, device, n_query_groups=...)``): generate on the decode state cache.  x holds the T new tokens, cos / sin the rope rows of their positions (``index_select(0, input_pos)`` of the
        cache, as the reference's GPT.forward passes them); ``input_pos`` itself is never read, so nothing syncs with the host.
        Without ``state`` every path is what it was."""
        B, T, C = x.size()
        if state is not None:
            y = self.attend_cached(x, cos, sin, state)
            return self.proj(y.reshape(B, T, self.head_size * self.n_head))      # model.py:453-455 (no transpose: quirk Q3)
        q_per_kv = self.n_head // self.n_query_groups
        total_qkv = q_per_kv + 2
        if self._one_kernel_qkv(x, input_pos, B, T, q_per_kv):
            return self._forward_one_kernel_qkv(x, cos, sin, B, T, q_per_kv)
        qkv = self.attn(x)
        fused = (self.fused_neighbours and x.device.type == "cuda" and input_pos is None and
                 ops.rope_qkv_supported(qkv.dtype, self.head_size, self.rope_n_elem))
        grouped = fused and self._grouped_training_route(x, qkv.dtype, B, q_per_kv)
        views = fused and q_per_kv > 1 and self.group_views
        if grouped:
            # training, grouped-query heads: K stays at its n_query_groups heads through RoPE and the linearmax prologue
            # (statistics and gradient once per key head).  group_views: neither K nor V is ever copied per query head --
            # (batch, group) is the kernels' batch axis and K, V are stride-0 views; else the prologue's store writes the copies
            q, k, v = ops.RopeQKVSplit.apply(qkv.view(B, T, self.n_query_groups, total_qkv, self.head_size), cos, sin,
                                             self.rope_n_elem, 4 if views else 2)
            y = fastmax_hack_grouped(q, k, v, q_per_kv, p=1)
            y = y.reshape(B, T, self.head_size * self.n_head)      # model.py:453-455 (no transpose: quirk Q3)
            return self.proj(y)
        elif fused:
            # de-interleave + RoPE (+ GQA expand, or group views: see ops.RopeQKVSplit) in one HIP pass
            q, k, v = ops.RopeQKVSplit.apply(qkv.view(B, T, self.n_query_groups, total_qkv, self.head_size), cos, sin,
                                             self.rope_n_elem, 3 if views else 1)
        else:
            # shapes the one-pass kernel does not take (decode with input_pos, rotary widths that are not whole 16-byte
            # pieces): plain slicing of the (B, T, group, slot, hs) view -- slots 0..q_per_kv-1 are the group's query heads,
            # then its key head, then its value head (model.py:397-420) -- with K, V repeated per query head
            q, k, v = ops.eager_rope_qkv_split(qkv.view(B, T, self.n_query_groups, total_qkv, self.head_size), cos, sin,
                                               self.rope_n_elem)
            k, v = (t.repeat_interleave(q_per_kv, dim=1) for t in (k, v))
        mask = input_pos is None                                   # model.py:462-466, 477-481
        if self.attn_alg == "linearmax":
            y = fastmax_hack(q, k, v, p=1, mask=mask)              # model.py:472
        else:
            y = fastmax(q, k, v, p=2, mask=mask)                   # model.py:485, minus the .cpu()/.cuda() hops
        y = y.reshape(B, T, self.head_size * self.n_head)          # model.py:453-455 (no transpose: quirk Q3)
        return self.proj(y)

    def _grouped_training_route(self, x, dtype, B, q_per_kv) -> bool:
        """training with grouped-query heads on a linearmax block: K stays at its n_query_groups heads through RoPE and the
        prologue (fastmax_hack_grouped).  ``dtype``: the QKV projection's output dtype; on the one-kernel route, which takes
        bf16 in and gives bf16 out, that is x's own"""
        return (self.attn_alg == "linearmax" and q_per_kv > 1 and torch.is_grad_enabled() and
                (x.requires_grad or any(p.requires_grad for p in self.attn.parameters())) and
                grouped_route_supported(x.device, dtype, self.head_size, B * self.n_head))

    def attend_cached(self, x, cos, sin, state):
        """the attention of ``forward(..., state=...)`` before the head-mixing reshape: x (B,T,C) -> (B, n_head, T, head_size) =
        masked p=2 fastmax (``linearmax`` block: masked first-order linearmax) at the T new positions over the state's tokens and
        the new ones; the state advances by T.  One token onto a non-empty state is a single step straight from the QKV
        projection's output, anything else an ``extend`` (a prefill on an empty state)."""
        if self.attn_alg == "linearmax":
            if isinstance(state, FastmaxDecodeState):
                raise NotImplementedError("a linearmax block generates on a LinearmaxDecodeState, not on a FastmaxDecodeState: its "
                                          "statistics run over the whole sequence, which the fastmax state caches do not carry")
            if not isinstance(state, LinearmaxDecodeState):
                raise TypeError(f"a linearmax block generates on a LinearmaxDecodeState, got {type(state).__name__}")
        elif isinstance(state, LinearmaxDecodeState):
            raise TypeError("a fastmax block generates on a FastmaxDecodeState(p=2), not on a LinearmaxDecodeState")
        B, T, _ = x.size()
        if cos.shape[0] != T or sin.shape[0] != T:
            raise ValueError(f"cos / sin should hold the rope rows of the {T} new positions, got {tuple(cos.shape)}, {tuple(sin.shape)}")
        q_per_kv = self.n_head // self.n_query_groups
        qkv = self.attn(x).view(B, T, self.n_query_groups, q_per_kv + 2, self.head_size)
        if T == 1 and state.count > 0:
            return state.step_qkv(qkv, cos, sin, self.rope_n_elem)
        return state.extend_qkv(qkv, cos, sin, self.rope_n_elem)

    def _one_kernel_qkv(self, x, input_pos, B, T, q_per_kv) -> bool:
        """can the qkv projection, the de-interleave and RoPE run as ONE kernel (nf4_gemm.hip's tile epilogue)?  Training-size bf16
        input on the hand-written GEMM route, whole heads per 256-column tile, and a K / V layout that needs no per-head copies
        (group views, or one query head per group)"""
        attn = self.attn
        if not (self.fused_neighbours and self.gemm_rope and x.device.type == "cuda" and input_pos is None and x.dtype == torch.bfloat16):
            return False
        if not isinstance(attn, lora.LoRAQKVLinear) or (q_per_kv > 1 and not self.group_views):
            return False
        return (ops.rope_qkv_supported(x.dtype, self.head_size, self.rope_n_elem) and
                attn.plan(x, (T, self.n_query_groups, q_per_kv, self.head_size, self.rope_n_elem)).rope)

    def _forward_one_kernel_qkv(self, x, cos, sin, B, T, q_per_kv):
        tables16 = cos.dtype == x.dtype and x.dtype in (torch.bfloat16, torch.float16)
        cos32, sin32 = ops._rope_tables_f32(cos, sin, T, self.rope_n_elem)
        grouped = self._grouped_training_route(x, x.dtype, B, q_per_kv)
        expand = (4 if grouped else 3) if q_per_kv > 1 else 0
        q, k, v = self.attn(x, rope=(cos32, sin32, B, T, self.n_query_groups, q_per_kv, self.head_size, self.rope_n_elem, tables16, expand))
        if grouped:
            y = fastmax_hack_grouped(q, k, v, q_per_kv, p=1)
        elif self.attn_alg == "linearmax":
            y = fastmax_hack(q, k, v, p=1, mask=True)
        else:
            y = fastmax(q, k, v, p=2, mask=True)
        return self.proj(y.reshape(B, T, self.head_size * self.n_head))


# head shapes of the BASELINE.json configs (lit_gpt/config.py:197-205, 1394-1411, 735-747) and of the reference config with the
# largest head size (pythia-1b, config.py:246-254: 8 heads of 256)
CONFIG_SHAPES = {
    "pythia-14m": dict(n_embd=128, n_head=4, n_query_groups=4, head_size=32, rotary_percentage=0.25, bias=True),
    "tiny-llama-1.1b": dict(n_embd=2048, n_head=32, n_query_groups=4, head_size=64, rotary_percentage=1.0, bias=False),
    "Llama-2-7b-hf": dict(n_embd=4096, n_head=32, n_query_groups=32, head_size=128, rotary_percentage=1.0, bias=False),
    "pythia-1b": dict(n_embd=2048, n_head=8, n_query_groups=8, head_size=256, rotary_percentage=0.25, bias=True),
    "Gemma-2b": dict(n_embd=2048, n_head=8, n_query_groups=1, head_size=256, rotary_percentage=1.0, bias=False),   # config.py:796-811 (multi-query)
}
