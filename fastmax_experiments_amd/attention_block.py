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
import importlib
from typing import NamedTuple, Union

import torch
import torch.nn as nn

from . import ops
from .attention_mechanisms.fastmax import MAX_HEADS_PER_LAUNCH, fastmax
from .attention_mechanisms.fastmax_hack import LinearmaxPlan, fastmax_hack_grouped, linearmax, linearmax_plan
from .decode import check_block_cache
from .lora import LoRALinear, LoRAQKVLinear
from .ops import apply_rope, build_rope_cache  # noqa: F401  (re-exported: the public RoPE formula lives beside its kernels)

_switches = importlib.import_module(linearmax.__module__)          # the module (its package rebinds the name to the function)


class AttentionPlan(NamedTuple):
    qkv: str                                 # how q, k, v are produced: "gemm_epilogue", "hip_pass" or "eager"
    kv_layout: int                           # the K / V layout handed on: one of ops.KV_LAYOUTS
    operator: Union[str, LinearmaxPlan]      # "fastmax" (p = 2), or the linearmax call's own plan


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
        Without ``state``: ``plan``, one of its three q, k, v producers, the operator."""
        B, T, C = x.size()
        if state is not None:
            y = self.attend_cached(x, cos, sin, state)
        else:
            plan = self.plan(x, input_pos)
            G, hs, n = self.n_query_groups, self.head_size, self.rope_n_elem
            q_per_kv = self.n_head // G
            if plan.qkv == "gemm_epilogue":
                tables16 = cos.dtype == x.dtype and x.dtype in (torch.bfloat16, torch.float16)
                cos32, sin32 = ops._rope_tables_f32(cos, sin, T, n)
                q, k, v = self.attn(x, rope=(cos32, sin32, B, T, G, q_per_kv, hs, n, tables16, plan.kv_layout))
            elif plan.qkv == "hip_pass":
                # de-interleave + RoPE (+ GQA expand, or group views: see ops.KV_LAYOUTS) in one HIP pass
                q, k, v = ops.RopeQKVSplit.apply(self.attn(x).view(B, T, G, q_per_kv + 2, hs), cos, sin, n, plan.kv_layout)
            else:
                # plain slicing of the (B, T, group, slot, hs) view -- slots 0..q_per_kv-1 are the group's query heads, then its
                # key head, then its value head (model.py:397-420) -- with K, V repeated per query head
                q, k, v = ops.eager_rope_qkv_split(self.attn(x).view(B, T, G, q_per_kv + 2, hs), cos, sin, n)
                k, v = (t.repeat_interleave(q_per_kv, dim=1) for t in (k, v))
            y = self._attend(q, k, v, plan.operator, input_pos is None, q_per_kv)
        return self.proj(y.reshape(B, T, self.head_size * self.n_head))      # model.py:453-455 (no transpose: quirk Q3)

    def plan(self, x, input_pos=None) -> AttentionPlan:
        """The one decision "how does forward(x, cos, sin, input_pos) run", from x's device, dtype, shape and grad state, the
        instance switches (fused_neighbours, group_views, gemm_rope) and the QKV projection's own plan; nothing is computed.
          qkv        "gemm_epilogue": projection, de-interleave and RoPE as ONE kernel (nf4_gemm.hip's tile epilogue) -- where the
                     projection's plan allows it and the K / V layout needs no per-head copies (group views, or one query head per
                     group); "hip_pass": ops.RopeQKVSplit after the projection; "eager": tensor slicing, for what the pass does
                     not take (decode with input_pos, rotary widths that are not whole 16-byte pieces)
          kv_layout  one of ops.KV_LAYOUTS.  Training a linearmax block with grouped-query heads keeps K at its n_query_groups
                     heads through RoPE and the prologue (statistics and gradient once per key head); group_views: neither K nor
                     V is ever copied per query head, else the prologue's store writes the copies
          operator   "fastmax" (p = 2), or the linearmax_plan record of the call as it is launched"""
        B, T = x.shape[:2]
        G, hs, n = self.n_query_groups, self.head_size, self.rope_n_elem
        q_per_kv = self.n_head // G
        mask = input_pos is None                                   # model.py:462-466, 477-481
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.attn.parameters()))
        hip_pass = self.fused_neighbours and x.device.type == "cuda" and mask and ops.rope_qkv_supported(x.dtype, hs, n)
        views = hip_pass and q_per_kv > 1 and self.group_views
        k_groups = (hip_pass and self.attn_alg == "linearmax" and q_per_kv > 1 and needs_grad and _switches.GROUPED_K
                    and B * self.n_head <= MAX_HEADS_PER_LAUNCH)
        if (hip_pass and self.gemm_rope and x.dtype == torch.bfloat16 and isinstance(self.attn, LoRAQKVLinear)
                and (views or q_per_kv == 1) and self.attn.plan(x, (T, G, q_per_kv, hs, n)).rope):
            qkv, layout = "gemm_epilogue", (ops.KV_GROUPS if q_per_kv == 1 else ops.K_GROUPS_V_VIEWS if k_groups else ops.KV_VIEWS)
        elif hip_pass:
            qkv = "hip_pass"
            layout = ((ops.K_GROUPS_V_VIEWS if views else ops.K_GROUPS_V_COPIES) if k_groups else
                      (ops.KV_VIEWS if views else ops.KV_COPIES))
        else:
            qkv, layout = "eager", ops.KV_COPIES
        if self.attn_alg != "linearmax":
            return AttentionPlan(qkv, layout, "fastmax")
        heads = (B * G, q_per_kv) if ops.KV_LAYOUTS[layout].v == "views" else (B, self.n_head)
        return AttentionPlan(qkv, layout, linearmax_plan(x.dtype, *heads, T, T, hs, 1, mask, needs_grad, q_per_kv if k_groups else 1,
                                                         k_groups and views))

    def _attend(self, q, k, v, operator, mask, q_per_kv):
        if operator == "fastmax":
            return fastmax(q, k, v, p=2, mask=mask)                # model.py:485, minus the .cpu()/.cuda() hops
        if operator.k_layout == "per_head":
            return linearmax(q, k, v, operator, p=1, mask=mask)      # model.py:472
        return fastmax_hack_grouped(q, k, v, q_per_kv, p=1, plan=operator)

    def attend_cached(self, x, cos, sin, state):
        """the attention of ``forward(..., state=...)`` before the head-mixing reshape: x (B,T,C) -> (B, n_head, T, head_size) =
        masked p=2 fastmax (``linearmax`` block: masked first-order linearmax) at the T new positions over the state's tokens and
        the new ones; the state advances by T.  One token onto a non-empty state is a single step straight from the QKV
        projection's output, anything else an ``extend`` (a prefill on an empty state).  A ``fastmax`` block also takes a
        ``FastmaxKVDecodeState`` (p=2; ``FastmaxKVDecodeState.for_attention``): the same function over a cache of K and V rows,
        for head sizes up to 256."""
        check_block_cache(self.attn_alg, state)
        B, T, _ = x.size()
        if cos.shape[0] != T or sin.shape[0] != T:
            raise ValueError(f"cos / sin should hold the rope rows of the {T} new positions, got {tuple(cos.shape)}, {tuple(sin.shape)}")
        q_per_kv = self.n_head // self.n_query_groups
        qkv = self.attn(x).view(B, T, self.n_query_groups, q_per_kv + 2, self.head_size)
        if T == 1 and state.count > 0:
            return state.step_qkv(qkv, cos, sin, self.rope_n_elem)
        return state.extend_qkv(qkv, cos, sin, self.rope_n_elem)


# head shapes of the BASELINE.json configs (lit_gpt/config.py:197-205, 1394-1411, 735-747) and of the reference config with the
# largest head size (pythia-1b, config.py:246-254: 8 heads of 256)
CONFIG_SHAPES = {
    "pythia-14m": dict(n_embd=128, n_head=4, n_query_groups=4, head_size=32, rotary_percentage=0.25, bias=True),
    "tiny-llama-1.1b": dict(n_embd=2048, n_head=32, n_query_groups=4, head_size=64, rotary_percentage=1.0, bias=False),
    "Llama-2-7b-hf": dict(n_embd=4096, n_head=32, n_query_groups=32, head_size=128, rotary_percentage=1.0, bias=False),
    "pythia-1b": dict(n_embd=2048, n_head=8, n_query_groups=8, head_size=256, rotary_percentage=0.25, bias=True),
    "Gemma-2b": dict(n_embd=2048, n_head=8, n_query_groups=1, head_size=256, rotary_percentage=1.0, bias=False),   # config.py:796-811 (multi-query)
    "pythia-70m": dict(n_embd=512, n_head=8, n_query_groups=8, head_size=64, rotary_percentage=0.25, bias=True),   # config.py:216-225, defaults 30-91
    "Mixtral-8x7B-v0.1": dict(n_embd=4096, n_head=32, n_query_groups=8, head_size=128, rotary_percentage=1.0, bias=False),   # config.py:1344-1362
}
