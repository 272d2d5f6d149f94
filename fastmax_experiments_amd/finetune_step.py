"""A launchable data-parallel QLoRA fine-tune step around the fastmax operator (`bench.py --workload dp_step`).

Step structure of the reference's `finetune/lora.py:fit` (207-226) with the batch sharded over one process per GPU:
    for each of `gradient_accumulation_iters` micro-batches:   logits -> loss -> backward(loss / iters)     (no collective)
    at the boundary:  ONE all-reduce of the flat LoRA-gradient bucket (RCCL over xGMI), AdamW step, zero_grad
(`lit_gpt/args.py:40-57` for the accumulation arithmetic; the reference itself runs FSDP through Lightning Fabric and refuses
quantisation with devices > 1, finetune/lora.py:80-85 -- there is no reference behaviour to match beyond "same update as one
process with the same global batch", which tests/test_dp_gloo.py checks).

The model is NOT lit-gpt's GPT: it is `n_layer` attention sub-layers (NF4 base + LoRA on q, v; fastmax or linearmax) with
residual connections and a frozen lm-head feeding the chunked cross entropy -- the parts of the step the hot path owns.
Inputs are synthetic hidden states (no embedding table, no tokenizer, no checkpoint: none can be fetched here).
"""
from __future__ import annotations

import time
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from . import dp


class AttentionStack(nn.Module):
    """n_layer x (x + CausalSelfAttention(x)) with QLoRA linears, then the lm-head loss of finetune/lora.py:216-219.
    ``block="full"``: n_layer whole decoder blocks (block.py: RMSNorm, attention, RMSNorm, gated MLP at the config's
    intermediate_size, both residual adds) in place of the bare attention sub-layers.  ``block="neox"``: n_layer whole
    parallel-residual blocks (neox_block.py: the LayerNorm pair, attention, the GELU MLP, the three-way add), what the pythia
    configs are.  ``method="adapter_v2"``: the same blocks without a LoRA branch, every linear an ``AdapterV2Linear`` and the
    adapter parameters and the norms trainable (finetune/adapter_v2.py), in place of the default ``"lora"``."""

    def __init__(self, config: str, n_layer: int, attn_alg: str, vocab: int = 32000, r: int = 8, alpha: int = 16,
                 lora_dropout: float = 0.05, block: str = "attention", method: str = "lora"):
        """r, alpha, lora_dropout: the reference's fine-tune defaults (finetune/lora.py:40-42)"""
        super().__init__()
        from .attention_block import CONFIG_SHAPES, CausalSelfAttention
        if block not in ("attention", "full", "neox"):
            raise ValueError(f"block should be 'attention', 'full' or 'neox', got {block!r}")
        if method not in ("lora", "adapter_v2"):
            raise ValueError(f"method should be 'lora' or 'adapter_v2', got {method!r}")
        self.method = method
        if method == "adapter_v2":
            r, lora_dropout = 0, 0.0
        shape = CONFIG_SHAPES[config]
        self.n_embd = shape["n_embd"]
        self.block = block
        if block == "full":
            from .block import Block
            self.blocks = nn.ModuleList(Block.from_config(config, attn_alg=attn_alg, r=r, alpha=alpha, dropout=lora_dropout)
                                        for _ in range(n_layer))
        elif block == "neox":
            from .neox_block import NeoXBlock
            self.blocks = nn.ModuleList(NeoXBlock.from_config(config, attn_alg=attn_alg, r=r, alpha=alpha, dropout=lora_dropout)
                                        for _ in range(n_layer))
        else:
            self.blocks = nn.ModuleList(CausalSelfAttention(attn_alg=attn_alg, r=r, alpha=alpha, dropout=lora_dropout, **shape) for _ in range(n_layer))
        if method == "adapter_v2":
            self._adapt()
        else:
            for b in self.blocks:
                attn = b if block == "attention" else b.attn
                nn.init.normal_(attn.attn.lora_B, std=0.02)       # a non-zero branch, so every LoRA gradient is exercised
        g = torch.Generator().manual_seed(1234)
        self.lm_head = nn.Parameter(torch.randn(vocab, self.n_embd, generator=g) * 0.02, requires_grad=False)
        self.rope_n_elem = (self.blocks[0] if block == "attention" else self.blocks[0].attn).rope_n_elem

    def _adapt(self):
        """the adapter-v2 form of the blocks: every linear adapted, only adapter parameters and norms trainable, and a seeded
        start away from scale 1 and bias 0, so every adapter gradient is exercised"""
        from .adapter_v2 import AdapterV2Linear, adapt, mark_only_adapter_v2_as_trainable
        adapt(self.blocks)
        mark_only_adapter_v2_as_trainable(self.blocks)
        g = torch.Generator().manual_seed(4321)
        for m in self.blocks.modules():
            if isinstance(m, AdapterV2Linear):
                # float32 master parameters, as the LoRA matrices of the default method are: a step of 1e-4 on a scale near 1 is
                # below half a bfloat16 unit and would be lost in a 16-bit parameter
                m.cast_params = True
                m.adapter_scale.data, m.adapter_bias.data = m.adapter_scale.data.float(), m.adapter_bias.data.float()
                with torch.no_grad():
                    m.adapter_scale.add_(torch.randn(m.adapter_scale.shape, generator=g) * 0.02)
                    m.adapter_bias.add_(torch.randn(m.adapter_bias.shape, generator=g) * 0.02)

    def prepare(self, device, quantize: bool = True):
        if quantize:
            for b in self.blocks:
                b.quantize_base()
        self.to(device)
        self.lm_head.data = self.lm_head.data.to(torch.bfloat16)
        if self.block != "attention":
            for b in self.blocks:                                 # the norms run in the activations' dtype ("bf16-true")
                b.norm_1.to(torch.bfloat16)
                if b.norm_2 is not None:
                    b.norm_2.to(torch.bfloat16)
        return self

    def forward(self, x, cos, sin):
        if self.block != "attention":
            return type(self.blocks[0]).run_sequence(self.blocks, x, cos, sin)
        for b in self.blocks:
            x = x + b(x, cos, sin)
        return x

    def loss(self, x, targets, cos, sin):
        from .loss import lm_head_cross_entropy
        return lm_head_cross_entropy(self.forward(x, cos, sin), self.lm_head, targets).float()


class ToyLoRA(nn.Module):
    """CPU stand-in with `lora_` parameters for the rehearsal of the multi-rank control flow (gloo): the attention operator
    has no CPU path, the step structure around it does not care."""

    def __init__(self, width: int = 32):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.base = nn.Parameter(torch.randn(width, width, generator=g) * 0.1)
        self.lora_A = nn.Parameter(torch.randn(4, width, generator=g) * 0.1)
        self.lora_B = nn.Parameter(torch.randn(width, 4, generator=g) * 0.1)

    def loss(self, x, targets, cos=None, sin=None):
        y = x @ self.base.T + (x @ self.lora_A.T) @ self.lora_B.T
        return ((y - targets) ** 2).mean()


def run(config: str, n_layer: int, attn_alg: str, seq: int, micro_batch: int, accum: int, steps: int, warmup: int, device,
        rank: int = 0, world: int = 1, toy: bool = False, precondition_ms: float = 0.0, graph: bool = False,
        lora_dropout: float = 0.05, block: str = "attention", optimizer: str = "torch", method: str = "lora") -> dict:
    """`warmup` untimed + `steps` timed optimizer steps; -> timings (seconds / milliseconds, this rank).
    ``optimizer``: "torch" (torch.optim.AdamW after the bucket's all-reduce-mean) or "flat" (optim.FlatAdamW: the boundary as one
    pass over the flat bucket).  ``method``: "lora", or "adapter_v2" (``AttentionStack``)."""
    if optimizer not in ("torch", "flat"):
        raise ValueError(f"optimizer should be 'torch' or 'flat', got {optimizer!r}")
    on_gpu = device.type == "cuda"
    multi = dist.is_available() and dist.is_initialized() and world > 1
    gen = torch.Generator(device=device).manual_seed(100 + rank)
    if toy:
        model = ToyLoRA().to(device)
        x = torch.randn(accum, micro_batch, seq, 32, device=device, generator=gen)
        tgt = torch.randn(accum, micro_batch, seq, 32, device=device, generator=gen)
        cos = sin = None
    else:
        from .attention_block import build_rope_cache
        model = AttentionStack(config, n_layer, attn_alg, lora_dropout=lora_dropout, block=block, method=method).prepare(device)
        model.train()
        x = torch.randn(accum, micro_batch, seq, model.n_embd, device=device, generator=gen).to(torch.bfloat16)
        tgt = torch.randint(0, model.lm_head.shape[0], (accum, micro_batch, seq), device=device, generator=gen)
        cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(seq, model.rope_n_elem, device=device))
    params = dp.trainable_lora_parameters(model) if method == "lora" else [p for p in model.parameters() if p.requires_grad]
    if optimizer == "flat":
        from .optim import FlatAdamW
        opt = FlatAdamW(dp.FlatGradBucket(params), lr=1e-4)
    else:
        opt = torch.optim.AdamW(params, lr=1e-4)
    train = dp.TrainArgs(global_batch_size=micro_batch * accum * world, micro_batch_size=micro_batch)
    st = dp.DataParallelStepper(model, opt, train, lambda m, b: m.loss(b[0], b[1], cos, sin), time_comm=True)
    assert st.accum == accum
    if graph and on_gpu and not toy:
        st.capture((x[0], tgt[0]))

    def sync():
        if on_gpu:
            torch.cuda.synchronize(device)

    def one_step():
        loss = None
        for m in range(accum):
            loss = st.micro_step((x[m], tgt[m]))
        return loss

    def protocol():
        for _ in range(warmup):
            one_step()
        sync()
        if multi:
            dist.barrier()
        sync()
        st.comm_ms.clear()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = one_step()
        sync()
        if multi:
            dist.barrier()
        sync()
        el = time.perf_counter() - t0
        if multi:
            t = torch.tensor([el], dtype=torch.float64, device=device if dist.get_backend() != "gloo" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, float(loss)

    if precondition_ms > 0:
        t_end = time.perf_counter() + precondition_ms * 1e-3
        while time.perf_counter() < t_end:
            one_step()
            sync()
    elapsed, last_loss = protocol()
    comm = st.comm_times_ms()
    return {"elapsed_s": elapsed, "step_ms": elapsed * 1e3 / steps, "allreduce_ms": (sum(comm) / len(comm)) if comm else 0.0,
            "bucket_bytes": st.bucket.nbytes, "trainable_params": sum(p.numel() for p in params), "last_loss": last_loss,
            "tokens_per_step": micro_batch * accum * seq * world, "optimizer_steps": st.step_count}
