#!/usr/bin/env python3
"""Time one decoder block (block.py) and its new kernels on an MI355X.

    python tools/bench_block.py [--tokens 4096] [--iters 20] [--attn fastmax]

1. per kernel of csrc/block_neighbours.hip: time per call, algorithmic bytes (every operand read or written once) and the
   achieved GB/s against the 8 TB/s of the part.  Each call goes through the Python wrapper (output allocation from the caching
   allocator, the ctypes call), so at tens of microseconds per kernel the figure is an upper bound of the kernel's time: for the
   kernel alone take a kernel trace in a run of its own.  The operands rotate through enough buffer sets to exceed the 256 MB
   Infinity Cache, so the bytes come from HBM, and the timed window is `--iters` passes over all the sets;
2. per block at the TinyLlama and Llama-2-7B shapes (bf16, NF4 base, LoRA on q, v): forward and forward + backward with
   `fused_neighbours` on against off, in the same process on the same device.
Prints one table per part; no time here is a pass criterion."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters          # ms


CACHE_BYTES = 256 << 20          # Infinity Cache: the buffer sets of one kernel together exceed twice this


def kernels(M, C, inter, iters):
    from fastmax_experiments_amd import block as B
    bf = torch.bfloat16
    e = 2
    nsets = max(2, -(-2 * CACHE_BYTES // (4 * M * C * e)))
    norm_sets = []
    w = torch.ones(C, device="cuda", dtype=bf)
    for _ in range(nsets):
        x, r, gy, gs = (torch.randn(M, C, device="cuda").to(bf) for _ in range(4))
        s, _, rstd = B.rms_norm_forward(x, r, w, 1e-5, False)
        norm_sets.append((x, r, gy, gs, s, rstd))
    msets = max(2, -(-2 * CACHE_BYTES // (3 * M * inter * e)))
    mlp_sets = [tuple(torch.randn(M, inter, device="cuda").to(bf) for _ in range(3)) for _ in range(msets)]

    def over(sets, call):
        def run():
            for t in sets:
                call(*t)
        return run, len(sets)

    rows = [
        ("rmsnorm fwd", over(norm_sets, lambda x, r, gy, gs, s, rstd: B.rms_norm_forward(x, None, w, 1e-5, False)), 2 * M * C * e),
        ("add + rmsnorm fwd", over(norm_sets, lambda x, r, gy, gs, s, rstd: B.rms_norm_forward(x, r, w, 1e-5, False)), 4 * M * C * e),
        ("rmsnorm bwd", over(norm_sets, lambda x, r, gy, gs, s, rstd: B.rms_norm_backward(gy, s, w, rstd, None, False, False)), 3 * M * C * e),
        ("rmsnorm bwd + ds_in", over(norm_sets, lambda x, r, gy, gs, s, rstd: B.rms_norm_backward(gy, s, w, rstd, gs, False, False)), 4 * M * C * e),
        ("rmsnorm bwd + dweight", over(norm_sets, lambda x, r, gy, gs, s, rstd: B.rms_norm_backward(gy, s, w, rstd, None, False, True)), 3 * M * C * e),
        ("silu(a) * b fwd", over(mlp_sets, lambda a, b, ga: B.gated_act_forward(a, b, "silu")), 3 * M * inter * e),
        ("silu(a) * b bwd", over(mlp_sets, lambda a, b, ga: B.gated_act_backward(a, b, ga, "silu")), 5 * M * inter * e),
        ("gelu(a) * b fwd", over(mlp_sets, lambda a, b, ga: B.gated_act_forward(a, b, "gelu")), 3 * M * inter * e),
    ]
    for name, (fn, n), nbytes in rows:
        ms = timed(fn, iters) / n
        gbs = nbytes / ms / 1e6
        print(f"| {name} | ({M}, {C if 'rmsnorm' in name else inter}) | {ms * 1e3:.1f} us | {nbytes / 1e6:.1f} MB | {gbs:.0f} GB/s | {100 * gbs / PEAK_GBS:.0f}% |")


def one_block(config, T, attn, iters):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block
    torch.manual_seed(0)
    blk = Block.from_config(config, attn_alg=attn).quantize_base().to("cuda")
    blk.norm_1.to(torch.bfloat16)
    blk.norm_2.to(torch.bfloat16)
    torch.nn.init.normal_(blk.attn.attn.lora_B, std=0.02)
    n_embd = blk.norm_1.weight.shape[0]
    x = torch.randn(1, T, n_embd, device="cuda").to(torch.bfloat16)
    cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(T, blk.attn.rope_n_elem, device="cuda"))
    gy = torch.randn_like(x)

    def fwd():
        with torch.no_grad():
            blk(x, cos, sin)

    def fwd_bwd():
        xx = x.detach().requires_grad_(True)
        blk(xx, cos, sin).backward(gy)

    res = {}
    for fused in (True, False):
        blk.fused_neighbours = fused
        res[fused] = (timed(fwd, iters), timed(fwd_bwd, iters))
    for i, what in enumerate(("forward", "forward + backward")):
        on, off = res[True][i], res[False][i]
        print(f"| {config} | {T} | {attn} | {what} | {on:.3f} ms | {off:.3f} ms | {off / on:.2f}x |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--attn", default="fastmax", choices=["fastmax", "linearmax"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block.py needs an MI355X")
    print("| kernel (bf16) | shape | time | algorithmic bytes | achieved | of 8 TB/s |\n|---|---|---|---|---|---|")
    for C, inter in ((2048, 5632), (4096, 11008)):
        kernels(args.tokens, C, inter, args.iters)
    print("\n| config | tokens | attention | pass | fused_neighbours on | off | off / on |\n|---|---|---|---|---|---|---|")
    for config in ("tiny-llama-1.1b", "Llama-2-7b-hf"):
        one_block(config, args.tokens, args.attn, args.iters)


if __name__ == "__main__":
    main()
