#!/usr/bin/env python3
"""Time the NeoX (pythia) decoder block (neox_block.py) and its kernels on an MI355X.

    python tools/bench_neox.py [--tokens 4096] [--iters 20] [--attn fastmax] [--reps 3]

1. per kernel of csrc/neox_block.hip: time per call, algorithmic bytes (every operand read or written once) and the achieved
   GB/s against the 8 TB/s of the part.  Each call goes through the Python wrapper (output allocation from the caching
   allocator, the ctypes call), so at tens of microseconds per kernel the figure is an upper bound of the kernel's time: for the
   kernel alone take a kernel trace in a run of its own.  The operands rotate through enough buffer sets to exceed the 256 MB
   Infinity Cache, so the bytes come from HBM, and the timed window is `--iters` passes over all the sets;
2. per block and per 6-block stack at the pythia-70m and pythia-1b shapes (bf16, NF4 base, LoRA on q, v): forward and
   forward + backward with `fused_neighbours` on against off;
3. per generated token through a 6-block pythia-70m stack on each decode state cache, on against off.
Both arms of every A/B run in the same process on the same device, alternating, `--reps` times each: the tables give the median
and the spread (lowest .. highest) of each arm.  Prints one table per part; no time here is a pass criterion."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0
CACHE_BYTES = 256 << 20          # Infinity Cache: the buffer sets of one kernel together exceed twice this


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


def kernels(M, C, inter, iters):
    from fastmax_experiments_amd import neox_block as N
    bf, e = torch.bfloat16, 2
    nsets = max(2, -(-2 * CACHE_BYTES // (6 * M * C * e)))
    w1, b1, w2, b2 = (torch.randn(C, device="cuda").to(bf) for _ in range(4))
    norm_sets = []
    for _ in range(nsets):
        x, m, h, g1, g2, gs = (torch.randn(M, C, device="cuda").to(bf) for _ in range(6))
        s, _, _, mean, rstd = N.layer_norm_forward(x, w1, b1, 1e-5, m, h, w2, b2)
        norm_sets.append((x, m, h, g1, g2, gs, s, mean, rstd))
    msets = max(2, -(-2 * CACHE_BYTES // (2 * M * inter * e)))
    mlp_sets = [tuple(torch.randn(M, inter, device="cuda").to(bf) for _ in range(2)) for _ in range(msets)]

    def over(sets, call):
        def run():
            for t in sets:
                call(*t)
        return run, len(sets)

    all4 = (True, True, True, True)
    rows = [
        ("layernorm fwd", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_forward(x, w1, b1, 1e-5)), 2 * M * C * e),
        ("layernorm pair fwd", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_forward(x, w1, b1, 1e-5, None, None, w2, b2)), 3 * M * C * e),
        ("m + h + x, pair fwd", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_forward(x, w1, b1, 1e-5, m, h, w2, b2)), 6 * M * C * e),
        ("layernorm bwd", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_backward(g1, s, w1, mu, rs)), 3 * M * C * e),
        ("pair bwd + ds_in", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_backward(g1, s, w1, mu, rs, g2, w2, gs)), 5 * M * C * e),
        ("pair bwd + ds_in + 4 parameter gradients", over(norm_sets, lambda x, m, h, g1, g2, gs, s, mu, rs: N.layer_norm_backward(g1, s, w1, mu, rs, g2, w2, gs, all4)), 5 * M * C * e),
        ("gelu fwd", over(mlp_sets, lambda a, ga: N.gelu_forward(a)), 2 * M * inter * e),
        ("gelu bwd", over(mlp_sets, lambda a, ga: N.gelu_backward(a, ga)), 3 * M * inter * e),
    ]
    for name, (fn, n), nbytes in rows:
        ms = timed(fn, iters) / n
        gbs = nbytes / ms / 1e6
        print(f"| {name} | ({M}, {inter if 'gelu' in name else C}) | {ms * 1e3:.1f} us | {nbytes / 1e6:.1f} MB | {gbs:.0f} GB/s | {100 * gbs / PEAK_GBS:.0f}% |",
              flush=True)


def ab(arms, reps):
    """arms: {label: callable -> ms}; the arms alternate, `reps` times each -> {label: (median, lowest, highest)}"""
    got = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            got[k].append(fn())
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def make_blocks(config, n, attn):
    from fastmax_experiments_amd.neox_block import NeoXBlock
    torch.manual_seed(0)
    blocks = []
    for _ in range(n):
        blk = NeoXBlock.from_config(config, attn_alg=attn).quantize_base().to("cuda")
        blk.norm_1.to(torch.bfloat16)
        blk.norm_2.to(torch.bfloat16)
        torch.nn.init.normal_(blk.attn.attn.lora_B, std=0.02)
        blocks.append(blk)
    return blocks


def set_fused(blocks, on):
    for b in blocks:
        b.fused_neighbours = on


def block_and_stack(config, T, attn, iters, reps):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.neox_block import NeoXStack
    for n, what in ((1, "block"), (6, "6-block stack")):
        stack = NeoXStack(make_blocks(config, n, attn))
        n_embd = stack.blocks[0].norm_1.weight.shape[0]
        x = torch.randn(1, T, n_embd, device="cuda").to(torch.bfloat16)
        cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(T, stack.blocks[0].attn.rope_n_elem, device="cuda"))
        gy = torch.randn_like(x)

        def fwd():
            with torch.no_grad():
                stack(x, cos, sin)

        def fwd_bwd():
            xx = x.detach().requires_grad_(True)
            stack(xx, cos, sin).backward(gy)

        for fn, name in ((fwd, "forward"), (fwd_bwd, "forward + backward")):
            def arm(on, fn=fn):
                set_fused(stack.blocks, on)
                return timed(fn, iters)
            r = ab({"on": lambda: arm(True), "off": lambda: arm(False)}, reps)
            print(f"| {config} | {what} | {T} | {attn} | {name} | {fmt(r['on'])} | {fmt(r['off'])} | {r['off'][0] / r['on'][0]:.2f}x |", flush=True)
        del stack


def per_token(config, alg, prompt, steps, reps):
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES, build_rope_cache
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    from fastmax_experiments_amd.neox_block import run_neox_blocks
    shape = CONFIG_SHAPES[config]
    blocks = [b.eval() for b in make_blocks(config, 6, alg)]
    H, G, hs, C = shape["n_head"], shape["n_query_groups"], shape["head_size"], shape["n_embd"]
    total = prompt + 3 + steps
    cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(total, blocks[0].attn.rope_n_elem, device="cuda"))
    pos = torch.arange(total, device="cuda")
    x = torch.randn(1, total, C, device="cuda").to(torch.bfloat16)

    def arm(on):
        set_fused(blocks, on)
        states = [FastmaxDecodeState(1, H, hs, "cuda", p=2, n_query_groups=G) if alg == "fastmax"
                  else LinearmaxDecodeState(1, H, hs, "cuda", n_query_groups=G) for _ in blocks]
        with torch.no_grad():
            run_neox_blocks(blocks, x[:, :prompt], cos[:prompt], sin[:prompt], pos[:prompt], states)
            t = [prompt]

            def step():
                i = t[0]
                run_neox_blocks(blocks, x[:, i:i + 1], cos[i:i + 1], sin[i:i + 1], pos[i:i + 1], states)
                t[0] += 1
            return timed(step, steps)          # 3 warm-up tokens, then `steps` timed ones

    r = ab({"on": lambda: arm(True), "off": lambda: arm(False)}, reps)
    print(f"| {config} | 6-block stack | {alg} | {prompt} | {fmt(r['on'])} | {fmt(r['off'])} | {r['off'][0] / r['on'][0]:.2f}x |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--attn", default="fastmax", choices=["fastmax", "linearmax"])
    ap.add_argument("--configs", default="pythia-70m,pythia-1b")
    ap.add_argument("--decode-steps", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neox.py needs an MI355X")
    print("| kernel (bf16) | shape | time | algorithmic bytes | achieved | of 8 TB/s |\n|---|---|---|---|---|---|")
    for C, inter in ((512, 2048), (2048, 8192)):
        kernels(args.tokens, C, inter, args.iters)
    print("\n| config | what | tokens | attention | pass | fused_neighbours on, median (lowest .. highest) | off | off / on |\n|---|---|---|---|---|---|---|---|")
    for config in args.configs.split(","):
        block_and_stack(config, args.tokens, args.attn, args.iters, args.reps)
    print("\n| config | what | decode cache | prompt | per token, fused_neighbours on, median (lowest .. highest) | off | off / on |\n|---|---|---|---|---|---|---|")
    for alg in ("fastmax", "linearmax"):
        per_token("pythia-70m", alg, 128, args.decode_steps, args.reps)


if __name__ == "__main__":
    main()
