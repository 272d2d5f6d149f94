#!/usr/bin/env python3
"""Wall time per generated token on an MI355X: the eager loop of generate() against GraphedDecoder (one graph replay per token).

    python tools/bench_generate.py [--prompt 128] [--new 128] [--reps 5] [--cases tiny-llama-1.1b,Llama-2-7b-hf,pythia-70m]
                                   [--llama-blocks 32] [--top-p 0.9] [--out profiles/r15_graphed_generate.md]

Shapes: tiny-llama-1.1b (22 blocks) and Llama-2-7b-hf (--llama-blocks of its 32) as BlockStack, pythia-70m as a 6-block NeoXStack;
bf16, NF4 base, LoRA on q and v; batch 1 and 8; both decode state caches.  The blocks of a stack are copies of one randomly
initialised block: the times do not depend on the values.

What is timed: a host clock around a whole generate() call that ends in a device synchronise, once for prompt + 1 tokens (the
prompt and the first draw, which both loops run the same eager way) and once for prompt + new; per token = the difference over
new - 1.  A round times both lengths of both arms, eager then graphed; `--reps` rounds in one process; the table gives each arm's
median and its spread (lowest .. highest).  The graph is recorded, and both arms are run once, before the first round.  Both
arms draw under the same seed and the tool stops if their tokens differ.  No time here is a pass criterion.

`--top-p P` adds a third arm, the graphed loop with nucleus sampling behind the top-k (a second GraphedDecoder and its own states),
timed in the same rounds; its tokens are checked against the eager loop's under the same top_p once, before the rounds."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOCAB = {"tiny-llama-1.1b": 32000, "Llama-2-7b-hf": 32000, "pythia-70m": 50304}
HEADER = ("| config | blocks | decode cache | batch | eager, per token: median (lowest .. highest) | graphed | eager / graphed | "
          "whole call, eager | graphed |\n|---|---|---|---|---|---|---|---|---|")
TOP_P_HEADER = ("| config | blocks | decode cache | batch | eager, per token: median (lowest .. highest) | graphed | eager / graphed | "
                "whole call, eager | graphed | graphed with top_p, per token | with / without top_p |\n|---|---|---|---|---|---|---|---|---|---|---|")


def make_stack(config, n, alg):
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.neox_block import NeoXBlock, NeoXStack
    neox = config.startswith("pythia")
    torch.manual_seed(0)
    blk = (NeoXBlock if neox else Block).from_config(config, attn_alg=alg).quantize_base()
    torch.nn.init.normal_(blk.attn.attn.lora_B, std=0.02)
    blocks = [copy.deepcopy(blk).to("cuda").eval() for _ in range(n)]
    for b in blocks:
        b.norm_1.to(torch.bfloat16)
        b.norm_2.to(torch.bfloat16)
    return (NeoXStack if neox else BlockStack)(blocks)


def make_states(config, alg, B, n):
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    s = CONFIG_SHAPES[config]
    H, G, hs = s["n_head"], s["n_query_groups"], s["head_size"]
    if alg == "fastmax":
        return [FastmaxDecodeState(B, H, hs, "cuda", p=2, n_query_groups=G) for _ in range(n)]
    return [LinearmaxDecodeState(B, H, hs, "cuda", n_query_groups=G) for _ in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out          # ms


def fmt(v, unit="ms"):
    return f"{statistics.median(v):.3f} {unit} ({min(v):.3f} .. {max(v):.3f})"


def case(config, stack, alg, B, args):
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES, build_rope_cache
    from fastmax_experiments_amd.generate import GraphedDecoder, NextTokenHead, Sampler, generate
    C, V = CONFIG_SHAPES[config]["n_embd"], VOCAB[config]
    T, total, n_blocks = args.prompt, args.prompt + args.new, len(stack.blocks)
    torch.manual_seed(1)
    head = NextTokenHead(C, V, norm_class="LayerNorm" if config.startswith("pythia") else "RMSNorm").to("cuda").to(torch.bfloat16).eval()
    wte = torch.randn(V, C, device="cuda").to(torch.bfloat16)
    cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(total, stack.blocks[0].attn.rope_n_elem, device="cuda"))
    prompt = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(2)).cuda()
    kw = dict(cos=cos, sin=sin, temperature=0.8, top_k=200)
    eager_states, states = make_states(config, alg, B, n_blocks), make_states(config, alg, B, n_blocks)
    decoder = GraphedDecoder(wte, stack, head, states, max_len=total, **kw)

    def eager(n):
        for s in eager_states:
            s.reset()
        return generate(wte, stack, head, eager_states, prompt, n, sampler=Sampler(7), **kw)

    def graphed(n):
        for s in states:
            s.reset()
        return decoder.generate(prompt, n, Sampler(7))

    arms = {"eager": eager, "graphed": graphed}
    if args.top_p is not None:
        p_states = make_states(config, alg, B, n_blocks)
        p_decoder = GraphedDecoder(wte, stack, head, p_states, max_len=total, top_p=args.top_p, **kw)

        def graphed_top_p(n):
            for s in p_states:
                s.reset()
            return p_decoder.generate(prompt, n, Sampler(7))

        arms["graphed top_p"] = graphed_top_p
    first = {k: fn(total) for k, fn in arms.items()}                      # warm-up of every shape; the capture
    if not torch.equal(first["eager"], first["graphed"]):
        raise SystemExit(f"{config} {alg} B={B}: the graphed tokens differ from the eager loop's")
    if args.top_p is not None:
        for s in eager_states:
            s.reset()
        if not torch.equal(first["graphed top_p"], generate(wte, stack, head, eager_states, prompt, total, sampler=Sampler(7),
                                                            top_p=args.top_p, **kw)):
            raise SystemExit(f"{config} {alg} B={B}: the graphed tokens with top_p differ from the eager loop's")
    per_token = {k: [] for k in arms}
    whole = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            short, _ = wall(lambda: fn(T + 1))
            long, out = wall(lambda: fn(total))
            if not torch.equal(out, first[k]):
                raise SystemExit(f"{config} {alg} B={B}: {k} does not reproduce its own tokens")
            per_token[k].append((long - short) / (args.new - 1))
            whole[k].append(long)
    assert decoder.captures == 1
    ratio = statistics.median(per_token["eager"]) / statistics.median(per_token["graphed"])
    line = (f"| {config} | {n_blocks} | {alg} | {B} | {fmt(per_token['eager'])} | {fmt(per_token['graphed'])} | {ratio:.2f}x | "
            f"{statistics.median(whole['eager']):.1f} ms | {statistics.median(whole['graphed']):.1f} ms |")
    if args.top_p is not None:
        with_p = statistics.median(per_token["graphed top_p"]) / statistics.median(per_token["graphed"])
        line += f" {fmt(per_token['graphed top_p'])} | {with_p:.3f}x |"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="tiny-llama-1.1b,Llama-2-7b-hf,pythia-70m")
    ap.add_argument("--llama-blocks", type=int, default=32)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--top-p", type=float, default=None, help="also time the graphed loop with this top_p behind the top-k")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate.py needs an MI355X")
    if args.new < 2:
        raise SystemExit("--new should be at least 2: the first token is not a decode step")
    n_blocks = {"tiny-llama-1.1b": 22, "Llama-2-7b-hf": args.llama_blocks, "pythia-70m": 6}
    lines = [f"{args.new} tokens after a {args.prompt}-token prompt, bf16, NF4 base; {args.reps} rounds, the arms alternating.\n",
             HEADER if args.top_p is None else TOP_P_HEADER]
    print("\n".join(lines), flush=True)
    for config in args.cases.split(","):
        for alg in ("fastmax", "linearmax"):
            stack = make_stack(config, n_blocks[config], alg)
            for B in (int(b) for b in args.batches.split(",")):
                lines.append(case(config, stack, alg, B, args))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
            del stack
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
