#!/usr/bin/env python3
"""Wall time per generated token on an MI355X: the eager loop of generate() against GraphedDecoder (one graph replay per token).

    python tools/bench_generate.py [--prompt 128] [--new 128] [--reps 5] [--cases tiny-llama-1.1b,Llama-2-7b-hf,pythia-70m]
                                   [--llama-blocks 32] [--top-p 0.9] [--out profiles/r15_graphed_generate.md]
    python tools/bench_generate.py --cases Mixtral-8x7B-v0.1 [--mixtral-blocks 4] [--algs fastmax]
    python tools/bench_generate.py --nf4-head nf4 --cases tiny-llama-1.1b,Llama-2-7b-hf [--algs fastmax]
    python tools/bench_generate.py --cases tiny-llama-1.1b,Llama-2-7b-hf,Gemma-2b --algs fastmax,fastmax-kv --blocks 4

Shapes: tiny-llama-1.1b (22 blocks) and Llama-2-7b-hf (--llama-blocks of its 32) as BlockStack, pythia-70m as a 6-block NeoXStack;
bf16, NF4 base, LoRA on q and v; batch 1 and 8; both decode state caches.  The blocks of a stack are copies of one randomly
initialised block: the times do not depend on the values.  Mixtral-8x7B-v0.1 (--mixtral-blocks of its 32) is a BlockStack
whose MLPs are ``moe.LLaMAMoE``: its eager arm runs with ``device_routed`` off (the route that reads the experts' row counts back
per layer), its graphed arm needs it on, and a third arm is the eager loop with it on.

What is timed: a host clock around a whole generate() call that ends in a device synchronise, once for prompt + 1 tokens (the
prompt and the first draw, which both loops run the same eager way) and once for prompt + new; per token = the difference over
new - 1.  A round times both lengths of both arms, eager then graphed; `--reps` rounds in one process; the table gives each arm's
median and its spread (lowest .. highest).  The graph is recorded, and both arms are run once, before the first round.  Both
arms draw under the same seed and the tool stops if their tokens differ.  No time here is a pass criterion.

`--top-p P` adds a third arm, the graphed loop with nucleus sampling behind the top-k (a second GraphedDecoder and its own states),
timed in the same rounds; its tokens are checked against the eager loop's under the same top_p once, before the rounds.

`--nf4-head nf4|nf4-dq` adds two arms, the eager and the graphed loop under a copy of the head after ``quantize_base()`` (with
their own states and GraphedDecoder), timed in the same rounds as the dense head's two.  The quantised head scores other weights,
so its tokens are checked against each other (graphed against eager), not against the dense head's.

`--algs fastmax-kv` runs the fastmax blocks on ``FastmaxKVDecodeState`` caches of prompt + new tokens (the decode cache column says
so); Gemma-2b (8 query heads on 1 KV head of 256) has no other cache.  `--blocks N` cuts every stack to N blocks."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXTRAL = "Mixtral-8x7B-v0.1"
VOCAB = {"tiny-llama-1.1b": 32000, "Llama-2-7b-hf": 32000, "pythia-70m": 50304, MIXTRAL: 32000, "Gemma-2b": 256000}
HEADER = ("| config | blocks | decode cache | batch | eager, per token: median (lowest .. highest) | graphed | eager / graphed | "
          "whole call, eager | graphed |\n|---|---|---|---|---|---|---|---|---|")
TOP_P_HEADER = ("| config | blocks | decode cache | batch | eager, per token: median (lowest .. highest) | graphed | eager / graphed | "
                "whole call, eager | graphed | graphed with top_p, per token | with / without top_p |\n|---|---|---|---|---|---|---|---|---|---|---|")


NF4_HEAD_HEADER = ("| config | blocks | decode cache | batch | eager, per token: median (lowest .. highest) | graphed | eager / graphed | "
                   "whole call, eager | graphed | eager, NF4 head, per token | graphed, NF4 head | dense / NF4 head, eager | graphed |\n"
                   "|---|---|---|---|---|---|---|---|---|---|---|---|---|")


MOE_HEADER = ("| config | blocks | decode cache | batch | eager (device_routed off), per token: median (lowest .. highest) | graphed | "
              "eager / graphed | whole call, eager | graphed | eager with device_routed on, per token | eager off / on |\n"
              "|---|---|---|---|---|---|---|---|---|---|---|")


def make_mixtral_stack(n, alg):
    """a block at the Mixtral width made on the device, expert by expert, quantized as it is made (the dense weights of all
    experts never coexist); n copies"""
    from fastmax_experiments_amd.block import CONFIG_MOE, Block, BlockStack, LLaMAMLP
    torch.manual_seed(0)
    E, k = CONFIG_MOE[MIXTRAL]["n_expert"], CONFIG_MOE[MIXTRAL]["n_expert_per_token"]
    with torch.device("cuda"):
        blk = Block.from_config(MIXTRAL, attn_alg=alg, n_expert=1, n_expert_per_token=1).to(torch.bfloat16).quantize_base()
        torch.nn.init.normal_(blk.attn.attn.lora_B, std=0.02)
        mlp = blk.mlp
        experts = list(mlp.experts)
        for _ in range(E - 1):
            experts.append(LLaMAMLP(mlp.n_embd, mlp.intermediate_size).to(torch.bfloat16).quantize_base())
        mlp.gate = type(mlp.gate)(mlp.n_embd, E, bias=False).to(torch.bfloat16)
    mlp.experts, mlp.n_expert, mlp.n_expert_per_token = torch.nn.ModuleList(experts), E, k
    return BlockStack([copy.deepcopy(blk).eval() for _ in range(n)])


def make_stack(config, n, alg):
    alg = "fastmax" if alg == "fastmax-kv" else alg          # the same blocks; the cache differs
    if config == MIXTRAL:
        return make_mixtral_stack(n, alg)
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


def make_states(config, alg, B, n, max_len=None):
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES
    from fastmax_experiments_amd.decode import FastmaxDecodeState, FastmaxKVDecodeState, LinearmaxDecodeState
    s = CONFIG_SHAPES[config]
    H, G, hs = s["n_head"], s["n_query_groups"], s["head_size"]
    if alg == "fastmax-kv":
        return [FastmaxKVDecodeState(B, H, hs, "cuda", max_len, torch.bfloat16, n_query_groups=G) for _ in range(n)]
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
    from fastmax_experiments_amd.moe import LLaMAMoE
    C, V = CONFIG_SHAPES[config]["n_embd"], VOCAB[config]
    moes = [b.mlp for b in stack.blocks if isinstance(getattr(b, "mlp", None), LLaMAMoE)]

    def routed(on):
        for m in moes:
            m.device_routed = on
    T, total, n_blocks = args.prompt, args.prompt + args.new, len(stack.blocks)
    torch.manual_seed(1)
    head = NextTokenHead(C, V, norm_class="LayerNorm" if config.startswith("pythia") else "RMSNorm").to("cuda").to(torch.bfloat16).eval()
    wte = torch.randn(V, C, device="cuda").to(torch.bfloat16)
    cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(total, stack.blocks[0].attn.rope_n_elem, device="cuda"))
    prompt = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(2)).cuda()
    kw = dict(cos=cos, sin=sin, temperature=0.8, top_k=200)
    eager_states, states = make_states(config, alg, B, n_blocks, total), make_states(config, alg, B, n_blocks, total)
    routed(True)
    decoder = GraphedDecoder(wte, stack, head, states, max_len=total, **kw)

    def eager(n, on=False):
        routed(on)
        for s in eager_states:
            s.reset()
        return generate(wte, stack, head, eager_states, prompt, n, sampler=Sampler(7), **kw)

    def graphed(n):
        routed(True)
        for s in states:
            s.reset()
        return decoder.generate(prompt, n, Sampler(7))

    arms = {"eager": eager, "graphed": graphed}
    if moes:
        arms["eager routed"] = lambda n: eager(n, True)
    if args.top_p is not None:
        p_states = make_states(config, alg, B, n_blocks, total)
        p_decoder = GraphedDecoder(wte, stack, head, p_states, max_len=total, top_p=args.top_p, **kw)

        def graphed_top_p(n):
            for s in p_states:
                s.reset()
            return p_decoder.generate(prompt, n, Sampler(7))

        arms["graphed top_p"] = graphed_top_p
    if args.nf4_head is not None:
        q_head = copy.deepcopy(head).quantize_base(double_quant=args.nf4_head == "nf4-dq")
        q_eager_states, q_states = make_states(config, alg, B, n_blocks, total), make_states(config, alg, B, n_blocks, total)
        q_decoder = GraphedDecoder(wte, stack, q_head, q_states, max_len=total, **kw)

        def eager_nf4_head(n):
            for s in q_eager_states:
                s.reset()
            return generate(wte, stack, q_head, q_eager_states, prompt, n, sampler=Sampler(7), **kw)

        def graphed_nf4_head(n):
            for s in q_states:
                s.reset()
            return q_decoder.generate(prompt, n, Sampler(7))

        arms["eager nf4 head"], arms["graphed nf4 head"] = eager_nf4_head, graphed_nf4_head
    first = {k: fn(total) for k, fn in arms.items()}                      # warm-up of every shape; the capture
    if args.nf4_head is not None and not torch.equal(first["eager nf4 head"], first["graphed nf4 head"]):
        raise SystemExit(f"{config} {alg} B={B}: under the NF4 head the graphed tokens differ from the eager loop's")
    if not torch.equal(first["eager"], first["graphed"]):
        raise SystemExit(f"{config} {alg} B={B}: the graphed tokens differ from the eager loop's")
    if moes and not torch.equal(first["eager"], first["eager routed"]):
        raise SystemExit(f"{config} {alg} B={B}: the eager tokens with device_routed on differ from those with it off")
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
    if args.nf4_head is not None:
        line += (f" {fmt(per_token['eager nf4 head'])} | {fmt(per_token['graphed nf4 head'])} | "
                 f"{statistics.median(per_token['eager']) / statistics.median(per_token['eager nf4 head']):.3f}x | "
                 f"{statistics.median(per_token['graphed']) / statistics.median(per_token['graphed nf4 head']):.3f}x |")
    if moes:
        off_on = statistics.median(per_token["eager"]) / statistics.median(per_token["eager routed"])
        line += f" {fmt(per_token['eager routed'])} | {off_on:.2f}x |"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="tiny-llama-1.1b,Llama-2-7b-hf,pythia-70m")
    ap.add_argument("--llama-blocks", type=int, default=32)
    ap.add_argument("--mixtral-blocks", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=None, help="at most this many blocks in every stack")
    ap.add_argument("--algs", default="fastmax,linearmax")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--top-p", type=float, default=None, help="also time the graphed loop with this top_p behind the top-k")
    ap.add_argument("--nf4-head", choices=("nf4", "nf4-dq"), default=None,
                    help="also time both loops under the head after quantize_base() (nf4-dq: double-quantised scales)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate.py needs an MI355X")
    if args.nf4_head is not None and (args.top_p is not None or MIXTRAL in args.cases.split(",")):
        raise SystemExit("--nf4-head, --top-p and the Mixtral case are timed in separate runs: each adds its own arms and columns")
    if args.new < 2:
        raise SystemExit("--new should be at least 2: the first token is not a decode step")
    if args.top_p is not None and MIXTRAL in args.cases.split(","):
        raise SystemExit("--top-p and the Mixtral case are timed in separate runs: each adds its own arm and columns")
    n_blocks = {"tiny-llama-1.1b": 22, "Llama-2-7b-hf": args.llama_blocks, "pythia-70m": 6, MIXTRAL: args.mixtral_blocks, "Gemma-2b": 18}
    if args.blocks is not None:
        n_blocks = {k: min(v, args.blocks) for k, v in n_blocks.items()}
    lines = [f"{args.new} tokens after a {args.prompt}-token prompt, bf16, NF4 base; {args.reps} rounds, the arms alternating.\n",
             NF4_HEAD_HEADER if args.nf4_head is not None else HEADER if args.top_p is None else TOP_P_HEADER]
    print("\n".join(lines), flush=True)
    for config in args.cases.split(","):
        if config == MIXTRAL:
            lines += ["", MOE_HEADER]
            print("\n".join(lines[-2:]), flush=True)
        for alg in args.algs.split(","):
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
