#!/usr/bin/env python3
"""Time the next-token head on an MI355X: norm + last-row logits + sample in HIP beside the tensor-op route.

    python tools/bench_next_token.py [--iters 50] [--rounds 5] [--out profiles/r12_next_token.md]

Sizes (n_embd, vocab): TinyLlama (2048, 32000), Llama-2-7B (4096, 32000), pythia-14m (128, 50304), each at B = 1 and 8, bf16,
top_k 200, temperature 0.8, on the hidden state of ONE new token, (B, 1, C).
    fused route:      NextTokenHead.forward   (RMSNorm kernel on the B rows, last_logits, sample: three launches, no host read)
    tensor-op route:  NextTokenHead.fused = False   (eager norm, the lm-head as nn.Linear, topk + scatter_ + softmax + multinomial)
The two routes alternate round by round in one process; per route the median and the spread of the rounds are printed.  Every
call takes the next of several heads whose weights together exceed 512 MiB, so that no call finds its weight in the 256 MiB
last-level cache.  Then each kernel alone the same way, with the logits pass's bytes V * C * e over its time beside the 8 TB/s
peak.  Times are device events around `--iters` calls after a warm-up; no time here is a pass criterion."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"tiny-llama-1.1b": (2048, 32000), "Llama-2-7b-hf": (4096, 32000), "pythia-14m": (128, 50304)}
PEAK_TBS = 8.0
TOP_K, TEMPERATURE = 200, 0.8


def timed(fn, iters):
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters          # microseconds


def case(config, B, args):
    from fastmax_experiments_amd.block import rms_norm_forward
    from fastmax_experiments_amd.generate import NextTokenHead, Sampler, last_logits
    C, V = SIZES[config]
    dev = torch.device("cuda")
    es = 2
    copies = min(64, (512 << 20) // (V * C * es) + 2)
    torch.manual_seed(0)
    heads = [NextTokenHead(C, V).to(dev, torch.bfloat16).eval() for _ in range(copies)]
    x = torch.randn(B, 1, C, device=dev).to(torch.bfloat16)
    sampler = Sampler(77)
    logits = heads[0].logits(x)
    normed = rms_norm_forward(x[:, -1], None, heads[0].ln_f.weight.detach(), 1e-5, False)[1]

    def route(fused):
        def fn(i):
            h = heads[i % copies]
            h.fused = fused
            with torch.no_grad():
                h(x, sampler, TEMPERATURE, TOP_K)
        return fn

    parts = {
        "norm": lambda i: rms_norm_forward(x[:, -1], None, heads[i % copies].ln_f.weight.detach(), 1e-5, False),
        "logits": lambda i: last_logits(normed, heads[i % copies].lm_head.weight.detach()),
        "sample": lambda i: sampler.sample(logits, TEMPERATURE, TOP_K),
    }
    times = {k: [] for k in ("fused", "tensor-op", *parts)}
    for _ in range(args.rounds):
        times["fused"].append(timed(route(True), args.iters))
        times["tensor-op"].append(timed(route(False), args.iters))
        for k, fn in parts.items():
            times[k].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    tbs = V * C * es / (med["logits"] * 1e-6) / 1e12
    lines = [f"| {config} | {B} | {med['fused']:.1f} ({min(times['fused']):.1f} .. {max(times['fused']):.1f}) | "
             f"{med['tensor-op']:.1f} ({min(times['tensor-op']):.1f} .. {max(times['tensor-op']):.1f}) | "
             f"{med['tensor-op'] / med['fused']:.2f}x | {med['norm']:.1f} | {med['logits']:.1f} | {med['sample']:.1f} | "
             f"{V * C * es / 1e6:.1f} | {tbs:.2f} | {100 * tbs / PEAK_TBS:.0f} % |"]
    del heads
    torch.cuda.empty_cache()
    return lines


HEADER = """| config | B | fused µs / token (rounds) | tensor-op µs / token (rounds) | tensor-op / fused | norm µs | logits µs | sample µs | weight MB | logits TB/s | of 8 TB/s |
|---|---|---|---|---|---|---|---|---|---|---|"""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_next_token.py measures on an MI355X; there is no device here")
    rows = []
    for config in SIZES:
        for B in (1, 8):
            rows += case(config, B, args)
            print(rows[-1], flush=True)
    table = "\n".join([HEADER] + rows)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"bf16, top_k {TOP_K}, temperature {TEMPERATURE}, {args.iters} calls per round, {args.rounds} rounds, median "
                    f"(min .. max)\n\n{table}\n")


if __name__ == "__main__":
    main()
