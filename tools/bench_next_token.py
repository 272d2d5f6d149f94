#!/usr/bin/env python3
"""Time the next-token head on an MI355X: norm + last-row logits + sample in HIP beside the tensor-op route.

    python tools/bench_next_token.py [--iters 50] [--rounds 5] [--tables head,sampler] [--top-p 0.9] [--out profiles/r12_next_token.md]
    python tools/bench_next_token.py --tables quantised [--out FILE]

Sizes (n_embd, vocab): TinyLlama (2048, 32000), Llama-2-7B (4096, 32000), pythia-14m (128, 50304), each at B = 1 and 8, bf16,
top_k 200, temperature 0.8, on the hidden state of ONE new token, (B, 1, C).
    fused route:      NextTokenHead.forward   (RMSNorm kernel on the B rows, last_logits, sample: three launches, no host read)
    tensor-op route:  NextTokenHead.fused = False   (eager norm, the lm-head as nn.Linear, topk + scatter_ + softmax + multinomial)
The two routes alternate round by round in one process; per route the median and the spread of the rounds are printed.  Every
call takes the next of several heads whose weights together exceed 512 MiB, so that no call finds its weight in the 256 MiB
last-level cache.  Then each kernel alone the same way, with the logits pass's bytes V * C * e over its time beside the 8 TB/s
peak.  Times are device events around `--iters` calls after a warm-up; no time here is a pass criterion.

The sampler table (top-p): the sampler alone on float32 logits (B, V) drawn once (normal, standard deviation 3), V = 32000 and
50304, B = 1 and 8, top_k None and 200, temperature 0.8.  Four arms alternate round by round: the top-k-only sampler kernel, the
same kernel with the nucleus filter (`--top-p`), and the tensor-op restatement (`_sample_tensor_ops`: topk + scatter_ + softmax
[+ sort + cumsum] + multinomial) without and with top-p.

The quantised table (`--tables quantised`): ``head.logits`` (the norm kernel and the last-row logits, two launches, float32 logits)
per call on the head shapes of pythia-70m (50304 x 512), tiny-llama-1.1b (32000 x 2048) and Llama-2-7b-hf (32000 x 4096), B = 1 and
8, bf16, with the head dense, ``quantize_base()`` (NF4, fp32 block scales) and ``quantize_base(double_quant=True)``.  The three arms
alternate round by round, each over copies of its head that together exceed 512 MiB.  Two times per arm: the eager call (device
events around `--iters` calls; at these sizes the host's two launches can be the longer part), and the same `--iters` calls
recorded once in a graph and replayed, which leaves the device's time.  Bytes per second are the weight stream's alone over the
replayed call's time: 2 V C for the dense head, codes + scales for the quantised ones (V C / 2 + 4 V C / 64, or
V C / 2 + V C / 64 + 4 ceil(V C / 64 / 256) + 1024 double-quantised)."""
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


def recorded(fn, iters):
    """`iters` calls of fn recorded in one graph on a side stream (after an eager warm-up there) -> what one replay takes, per call"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for i in range(iters):
            fn(i)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for i in range(iters):
            fn(i)
    torch.cuda.current_stream().wait_stream(stream)

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(4):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (4 * iters)          # microseconds
    return replay


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


QUANTISED_SIZES = {"pythia-70m": (512, 50304), "tiny-llama-1.1b": (2048, 32000), "Llama-2-7b-hf": (4096, 32000)}


def head_bytes(arm, C, V):
    """the bytes of lm_head one call streams"""
    blocks = V * C // 64
    return {"dense": 2 * V * C, "nf4": V * C // 2 + 4 * blocks, "nf4-dq": V * C // 2 + blocks + 4 * -(-blocks // 256) + 1024}[arm]


def quantised_case(config, B, args):
    import copy
    from fastmax_experiments_amd.generate import NextTokenHead
    C, V = QUANTISED_SIZES[config]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    norm = "LayerNorm" if config.startswith("pythia") else "RMSNorm"
    dense = NextTokenHead(C, V, norm_class=norm).to(dev, torch.bfloat16).eval()
    x = torch.randn(B, 1, C, device=dev).to(torch.bfloat16)
    heads, nbytes = {}, {}
    for arm, dq in (("dense", None), ("nf4", False), ("nf4-dq", True)):
        first = copy.deepcopy(dense) if dq is None else copy.deepcopy(dense).quantize_base(dq)
        nbytes[arm] = head_bytes(arm, C, V)
        copies = min(64, (512 << 20) // nbytes[arm] + 2)
        heads[arm] = [first] + [copy.deepcopy(first) for _ in range(copies - 1)]
    with torch.no_grad():
        ref = heads["nf4"][0].logits(x)
        for arm in ("nf4", "nf4-dq"):                 # every copy scores once eagerly (its scales struct), and they agree
            for h in heads[arm]:
                got = h.logits(x)
                if arm == "nf4" and not torch.equal(got, ref):
                    raise SystemExit(f"{config} B={B}: two copies of the NF4 head give different logits")

    def route(arm):
        hs = heads[arm]

        def fn(i):
            with torch.no_grad():
                hs[i % len(hs)].logits(x)
        return fn

    replays = {arm: recorded(route(arm), args.iters) for arm in heads}
    times, device = {arm: [] for arm in heads}, {arm: [] for arm in heads}
    for _ in range(args.rounds):
        for arm in heads:
            times[arm].append(timed(route(arm), args.iters))
        for arm in heads:
            device[arm].append(replays[arm]())
    med = {k: statistics.median(v) for k, v in times.items()}
    played = {k: statistics.median(v) for k, v in device.items()}
    cells = []
    for arm in heads:
        tbs = nbytes[arm] / (played[arm] * 1e-6) / 1e12
        cells.append(f"{med[arm]:.1f} ({min(times[arm]):.1f} .. {max(times[arm]):.1f}) | "
                     f"{played[arm]:.1f} ({min(device[arm]):.1f} .. {max(device[arm]):.1f}) | {nbytes[arm] / 1e6:.1f} | {tbs:.2f}")
    del heads, replays
    torch.cuda.empty_cache()
    return (f"| {config} | {V} x {C} | {B} | " + " | ".join(cells) +
            f" | {played['dense'] / played['nf4']:.2f}x | {played['dense'] / played['nf4-dq']:.2f}x |")


QUANTISED_HEADER = """| config | V x C | B | dense: eager µs / call (rounds) | replayed µs / call (rounds) | MB | TB/s | NF4: eager | replayed | MB | TB/s | NF4-dq: eager | replayed | MB | TB/s | replayed, dense / NF4 | dense / NF4-dq |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"""


def sampler_case(V, B, top_k, args):
    from fastmax_experiments_amd.generate import Sampler, _sample_tensor_ops
    logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(V + B)) * 3).cuda()
    sampler, p = Sampler(77), args.top_p
    arms = {
        "top-k": lambda i: sampler.sample(logits, TEMPERATURE, top_k),
        "top-k + top-p": lambda i: sampler.sample(logits, TEMPERATURE, top_k, top_p=p),
        "tensor-op": lambda i: _sample_tensor_ops(logits, TEMPERATURE, top_k),
        "tensor-op + top-p": lambda i: _sample_tensor_ops(logits, TEMPERATURE, top_k, p),
    }
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    kept = sampler.keep_mask(logits, top_k, top_p=p, temperature=TEMPERATURE).sum(1)
    cells = " | ".join(f"{med[k]:.1f} ({min(times[k]):.1f} .. {max(times[k]):.1f})" for k in arms)
    return (f"| {V} | {B} | {top_k} | {cells} | {med['top-k + top-p'] - med['top-k']:+.1f} | "
            f"{med['top-k + top-p'] / med['top-k']:.2f}x | {med['tensor-op + top-p'] / med['top-k + top-p']:.1f}x | "
            f"{int(kept.min())} .. {int(kept.max())} |")


SAMPLER_HEADER = """| V | B | top_k | top-k kernel µs / call (rounds) | top-k + top-p kernel | tensor-op top-k | tensor-op top-k + top-p | nucleus costs µs | kernel, with / without | tensor-op / kernel, with top-p | kept per row |
|---|---|---|---|---|---|---|---|---|---|---|"""

HEADER = """| config | B | fused µs / token (rounds) | tensor-op µs / token (rounds) | tensor-op / fused | norm µs | logits µs | sample µs | weight MB | logits TB/s | of 8 TB/s |
|---|---|---|---|---|---|---|---|---|---|---|"""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tables", default="head,sampler", help="which tables to measure: head, sampler, quantised")
    ap.add_argument("--top-p", type=float, default=0.9, help="the sampler table's top_p")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_next_token.py measures on an MI355X; there is no device here")
    tables = []
    if "head" in args.tables.split(","):
        rows = []
        for config in SIZES:
            for B in (1, 8):
                rows += case(config, B, args)
                print(rows[-1], flush=True)
        tables.append(f"bf16, top_k {TOP_K}, temperature {TEMPERATURE}, {args.iters} calls per round, {args.rounds} rounds, median "
                      "(min .. max)\n\n" + "\n".join([HEADER] + rows))
    if "sampler" in args.tables.split(","):
        rows = []
        for V in (32000, 50304):
            for B in (1, 8):
                for top_k in (None, TOP_K):
                    rows.append(sampler_case(V, B, top_k, args))
                    print(rows[-1], flush=True)
        tables.append(f"the sampler alone, float32 logits, temperature {TEMPERATURE}, top_p {args.top_p}, {args.iters} calls per round, "
                      f"{args.rounds} rounds, the four arms alternating, median (min .. max)\n\n" + "\n".join([SAMPLER_HEADER] + rows))
    if "quantised" in args.tables.split(","):
        rows = []
        for config in QUANTISED_SIZES:
            for B in (1, 8):
                rows.append(quantised_case(config, B, args))
                print(rows[-1], flush=True)
        tables.append(f"head.logits (norm + last-row logits), bf16 in, float32 logits, {args.iters} calls per round, {args.rounds} rounds, "
                      "the three arms alternating, median (min .. max); MB and TB/s: the weight stream alone over the replayed call's time\n\n" +
                      "\n".join([QUANTISED_HEADER] + rows))
    print("\n\n".join(tables))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n\n".join(tables) + "\n")


if __name__ == "__main__":
    main()
