#!/usr/bin/env python3
"""Time the adapter-v2 kernels (csrc/adapter_v2.hip) against the tensor-op form on an MI355X.

    python tools/bench_adapter_v2.py [--rows 16384] [--iters 20] [--rounds 5] [--no-step]

1. per width N, in bf16 with bf16 parameters: device time of the forward and of forward + backward of
   ``scale * (z + bias)`` alone (z given, not the linear in front of it), replayed from a HIP graph so that no host time is in
   the figure.  ``kernels`` is ``adapter_v2.adapter_v2`` (what ``AdapterV2Linear.fused = True`` runs), ``tensor ops`` the
   reference's expression with torch's autograd (``fused = False``).  The two alternate ``--rounds`` times in this process; the
   table holds the median and the spread (max - min over the rounds, relative to the median).  The operands rotate through
   enough buffer sets to exceed the 256 MB Infinity Cache.  Bytes are what each pass must move from the shapes: 2 M N es
   forward, 3 M N es plus the partial sums written and read backward; the share is of the 8 TB/s of the part.
2. one decode-size call (M = 1), eager: host time per call decides there, so it is a host clock around a synchronised loop.
3. the per-step time of ``finetune_step.run(method="adapter_v2")`` with the kernels on and off, alternating.
Prints one table per part; no time here is a pass criterion."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0
CACHE_BYTES = 256 << 20
WIDTHS = (("tiny-llama-1.1b qkv", 2560), ("tiny-llama-1.1b n_embd", 2048), ("tiny-llama-1.1b mlp", 5632),
          ("Llama-2-7b qkv", 12288), ("Llama-2-7b n_embd", 4096), ("Llama-2-7b mlp", 11008))


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def replay_ms(g, iters):
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def passes(M, N):
    """(forward, forward + backward) callables per variant over rotating buffer sets, and the number of sets"""
    from fastmax_experiments_amd import adapter_v2 as av2
    bf = torch.bfloat16
    nsets = max(2, -(-2 * CACHE_BYTES // (4 * M * N * 2)))
    scale = (1.0 + 0.1 * torch.randn(N, device="cuda")).to(bf).requires_grad_(True)
    bias = (0.1 * torch.randn(N, device="cuda")).to(bf).requires_grad_(True)
    sets = [(torch.randn(M, N, device="cuda").to(bf).requires_grad_(True), torch.randn(M, N, device="cuda").to(bf))
            for _ in range(nsets)]
    forms = {"kernels": av2.adapter_v2, "tensor ops": lambda z, s, b: s * (z + b)}
    out = {}
    for name, form in forms.items():
        def fwd(form=form):
            with torch.no_grad():
                for z, _ in sets:
                    form(z, scale, bias)

        def fwd_bwd(form=form):
            for z, gy in sets:
                torch.autograd.grad(form(z, scale, bias), (z, scale, bias), gy)

        out[name] = (fwd, fwd_bwd)
    return out, nsets


def widths(M, iters, rounds):
    from fastmax_experiments_amd import adapter_v2 as av2
    print("| width | (M, N) | pass | kernels | spread | tensor ops | spread | tensor ops / kernels | kernel bytes | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for label, N in WIDTHS:
        forms, nsets = passes(M, N)
        graphs = {name: [graph_of(f) for f in fs] for name, fs in forms.items()}
        times = {name: ([], []) for name in forms}
        for _ in range(rounds):
            for name in forms:
                for i in range(2):
                    times[name][i].append(replay_ms(graphs[name][i], iters) / nsets)
        part = av2.adapter_backward_workspace(M, N, torch.bfloat16, True)
        nbytes = (2 * M * N * 2, 2 * M * N * 2 + 3 * M * N * 2 + 2 * part + 2 * N * 4)       # forward; forward + backward
        for i, what in enumerate(("forward", "forward + backward")):
            med = {name: statistics.median(times[name][i]) for name in forms}
            spr = {name: (max(times[name][i]) - min(times[name][i])) / med[name] for name in forms}
            gbs = nbytes[i] / med["kernels"] / 1e6
            print(f"| {label} | ({M}, {N}) | {what} | {med['kernels'] * 1e3:.1f} us | {100 * spr['kernels']:.1f}% | "
                  f"{med['tensor ops'] * 1e3:.1f} us | {100 * spr['tensor ops']:.1f}% | {med['tensor ops'] / med['kernels']:.2f}x | "
                  f"{nbytes[i] / 1e6:.1f} MB | {100 * gbs / PEAK_GBS:.0f}% |")
        del graphs, forms


def decode(rounds, calls=2000):
    from fastmax_experiments_amd import adapter_v2 as av2
    print("\n| decode-size call (M = 1, eager, host clock) | N | kernels | spread | tensor ops | spread |\n|---|---|---|---|---|---|")
    for N in (2048, 11008):
        z = torch.randn(1, N, device="cuda").to(torch.bfloat16)
        scale, bias = torch.ones(N, device="cuda", dtype=torch.bfloat16), torch.zeros(N, device="cuda", dtype=torch.bfloat16)
        forms = {"kernels": lambda: av2.adapter_v2(z, scale, bias), "tensor ops": lambda: scale * (z + bias)}
        times = {name: [] for name in forms}
        with torch.no_grad():
            for _ in range(rounds):
                for name, fn in forms.items():
                    for _ in range(20):
                        fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / calls * 1e6)
        med = {name: statistics.median(t) for name, t in times.items()}
        spr = {name: (max(t) - min(t)) / med[name] for name, t in times.items()}
        print(f"| forward | {N} | {med['kernels']:.1f} us | {100 * spr['kernels']:.0f}% | {med['tensor ops']:.1f} us | "
              f"{100 * spr['tensor ops']:.0f}% |")


def step(rounds):
    from fastmax_experiments_amd import adapter_v2 as av2, finetune_step
    print("\n| finetune_step.run(method='adapter_v2'), tiny-llama-1.1b, 2 full blocks, 2 x 2048 tokens | kernels on | off | off / on |")
    print("|---|---|---|---|")
    times = {True: [], False: []}
    default = av2.FUSED_DEFAULT
    try:
        for _ in range(rounds):
            for on in (True, False):
                av2.FUSED_DEFAULT = on
                r = finetune_step.run("tiny-llama-1.1b", 2, "fastmax", seq=2048, micro_batch=2, accum=1, steps=20, warmup=5,
                                      device=torch.device("cuda"), block="full", method="adapter_v2")
                times[on].append(r["step_ms"])
    finally:
        av2.FUSED_DEFAULT = default
    on, off = statistics.median(times[True]), statistics.median(times[False])
    print(f"| step (median of {rounds}; all: on {', '.join(f'{t:.2f}' for t in times[True])}; off "
          f"{', '.join(f'{t:.2f}' for t in times[False])}) | {on:.2f} ms | {off:.2f} ms | {off / on:.3f}x |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adapter_v2.py needs an MI355X")
    widths(args.rows, args.iters, args.rounds)
    decode(args.rounds)
    if not args.no_step:
        step(max(3, args.rounds // 2))


if __name__ == "__main__":
    main()
