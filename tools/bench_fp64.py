#!/usr/bin/env python
"""float64 fastmax: device time of the float64 kernels (csrc/fastmax_f64.hip) beside the two things a float64 call could run instead.

Per shape, forward and forward + backward, three routes on the same seeded float64 inputs:
  f64     fastmax(...) with FP64_KERNELS on: the float64 matrix-instruction kernels
  f32     the same call with FP64_KERNELS off (FASTMAX_FP64=0): inputs cast to float32, the float32 kernels, the result cast back
  dense   a float64 tensor-op restatement: compute_attn (the dense attention matrix), then matmul; autograd for the backward
The routes differ in precision (f32 carries float32 rounding), so this is a price list, not a race.

Timing: device events around ``--iters`` back-to-back calls after ``--warmup`` calls of every route and shape; ``--rounds`` such
windows per route, the routes alternating inside a round; the median window is reported with the spread (min .. max).
FLOP/s: the float64 operations the tile kernels perform on the visible (query, key) pairs -- 4 D per pair forward (two
products), 14 D per pair backward (three products in the dQ kernel, four in the dK / dV kernel) -- over the f64 route's time.
Prints a markdown table and one JSON line; needs an MI355X (no device: raises).
"""
import argparse
import importlib
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # (B, H, Nq, Nk, D, p, mask)
    (2, 8, 2048, 2048, 64, 2, True),
    (1, 8, 4096, 4096, 128, 2, True),
    (2, 8, 2048, 2048, 64, 1, False),
]


def pairs(B, H, Nq, Nk, mask):
    return B * H * (Nq * (Nq + 1) // 2 if mask else Nq * Nk)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--routes", default="f64,f32,dense")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_fp64 needs an MI355X: there is nothing to time without a device")
    fm = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax")
    routes = args.routes.split(",")

    def run(route, q, k, v, go, p, mask, backward):
        if route == "dense":
            nt = 8.0 * q.shape[-1] ** 0.5
            o = torch.matmul(fm.fastattention_einops.compute_attn(q, k, mask, nt, p), v)
        else:
            fm.FP64_KERNELS = route == "f64"
            o = fm.fastmax(q, k, v, mask=mask, p=p)
        if backward:
            o.backward(go)
            q.grad = k.grad = v.grad = None
        return o

    def window(route, ts, p, mask, backward, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            run(route, *ts, p, mask, backward)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / n

    rows = []
    for (B, H, Nq, Nk, D, p, mask) in SHAPES:
        gen = torch.Generator().manual_seed(0)
        q = torch.randn(B, H, Nq, D, dtype=torch.float64, generator=gen).cuda()
        k, v = (torch.randn(B, H, Nk, D, dtype=torch.float64, generator=gen).cuda() for _ in range(2))
        go = torch.randn(B, H, Nq, D, dtype=torch.float64, generator=gen).cuda()
        for backward in (False, True):
            ts = tuple(t.clone().requires_grad_(backward) for t in (q, k, v)) + (go,)
            with torch.set_grad_enabled(backward):
                for route in routes:
                    window(route, ts, p, mask, backward, args.warmup)
                times = {r: [] for r in routes}
                for _ in range(args.rounds):
                    for route in routes:
                        times[route].append(window(route, ts, p, mask, backward, args.iters))
            row = dict(shape=[B, H, Nq, Nk, D], p=p, mask=mask, what="fwd+bwd" if backward else "fwd",
                       ms={r: statistics.median(t) for r, t in times.items()},
                       spread_ms={r: [min(t), max(t)] for r, t in times.items()})
            if "f64" in routes:
                flop = pairs(B, H, Nq, Nk, mask) * D * (18 if backward else 4)
                row["f64_tflops"] = flop / (row["ms"]["f64"] * 1e-3) / 1e12
            rows.append(row)
    fm.FP64_KERNELS = True
    print("| shape (B,H,Nq,Nk,D) | p | mask | what | " + " | ".join(f"{r} ms (min .. max)" for r in routes) + " | f64 TFLOP/s |")
    print("|---|---|---|---|" + "---|" * (len(routes) + 1))
    for r in rows:
        cells = " | ".join(f"{r['ms'][x]:.3f} ({r['spread_ms'][x][0]:.3f} .. {r['spread_ms'][x][1]:.3f})" for x in routes)
        print(f"| {tuple(r['shape'])} | {r['p']} | {r['mask']} | {r['what']} | {cells} | {r.get('f64_tflops', float('nan')):.2f} |")
    print(json.dumps(dict(bench="fp64", iters=args.iters, warmup=args.warmup, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
