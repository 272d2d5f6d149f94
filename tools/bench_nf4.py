#!/usr/bin/env python3
"""Time the NF4 + LoRA linear (forward; dx through a bare NF4Linear) against a dense bf16 library GEMM of the same shape,
and the host-bound call: one row under no_grad, wall clock per call.  Row counts to run may be given as arguments."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fastmax_experiments_amd import lora

SHAPES = ((1, 4096, 4096), (64, 4096, 4096), (256, 4096, 4096), (512, 4096, 4096), (1024, 4096, 4096), (2048, 4096, 4096),
          (4096, 4096, 4096), (2048, 4096, 11008), (16384, 2048, 2560), (16384, 4096, 4096), (8192, 4096, 12288), (16384, 4096, 11008))


def timeit(fn, iters=50, rounds=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts)


def host_us(fn, iters=2000, rounds=5):
    """wall-clock microseconds per call with the queue never drained in between: what the host spends issuing it"""
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        ts.append((time.perf_counter() - t0) / iters * 1e6)
        torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    want = {int(a) for a in sys.argv[1:]}
    print("| M (tokens) | K | N | NF4+LoRA fwd ms | TFLOP/s | dx ms | TFLOP/s | dense bf16 F.linear ms | TFLOP/s | host us / call |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for M, K, N in SHAPES:
        if want and M not in want:
            continue
        torch.manual_seed(0)
        layer = lora.LoRALinear(K, N, r=8, lora_alpha=16, bias=False)
        torch.nn.init.normal_(layer.lora_B, std=0.02)
        dense_w = layer.linear.weight.data.to("cuda", torch.bfloat16)
        layer.quantize_base().cuda()
        if os.environ.get("FASTMAX_NF4_CACHE") == "1":
            layer.linear.cache_dense()
        base = layer.linear
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        gy = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
        with torch.no_grad():
            t_f = timeit(lambda: layer(x))
            t_d = timeit(lambda: torch.nn.functional.linear(x, dense_w))
            t_h = host_us(lambda: layer(x)) if M == 1 else float("nan")
            t_base = timeit(lambda: base(x))
        xx = x.detach().requires_grad_(True)
        t_b = timeit(lambda: base(xx).backward(gy)) - t_base
        fl = 2 * M * K * N / 1e9
        print(f"| {M} | {K} | {N} | {t_f:.3f} | {fl / t_f:.0f} | {t_b:.3f} | {fl / t_b:.0f} | {t_d:.3f} | {fl / t_d:.0f} | {t_h:.1f} |", flush=True)


if __name__ == "__main__":
    main()
