#!/usr/bin/env python3
"""Time the accumulation boundary of the fine-tune step on an MI355X: the tensor-op chain against optim.FlatAdamW.

    python tools/bench_optim.py [--iters 200] [--rounds 5] [--world 8] [--max-norm 1.0] [--skip-step]

1. the boundary alone, at the LoRA sizes of TinyLlama and Llama-2-7B (r = 8 on q, v; one lora_A and one lora_B per layer, as
   lit_gpt's fused qkv LoRA lays them out), float32 parameters in a float32 bucket and bf16 parameters in a float32 bucket:
       torch route:  flat.div_(world); [scatter]; clip_grad_norm_; torch.optim.AdamW.step(); bucket.zero()
       flat route:   FlatAdamW.step(grad_scale=1/world, max_norm=...)
   Both routes start from the same gradient copied into the bucket (the copy is timed alone and printed, not subtracted).  The
   routes alternate round by round in one process; per route the median and the spread of the rounds are printed.  Launch counts
   are known from the code (profiles/r10_flat_adamw.md), not measured here.
2. `finetune_step.run` per optimizer step with either optimizer (`--skip-step` leaves it out).
Times are device events around `--iters` calls after a warm-up; no time here is a pass criterion."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (n_layer, n_embd, q + v output rows) of the reference's configs
LORA_SHAPES = {"tiny-llama-1.1b": (22, 2048, 32 * 64 + 4 * 64), "Llama-2-7b-hf": (32, 4096, 32 * 128 + 32 * 128)}
R = 8


def lora_parameters(config, dtype, dev):
    layers, n_embd, qv_rows = LORA_SHAPES[config]
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for _ in range(layers):
        out.append(torch.nn.Parameter((torch.randn(2 * R, n_embd, device=dev, generator=g) * 0.02).to(dtype)))     # lora_A
        out.append(torch.nn.Parameter((torch.randn(qv_rows, R, device=dev, generator=g) * 0.02).to(dtype)))        # lora_B
    return out


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters          # microseconds


def boundary(config, dtype, args):
    from fastmax_experiments_amd import dp
    from fastmax_experiments_amd.optim import FlatAdamW
    dev = torch.device("cuda")
    world = args.world
    p_torch, p_flat = lora_parameters(config, dtype, dev), lora_parameters(config, dtype, dev)
    b_torch, b_flat = dp.FlatGradBucket(p_torch), dp.FlatGradBucket(p_flat)
    o_torch = torch.optim.AdamW(p_torch, lr=1e-4)
    o_flat = FlatAdamW(b_flat, lr=1e-4)
    n = b_torch.flat.numel()
    grad = torch.randn(n, device=dev) * 1e-3

    def torch_route():
        b_torch.flat.copy_(grad)
        b_torch.flat.div_(world)
        b_torch.scatter()                              # what all_reduce_mean does after the collective (16-bit parameters)
        if args.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(b_torch.params, args.max_norm)
        o_torch.step()
        b_torch.zero()

    def flat_route():
        b_flat.flat.copy_(grad)
        o_flat.step(grad_scale=1.0 / world, max_norm=args.max_norm)

    def copy_only():
        b_flat.flat.copy_(grad)

    times = {"torch": [], "flat": [], "copy": []}
    for _ in range(args.rounds):
        for name, fn in (("torch", torch_route), ("flat", flat_route), ("copy", copy_only)):
            times[name].append(timed(fn, args.iters))
    vec, elem = o_flat.route_counts()
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    print(f"{config:16s} {str(dtype).split('.')[-1]:9s} n = {n:8d}  tensors = {len(p_flat):3d}  chunks = {vec + elem} ({vec} vector, {elem} element)")
    for k in ("torch", "flat", "copy"):
        print(f"    {k:6s} {med[k]:9.1f} us   (rounds {spread[k][0]:.1f} .. {spread[k][1]:.1f})")
    print(f"    torch / flat = {med['torch'] / med['flat']:.2f}x   without the copy: "
          f"{(med['torch'] - med['copy']) / max(med['flat'] - med['copy'], 1e-9):.2f}x")


def whole_step(args):
    from fastmax_experiments_amd import finetune_step
    dev = torch.device("cuda")
    res = {"torch": [], "flat": []}
    for _ in range(args.step_rounds):
        for opt in ("torch", "flat"):
            r = finetune_step.run(args.config, args.layers, "fastmax", args.seq, 2, 2, args.steps, 3, dev, optimizer=opt)
            res[opt].append(r["step_ms"])
    print(f"finetune_step.run {args.config}, {args.layers} layers, seq {args.seq}, micro-batch 2 x accum 2, {args.steps} steps per round")
    for opt in ("torch", "flat"):
        print(f"    {opt:6s} {statistics.median(res[opt]):9.3f} ms / step   (rounds {min(res[opt]):.3f} .. {max(res[opt]):.3f})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--world", type=int, default=8, help="the divisor of the torch route / 1 over the flat route's grad_scale")
    ap.add_argument("--max-norm", type=float, default=1.0, help="negative: no clipping in either route")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--config", default="tiny-llama-1.1b")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    if args.max_norm is not None and args.max_norm < 0:
        args.max_norm = None
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on an MI355X; there is no device here")
    for config in LORA_SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            boundary(config, dtype, args)
    if not args.skip_step:
        whole_step(args)


if __name__ == "__main__":
    main()
