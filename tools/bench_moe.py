#!/usr/bin/env python3
"""Time the mixture-of-experts MLP (fastmax_experiments_amd/moe.py) from the router to the combine on an MI355X, routing kernels
on against off (``fused_neighbours``), and at decode sizes the device-routed expert kernels (``device_routed``) beside both, on
the same commit in the same process.

    python tools/bench_moe.py [--iters 10] [--reps 3] [--n-embd 4096 --intermediate 14336 --experts 8 --per-token 2]

The default is the Mixtral-8x7B width in bf16 with the experts' linears in NF4.  Sizes: 4096 tokens forward + backward (the gate
is the trainable part: the NF4 experts are frozen), and 1, 8 and 16 tokens forward (decode), where the arm "device" is
``device_routed = True``: gate, route, experts_up, experts_down, combine.  Per size and arm the table gives
  * device kernels per call, counted by torch.profiler over ONE call in a pass of its own (never inside a timed window);
  * host reads per call: ``moe._read_offsets`` calls on the fused route, ``torch.where`` calls on the tensor-op route;
  * ms per call: device events around `--iters` calls after a warm-up at the same size, the two arms alternating `--reps` times;
    median (lowest .. highest).
The experts' matrix products run in every arm and take most of the time at 4096 tokens; no time here is a pass criterion.
A second table times experts_up + experts_down ALONE on the routing of the same rows and sets the NF4 code and scale bytes of
the experts that have rows (each read once by the pair) against that time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def build(n_embd, inter, E, k, device="cuda"):
    """expert by expert on the device, quantized as it is made: the dense weights of all experts never coexist"""
    from fastmax_experiments_amd import block
    from fastmax_experiments_amd.moe import LLaMAMoE
    torch.manual_seed(0)
    with torch.device(device):
        moe = LLaMAMoE(n_embd, inter, 1, 1).to(torch.bfloat16)
        experts = [moe.experts[0].quantize_base()]
        for _ in range(E - 1):
            experts.append(block.LLaMAMLP(n_embd, inter).to(torch.bfloat16).quantize_base())
        gate = type(moe.gate)(n_embd, E, bias=False).to(torch.bfloat16)
    moe.experts, moe.gate, moe.n_expert, moe.n_expert_per_token = torch.nn.ModuleList(experts), gate, E, k
    return moe


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError as err:                    # a profiler without device tracing: say so in the table, time the rest
        return f"not measured ({type(err).__name__})"
    return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA") and "emcpy" not in ev.name and "emset" not in ev.name)


def count_reads(fn):
    """(offset reads, torch.where calls) of one call"""
    from fastmax_experiments_amd import moe as moe_mod
    n = [0, 0]
    real_read, real_where = moe_mod._read_offsets, torch.where
    moe_mod._read_offsets = lambda o: n.__setitem__(0, n[0] + 1) or real_read(o)
    torch.where = lambda *a, **kw: n.__setitem__(1, n[1] + 1) or real_where(*a, **kw)
    try:
        fn()
    finally:
        moe_mod._read_offsets, torch.where = real_read, real_where
    return n[0] + n[1]


def fmt(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-embd", type=int, default=4096)
    ap.add_argument("--intermediate", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--per-token", type=int, default=2)
    ap.add_argument("--no-kernel-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py needs an MI355X")
    moe = build(args.n_embd, args.intermediate, args.experts, args.per_token)
    print(f"LLaMAMoE n_embd {args.n_embd}, intermediate {args.intermediate}, {args.experts} experts, {args.per_token} per token, "
          "bf16, experts NF4\n")
    print("| tokens | pass | arm | device kernels | host reads | ms per call, median (lowest .. highest) | off / arm |\n|---|---|---|---|---|---|---|",
          flush=True)

    def select(arm):
        moe.fused_neighbours = arm != "off"
        moe.device_routed = arm == "device"

    for tokens, train in ((4096, True), (16, False), (8, False), (1, False)):
        x = torch.randn(1, tokens, args.n_embd, device="cuda").to(torch.bfloat16)
        gy = torch.randn_like(x)

        def call():
            if train:
                for p in moe.parameters():
                    p.grad = None
                moe(x.detach().requires_grad_(True)).backward(gy)
            else:
                with torch.no_grad():
                    moe(x)

        arms = ("on", "off") if train else ("on", "off", "device")
        ms, kernels, reads = {a: [] for a in arms}, {}, {}
        for arm in arms:
            select(arm)
            reads[arm] = count_reads(call)
            kernels[arm] = "not counted" if args.no_kernel_count else count_kernels(call)
        for _ in range(args.reps):
            for arm in arms:
                select(arm)
                ms[arm].append(timed(call, args.iters))
        select("on")
        for arm in arms:
            ratio = statistics.median(ms["off"]) / statistics.median(ms[arm])
            print(f"| {tokens} | {'forward + backward' if train else 'forward'} | {arm} | {kernels[arm]} | {reads[arm]} | "
                  f"{fmt(ms[arm])} | {'' if arm == 'off' else f'{ratio:.2f}x'} |", flush=True)
    expert_kernels(moe, args)


def expert_kernels(moe, args):
    """experts_up + experts_down alone, on the routing of random rows: time, and the active experts' NF4 bytes over it"""
    from fastmax_experiments_amd import moe as moe_mod
    C, I, k = args.n_embd, args.intermediate, args.per_token
    per_expert = 3 * (C * I // 2 + C * I // 64 * 4)                    # codes and float32 block scales of fc_1, fc_2, proj
    table = moe.expert_table()
    print("\n| tokens | experts with rows | NF4 code + scale bytes read | experts_up + experts_down, ms: median (lowest .. highest) | "
          "GB/s |\n|---|---|---|---|---|", flush=True)
    for tokens in (16, 8, 1):
        x = torch.randn(tokens, C, device="cuda").to(torch.bfloat16)
        with torch.no_grad():
            _, _, _, offsets, row_of, _ = moe_mod.route(moe.gate(x), k)
        bounds = offsets.tolist()
        active = sum(1 for a, b in zip(bounds, bounds[1:]) if b > a)

        def pair():
            moe_mod.experts_down(moe_mod.experts_up(x, table, offsets, row_of, k, I), table, offsets, k, C)

        ms = [timed(pair, args.iters) for _ in range(args.reps)]
        nbytes = active * per_expert
        print(f"| {tokens} | {active} of {args.experts} | {nbytes / 1e6:.1f} MB | {fmt(ms)} | {nbytes / statistics.median(ms) / 1e6:.0f} |",
              flush=True)


if __name__ == "__main__":
    main()
