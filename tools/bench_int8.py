#!/usr/bin/env python3
"""Time the int8 linear ("bnb.int8", csrc/int8_linear.hip) on an MI355X beside the dense bf16 product and the NF4 few-rows route.

    python tools/bench_int8.py [--iters 20] [--rounds 5] [--out profiles/r27_int8_linear.md]

Widths (K -> N): (2048 -> 5632), (4096 -> 4096), (4096 -> 11008), (11008 -> 4096); bf16 activations, standard normal, so no
column reaches the threshold 6 but for the stray one in a few thousand (the usual case).  M = 1, 8, 16 run the few-rows kernel,
M = 512, 4096 the tile kernel.  Arms, alternating round by round in one process.  Each arm rotates over its own copies of the
weight, as many as make 512 MiB of THAT arm's bytes (int8 codes, bf16, or NF4 codes + scales), and a replay makes at least one call
per copy, so that no arm finds its weight in the 256 MiB last-level cache:
    int8        Int8Linear.forward: the activation pass (two launches) and the product
    act pass    fastmax_hip_int8_quantize_rows alone (the same two launches)
    dense       F.linear on the dequantised bf16 weight (the library GEMM)
    nf4         NF4Linear.forward, the few-rows route (M <= 16 only)
Every arm's calls (`--iters`, a quarter of it at M = 4096, and never fewer than its copies) are recorded once in a graph and replayed: what is printed is the device's time per call, the median
of the rounds and their spread.  GB/s: the bytes of weight codes the call has to read (N K for int8, 2 N K dense, N K / 2 + N K / 16
for NF4) over its time.  No time here is a pass criterion."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_next_token import recorded          # noqa: E402

WIDTHS = [(2048, 5632), (4096, 4096), (4096, 11008), (11008, 4096)]
ROWS = [1, 8, 16, 512, 4096]


def case(K, N, M, args):
    from fastmax_experiments_amd import _lib
    from fastmax_experiments_amd.lora import Int8Linear, NF4Linear
    dev = torch.device("cuda")
    nbytes = {"int8": N * K, "dense": 2 * N * K, "nf4": N * K // 2 + N * K // 16}          # the weight stream of one call
    copies = {name: (512 << 20) // b + 2 for name, b in nbytes.items()}
    if M > _lib.INT8_FEW_ROWS:
        del copies["nf4"]
    torch.manual_seed(0)
    int8, dense, nf4 = [], [], []
    for i in range(max(copies.values())):
        lin = torch.nn.Linear(K, N, bias=False).to(dev, torch.bfloat16)
        if i < copies["int8"]:
            int8.append(Int8Linear.from_linear(lin))
        if i < copies["dense"]:
            dense.append(Int8Linear.from_linear(lin).dequantize(torch.bfloat16))
        if i < copies.get("nf4", 0):
            nf4.append(NF4Linear.from_linear(lin))
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    ca = torch.empty((M, K), dtype=torch.int8, device=dev)
    sca = torch.empty(M, dtype=torch.float32, device=dev)
    flags = torch.empty(K, dtype=torch.uint8, device=dev)
    lst, cnt = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.lib()

    def act_pass(i):
        rc = L.fastmax_hip_int8_quantize_rows(x.data_ptr(), K, _lib.BF16, 6.0, ca.data_ptr(), sca.data_ptr(), flags.data_ptr(),
                                              lst.data_ptr(), cnt.data_ptr(), M, K, torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    arms = {"int8": (lambda i: int8[i % len(int8)](x), nbytes["int8"]), "act pass": (act_pass, 0),
            "dense": (lambda i: F.linear(x, dense[i % len(dense)]), nbytes["dense"])}
    if nf4:
        arms["nf4"] = (lambda i: nf4[i % len(nf4)](x), nbytes["nf4"])
    iters = args.iters if M <= 512 else max(4, args.iters // 4)
    with torch.no_grad():
        replays = {name: recorded(fn, max(iters, copies.get(name, 0))) for name, (fn, _) in arms.items()}
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, replay in replays.items():
                times[name].append(replay())
    cells = []
    for name in ("int8", "act pass", "dense", "nf4"):
        if name not in arms:
            cells.append("-")
            continue
        t = statistics.median(times[name])
        spread = (max(times[name]) - min(times[name])) / t
        gbs = f", {arms[name][1] / t / 1e3:.0f} GB/s" if arms[name][1] else ""
        cells.append(f"{t:.1f} us (+-{100 * spread:.0f}%{gbs})")
    outliers = int(cnt.item())
    return f"| {K} -> {N} | {M} | {outliers} | " + " | ".join(cells) + f" | {statistics.median(times['dense']) / statistics.median(times['int8']):.2f} |"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["| K -> N | M | outlier columns | int8 (whole call) | activation pass alone | dense bf16 F.linear | NF4 few-rows | dense / int8 |",
             "|---|---|---|---|---|---|---|---|"]
    for K, N in WIDTHS:
        for M in ROWS:
            lines.append(case(K, N, M, args))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
