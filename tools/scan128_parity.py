#!/usr/bin/env python3
"""Digests of what the eight-wave causal scans at 64 < D <= 128 return, for comparing two builds bit for bit on one MI355X.

    python tools/scan128_parity.py                 # one line per case: name, then a digest per returned tensor
    python tools/scan128_parity.py --write         # rewrites tests/golden/scan128_parity.json
    python tools/scan128_parity.py --twice         # runs every case twice and says which reproduce their own digests

Every case builds its inputs on the CPU from a fixed seed, runs forward and, where the case trains, backward, and prints the
first 16 hex digits of the SHA-256 of the output and of every gradient.  B * H = 2, so a case takes milliseconds; the shapes
are the smallest that reach every instantiation of fwd_p1_mfma_bf16_d128_kernel, fwd_p1_mfma_d128_2p_kernel and
scan_d128_2p_kernel on the buffer-descriptor route (the pointer route needs a (b,h) slab of 1 GiB and is not run):
N = 130 is 3 chunks, the last of 2 rows, unsplit; 576 is 9 chunks in 2 segments forwards and 1 backwards; 1100 is 18 chunks,
the last of 12 rows, in 4 segments forwards and 2 backwards (the STATE_ONLY launches).  The kernels have no atomics: every
case reproduced its own digests when it was recorded (--twice).  tests/test_scan128_gpu.py holds the library to
tests/golden/scan128_parity.json, recorded with the build before csrc/fastmax_scan128.h existed.
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scan128_parity.json")
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
_NAME = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}
# name: (kind, shape, dtype, forward kernel, backward kernel, forward segments)
CASES = {}
for _dt, _ds in ((BF16, (72, 128)), (FP32, (68, 128)), (FP16, (72, 128))):
    for _D in _ds:
        for _N, _nseg in ((130, 1), (576, 2), (1100, 4)):
            CASES[f"fwd_{_NAME[_dt]}_d{_D}_n{_N}"] = ("fwd", (1, 2, _N, _D), _dt, "FWD_SCAN_BF16" if _dt == BF16 else "FWD_SCAN_D128_2P", None, _nseg)
for _dt, _N, _D, _nseg in ((BF16, 576, 128, 2), (FP32, 576, 128, 2), (FP32, 300, 128, 1), (FP16, 1100, 72, 4)):
    CASES[f"hack_{_NAME[_dt]}_d{_D}_n{_N}"] = ("hack", (1, 2, _N, _D), _dt, "FWD_SCAN_BF16" if _dt == BF16 else "FWD_SCAN_D128_2P", None, _nseg)
for _dt, _ds in ((FP32, (128, 68)), (FP16, (128, 72))):
    for _D in _ds:
        for _N, _nseg in ((576, 2), (1100, 4)):
            CASES[f"train_{_NAME[_dt]}_d{_D}_n{_N}"] = ("train", (1, 2, _N, _D), _dt, "FWD_SCAN_D128_2P", "BWD_SCAN", _nseg)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def inputs(name):
    """q, k, v, grad_o of a case on the GPU, from its seed"""
    _, shape, dtype = CASES[name][:3]
    g = torch.Generator().manual_seed(21)
    return tuple(torch.randn(shape, generator=g).to(dtype).cuda() for _ in range(4))


def planned(name):
    """(forward kernel, backward kernel, forward segments) the library plans for a case"""
    from fastmax_experiments_amd import ops
    q, k, v, go = inputs(name)
    plan = ops.planned_kernels(q, k, v, 1, True, grad_o=go if CASES[name][0] == "train" else None)
    return plan["fwd_kernel"], plan["bwd_kernel"], plan["nseg"]


def run_case(name):
    """{tensor name: digest} of one case"""
    fm = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax")
    fh = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax_hack")
    kind = CASES[name][0]
    q, k, v, go = inputs(name)
    out = {}
    with torch.set_grad_enabled(kind == "train"):
        for t in (q, k, v):
            t.requires_grad_(kind == "train")
        out["o"] = (fh.fastmax_hack if kind == "hack" else fm.fastmax)(q, k, v, p=1, mask=True)
        if kind == "train":
            out["o"].backward(go)
            out.update(dq=q.grad, dk=k.grad, dv=v.grad)
    torch.cuda.synchronize()
    return {n: digest(t) for n, t in out.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", nargs="?", const=GOLDEN, metavar="FILE",
                    help="rewrite tests/golden/scan128_parity.json (or FILE) from this build's answers")
    ap.add_argument("--twice", action="store_true", help="run every case twice: which reproduce their own digests?")
    args = ap.parse_args()
    table = {}
    for name in CASES:
        table[name] = run_case(name)
        again = "" if not args.twice else (" reproduced" if run_case(name) == table[name] else " NOT REPRODUCED")
        print(f"{name} " + " ".join(f"{k}={v}" for k, v in table[name].items()) + again, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("{\n" + ",\n".join(f'"{n}":{json.dumps(table[n], separators=(",", ":"))}' for n in CASES) + "\n}\n")
