#!/usr/bin/env python3
"""Digests of what linearmax and the attention sub-layer return, for comparing two trees bit for bit on one MI355X.

    python tools/attention_parity.py                 # one line per case: name, then a digest per returned tensor
    python tools/attention_parity.py --write         # rewrites tests/golden/attention_parity.json
    python tools/attention_parity.py --twice         # runs every case twice and says which reproduce their own digests

Every case builds its inputs (and the block its weights) on the CPU from a fixed seed, runs forward and, where the case
trains, backward, and prints the first 16 hex digits of the SHA-256 of the output and of every gradient.  The attention of
every case runs in libfastmax_hip.so, and the block's T = 640 keeps its NF4 linears on the few-rows kernels; the one library
GEMM left is the rank-r F.linear of that route, and every case reproduced its own digests when it was recorded (--twice).
tests/test_block_gpu.py holds them to tests/golden/attention_parity.json, recorded before the route plans existed.
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_parity.json")
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
CASES = {
    # name: (kind, shape, dtype, options)
    "one_node_d64": ("op", (1, 2, 512, 64), BF16, {}),
    "one_node_d128": ("op", (1, 2, 512, 128), BF16, {}),
    "two_node_n511": ("op", (1, 2, 511, 64), BF16, {}),
    "two_node_fp32_d128": ("op", (1, 2, 512, 128), FP32, {}),
    "prologue_fp16_d40": ("op", (1, 2, 260, 40), FP16, {}),
    "unmasked_n130": ("op", (1, 2, 130, 64), BF16, {"mask": False}),
    "fused_forward_fp32_d128": ("op", (1, 2, 300, 128), FP32, {"grad": False}),
    "grouped_views": ("grouped", (2, 2, 4, 640, 64), BF16, {"views": True}),
    "grouped_copies": ("grouped", (2, 2, 4, 640, 64), BF16, {"views": False}),
    "block_linearmax_train": ("block", (2, 640), BF16, {"alg": "linearmax"}),
    "block_fastmax_train": ("block", (2, 640), BF16, {"alg": "fastmax"}),
    "block_linearmax_no_grad": ("block", (2, 640), BF16, {"alg": "linearmax", "grad": False}),
}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run_case(name, tensors=False):
    """{tensor name: digest} of one case (``tensors``: the tensors themselves, on the CPU)"""
    from fastmax_experiments_amd import lora
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    fh = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax_hack")
    kind, shape, dtype, opt = CASES[name]
    grad = opt.get("grad", True)
    g = torch.Generator().manual_seed(12)
    out = {}
    with torch.set_grad_enabled(grad):
        if kind == "op":
            q, k, v, go = (torch.randn(shape, generator=g).to(dtype).cuda() for _ in range(4))
            leaves = dict(dq=q, dk=k, dv=v)
            for t in leaves.values():
                t.requires_grad_(grad)
            y = fh.fastmax_hack(q, k, v, p=1, mask=opt.get("mask", True))
        elif kind == "grouped":
            B, G, rep, N, D = shape
            q = torch.randn((B * G, rep, N, D) if opt["views"] else (B, G * rep, N, D), generator=g).to(dtype).cuda()
            k, v = (torch.randn(B, G, N, D, generator=g).to(dtype).cuda() for _ in range(2))
            go = torch.randn(q.shape, generator=g).to(dtype).cuda()
            leaves = dict(dq=q, dk=k, dv=v)
            for t in leaves.values():
                t.requires_grad_(True)
            vv = v.view(B * G, 1, N, D).expand(B * G, rep, N, D) if opt["views"] else v.repeat_interleave(rep, dim=1)
            y = fh.fastmax_hack_grouped(q, k, vv, rep, p=1)
        else:
            B, T = shape
            torch.manual_seed(11)
            blk = CausalSelfAttention(256, 8, n_query_groups=2, attn_alg=opt["alg"], r=8, alpha=16, to_projection=True).to(dtype)
            for layer in (blk.attn, blk.proj):
                torch.nn.init.normal_(layer.lora_B, std=0.05, generator=g)
            blk.quantize_base().cuda()
            lora.mark_only_lora_as_trainable(blk)
            cos, sin = build_rope_cache(T, blk.rope_n_elem, device="cuda")
            x = torch.randn(B, T, 256, generator=g).to(dtype).cuda().requires_grad_(grad)
            go = torch.randn(B, T, 256, generator=g).to(dtype).cuda()
            leaves = dict(dx=x, dA=blk.attn.lora_A, dB=blk.attn.lora_B, dA_proj=blk.proj.lora_A, dB_proj=blk.proj.lora_B)
            y = blk(x, cos, sin)
        out["y"] = y
        if grad:
            y.backward(go.to(y.dtype))
            out.update({n: t.grad for n, t in leaves.items()})
    torch.cuda.synchronize()
    return {n: (t.detach().cpu() if tensors else digest(t)) for n, t in out.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", nargs="?", const=GOLDEN, metavar="FILE",
                    help="rewrite tests/golden/attention_parity.json (or FILE) from this tree's answers")
    ap.add_argument("--twice", action="store_true", help="run every case twice: which reproduce their own digests?")
    ap.add_argument("--save", metavar="FILE", help="torch.save the tensors of every case, for a comparison at a tolerance")
    args = ap.parse_args()
    table = {}
    for name in CASES:
        table[name] = run_case(name)
        again = "" if not args.twice else (" reproduced" if run_case(name) == table[name] else " NOT REPRODUCED")
        print(f"{name} " + " ".join(f"{k}={v}" for k, v in table[name].items()) + again, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("{\n" + ",\n".join(f'"{n}":{json.dumps(table[n], separators=(",", ":"))}' for n in CASES) + "\n}\n")
    if args.save:
        torch.save({name: run_case(name, tensors=True) for name in CASES}, args.save)
