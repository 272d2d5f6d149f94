#!/usr/bin/env python3
"""Digests of what the QLoRA layers return, for comparing two trees bit for bit on one MI355X.

    python tools/qlora_parity.py                 # one line per case: name, then a digest per returned tensor
    python tools/qlora_parity.py --write         # rewrites tests/golden/qlora_parity.json (the all-HIP cases)

Every case builds its layer and inputs on the CPU from a fixed seed, runs forward and backward through the public layer
classes only, and prints the first 16 hex digits of the SHA-256 of y, dx, dA and dB.  The cases in ALL_HIP run no library
GEMM (every product is one of libfastmax_hip.so's kernels), so their digests are a property of the kernels and the operand
values: tests/test_lora_gpu.py holds them to tests/golden/qlora_parity.json.  The others contain a torch GEMM (the rank-r
F.linear of the few-rows route) and are compared only between two runs on the same machine.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "qlora_parity.json")
K, N = 256, 384
CASES = {
    # name: (kind, rows, options)
    "lora_m2304": ("linear", (2304,), {}),
    "lora_dropout_m2304": ("linear", (2304,), {"lora_dropout": 0.5}),
    "qkv_gqa_3x700": ("qkv", (3, 700), {}),
    "double_quant_m2304": ("linear", (2304,), {"double_quant": True}),
    "cache_dense_m16": ("linear", (16,), {"cache_dense": True}),
    "cache_dense_m2304": ("linear", (2304,), {"cache_dense": True}),
    "resident_bytes_0_m2304": ("linear", (2304,), {"resident_bytes": 0}),
    "route_fused_m2304": ("linear", (2304,), {"route": "fused"}),
    "dense_base_2x1500": ("linear", (2, 1500), {"quantize": False}),
    "bare_nf4_m75": ("bare", (75,), {}),
    "bare_nf4_m2304": ("bare", (2304,), {}),
    "rope_block_5x3328": ("block", (5, 3328), {}),
    "fp16_m2304": ("linear", (2304,), {"dtype": torch.float16}),
    "few_rows_m75_bf16": ("linear", (75,), {}),
    "few_rows_m75_fp32": ("linear", (75,), {"dtype": torch.float32}),
}
ALL_HIP = [name for name in CASES if not name.startswith(("fp16", "few_rows"))]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run_case(name):
    """{tensor name: digest} of one case"""
    from fastmax_experiments_amd import lora
    from fastmax_experiments_amd.attention_block import CausalSelfAttention, build_rope_cache
    kind, rows, opt = CASES[name]
    dtype = opt.get("dtype", torch.bfloat16)
    pdt = torch.float32 if dtype == torch.float32 else torch.bfloat16
    saved = lora.QLORA_ROUTE, lora.RESIDENT_BYTES
    lora.QLORA_ROUTE = opt.get("route", saved[0])
    lora.RESIDENT_BYTES = opt.get("resident_bytes", saved[1])
    try:
        torch.manual_seed(11)
        g = torch.Generator().manual_seed(12)
        if kind == "bare":
            lin = torch.nn.Linear(K, N)
            layer = adapted = lora.NF4Linear.from_linear(lin).cuda()
        elif kind == "block":
            layer = CausalSelfAttention(n_embd=K, n_head=8, n_query_groups=2, head_size=32, r=8, alpha=16, bias=True).to(pdt)
            adapted = layer.attn
        elif kind == "qkv":
            layer = adapted = lora.LoRAQKVLinear(K, N, n_head=8, n_query_groups=2, r=8, lora_alpha=16,
                                                 enable_lora=(True, False, True)).to(pdt)
        else:
            layer = adapted = lora.LoRALinear(K, N, r=8, lora_alpha=16, lora_dropout=opt.get("lora_dropout", 0.0), bias=True).to(pdt)
        if kind != "bare":
            torch.nn.init.normal_(adapted.lora_B, std=0.05, generator=g)
            if opt.get("quantize", True):
                layer.quantize_base(opt.get("double_quant", False))
            layer.cuda()
            lora.mark_only_lora_as_trainable(layer)
            if opt.get("cache_dense"):
                adapted.linear.cache_dense()
            layer.train()
        x = torch.randn(*rows, K, generator=g).to(dtype).cuda().requires_grad_(True)
        out_width = K if kind == "block" else N
        gy = torch.randn(*rows, out_width, generator=g).to(dtype).cuda()
        torch.manual_seed(13)                                    # the dropout seed comes from torch's device generator
        if kind == "block":
            cos, sin = build_rope_cache(rows[1], layer.rope_n_elem, device="cuda")
            y = layer(x, cos, sin)
        else:
            y = layer(x)
        y.backward(gy)
        torch.cuda.synchronize()
        out = {"y": digest(y), "dx": digest(x.grad)}
        if kind != "bare":
            out.update(dA=digest(adapted.lora_A.grad), dB=digest(adapted.lora_B.grad))
        return out
    finally:
        lora.QLORA_ROUTE, lora.RESIDENT_BYTES = saved


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite tests/golden/qlora_parity.json from this tree's answers")
    args = ap.parse_args()
    table = {}
    for name in CASES:
        table[name] = run_case(name)
        print(f"{name} " + " ".join(f"{k}={v}" for k, v in table[name].items()), flush=True)
    if args.write:
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f'"{n}":{json.dumps(table[n], separators=(",", ":"))}' for n in ALL_HIP) + "\n}\n")
