"""Record which route the QLoRA linear takes, without a GPU: for a grid of plain-data arguments the answer of
lora.qlora_plan -- the frozen product's route, where the LoRA branch and its dropout run, the rank padding and whether the
qkv + RoPE epilogue may be used -- or the exception it raises.

    python tools/qlora_routes.py            # prints the table
    python tools/qlora_routes.py --write    # rewrites tests/golden/qlora_routes.json

tests/test_lora_cpu.py compares the plan against the committed file row by row.  The committed answers are what the layers
ran before the plan existed (recorded on an MI355X by watching which autograd Function, and which branch of it, each row
took): a row that differs is a bug in the plan, not a reason to rewrite the file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "qlora_routes.json")
K, N = 256, 384                                  # N = (8 + 4) * 32: 8 heads in 2 groups of head size 32
MS = [1, 16, 17, 75, 2047, 2048, 16640]
ROPE = {16640: [3328, 2, 4, 32, 32], 2048: [2048, 2, 4, 32, 32]}        # M -> (T, groups, q per kv, head size, rope_n)
DEFAULTS = dict(base="nf4", device="cuda", dtype="bf16", M=2048, rank=8, lora_dropout=0.0, training=True, cache_dense=False,
                merged=False, route="gemm", dense_lora_gemm=True, gemm_rope=True, rope_shape=None)


def rows():
    """the thinned cross product: every base kind, dtype and row count with a small and a too-large rank; every rank, the
    decoded-weight cache, dropout, merged layers, the two switches and the epilogue where they can change an answer"""
    out = []

    def emit(**kw):
        row = dict(DEFAULTS, **kw)
        if row not in out:
            out.append(row)

    for base in ("nf4", "dense", "dense_bias_trains"):
        for dtype in ("bf16", "fp16", "fp32"):
            for M in MS:
                for rank in (8, 40):
                    emit(base=base, dtype=dtype, M=M, rank=rank)
    for base in ("nf4", "dense"):
        for dtype in ("bf16", "fp16"):
            for M in (75, 2048):
                for rank in (16, 24, 32):
                    emit(base=base, dtype=dtype, M=M, rank=rank)
    for dtype in ("bf16", "fp16", "fp32"):
        for M in MS:
            for rank in (8, 24, 40):
                emit(dtype=dtype, M=M, rank=rank, cache_dense=True)
    for base in ("nf4", "dense"):
        for dtype in ("bf16", "fp32"):
            for M in (75, 2048):
                for training in (True, False):
                    emit(base=base, dtype=dtype, M=M, lora_dropout=0.05, training=training)
    for M in (75, 2048):
        for dtype in ("bf16", "fp32"):
            emit(M=M, dtype=dtype, merged=True)
            emit(M=M, dtype=dtype, merged=True, cache_dense=True)
        emit(base="dense", M=M, merged=True)
    for dtype in ("bf16", "fp16"):
        for M in (75, 2048, 16640):
            for cache in (False, True):
                emit(dtype=dtype, M=M, cache_dense=cache, route="fused")
    emit(base="dense", route="fused")
    emit(route="fused", lora_dropout=0.05)
    for M in (2048, 16640):
        emit(base="dense", M=M, dense_lora_gemm=False)
    emit(device="cpu")
    emit(device="cpu", merged=True)
    emit(device="cpu", base="dense")
    emit(device="cpu", base="dense", dtype="fp32", M=75)
    # the qkv projection of an attention sub-layer (q and v adapted: rank 16) asking for the RoPE epilogue
    for M in (16640, 2048):
        emit(M=M, rank=16, rope_shape=ROPE[M])
    big = dict(M=16640, rank=16, rope_shape=ROPE[16640])
    emit(cache_dense=True, **big)
    emit(route="fused", **big)
    emit(route="fused", cache_dense=True, **big)
    emit(base="dense", **big)
    emit(base="dense", dense_lora_gemm=False, **big)
    emit(gemm_rope=False, **big)
    emit(lora_dropout=0.05, **big)
    return out


def answer(row):
    """the plan's answer for one row, as the JSON holds it"""
    import torch
    from fastmax_experiments_amd import lora
    saved = lora.QLORA_ROUTE, lora.DENSE_LORA_GEMM, lora.GEMM_ROPE
    lora.QLORA_ROUTE, lora.DENSE_LORA_GEMM, lora.GEMM_ROPE = row["route"], row["dense_lora_gemm"], row["gemm_rope"]
    try:
        plan = lora.qlora_plan("dense" if row["base"].startswith("dense") else row["base"], row["device"],
                               {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[row["dtype"]],
                               row["M"], K, N, rank=row["rank"], drop_p=row["lora_dropout"] if row["training"] else 0.0,
                               cache_dense=row["cache_dense"], lora_enabled=not row["merged"],
                               bias_trains=row["base"] == "dense_bias_trains", rope_shape=row["rope_shape"])
        return plan._asdict()
    except (RuntimeError, NotImplementedError) as e:
        return {"raises": type(e).__name__}
    finally:
        lora.QLORA_ROUTE, lora.DENSE_LORA_GEMM, lora.GEMM_ROPE = saved


def dumps(rows_, answers):
    """one row per line: small and diffable"""
    js = lambda x: json.dumps(x, separators=(",", ":"))          # noqa: E731
    return "[\n" + ",\n".join(js({"args": r, "plan": a}) for r, a in zip(rows_, answers)) + "\n]\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite tests/golden/qlora_routes.json")
    args = ap.parse_args()
    text = dumps(rows(), [answer(r) for r in rows()])
    if args.write:
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(f"{GOLDEN}: {len(text)} bytes")
    else:
        sys.stdout.write(text)
