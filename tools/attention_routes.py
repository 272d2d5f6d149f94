"""Record which route a linearmax call and the attention sub-layer take: for a grid of plain-data arguments the answer of
fastmax_hack.linearmax_plan (operator rows) and of CausalSelfAttention.plan (block rows), or the exception they raise.

    python tools/attention_routes.py            # prints the table (the plans' answers; no device needed)
    python tools/attention_routes.py --write    # rewrites tests/golden/attention_routes.json from the plans' answers
    python tools/attention_routes.py --record FILE   # MI355X: runs every row and writes what was OBSERVED to run to FILE

tests/test_attention_routes_cpu.py compares the plans against the committed file row by row.  The committed answers were
recorded with --record before the plans existed: a row that differs is a bug in the plan, not a reason to rewrite the file.

--record wraps the entry points the routes go through and turns what it saw into the plan record:
    operator      ops.linearmax_forward_fused answered a train=False call -> "fused_forward"; a train=True call -> "one_node";
                  else ops.forward ran with causal=False -> "unmasked", with causal=True -> "two_node"
    prologue      "in_scan" with the two operators above; else ops.normalize_cast answered -> "cast"; ops.normalize ran -> "f32"
    prologue_bwd  the ``fuse`` bits ops.linearmax_backward was given: 3 -> "both", 2 -> "q"; it never ran -> "none"
    k_layout      the ``rep`` ops.normalize_cast was given (> 1: "group_copies"), else how K was handed over: at its groups
                  beside (B*G, rep, N, D) queries -> "group_views", else "per_head"
    slices        how many times the operator's forward entry point ran
    qkv           lora.hip_gemm_rope ran -> "gemm_epilogue"; ops.RopeQKVSplit.forward ran -> "hip_pass"; else "eager"
    kv_layout     the ``expand`` RopeQKVSplit.forward was given / the last entry of the ``rope`` tuple the qkv projection was
                  given; on the eager route K, V are repeated per query head: KV_COPIES
    operator (block)  attention_block.fastmax ran -> "fastmax", else the operator record above
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_routes.json")
OP = dict(kind="op", device="cuda", dtype="bf16", B=1, H=2, N=512, D=64, p=1, mask=True, grad=True, rep=1, views=False,
          fused_training=True)
# 256 wide, 8 heads of 32: the block of tests/test_block_gpu.py; T = 75 keeps every linear on the few-rows kernels
BLOCK = dict(kind="block", alg="linearmax", groups=2, dtype="bf16", B=2, T=75, grad=True, input_pos=False, rotary=1.0,
             fused_neighbours=True, group_views=True, gemm_rope=True, grouped_k=True)
DS = [16, 32, 36, 40, 64, 72, 128, 136, 256]
NS = [17, 511, 512, 700]


def rows():
    """the thinned cross product: every dtype, head size and length with and without gradients; mask and p where they change
    the operator; grouped heads as views and as copies; the switches; then the block with each input that moves its plan"""
    out = []

    def emit(base, **kw):
        row = dict(base, **kw)
        if row not in out:
            out.append(row)

    for dtype in ("bf16", "fp16", "fp32"):
        for D in DS:
            for N in NS:
                for grad in (True, False):
                    emit(OP, dtype=dtype, D=D, N=N, grad=grad)
    for D in (16, 40, 64, 128, 136):
        for grad in (True, False):
            emit(OP, dtype="fp64", D=D, grad=grad)
    for dtype in ("bf16", "fp32"):
        for D in (40, 64, 136):
            for grad in (True, False):
                emit(OP, dtype=dtype, D=D, N=130, mask=False, grad=grad)
                emit(OP, dtype=dtype, D=D, p=2, grad=grad)
    emit(OP, dtype="fp64", N=130, mask=False)
    emit(OP, D=264)                                                     # past FASTMAX_MAX_D: raises before anything is launched
    emit(OP, D=264, grad=False)
    emit(OP, device="cpu")
    emit(OP, device="cpu", grad=False)
    emit(OP, B=3, H=30000, N=16, D=16, grad=False)                      # B H > 65535: batch slices
    for views in (True, False):
        for dtype in ("bf16", "fp32"):
            for N in (511, 640):
                for D in (64, 128):
                    emit(OP, dtype=dtype, B=2, H=8, rep=4, views=views, N=N, D=D)
        emit(OP, B=2, H=8, rep=4, views=views, N=640, p=2)
        emit(OP, B=2, H=8, rep=4, views=views, N=640, fused_training=False)
    for dtype in ("bf16", "fp32"):
        for N in (512, 700):
            emit(OP, dtype=dtype, N=N, fused_training=False)
    for alg in ("linearmax", "fastmax"):
        for groups in (2, 8):
            for grad in (True, False):
                emit(BLOCK, alg=alg, groups=groups, grad=grad)
            emit(BLOCK, alg=alg, groups=groups, input_pos=True, grad=False)
        emit(BLOCK, alg=alg, rotary=0.25)                                   # 8 of 32 dims: not whole 16-byte pieces per half
        for switch in ("fused_neighbours", "group_views", "gemm_rope"):
            emit(BLOCK, alg=alg, **{switch: False})
        emit(BLOCK, alg=alg, dtype="fp32")
        # training-size rows: the smallest shape at which the QLoRA plan allows the qkv + RoPE epilogue (tools/qlora_routes.py)
        emit(BLOCK, alg=alg, B=5, T=3328)
    emit(BLOCK, grouped_k=False)
    emit(BLOCK, T=640)
    emit(BLOCK, T=640, group_views=False)
    emit(BLOCK, B=5, T=3328, gemm_rope=False)
    emit(BLOCK, B=5, T=3328, group_views=False)
    emit(BLOCK, B=5, T=3328, groups=8)
    emit(BLOCK, B=5, T=3328, grad=False)
    return out


def _dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "fp64": torch.float64}[name]


def _block(row):
    import torch
    from fastmax_experiments_amd import attention_block as ab
    torch.manual_seed(0)
    blk = ab.CausalSelfAttention(256, 8, n_query_groups=row["groups"], rotary_percentage=row["rotary"], attn_alg=row["alg"])
    blk.quantize_base()
    blk.fused_neighbours, blk.group_views, blk.gemm_rope = row["fused_neighbours"], row["group_views"], row["gemm_rope"]
    return blk


class _Input:
    """stands for the block's input where no device exists: what CausalSelfAttention.plan reads of x, nothing else"""

    def __init__(self, shape, dtype, requires_grad):
        import torch
        self.shape, self.dtype, self.requires_grad, self.device = torch.Size(shape), dtype, requires_grad, torch.device("cuda")

    def size(self):
        return self.shape

    def numel(self):
        return self.shape.numel()


def _plan_dict(plan):
    return {k: (_plan_dict(v) if hasattr(v, "_asdict") else v) for k, v in plan._asdict().items()}


def answer(row):
    """the plan's answer for one row, as the JSON holds it"""
    import importlib
    import torch
    fh = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax_hack")
    saved = fh.FUSED_TRAINING, fh.GROUPED_K
    try:
        if row["kind"] == "op":
            fh.FUSED_TRAINING = row["fused_training"]
            G = row["H"] // row["rep"]
            B, H = (row["B"] * G, row["rep"]) if row["views"] else (row["B"], row["H"])
            plan = fh.linearmax_plan(_dtype(row["dtype"]), B, H, row["N"], row["N"], row["D"], p=row["p"], mask=row["mask"],
                                     needs_grad=row["grad"], rep=row["rep"], views=row["views"])
        else:
            fh.GROUPED_K = row["grouped_k"]
            blk = _block(row)
            x = _Input((row["B"], row["T"], 256), _dtype(row["dtype"]), row["grad"])
            with torch.set_grad_enabled(row["grad"]):
                plan = blk.plan(x, 0 if row["input_pos"] else None)
        return _plan_dict(plan)
    except (RuntimeError, NotImplementedError) as e:
        return {"raises": type(e).__name__}
    finally:
        fh.FUSED_TRAINING, fh.GROUPED_K = saved


def record(row):
    """run the row on the device and say what ran (see the module docstring for which observation gives which field)"""
    import importlib
    import torch
    from fastmax_experiments_amd import attention_block as ab, lora, ops
    fh = importlib.import_module("fastmax_experiments_amd.attention_mechanisms.fastmax_hack")
    seen = dict(fused=0, train=0, unmasked=0, masked=0, cast=0, cast_rep=1, f32=0, fuse=None, hip_pass=None, gemm=None,
                fastmax=0)
    saved = []

    def wrap(owner, name, before=None, after=None, static=False):
        f = getattr(owner, name)
        saved.append((owner, name, owner.__dict__[name] if static else f))

        def g(*a, **kw):
            if before:
                before(*a, **kw)
            r = f(*a, **kw)
            if after:
                after(r, *a, **kw)
            return r
        setattr(owner, name, staticmethod(g) if static else g)

    def fused_after(r, q, k, v, return_stats=False, train=False):
        if r is not None:
            seen["train" if train else "fused"] += 1

    def cast_after(r, x, rep=1):
        if r is not None:
            seen["cast"] += 1
            seen["cast_rep"] = max(seen["cast_rep"], rep)

    def fwd_before(q, k, v, p, causal, *a, **kw):
        seen["masked" if causal else "unmasked"] += 1

    wrap(ops, "linearmax_forward_fused", after=fused_after)
    wrap(ops, "normalize_cast", after=cast_after)
    wrap(ops, "normalize", before=lambda x: seen.__setitem__("f32", seen["f32"] + 1))
    wrap(ops, "forward", before=fwd_before)
    wrap(ops, "linearmax_backward", before=lambda *a, **kw: seen.__setitem__("fuse", kw.get("fuse", 0)))
    wrap(ops.RopeQKVSplit, "forward", before=lambda ctx, qkv, cos, sin, n, expand=1: seen.__setitem__("hip_pass", int(expand)),
         static=True)
    wrap(lora, "hip_gemm_rope", before=lambda *a, **kw: seen.__setitem__("gemm", True))
    wrap(lora, "qlora_linear_thin", before=lambda x, base, A, ebt, rope=None, *a, **kw:
         seen.__setitem__("gemm_layout", None if rope is None else int(rope[-1])))
    wrap(ab, "fastmax", before=lambda *a, **kw: seen.__setitem__("fastmax", 1))
    switches = fh.FUSED_TRAINING, getattr(fh, "GROUPED_K", None), os.environ.get("FASTMAX_GROUPED_K")
    views = False
    try:
        g = torch.Generator().manual_seed(0)
        if row["kind"] == "op":
            fh.FUSED_TRAINING = row["fused_training"]
            dt, B, H, N, D, rep = _dtype(row["dtype"]), row["B"], row["H"], row["N"], row["D"], row["rep"]
            G = H // rep
            views = row["views"] and rep > 1
            q = torch.randn((B * G, rep, N, D) if views else (B, H, N, D), generator=g).to(dt)
            k = torch.randn(B, G, N, D, generator=g).to(dt)
            v = torch.randn(B, G, N, D, generator=g).to(dt)
            q, k, v = (t.to(row["device"]).requires_grad_(row["grad"]) for t in (q, k, v))
            with torch.set_grad_enabled(row["grad"]):
                if rep > 1:
                    vv = v.view(B * G, 1, N, D).expand(B * G, rep, N, D) if views else v.repeat_interleave(rep, dim=1)
                    o = fh.fastmax_hack_grouped(q, k, vv, rep, p=row["p"])
                else:
                    o = fh.fastmax_hack(q, k, v, p=row["p"], mask=row["mask"])
                if row["grad"]:
                    o.float().sum().backward()
        else:
            if hasattr(fh, "GROUPED_K"):
                fh.GROUPED_K = row["grouped_k"]
            os.environ["FASTMAX_GROUPED_K"] = "1" if row["grouped_k"] else "0"          # read per call before GROUPED_K existed
            blk = _block(row).cuda()
            dt, B, T = _dtype(row["dtype"]), row["B"], row["T"]
            cos, sin = ab.build_rope_cache(T, blk.rope_n_elem, device="cuda")
            x = torch.randn(B, T, 256, generator=g).to(dt).cuda().requires_grad_(row["grad"])
            with torch.set_grad_enabled(row["grad"]):
                y = blk(x, cos, sin, torch.arange(T, device="cuda") if row["input_pos"] else None)
                if row["grad"]:
                    y.float().sum().backward()
        torch.cuda.synchronize()
    except (RuntimeError, NotImplementedError) as e:
        if "HIP error" in str(e) or "illegal" in str(e):          # a device error is no answer of the route: stop here
            raise
        return {"raises": type(e).__name__}
    finally:
        for owner, name, f in saved:
            setattr(owner, name, f)
        fh.FUSED_TRAINING = switches[0]
        if switches[1] is not None:
            fh.GROUPED_K = switches[1]
        if switches[2] is None:
            os.environ.pop("FASTMAX_GROUPED_K", None)
        else:
            os.environ["FASTMAX_GROUPED_K"] = switches[2]

    def operator():
        if seen["fused"] or seen["train"]:
            kind, prologue = ("fused_forward" if seen["fused"] else "one_node"), "in_scan"
        else:
            kind, prologue = ("unmasked" if seen["unmasked"] else "two_node"), ("f32" if seen["f32"] else "cast")
        if row["kind"] == "block":
            hp, gl = seen["hip_pass"], seen.get("gemm_layout")
            layout = {2: "group_copies", 4: "group_views"}.get(hp if hp is not None else gl, "per_head")
        else:
            layout = "group_copies" if seen["cast_rep"] > 1 else ("group_views" if views else "per_head")
        return dict(operator=kind, prologue=prologue, prologue_bwd={None: "none", 3: "both", 2: "q"}[seen["fuse"]],
                    k_layout=layout, slices=seen["fused"] + seen["train"] + seen["unmasked"] + seen["masked"])

    if row["kind"] == "op":
        return operator()
    if seen["gemm"]:
        qkv, layout = "gemm_epilogue", seen["gemm_layout"]
    elif seen["hip_pass"] is not None:
        qkv, layout = "hip_pass", seen["hip_pass"]
    else:
        qkv, layout = "eager", 1
    return dict(qkv=qkv, kv_layout=layout, operator="fastmax" if seen["fastmax"] else operator())


def dumps(rows_, answers):
    """one row per line: small and diffable"""
    js = lambda x: json.dumps(x, separators=(",", ":"))          # noqa: E731
    return "[\n" + ",\n".join(js({"args": r, "plan": a}) for r, a in zip(rows_, answers)) + "\n]\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite tests/golden/attention_routes.json from the plans")
    ap.add_argument("--record", metavar="FILE", help="run every row on the device and write what ran to FILE")
    args = ap.parse_args()
    if args.record:
        text = dumps(rows(), [record(r) for r in rows()])
        with open(args.record, "w") as f:
            f.write(text)
        print(f"{args.record}: {len(rows())} rows")
    else:
        text = dumps(rows(), [answer(r) for r in rows()])
        if args.write:
            with open(GOLDEN, "w") as f:
                f.write(text)
            print(f"{GOLDEN}: {len(text)} bytes")
        else:
            sys.stdout.write(text)
