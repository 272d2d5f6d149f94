"""Record what the host side of libfastmax_hip.so decides, without a GPU: for a grid of problems the selected path, the
workspace sizes, the kept-state bytes and the linearmax-train coverage, and for argument sets that are rejected before any
launch the return code of every entry point of csrc/fastmax_api.hip.

    python tools/dispatch_table.py            # prints the table
    python tools/dispatch_table.py --write    # rewrites tests/golden/dispatch_table.json

tests/test_dispatch_table_cpu.py compares the library against the committed file row by row.  All calls are plain host
arithmetic: the pointers are made-up addresses that are never dereferenced, and no case passes validation and reaches a launch.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from fastmax_experiments_amd import _lib  # noqa: E402
from fastmax_experiments_amd._lib import Problem, F32, BF16, F16  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")
COLUMNS = ["B", "H", "Nq", "Nk", "D", "in_dtype", "out_dtype", "p", "causal", "path",
           "select_path", "forward_workspace", "backward_workspace", "linearmax_forward_auto_workspace",
           "linearmax_train_supported", "state_bytes", "state_bytes_q_plus_8", "state_bytes_k_stride_plus_8",
           "state_bytes_o_plus_8"]

BH = {1: (1, 1), 8: (2, 4), 64: (4, 16), 512: (8, 64)}
NS = [1, 15, 16, 64, 257, 448, 512, 4096, 16384, 20001]
UNEQUAL = [(1, 4096), (8, 64), (15, 257), (63, 512), (64, 512), (64, 511), (512, 64), (16, 16384)]      # unmasked Nq != Nk
DS = [8, 50, 64, 72, 128, 136, 256]                      # 264 > FASTMAX_MAX_D: a few rows of its own below
DTYPES = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)]
PATHS = [0, 1, 2, 3, 4]
ADDR = {"q": 0x10000000, "k": 0x20000000, "v": 0x30000000, "o": 0x40000000, "go": 0x50000000, "dq": 0x60000000,
        "dk": 0x70000000, "dv": 0x80000000, "ws": 0x90000000, "g": 0xA0000000, "x": 0xB0000000, "y": 0xC0000000,
        "inv": 0xD0000000, "inv2": 0xD1000000, "st": 0xE0000000}


def problems():
    """the thinned cross product: every dtype pair, head size and length everywhere; B*H and the forced paths where they
    can change an answer (B*H: the sequence split of the p=1 scans, N >= 512)"""
    seen = set()

    def emit(bh, nq, nk, d, dts, p, causal, path):
        key = (bh, nq, nk, d, dts, p, causal, path)
        if key not in seen:
            seen.add(key)
            return [key]
        return []

    out = []
    for d in DS:
        for dts in DTYPES:
            same = dts[0] == dts[1]
            # p = 1 masked: the scans
            for n in NS:
                for path in (0, 3):
                    for bh in (BH if (n >= 512 and same) else (8,)):
                        out += emit(bh, n, n, d, dts, 1, 1, path)
                if n in (1, 16, 257, 512, 20001):
                    for path in (1, 2, 4):
                        out += emit(8, n, n, d, dts, 1, 1, path)
            # p = 1 unmasked
            for nq, nk in [(n, n) for n in NS] + UNEQUAL:
                for path in (PATHS if dts == (F32, F32) else (0,)):
                    out += emit(8, nq, nk, d, dts, 1, 0, path)
                if nk >= 512 and nq >= 64 and dts[1] == F32 and dts[0] != F16:
                    for bh in (1, 64, 512):
                        out += emit(bh, nq, nk, d, dts, 1, 0, 0)
            # p = 2
            for n in (1, 15, 16, 257, 4096, 20001):
                for path in (PATHS if dts == (F32, F32) else (0,)):
                    out += emit(8, n, n, d, dts, 2, 1, path)
                    out += emit(8, n, n, d, dts, 2, 0, path)
            for nq, nk in UNEQUAL[:6]:
                for path in (PATHS if dts == (F32, F32) else (0,)):
                    out += emit(8, nq, nk, d, dts, 2, 0, path)
    for p in (1, 2):
        for causal in (0, 1):
            for path in PATHS:
                out += emit(8, 512, 512, 264, (F32, F32), p, causal, path)
    return out


def strides(h, n, d, bump=0):
    return (ctypes.c_int64 * 3)(h * n * d, n * d, d + bump)


def row(L, key):
    bh, nq, nk, d, (idt, odt), p, causal, path = key
    b, h = BH[bh]
    prob = Problem(b, h, nq, nk, d, idt, odt, p, causal, 1.0, 0.5, float(nq), path)
    pr = ctypes.byref(prob)
    es = 4 if idt == F32 else 2

    def state_bytes(dq=0, dstride=0, do=0):
        return L.fastmax_hip_forward_state_bytes(pr, ADDR["q"] + dq, strides(h, nq, d), ADDR["k"], strides(h, nk, d, dstride),
                                                 ADDR["v"], strides(h, nk, d), ADDR["o"] + do)

    return [b, h, nq, nk, d, idt, odt, p, causal, path,
            L.fastmax_hip_select_path(pr), L.fastmax_hip_forward_workspace(pr), L.fastmax_hip_backward_workspace(pr),
            L.fastmax_hip_linearmax_forward_auto_workspace(pr), L.fastmax_hip_linearmax_train_supported(pr),
            state_bytes(), state_bytes(dq=8), state_bytes(dstride=8 // es), state_bytes(do=8)]


def rejected(L):
    """[entry point, what is wrong, return code] for calls that never reach a launch"""
    out = []

    def prob(B=1, H=2, Nq=512, Nk=None, D=64, idt=F32, odt=None, p=1, causal=1, path=0):
        return Problem(B, H, Nq, Nq if Nk is None else Nk, D, idt, idt if odt is None else odt, p, causal, 1.0, 0.5, 0.0, path)

    def attn_args(pb, bad):
        """the operands shared by the attention entry points; `bad` names what is wrong: 'null:<x>', '<x>+8' (address),
        '<x>_stride+8' (row stride)"""
        es = 4 if pb.in_dtype == F32 else 2
        a = {}
        for name, n in (("q", pb.Nq), ("k", pb.Nk), ("v", pb.Nk), ("go", pb.Nq)):
            a[name] = ADDR[name] + (8 if bad == name + "+8" else 0)
            a[name + "_s"] = strides(pb.H, n, pb.D, 8 // es if bad == name + "_stride+8" else 0)
        for name in ("o", "dq", "dk", "dv", "g", "inv", "inv2", "st"):
            a[name] = ADDR[name] + (8 if bad == name + "+8" else 0)
        if bad.startswith("null:"):
            a[bad[5:]] = None
        return a

    def fwd(pb, bad="", ws=None, wsb=0):
        a = attn_args(pb, bad)
        return L.fastmax_hip_forward(None if bad == "null:prob" else ctypes.byref(pb), a["q"], a["q_s"], a["k"], a["k_s"], a["v"],
                                     a["v_s"], a["o"], a["g"], ws, wsb, None)

    def bwd(pb, bad="", ws=None, wsb=0, states=True):
        a = attn_args(pb, bad)
        pr = None if bad == "null:prob" else ctypes.byref(pb)
        args = [pr, a["q"], a["q_s"], a["k"], a["k_s"], a["v"], a["v_s"], a["o"], a["g"], a["go"], a["go_s"], a["dq"], a["dk"],
                a["dv"], ws, wsb]
        if states:
            return L.fastmax_hip_backward_with_states(*args, a["st"], 1 << 30, None)
        return L.fastmax_hip_backward(*args, None)

    def lm_fwd(pb, bad="", ws=None, wsb=0, auto=False):
        a = attn_args(pb, bad)
        pr = None if bad == "null:prob" else ctypes.byref(pb)
        if auto:
            return L.fastmax_hip_linearmax_forward_auto(pr, a["q"], a["q_s"], a["k"], a["k_s"], a["v"], a["v_s"], a["inv"], a["inv2"],
                                                        None, None, a["o"], a["g"], ws, wsb, None)
        return L.fastmax_hip_linearmax_forward(pr, a["q"], a["q_s"], a["k"], a["k_s"], a["v"], a["v_s"], a["inv"], a["inv2"], a["o"],
                                               a["g"], ws, wsb, None)

    def lm_bwd(pb, bad="", ws=None, wsb=0):
        a = attn_args(pb, bad)
        pr = None if bad == "null:prob" else ctypes.byref(pb)
        return L.fastmax_hip_linearmax_backward(pr, a["q"], a["q_s"], a["k"], a["k_s"], a["v"], a["v_s"], a["o"], a["g"], a["go"],
                                                a["go_s"], a["inv"], a["inv2"], None, None, a["dq"], a["dk"], a["dv"], ws, wsb,
                                                a["st"], 1 << 30, 0, None)

    bad_problems = [("p=3", prob(p=3)), ("D=264", prob(D=264)), ("B=0", prob(B=0)), ("causal Nq!=Nk", prob(Nq=512, Nk=64)),
                    ("B*H>65535", prob(B=256, H=256)), ("in_dtype=3", prob(idt=3, odt=0)), ("out_dtype=-1", prob(odt=-1))]
    calls = [("fastmax_hip_forward", fwd), ("fastmax_hip_backward_with_states", bwd),
             ("fastmax_hip_backward", lambda pb, bad="", **kw: bwd(pb, bad, states=False, **kw)),
             ("fastmax_hip_linearmax_forward", lm_fwd),
             ("fastmax_hip_linearmax_forward_auto", lambda pb, bad="", **kw: lm_fwd(pb, bad, auto=True, **kw)),
             ("fastmax_hip_linearmax_backward", lm_bwd)]
    for name, f in calls:
        is_bwd = "backward" in name
        is_lm = "linearmax" in name
        out.append([name, "null:prob", f(prob(), "null:prob")])
        for label, pb in bad_problems:
            out.append([name, label, f(pb)])
        nullable = ["q", "k", "v", "o", "q_s", "k_s", "v_s"] + (["g", "go", "go_s", "dq", "dk", "dv"] if is_bwd else []) + \
                   (["inv", "inv2"] if is_lm else [])
        for x in nullable:
            out.append([name, "null:" + x, f(prob(), "null:" + x)])
        # a workspace that is missing or one byte short, for a problem of every kernel family that needs one
        ws_cases = [("split f32 D=64", prob()), ("split bf16 D=128", prob(D=128, idt=BF16)), ("split f32 D=128", prob(D=128)),
                    ("split f16 D=64", prob(idt=F16))]
        if not is_lm:
            ws_cases.append(("unmasked linear", prob(Nq=64, Nk=512, causal=0)))
        if is_bwd and not is_lm:
            ws_cases += [("forced quadratic", prob(path=1)), ("p=2 N=256", prob(Nq=256, p=2)), ("p=2 N=64", prob(Nq=64, p=2)),
                         ("p=1 N=64", prob(Nq=64)), ("D=256 bf16", prob(D=256, idt=BF16)), ("D=256 f32", prob(D=256)),
                         ("misaligned q", None)]
        for label, pb in ws_cases:
            if label == "misaligned q":
                out.append([name, "workspace null, " + label, f(prob(), "q+8")])
                continue
            if is_lm and is_bwd and not L.fastmax_hip_linearmax_train_supported(ctypes.byref(pb)):
                out.append([name, "not covered: " + label, f(pb)])
                continue
            out.append([name, "workspace null, " + label, f(pb)])
            if name == "fastmax_hip_linearmax_forward_auto":
                need = L.fastmax_hip_linearmax_forward_auto_workspace(ctypes.byref(pb))
            elif is_bwd:
                need = 0          # backward_workspace is the maximum over the families: one byte less could still launch
            else:
                need = L.fastmax_hip_forward_workspace(ctypes.byref(pb))
            if need:
                out.append([name, "workspace one byte short, " + label, f(pb, ws=ADDR["ws"], wsb=need - 1)])
        if is_lm:
            for label, pb in (("p=2", prob(p=2)), ("unmasked", prob(causal=0)), ("D=50", prob(D=50)), ("D=136", prob(D=136)),
                              ("bf16 in, f32 out", prob(idt=BF16, odt=F32))):
                out.append([name, "not covered: " + label, f(pb)])
            bads = ["q+8", "k+8", "v+8", "o+8", "q_stride+8", "k_stride+8", "v_stride+8"]
            if is_bwd:
                bads += ["go+8", "go_stride+8", "dq+8", "dk+8", "dv+8"]
            for bad in bads:
                out.append([name, bad, f(prob(), bad, ws=ADDR["ws"], wsb=1 << 40)])
    # fastmax_hip_forward: forced paths
    for label, pb in (("forced recurrent, p=2", prob(p=2, path=2)), ("forced mfma, D=256", prob(D=256, path=3)),
                      ("forced recurrent, D=256", prob(D=256, path=2)), ("forced quadratic_mfma, D=50", prob(D=50, path=4)),
                      ("forced mfma, unmasked short", prob(Nq=16, Nk=16, causal=0, path=3)), ("forced mfma, D=50", prob(D=50, path=3))):
        out.append(["fastmax_hip_forward", label, fwd(pb)])
    for pb_label, pb in (("forced mfma", prob(path=3)), ("forced quadratic_mfma p=2", prob(p=2, path=4)),
                         ("forced mfma unmasked linear", prob(Nq=64, Nk=512, causal=0, path=3))):
        for bad in ("q+8", "k+8", "v+8", "o+8", "q_stride+8", "k_stride+8", "v_stride+8"):
            out.append(["fastmax_hip_forward", pb_label + ", " + bad, fwd(pb, bad, ws=ADDR["ws"], wsb=1 << 40)])

    # the linearmax prologue family
    B, H, N, D = 2, 4, 300, 64
    xs = strides(H, N, D)
    x, y, inv, inv2, ws = ADDR["x"], ADDR["y"], ADDR["inv"], ADDR["inv2"], ADDR["ws"]
    big = 1 << 40
    shapes = [("B=0", (0, H, N, D)), ("H=0", (B, 0, N, D)), ("N=0", (B, H, 0, D)), ("D=0", (B, H, N, 0)), ("D=257", (B, H, N, 257))]

    def fam(name, call, nulls, need, extra=()):
        """call(ptrs: dict, dims, ws, wsb) -> rc"""
        ptrs = dict(x=x, xs=xs, y=y, inv=inv, x1=ADDR["k"], x1s=xs, inv1=inv2, gy=ADDR["go"], gx=ADDR["dq"])
        for nm in nulls:
            out.append([name, "null:" + nm, call(dict(ptrs, **{nm: None}), (B, H, N, D), ws, big)])
        for label, dims in list(shapes) + list(extra):
            out.append([name, label, call(ptrs, dims, ws, big)])
        out.append([name, "workspace null", call(ptrs, (B, H, N, D), None, big)])
        out.append([name, "workspace one byte short", call(ptrs, (B, H, N, D), ws, need - 1)])

    fam("fastmax_hip_normalize", lambda p, d, w, wb: L.fastmax_hip_normalize(p["x"], p["xs"], F32, p["y"], p["inv"], *d, w, wb, None),
        ["x", "xs", "y"], L.fastmax_hip_normalize_workspace(B, H))
    fam("fastmax_hip_normalize_stats", lambda p, d, w, wb: L.fastmax_hip_normalize_stats(p["x"], p["xs"], F32, p["inv"], *d, w, wb, None),
        ["x", "xs", "inv"], L.fastmax_hip_normalize_workspace(B, H))
    fam("fastmax_hip_normalize_stats2",
        lambda p, d, w, wb: L.fastmax_hip_normalize_stats2(p["x"], p["xs"], p["x1"], p["x1s"], F32, p["inv"], p["inv1"], *d, w, wb, None),
        ["x", "xs", "x1", "x1s", "inv", "inv1"], L.fastmax_hip_normalize_stats2_workspace(B, H, N), [("B*H>65535", (256, 256, N, D))])
    fam("fastmax_hip_normalize_cast", lambda p, d, w, wb: L.fastmax_hip_normalize_cast(p["x"], p["xs"], F32, p["y"], p["inv"], *d, w, wb, None),
        ["x", "xs", "y", "inv"], L.fastmax_hip_normalize_workspace(B, H))
    out.append(["fastmax_hip_normalize_cast", "dtype=3", L.fastmax_hip_normalize_cast(x, xs, 3, y, inv, B, H, N, D, ws, big, None)])
    out.append(["fastmax_hip_normalize_cast", "dtype=-1", L.fastmax_hip_normalize_cast(x, xs, -1, y, inv, B, H, N, D, ws, big, None)])
    fam("fastmax_hip_normalize_backward",
        lambda p, d, w, wb: L.fastmax_hip_normalize_backward(p["x"], p["xs"], F32, p["gy"], p["inv"], p["gx"], *d, w, wb, None),
        ["x", "xs", "gy", "inv", "gx"], L.fastmax_hip_normalize_backward_workspace(B, H, N))
    rep = 3

    def expand_dims(d):
        return (d[0], d[1], rep, d[2], d[3])

    fam("fastmax_hip_normalize_cast_expand",
        lambda p, d, w, wb: L.fastmax_hip_normalize_cast_expand(p["x"], p["xs"], F32, p["y"], p["inv"], *expand_dims(d), w, wb, None),
        ["x", "xs", "y", "inv"], 4 * B * H * ((N + 255) // 256))
    out.append(["fastmax_hip_normalize_cast_expand", "rep=0", L.fastmax_hip_normalize_cast_expand(x, xs, F32, y, inv, B, H, 0, N, D, ws, big, None)])
    out.append(["fastmax_hip_normalize_cast_expand", "dtype=3", L.fastmax_hip_normalize_cast_expand(x, xs, 3, y, inv, B, H, rep, N, D, ws, big, None)])
    fam("fastmax_hip_normalize_backward_expand",
        lambda p, d, w, wb: L.fastmax_hip_normalize_backward_expand(p["x"], p["xs"], F32, p["gy"], p["inv"], p["gx"], *expand_dims(d), w, wb, None),
        ["x", "xs", "gy", "inv", "gx"], B * H * ((N + 85) // 86) * 12 + 16)          # rep = 3: blocks of ceil(256 / 3) = 86 tokens
    out.append(["fastmax_hip_normalize_backward_expand", "rep=0",
                L.fastmax_hip_normalize_backward_expand(x, xs, F32, ADDR["go"], inv, ADDR["dq"], B, H, 0, N, D, ws, big, None)])
    # host-only size queries of the family
    for b, h, n in ((1, 1, 1), (2, 4, 300), (8, 64, 4096), (3, 5, 256), (3, 5, 257)):
        out.append(["fastmax_hip_normalize_workspace", f"{b},{h}", L.fastmax_hip_normalize_workspace(b, h)])
        out.append(["fastmax_hip_normalize_stats2_workspace", f"{b},{h},{n}", L.fastmax_hip_normalize_stats2_workspace(b, h, n)])
        out.append(["fastmax_hip_normalize_backward_workspace", f"{b},{h},{n}", L.fastmax_hip_normalize_backward_workspace(b, h, n)])
    return out


def table():
    L = _lib.lib()
    return {"columns": COLUMNS, "cases": [row(L, key) for key in problems()], "rejected": rejected(L)}


def dumps(t):
    """one case per line, no spaces: small and diffable"""
    js = lambda x: json.dumps(x, separators=(",", ":"))          # noqa: E731
    return ('{"columns":' + js(t["columns"]) + ',\n"cases":[\n' + ",\n".join(js(r) for r in t["cases"]) +
            '\n],\n"rejected":[\n' + ",\n".join(js(r) for r in t["rejected"]) + "\n]}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite tests/golden/dispatch_table.json")
    args = ap.parse_args()
    text = dumps(table())
    if args.write:
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(f"{GOLDEN}: {len(text)} bytes")
    else:
        sys.stdout.write(text)
