#!/usr/bin/env python3
"""Generation-time shapes: N_q new tokens against N_k cached keys (unmasked, lit_gpt/model.py:464-466), and the opt-in
decode state caches (p=1 and p=2).  Markdown to stdout.  `--p2`: the second-order rows only.
`--extend`: multi-token continuation of the second-order cache (`extend`, `prefill(chunk=C)`), all rows, event times.
`--extend-case B,H,Hkv,D,T` and `--prefill-case B,H,N,D,C` (C = 0: the one-shot prefill) run ONE row, for a
`rocprofv3 --kernel-trace --stats` run whose per-kernel totals then belong to that row alone.
`--block`: per-token time of the attention block generating on the second-order cache (`forward(..., state=...)`), the fused
step beside the two-launch route (split + step), eager and as a HIP graph replay (`--no-graph`: eager only).
`--block-case NAME,B,FUSED` runs ONE arm eagerly for a kernel trace (NAME: a key of attention_block.CONFIG_SHAPES).
`--linearmax`: per-token time of `LinearmaxDecodeState.step` after 512- and 16384-token prompts, beside the masked linearmax
forward over the whole prefix (the only route without the cache) and the second-order cache's step.
`--kv`: one step of the KV-cache decode route (`FastmaxKVDecodeState`) against one p=2 state step, both replayed from a graph and
alternating in one process, at TinyLlama, Llama-2-7b and Gemma-2b head shapes, bf16, B 1 and 8, lengths 512 .. 32768.
`--kv-trace ORDER.json` runs the same cells eagerly under `rocprofv3 --kernel-trace --stats`; `--kv-trace-table DIR ORDER.json`
turns that trace into per-kernel times and bytes/s on the live cache prefix."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from attention_mechanisms.fastmax import fastmax
from fastmax_experiments_amd.decode import FastmaxDecodeState


def timeit(fn, iters=20, rounds=5):
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


import ctypes
from fastmax_experiments_amd import _lib, ops


def bench_p2():
    """Second-order decode state cache (FastmaxDecodeState(p=2)): step time rotating over enough independent states (one per
    layer of a 22-layer model, more when that is under 512 MiB) that the step streams HBM and not the 256 MiB Infinity Cache,
    beside the unmasked p=2 call over a 4096-token KV cache it replaces; prefill-state kernel beside the masked p=2 forward.
    Event times include the host side of each call: take kernel times from a rocprofv3 --kernel-trace --stats run."""
    print("| p=2 case | (B,H,Hkv,D) | states | state MB | bytes/step MB | ms/step | TB/s |")
    print("|---|---|---|---|---|---|---|")
    for B, H, Hkv, D in ((1, 32, 32, 64), (1, 32, 32, 128), (8, 32, 32, 64), (1, 32, 4, 64)):
        L = _lib.lib()
        sb = B * Hkv * (D + 1) * (D + 2) // 2 * ((D + 4) // 4 * 4) * 4           # the state proper (scratch excluded)
        full = L.fastmax_hip_p2_decode_state_bytes(B, Hkv, D)
        n = max(22, -(-(512 << 20) // full))
        states = [FastmaxDecodeState(B, H, D, device="cuda", p=2, n_query_groups=Hkv) for _ in range(n)]
        q, k, v = (torch.randn(B, h, 64, D, device="cuda").to(torch.bfloat16) for h in (H, Hkv, Hkv))
        for st in states:
            st.prefill(q, k, v)
        q1 = torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16)
        k1, v1 = (torch.randn(B, Hkv, 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))

        def steps():
            for st in states:
                st.step(q1, k1, v1)
        with torch.no_grad():
            ms = timeit(steps, iters=2, rounds=5) / n
        print(f"| decode state cache step | ({B},{H},{Hkv},{D}) | {n} | {sb / 1e6:.2f} | {2 * sb / 1e6:.2f} | {ms:.4f} | "
              f"{2 * sb / (ms * 1e-3) / 1e12:.2f} |", flush=True)
        del states
        qc = torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16)
        kc, vc = (torch.randn(B, H, 4096, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        with torch.no_grad():
            ms = timeit(lambda: fastmax(qc, kc, vc, mask=False, p=2))
        print(f"| unmasked over a 4096-token KV cache | ({B},{H},{H},{D}) | | | | {ms:.4f} | |", flush=True)
    print()
    print("| p=2 prefill | (B,H,N,D) | ms |")
    print("|---|---|---|")
    for B, H, N, D in ((1, 32, 4096, 64), (1, 32, 4096, 128)):
        q, k, v = (torch.randn(B, H, N, D, device="cuda").to(torch.bfloat16) for _ in range(3))
        st = FastmaxDecodeState(B, H, D, device="cuda", p=2)
        prob = ops._problem(k, k, k.dtype, k.dtype, 2, True, st.nt, 0.0)
        L = _lib.lib()

        def prefill_state():
            _lib.check(L.fastmax_hip_p2_prefill_state(ctypes.byref(prob), k.data_ptr(), ops._strides(k), v.data_ptr(),
                                                      ops._strides(v), st.state.data_ptr(), ops._stream(k.device)), "prefill")
        with torch.no_grad():
            ms_s = timeit(prefill_state)
            ms_f = timeit(lambda: fastmax(q, k, v, mask=True, p=2))
        print(f"| prefill-state kernel | ({B},{H},{N},{D}) | {ms_s:.4f} |", flush=True)
        print(f"| masked p=2 forward | ({B},{H},{N},{D}) | {ms_f:.4f} |", flush=True)


EXTEND_SHAPES = ((1, 32, 32, 64), (1, 32, 32, 128), (8, 32, 32, 64), (1, 32, 4, 64))
PREFILL_CASES = ((1, 32, 4096, 64), (1, 32, 16384, 64), (1, 32, 32768, 64), (1, 32, 65536, 64), (1, 32, 4096, 128), (1, 32, 32768, 128))


def _rotating_states(B, H, Hkv, D, cached=4096):
    """enough independent states to exceed the Infinity Cache (as bench_p2), each holding `cached` tokens.  The state is
    written by fastmax_hip_p2_prefill_state alone, so the setup launches none of the kernels that `extend` or `step` use."""
    L = _lib.lib()
    full = L.fastmax_hip_p2_decode_state_bytes(B, Hkv, D)
    n = max(22, -(-(512 << 20) // full))
    k, v = (torch.randn(B, Hkv, cached, D, device="cuda").to(torch.bfloat16) for _ in range(2))
    first = FastmaxDecodeState(B, H, D, device="cuda", p=2, n_query_groups=Hkv)
    prob = ops._problem(k, k, k.dtype, k.dtype, 2, True, first.nt, 0.0)
    _lib.check(L.fastmax_hip_p2_prefill_state(ctypes.byref(prob), k.data_ptr(), ops._strides(k), v.data_ptr(), ops._strides(v),
                                              first.state.data_ptr(), ops._stream(k.device)), "prefill")
    states = [first]
    for _ in range(n - 1):
        st = FastmaxDecodeState(B, H, D, device="cuda", p=2, n_query_groups=Hkv)
        st.state.copy_(first.state)
        states.append(st)
    for st in states:
        st.count = cached
    return states


def extend_case(B, H, Hkv, D, T, rounds=3):
    """-> (ms per extend(T), ms per T single steps, states, extend calls, step sequences); both rotate over the states"""
    states = _rotating_states(B, H, Hkv, D)
    n = len(states)
    q = torch.randn(B, H, T, D, device="cuda").to(torch.bfloat16)
    k, v = (torch.randn(B, Hkv, T, D, device="cuda").to(torch.bfloat16) for _ in range(2))
    q1, k1, v1 = q[:, :, :1].contiguous(), k[:, :, :1].contiguous(), v[:, :, :1].contiguous()

    def extends():
        for st in states:
            st.extend(q, k, v)

    def steps():
        for i in range(T):
            states[i % n].step(q1, k1, v1)
    with torch.no_grad():
        ms_e = timeit(extends, iters=1, rounds=rounds) / n
        ms_s = timeit(steps, iters=1, rounds=rounds)
    return ms_e, ms_s, n, n * (rounds + 1), rounds + 1


def prefill_case(B, H, N, D, C, rounds=3):
    """-> (ms per prefill, calls): C = 0 is the one-shot prefill (masked tiles + prefill-state kernel), else prefill(chunk=C)"""
    q, k, v = (torch.randn(B, H, N, D, device="cuda").to(torch.bfloat16) for _ in range(3))
    st = FastmaxDecodeState(B, H, D, device="cuda", p=2)

    def run():
        st.count = 0
        st.state.zero_()
        st.prefill(q, k, v, chunk=C or None)
    with torch.no_grad():
        return timeit(run, iters=1, rounds=rounds), rounds + 1


def bench_extend():
    """extend(T) onto 4096 cached tokens next to T single steps, then prefill(chunk=C) next to the one-shot prefill.
    Event times (they include the host side of each call, and state.zero_() in the prefill rows)."""
    print("| extend | (B,H,Hkv,D) | T | states | extend(T) ms | T steps ms | steps / extend |")
    print("|---|---|---|---|---|---|---|")
    for B, H, Hkv, D in EXTEND_SHAPES:
        for T in (8, 64, 512):
            ms_e, ms_s, n, _, _ = extend_case(B, H, Hkv, D, T)
            print(f"| extend vs steps | ({B},{H},{Hkv},{D}) | {T} | {n} | {ms_e:.4f} | {ms_s:.4f} | {ms_s / ms_e:.1f} |", flush=True)
    print()
    print("| p=2 prefill | (B,H,N,D) | one-shot ms | chunk 1024 ms | chunk 2048 ms | chunk 4096 ms |")
    print("|---|---|---|---|---|---|")
    for B, H, N, D in PREFILL_CASES:
        ms = [prefill_case(B, H, N, D, C)[0] for C in (0, 1024, 2048, 4096)]
        print(f"| one-shot vs chunked | ({B},{H},{N},{D}) | " + " | ".join(f"{x:.3f}" for x in ms) + " |", flush=True)


BLOCK_CASES = (("tiny-llama-1.1b", 22), ("Llama-2-7b-hf", 32))          # (attention_block.CONFIG_SHAPES key, layers of the model)


def _block_setup(name, n_layer, B, prompt=512):
    """the sub-layer with merged weights (no LoRA branch) on a 4-bit base, bf16 activations: one block, and one state per layer
    of the model, each holding the same `prompt` tokens -- the per-token working set of a real generation loop (the weights
    of ONE layer, though: the projections read theirs from cache more often than a full model's would, in both columns alike)."""
    from fastmax_experiments_amd.attention_block import CONFIG_SHAPES, CausalSelfAttention, build_rope_cache
    cfg = CONFIG_SHAPES[name]
    torch.manual_seed(0)
    blk = CausalSelfAttention(r=0, **cfg).to("cuda", torch.bfloat16).eval().quantize_base()
    H, G, hs = cfg["n_head"], cfg["n_query_groups"], cfg["head_size"]
    cos, sin = build_rope_cache(prompt + 1, blk.rope_n_elem, device="cuda")
    first = FastmaxDecodeState(B, H, hs, device="cuda", p=2, n_query_groups=G)
    xp = torch.randn(B, prompt, cfg["n_embd"], device="cuda").to(torch.bfloat16)
    blk(xp, cos[:prompt], sin[:prompt], None, first)
    states = [first]
    for _ in range(n_layer - 1):
        st = FastmaxDecodeState(B, H, hs, device="cuda", p=2, n_query_groups=G)
        st.state.copy_(first.state)
        st.count = first.count
        states.append(st)
    x1 = torch.randn(B, 1, cfg["n_embd"], device="cuda").to(torch.bfloat16)
    return blk, states, x1, cos[prompt:prompt + 1].contiguous(), sin[prompt:prompt + 1].contiguous()


def _block_arms(blk, states, x1, c, s):
    """-> {arm: function that runs one token through the block once per state}"""
    def tokens(fused):
        def run():
            for st in states:
                st.fused_step = fused
                blk(x1, c, s, None, st)
        return run
    return {"fused": tokens(True), "split+step": tokens(False)}


def _alternate(arms, rounds, iters):
    """`rounds` timed windows per arm, the arms alternating inside one process -> {arm: [ms per call of the arm's function]}"""
    ts = {a: [] for a in arms}
    for f in arms.values():
        f(); f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for a, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record(); torch.cuda.synchronize()
            ts[a].append(e0.elapsed_time(e1) / iters)
    return ts


def bench_block(graph=True, rounds=9):
    """Per token and layer, microseconds: median, min and spread ((max - min) / median) over `rounds` windows per arm, the two
    arms alternating.  Eager times include the host side of each call (Python, ctypes, allocator) and are bounded by it at
    these sizes; the graph rows replay the same launches without the host: they are the device-side figure."""
    print("| block decode | mode | B | layers | fused us | min | spread | split+step us | min | spread | split+step / fused |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, n_layer in BLOCK_CASES:
        for B in (1, 8):
            blk, states, x1, c, s = _block_setup(name, n_layer, B)
            arms = _block_arms(blk, states, x1, c, s)
            modes = []
            with torch.no_grad():
                modes.append(("eager", _alternate(arms, rounds, iters=5)))
                if graph:
                    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for f in arms.values():
                            f()
                    torch.cuda.current_stream().wait_stream(side)
                    replays = {}
                    for a, f in arms.items():
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            f()
                        replays[a] = g.replay
                    modes.append(("graph replay", _alternate(replays, rounds, iters=20)))
            for mode, ts in modes:
                cells = []
                for a in ("fused", "split+step"):
                    us = [t * 1e3 / n_layer for t in ts[a]]
                    med = statistics.median(us)
                    cells += [f"{med:.2f}", f"{min(us):.2f}", f"{(max(us) - min(us)) / med * 100:.1f}%"]
                ratio = statistics.median(ts["split+step"]) / statistics.median(ts["fused"])
                print(f"| {name} | {mode} | {B} | {n_layer} | " + " | ".join(cells) + f" | {ratio:.3f} |", flush=True)
            del blk, states, arms


def bench_linearmax():
    """First-order linearmax decode state cache: `step` per token and layer, one state per layer of the model visited in turn
    (22 / 32), after prompts of 512 and 16384 tokens; beside it what one more token costs without the cache (fastmax_hack over
    the prefix + 1 tokens, of which only the last row is wanted; K and V as the block's stride-0 group views) and the p=2
    cache's step at the same shape (its cost does not depend on the prompt: 64-token prefill).  Event times, host side
    included."""
    from attention_mechanisms.fastmax_hack import fastmax_hack
    from fastmax_experiments_amd.decode import LinearmaxDecodeState
    print("| shape (H, G, hs) | B | prompt | state KB/layer | linearmax step us/token.layer | masked forward over the prefix us | "
          "p=2 cache step us/token.layer |")
    print("|---|---|---|---|---|---|---|")
    for name, H, G, D, layers in (("TinyLlama", 32, 4, 64, 22), ("Llama-2-7B", 32, 32, 128, 32)):
        for B in (1, 8):
            q1 = torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16)
            k1, v1 = (torch.randn(B, G, 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))
            p2 = [FastmaxDecodeState(B, H, D, device="cuda", p=2, n_query_groups=G) for _ in range(layers)]
            qs, ks, vs = (torch.randn(B, h, 64, D, device="cuda").to(torch.bfloat16) for h in (H, G, G))
            with torch.no_grad():
                for st in p2:
                    st.prefill(qs, ks, vs)
                us_p2 = timeit(lambda: [st.step(q1, k1, v1) for st in p2], iters=3, rounds=5) / layers * 1e3
            del p2
            for N in (512, 16384):
                q = torch.randn(B, H, N + 1, D, device="cuda").to(torch.bfloat16)
                k, v = (torch.randn(B, G, N + 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))
                states = [LinearmaxDecodeState(B, H, D, "cuda", n_query_groups=G) for _ in range(layers)]
                states[0].prefill(q[:, :, :N], k[:, :, :N], v[:, :, :N])
                for st in states[1:]:
                    st.state.copy_(states[0].state)
                    st.count = N
                r = H // G
                qg = q.reshape(B * G, r, N + 1, D)
                kg, vg = (t.reshape(B * G, 1, N + 1, D).expand(B * G, r, N + 1, D) for t in (k, v))
                with torch.no_grad():
                    us = timeit(lambda: [st.step(q1, k1, v1) for st in states], iters=3, rounds=5) / layers * 1e3
                    us_fwd = timeit(lambda: fastmax_hack(qg, kg, vg, p=1, mask=True), iters=3, rounds=5) * 1e3
                kb = states[0].state.numel() * 4 / 1024
                print(f"| {name} ({H}, {G}, {D}) | {B} | {N} | {kb:.0f} | {us:.1f} | {us_fwd:.1f} | {us_p2:.1f} |", flush=True)
                del states, q, k, v, qg, kg, vg


# ---- the KV-cache decode route against the second-order state ---------------------------------------------------------------
KV_SHAPES = (("TinyLlama", 32, 4, 64, 22), ("Llama-2-7b", 32, 32, 128, 32), ("Gemma-2b", 8, 1, 256, 18))     # name, H, Hkv, D, layers
KV_LENGTHS = (512, 2048, 8192, 32768)
KV_BUDGET = 40 << 30          # bytes of caches per cell: fewer states than layers where a layer's cache is gigabytes
KV_TRACE_STEPS = 3            # steps per state in the kernel-trace run


def _kv_cells():
    for name, H, Hkv, D, layers in KV_SHAPES:
        for B in (1, 8):
            for n in KV_LENGTHS:
                live = B * Hkv * (n + 1) * 2 * D * 2                       # bf16 bytes a step reads: the issue's byte count
                yield name, H, Hkv, D, B, n, live, max(2, min(layers, KV_BUDGET // (B * Hkv * (n + 128) * 2 * D * 2)))


def _kv_states(H, Hkv, D, B, n, count):
    """`count` KV caches holding the same n random tokens (written by the load entry point: no kernel of the step runs)"""
    from fastmax_experiments_amd.decode import FastmaxKVDecodeState
    k, v = (torch.randn(B, Hkv, n, D, device="cuda").to(torch.bfloat16) for _ in range(2))
    states = []
    for _ in range(count):
        st = FastmaxKVDecodeState(B, H, D, "cuda", n + 1, torch.bfloat16, n_query_groups=Hkv)
        ops._call("fastmax_hip_kv_decode_load", st.state.device,
                  (*ops._qkv(k, v), st.state.data_ptr(), B, Hkv, n, D, st.max_len, _lib.BF16))
        st._count = n
        states.append(st)
    return states


def _graph_of(fn):
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(); fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def bench_kv(rounds=7):
    """One KV step against one p=2 state step, per layer: a graph of one step on each of `states` independent caches (one per
    layer of the model, fewer where the caches would pass KV_BUDGET), replayed; the two routes alternate inside each round.
    The KV graph takes every cache back to its length after the step (one one-thread launch per cache), so that every replay
    reads the same prefix: its time is inside the KV column.  Event times; kernel times and rates come from `--kv-trace`."""
    print("| shape (H, Hkv, D) | B | length | states | live cache MB/step | KV step us: median (min, spread) | state MB/step | "
          "p=2 state step us: median (min, spread) | KV / state |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, H, Hkv, D, B, n, live, count in _kv_cells():
        q1 = torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16)
        k1, v1 = (torch.randn(B, Hkv, 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        kv = _kv_states(H, Hkv, D, B, n, count)

        def kv_steps():
            for st in kv:
                st.step(q1, k1, v1)
                st.count = n

        arms = {"kv": None}
        with torch.no_grad():
            arms["kv"] = _graph_of(kv_steps)
            sb = 0
            if D <= 128:
                p2 = [FastmaxDecodeState(B, H, D, device="cuda", p=2, n_query_groups=Hkv) for _ in range(count)]
                qs, ks, vs = (torch.randn(B, h, 64, D, device="cuda").to(torch.bfloat16) for h in (H, Hkv, Hkv))
                for st in p2:
                    st.prefill(qs, ks, vs)
                arms["state"] = _graph_of(lambda: [st.step(q1, k1, v1) for st in p2])
                sb = 2 * B * Hkv * (D + 1) * (D + 2) // 2 * ((D + 4) // 4 * 4) * 4          # read and rewritten (bench_p2's count)
            iters = max(2, min(200, int(4e9 / (live * count))))
            ts = _alternate(arms, rounds, iters)
        cells = {}
        for a, t in ts.items():
            us = [x * 1e3 / count for x in t]
            med = statistics.median(us)
            cells[a] = (med, f"{med:.1f} ({min(us):.1f}, {(max(us) - min(us)) / med * 100:.0f}%)")
        state = f"{sb / 1e6:.2f} | {cells['state'][1]} | {cells['kv'][0] / cells['state'][0]:.2f}" if "state" in cells else "- | no such route | -"
        print(f"| {name} ({H}, {Hkv}, {D}) | {B} | {n} | {count} | {live / 1e6:.1f} | {cells['kv'][1]} | {state} |", flush=True)
        del kv, arms
        torch.cuda.empty_cache()


def kv_trace(path):
    """for a `rocprofv3 --kernel-trace --stats` run: every cell of `--kv` in turn, KV_TRACE_STEPS eager steps on each cache (the
    length taken back after each), and the cells' order written to `path` for `--kv-trace-table`"""
    import json
    order = []
    with torch.no_grad():
        for name, H, Hkv, D, B, n, live, count in _kv_cells():
            count = min(count, 4)
            q1 = torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16)
            k1, v1 = (torch.randn(B, Hkv, 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))
            kv = _kv_states(H, Hkv, D, B, n, count)
            for _ in range(KV_TRACE_STEPS):
                for st in kv:
                    st.step(q1, k1, v1)
                    st.count = n
            torch.cuda.synchronize()
            order.append(dict(name=name, H=H, Hkv=Hkv, D=D, B=B, length=n, live=live, steps=KV_TRACE_STEPS * count))
            del kv
            torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(order, f)
    print(f"{len(order)} cells -> {path}")


def kv_trace_table(trace_dir, path):
    """the kernel trace of a `--kv-trace` run as one row per cell: microseconds per step of each kernel of the step (mean over the
    cell's steps, the first step of each cell left out) and bytes/s of the live cache prefix over the attend kernel's time and
    over the whole step's, beside the 6.3 TB/s copy rate of the chip"""
    import csv, glob, json
    order = json.load(open(path))
    kinds = ("kv_append_kernel", "kv_attend_kernel", "kv_combine_kernel", "kv_commit_kernel")
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            kind = next((k for k in kinds if k in r["Kernel_Name"]), None)
            if kind:
                rows.append((int(r["Start_Timestamp"]), kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per = {k: [d for _, kind, d in rows if kind == k] for k in kinds}
    total = sum(c["steps"] for c in order)
    for k in kinds:
        if len(per[k]) != total:
            raise SystemExit(f"{k}: {len(per[k])} dispatches in the trace, the run made {total} steps")
    print("| shape (H, Hkv, D) | B | length | live cache MB | append us | attend us | combine us | commit us | attend TB/s | "
          "whole step TB/s | of 6.3 TB/s (attend) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    at = 0
    for c in order:
        sl = slice(at + 1, at + c["steps"])
        at += c["steps"]
        us = {k: statistics.mean(per[k][sl]) for k in kinds}
        rate, whole = c["live"] / us["kv_attend_kernel"] / 1e6, c["live"] / sum(us.values()) / 1e6
        print(f"| {c['name']} ({c['H']}, {c['Hkv']}, {c['D']}) | {c['B']} | {c['length']} | {c['live'] / 1e6:.1f} | "
              + " | ".join(f"{us[k]:.1f}" for k in kinds) + f" | {rate:.2f} | {whole:.2f} | {rate / 6.3 * 100:.0f}% |")


def _case_arg(flag):
    return tuple(int(x) for x in sys.argv[sys.argv.index(flag) + 1].split(","))


if "--kv-trace-table" in sys.argv:
    i = sys.argv.index("--kv-trace-table")
    kv_trace_table(sys.argv[i + 1], sys.argv[i + 2])
    sys.exit(0)
if "--kv-trace" in sys.argv:
    kv_trace(sys.argv[sys.argv.index("--kv-trace") + 1])
    sys.exit(0)
if "--kv" in sys.argv:
    bench_kv()
    sys.exit(0)

if "--linearmax" in sys.argv:
    bench_linearmax()
    sys.exit(0)
if "--block-case" in sys.argv:
    name, B, fused = sys.argv[sys.argv.index("--block-case") + 1].split(",")
    blk, states, x1, c, s = _block_setup(name, dict(BLOCK_CASES)[name], int(B))
    arm = _block_arms(blk, states, x1, c, s)["fused" if int(fused) else "split+step"]
    with torch.no_grad():
        ms = timeit(arm, iters=5, rounds=3)
    print(f"block-case {name} B={B} fused={fused}: tokens through the block = {len(states) * 16}, event ms per token and layer "
          f"{ms / len(states):.4f}")
    sys.exit(0)
if "--block" in sys.argv:
    bench_block(graph="--no-graph" not in sys.argv)
    sys.exit(0)
if "--extend-case" in sys.argv:
    B, H, Hkv, D, T = _case_arg("--extend-case")
    ms_e, ms_s, n, ne, ns = extend_case(B, H, Hkv, D, T)
    print(f"extend-case ({B},{H},{Hkv},{D}) T={T}: states={n} extend_calls={ne} step_sequences={ns} "
          f"event ms: extend {ms_e:.4f}, {T} steps {ms_s:.4f}")
    sys.exit(0)
if "--prefill-case" in sys.argv:
    B, H, N, D, C = _case_arg("--prefill-case")
    ms, calls = prefill_case(B, H, N, D, C)
    print(f"prefill-case ({B},{H},{N},{D}) chunk={C}: calls={calls} event ms {ms:.4f}")
    sys.exit(0)
if "--extend" in sys.argv:
    bench_extend()
    sys.exit(0)
if "--p2" in sys.argv:          # the second-order rows only (for a profiler run)
    bench_p2()
    sys.exit(0)

print("| case | (B,H,Nq,Nk,D) | dtype | p | ms |")
print("|---|---|---|---|---|")
for B, H, Nq, Nk, D, dt, p in ((1, 32, 1, 4096, 64, torch.bfloat16, 2), (1, 32, 1, 4096, 128, torch.bfloat16, 2), (8, 32, 1, 4096, 64, torch.bfloat16, 2),
                               (1, 32, 1, 16384, 128, torch.bfloat16, 1), (1, 32, 16, 4096, 64, torch.bfloat16, 2), (1, 32, 128, 4096, 64, torch.bfloat16, 2)):
    q = torch.randn(B, H, Nq, D, device="cuda").to(dt)
    k, v = (torch.randn(B, H, Nk, D, device="cuda").to(dt) for _ in range(2))
    with torch.no_grad():
        ms = timeit(lambda: fastmax(q, k, v, mask=False, p=p))
    print(f"| unmasked over the KV cache | ({B},{H},{Nq},{Nk},{D}) | {str(dt).split('.')[-1]} | {p} | {ms:.4f} |", flush=True)
for B, H, T, D in ((1, 32, 4096, 64), (1, 32, 16384, 128), (8, 32, 4096, 64)):
    q, k, v = (torch.randn(B, H, T, D, device="cuda").to(torch.bfloat16) for _ in range(3))
    st = FastmaxDecodeState(B, H, D, device="cuda")
    st.prefill(q, k, v)
    q1, k1, v1 = (torch.randn(B, H, 1, D, device="cuda").to(torch.bfloat16) for _ in range(3))
    with torch.no_grad():
        ms = timeit(lambda: st.step(q1, k1, v1))
    print(f"| decode state cache step (p=1, opt-in) | ({B},{H},1,{T},{D}) | bfloat16 | 1 | {ms:.4f} |", flush=True)

print()
bench_p2()
print()

# the frozen 4-bit linear at generation-size row counts (merged weights: no LoRA branch), eager and as a HIP graph replay
from fastmax_experiments_amd import lora
for M, K, N in ((1, 4096, 4096), (16, 4096, 4096), (1, 4096, 11008), (1, 11008, 4096)):
    lin = torch.nn.Linear(K, N, bias=False)
    q4 = lora.NF4Linear.from_linear(lin).cuda()
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    wd = q4.dequantize(torch.bfloat16)
    with torch.no_grad():
        t_e = timeit(lambda: q4(x))
        t_d = timeit(lambda: torch.nn.functional.linear(x, wd))
        q4(x)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            q4(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(10):
                y = q4(x)
        t_g = timeit(lambda: graph.replay()) / 10
    print(f"| NF4 linear (M,K,N)=({M},{K},{N}): eager {t_e * 1e3:.1f} us, graph replay {t_g * 1e3:.1f} us = {N * K / 2 / t_g / 1e6:.0f} GB/s of codes; bf16 F.linear {t_d * 1e3:.1f} us | | bfloat16 | | {t_g:.4f} |", flush=True)
