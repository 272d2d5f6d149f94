"""Times softmax attention on an MI355X (profiles/r28_softmax.md): the causal prefill kernel against
torch.nn.functional.scaled_dot_product_attention (K / V expanded per query head) and fastmax(p=2); one SoftmaxKVDecodeState.step,
replayed from a captured graph, against FastmaxKVDecodeState.step, with the achieved bytes per second on the cache.

``--backward`` instead times forward + backward of ops.softmax_attention_with_grad (profiles/r29_softmax_backward.md) on the two
prefill shapes against the same two, forward + backward.

Every timed call rotates over enough operand sets to pass the last-level cache (256 MiB) between two uses of one set; the figure
is the median of ``--reps`` timings of ``--inner`` calls after ``--warmup`` untimed ones.  Prints one JSON line per case."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastmax_experiments_amd import ops                                                      # noqa: E402
from fastmax_experiments_amd.attention_mechanisms.fastmax import fastmax                      # noqa: E402
from fastmax_experiments_amd.decode import FastmaxKVDecodeState, SoftmaxKVDecodeState        # noqa: E402

LLC = 256 << 20


def timed(fn, nsets, a):
    """median milliseconds of one fn(i) call, i rotating over the operand sets"""
    for i in range(a.warmup):
        fn(i % nsets)
    ms = []
    for r in range(a.reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(a.inner):
            fn((r * a.inner + i) % nsets)
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop) / a.inner)
    return sorted(ms)[len(ms) // 2]


def prefill(B, H, Hkv, N, D, a):
    dt = torch.bfloat16
    nsets = max(2, math.ceil(LLC / (2 * (2 * B * H + 2 * B * Hkv) * N * D)) + 1)
    sets = [(torch.randn(B, H, N, D, device="cuda").to(dt), torch.randn(B, Hkv, N, D, device="cuda").to(dt),
             torch.randn(B, Hkv, N, D, device="cuda").to(dt)) for _ in range(nsets)]
    wide = [tuple(t.repeat_interleave(H // Hkv, 1) for t in s[1:]) for s in sets]
    flops = 4 * B * H * N * N * D / 2
    with torch.no_grad():
        t_soft = timed(lambda i: ops.softmax_attention(*sets[i]), nsets, a)
        t_sdpa = timed(lambda i: torch.nn.functional.scaled_dot_product_attention(sets[i][0], *wide[i], is_causal=True), nsets, a)
        t_p2 = timed(lambda i: fastmax(sets[i][0], *wide[i], p=2, mask=True), nsets, a)
    print(json.dumps(dict(case="prefill", shape=[B, H, N, D], kv_heads=Hkv, softmax_ms=t_soft, softmax_tflops=flops / t_soft / 1e9,
                          sdpa_ms=t_sdpa, fastmax_p2_ms=t_p2, operand_sets=nsets)), flush=True)


def train(B, H, Hkv, N, D, a):
    """forward + backward: the HIP route on K/V at their KV heads; SDPA and fastmax(p=2) on K/V expanded inside the graph"""
    dt, r = torch.bfloat16, H // Hkv
    nsets = max(2, math.ceil(LLC / (2 * (3 * B * H + 2 * B * Hkv) * N * D)) + 1)
    sets = [tuple(torch.randn(B, h, N, D, device="cuda").to(dt).requires_grad_(True) for h in (H, Hkv, Hkv)) for _ in range(nsets)]
    dO = [torch.randn(B, N, H, D, device="cuda").to(dt).transpose(1, 2) for _ in range(nsets)]          # as the block hands it back

    def step(i, fn, widen):
        q, k, v = sets[i]
        kv = (k.repeat_interleave(r, 1), v.repeat_interleave(r, 1)) if widen else (k, v)
        torch.autograd.grad(fn(q, *kv), (q, k, v), dO[i])

    flops = (4 + 10) * B * H * N * N * D / 2          # 2 products forward, 5 backward (the tile kernels do 7)
    t_soft = timed(lambda i: step(i, ops.softmax_attention_with_grad, False), nsets, a)
    t_sdpa = timed(lambda i: step(i, lambda q, k, v: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True), True), nsets, a)
    t_p2 = timed(lambda i: step(i, lambda q, k, v: fastmax(q, k, v, p=2, mask=True), True), nsets, a)
    print(json.dumps(dict(case="forward+backward", shape=[B, H, N, D], kv_heads=Hkv, softmax_ms=t_soft,
                          softmax_tflops=flops / t_soft / 1e9, sdpa_ms=t_sdpa, fastmax_p2_ms=t_p2, operand_sets=nsets)), flush=True)


def decode(name, B, H, Hkv, D, cached, a):
    dt = torch.bfloat16
    cache_bytes = 2 * B * Hkv * cached * D * 2
    nsets = max(2, math.ceil(LLC / cache_bytes) + 1)
    row = {"case": "decode", "config": name, "B": B, "cached": cached, "operand_sets": nsets}
    for key, cls in (("softmax", SoftmaxKVDecodeState), ("fastmax", FastmaxKVDecodeState)):
        states = [cls(B, H, D, "cuda", cached + 8, dt, n_query_groups=Hkv) for _ in range(nsets)]
        q, k, v = (torch.randn(B, h, 1, D, device="cuda").to(dt) for h in (H, Hkv, Hkv))
        fill = torch.randn(B, Hkv, cached, D, device="cuda").to(dt)
        graphs = []
        for st in states:                     # a captured step on a cache of `cached` tokens; each replay cuts the length back
            ops._call("fastmax_hip_kv_decode_load", st.state.device, (*ops._qkv(fill, fill), st.state.data_ptr(), B, Hkv, cached, D,
                                                                      st.max_len, ops._DT[dt]))
            st._count = cached
            st.step(q, k, v)
            st.count = cached
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st.step(q, k, v)
                st.count = cached
            st._count = cached
            graphs.append(g)
        t = timed(lambda i: graphs[i].replay(), nsets, a)
        row[key + "_us"] = 1e3 * t
        row[key + "_cache_TBps"] = cache_bytes / t / 1e9
        del graphs, states
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--backward", action="store_true", help="time forward + backward on the two prefill shapes, nothing else")
    a = ap.parse_args()
    if a.backward:
        train(8, 32, 4, 2048, 64, a)
        train(1, 32, 32, 4096, 128, a)
        sys.exit(0)
    prefill(8, 32, 4, 2048, 64, a)
    prefill(1, 32, 32, 4096, 128, a)
    for name, H, Hkv, D in (("tiny-llama-1.1b", 32, 4, 64), ("Llama-2-7b-hf", 32, 32, 128)):
        for B in (1, 8):
            for cached in (2048, 16384):
                decode(name, B, H, Hkv, D, cached, a)
