"""Times LLaMA-Adapter's gated prefix term on an MI355X (profiles/r30_prefix_attention.md), bf16, aT = 10, forward and forward +
backward on (8, 32, 2048, 64) with 4 KV heads and (1, 32, 4096, 128):
    (a) the quadratic operator alone (ops.softmax_attention_with_grad)
    (b) with the HIP term behind it (ops.prefix_attention_add)
    (c) with the tensor-op restatement of the term (adapter.prefix_attention_tensor_ops: SDPA with the ones mask, multiply, add)
    (d) the two kernels alone, with their achieved bytes per second on their algorithmic bytes (forward: q + y + out; backward:
        q + dO + dq + the partials)
and one decode step (B = 8, 2048 cached tokens, tiny-llama heads) replayed from a captured graph, adapter on against off.

Timing as tools/bench_softmax.py: operand sets rotate past the last-level cache; the median of ``--reps`` timings of ``--inner``
calls after ``--warmup`` untimed ones.  Prints one JSON line per case."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_softmax import LLC, timed                                                          # noqa: E402
from fastmax_experiments_amd import _lib, ops                                                 # noqa: E402
from fastmax_experiments_amd.adapter import prefix_attention_tensor_ops                       # noqa: E402
from fastmax_experiments_amd.decode import SoftmaxKVDecodeState                                # noqa: E402

AT = 10


def shape_case(B, H, Hkv, N, D, a):
    dt = torch.bfloat16
    nsets = max(2, math.ceil(LLC / (2 * (4 * B * H + 2 * B * Hkv) * N * D)) + 1)
    sets = [tuple(torch.randn(B, h, N, D, device="cuda").to(dt).requires_grad_(True) for h in (H, Hkv, Hkv)) for _ in range(nsets)]
    dO = [torch.randn(B, N, H, D, device="cuda").to(dt).transpose(1, 2) for _ in range(nsets)]          # as the block hands it back
    ak, av = (torch.randn(Hkv, AT, D, device="cuda").to(dt).requires_grad_(True) for _ in range(2))
    gate = ((torch.rand(1, 1, H, 1, device="cuda") * 0.75 + 0.25)).requires_grad_(True)
    terms = {"a_operator": None, "b_hip_term": lambda y, q: ops.prefix_attention_add(y, q, ak, av, gate),
             "c_tensor_op_term": lambda y, q: prefix_attention_tensor_ops(y, q, ak, av, gate.to(dt))}

    def run(i, term, backward):
        q, k, v = sets[i]
        y = ops.softmax_attention_with_grad(q, k, v)
        out = y if term is None else term(y, q)
        if backward:
            torch.autograd.grad(out, (q, k, v) if term is None else (q, k, v, ak, av, gate), dO[i])

    row = dict(case="prefix", shape=[B, H, N, D], kv_heads=Hkv, aT=AT, operand_sets=nsets)
    for name, term in terms.items():
        with torch.no_grad():
            row[name + "_fwd_ms"] = timed(lambda i: run(i, term, False), nsets, a)
        row[name + "_fwd_bwd_ms"] = timed(lambda i: run(i, term, True), nsets, a)
    # (d) the kernels alone
    ys = [torch.randn(B, H, N, D, device="cuda").to(dt) for _ in range(nsets)]
    with torch.no_grad():
        t_f = timed(lambda i: ops.prefix_attention_forward(ys[i], sets[i][0], ak, av, gate), nsets, a)
    outs = [ops.prefix_attention_add(ys[i], sets[i][0], ak, av, gate) for i in range(nsets)]
    t_b = timed(lambda i: torch.autograd.grad(outs[i], (sets[i][0], ak, av, gate), dO[i], retain_graph=True), nsets, a)
    rows = 2 * B * H * N * D
    row.update(fwd_kernel_ms=t_f, fwd_kernel_TBps=3 * rows / t_f / 1e9, bwd_kernels_ms=t_b,
               bwd_kernels_TBps=(3 * rows + _lib.lib().fastmax_hip_prefix_backward_workspace(B, H, N, D)) / t_b / 1e9)
    print(json.dumps(row), flush=True)


def decode_case(B, H, Hkv, D, cached, a):
    dt = torch.bfloat16
    cache_bytes = 2 * B * Hkv * cached * D * 2
    nsets = max(2, math.ceil(LLC / cache_bytes) + 1)
    ak, av = (torch.randn(Hkv, AT, D, device="cuda").to(dt) for _ in range(2))
    gate = torch.rand(1, 1, H, 1, device="cuda") * 0.75 + 0.25
    row = dict(case="decode", B=B, heads=[H, Hkv, D], cached=cached, operand_sets=nsets)
    for key, prefix in (("adapter_off", None), ("adapter_on", (ak, av, gate))):
        states = [SoftmaxKVDecodeState(B, H, D, "cuda", cached + 8, dt, n_query_groups=Hkv) for _ in range(nsets)]
        q, k, v = (torch.randn(B, h, 1, D, device="cuda").to(dt) for h in (H, Hkv, Hkv))
        fill = torch.randn(B, Hkv, cached, D, device="cuda").to(dt)
        graphs = []
        for st in states:                     # a captured step on a cache of `cached` tokens; each replay cuts the length back
            st.prefix = prefix
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
        row[key + "_us"] = 1e3 * timed(lambda i: graphs[i].replay(), nsets, a)
        del graphs, states
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    shape_case(8, 32, 4, 2048, 64, a)
    shape_case(1, 32, 32, 4096, 128, a)
    decode_case(8, 32, 4, 64, 2048, a)
