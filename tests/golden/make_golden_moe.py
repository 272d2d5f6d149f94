#!/usr/bin/env python3
"""Golden vectors for the mixture-of-experts MLP, by RUNNING THE REFERENCE's own pure-torch code.

    python tests/golden/make_golden_moe.py          (where make_golden_neighbours.py runs: it needs the reference's tree)

Like make_golden_block.py: LLaMAMLP (lit_gpt/model.py:622-633) and LLaMAMoE (644-674) are located by name in the file's syntax
tree and executed as they stand, in a namespace that holds nothing but torch; `Config` is bound to types.SimpleNamespace, which
is what the cases pass in.  Only data is stored (.npz, the call arguments and the seed in `meta`; 16-bit tensors as the float32
values they hold exactly): x, every parameter, the gate's output `router` (caught by a forward hook), y, a seeded cotangent gy,
dx and every parameter gradient.  The parameters are torch's default initialisation under SEED rounded to values bfloat16 holds,
in every case, which keeps the float32 files under 256 KB.

Two conditions are asserted here, so that the fixtures do not hang on how a tie or a near-tie is broken:
  * in every row the k-th and the (k+1)-th largest router values are at least 4 units in the last place of the dtype apart;
  * the M = 5 cases leave at least one expert without tokens (its gradients are zero).
Step SEED if an initialisation change breaks either.
"""
import ast
import os
import types

import numpy as np
import torch
import torch.nn as nn

from make_golden_neighbours import REF, save

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"f32": 23, "bf16": 7, "f16": 10}
SEED = 1
N_EMBD, INTERMEDIATE = 32, 48
# (dtype, M, E, k)
CASES = ([(dt, 37, 8, 2) for dt in ("f32", "bf16", "f16")] + [(dt, 33, 6, 3) for dt in ("f32", "bf16")] +
         [(dt, 5, 8, 2) for dt in ("f32", "bf16")])


def extract_moe():
    path = os.path.join(REF, "model.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    names = ["LLaMAMLP", "LLaMAMoE"]
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    if [n.name for n in picked] != names:
        raise RuntimeError(f"{path}: {names} not found")
    ns = {"torch": torch, "nn": nn, "Config": types.SimpleNamespace}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns["LLaMAMoE"]


def kth_gap_ulp(router, k, dt):
    """the smallest distance, over the rows, between the k-th and the (k+1)-th largest value, in ulp of dt at the larger one"""
    r = np.sort(router.astype(np.float64), axis=1)[:, ::-1]
    hi, lo = r[:, k - 1], r[:, k]
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(hi), np.abs(lo)))) - MANT[dt])
    return float(((hi - lo) / ulp).min())


def main():
    torch.set_num_threads(4)
    LLaMAMoE = extract_moe()
    for dt, M, E, k in CASES:
        torch.manual_seed(SEED)
        config = types.SimpleNamespace(n_embd=N_EMBD, intermediate_size=INTERMEDIATE, bias=False, n_expert=E, n_expert_per_token=k)
        moe = LLaMAMoE(config)
        with torch.no_grad():                          # parameters that bfloat16 holds exactly: the float32 files stay small
            for p in moe.parameters():
                p.copy_(p.bfloat16().float())
        moe.to(DT[dt])
        caught = {}
        moe.gate.register_forward_hook(lambda m, inp, out: caught.__setitem__("router", out.detach().clone()))
        x = (1.5 * torch.randn(1, M, N_EMBD)).to(DT[dt]).requires_grad_(True)
        y = moe(x)
        gy = torch.randn(tuple(y.shape)).to(DT[dt])
        y.backward(gy)
        router = caught["router"].float().numpy()
        gap = kth_gap_ulp(router, k, dt)
        assert gap >= 4.0, (dt, M, E, k, gap)
        used = np.unique(np.argsort(-router, axis=1, kind="stable")[:, :k])
        if M == 5:
            assert len(used) < E, (dt, M, E, k, used)
        arrays = dict(x=x.detach(), y=y.detach(), gy=gy, dx=x.grad, **caught)
        for n, p in moe.named_parameters():
            arrays[n.replace(".", "_")] = p.detach()
            arrays["d_" + n.replace(".", "_")] = torch.zeros_like(p) if p.grad is None else p.grad
        save(f"moe_{dt}_m{M}_e{E}_k{k}",
             dict(fn="LLaMAMoE", n_embd=N_EMBD, intermediate_size=INTERMEDIATE, n_expert=E, n_expert_per_token=k, dtype=dt, rows=M,
                  seed=SEED, min_kth_gap_ulp=gap, experts_used=[int(e) for e in used]), **arrays)


if __name__ == "__main__":
    main()
