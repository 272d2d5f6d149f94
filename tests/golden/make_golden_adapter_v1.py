#!/usr/bin/env python3
"""Golden vector for LLaMA-Adapter (adapter v1), in the manner of make_golden_adapter_v2.py.

    python tests/golden/make_golden_adapter_v1.py          (where make_golden_neighbours.py runs: it needs the reference's tree)

  * lit_gpt/model.py     CausalSelfAttention, apply_rope, build_rope_cache
  * lit_gpt/adapter.py   CausalSelfAttention (104-158), on top of the one above
located by name in the files' syntax trees and executed as they stand; `Config` is a plain namespace of the fields they read.

`adapter_v1_gqa.npz`: float32, CPU, 4 heads on 2 query groups, block index 2 = adapter_start_layer, aT = 10, a non-zero gate.
Stored: the module's weights, the input, the rope rows and the output of forward().
"""
import ast
import math
import os
import types
import typing

import torch
import torch.nn as nn

from make_golden_neighbours import REF, rand, save


def pick(file, names, ns):
    """definitions `names` of lit_gpt/`file`, executed as they stand in `ns` (plus torch, nn, math and the typing names)"""
    path = os.path.join(REF, file)
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    picked = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    if sorted(n.name for n in picked) != sorted(names):
        raise RuntimeError(f"{path}: {names} not found")
    ns = {"torch": torch, "nn": nn, "math": math, "Config": object, "KVCache": object, **ns}
    ns.update({k: getattr(typing, k) for k in ("Any", "Dict", "Optional", "Tuple")})
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    torch.set_num_threads(4)
    base, build_rope_cache = pick("model.py", ["CausalSelfAttention", "build_rope_cache", "apply_rope"], {})[:2]
    adapted, = pick("adapter.py", ["CausalSelfAttention"], {"BaseCausalSelfAttention": base})
    cfg = types.SimpleNamespace(n_embd=32, n_head=4, n_query_groups=2, head_size=8, bias=True, rope_n_elem=8, attn_alg="quadratic",
                                adapter_prompt_length=10, adapter_start_layer=2)
    torch.manual_seed(0)
    m = adapted(cfg, 2)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(rand(p.shape, 900 + i, 0.5))
    B, T = 2, 13
    x = rand((B, T, cfg.n_embd), 950, 1.0)
    cos, sin = build_rope_cache(T, cfg.rope_n_elem)
    with torch.no_grad():
        y = m(x, cos, sin)
    save("adapter_v1_gqa", dict(fn="lit_gpt.adapter.CausalSelfAttention.forward", block_idx=2, **vars(cfg)), x=x, cos=cos, sin=sin, y=y,
         **{k: v for k, v in m.state_dict().items()})


if __name__ == "__main__":
    main()
