#!/usr/bin/env python3
"""Golden vectors for adapter-v2 fine-tuning, in the manner of make_golden_neox.py.

    python tests/golden/make_golden_adapter_v2.py          (where make_golden_neighbours.py runs: it needs the reference's tree)

  * lit_gpt/adapter_v2.py   AdapterV2Linear (50-62) and adapter_filter (34-47), located by name in the file's syntax tree and
                            executed as they stand, in a namespace that holds `torch`, `nn` and `Any` (bound to `object`)

Only inputs, parameters, outputs and the gradients of backward() on a seeded cotangent are stored (.npz, the call arguments in
`meta`; 16-bit tensors as the float32 values they hold exactly).  z = linear(x) and its gradient dz are caught by a forward hook
on the module's `linear`.  The stored dscale / dbias are torch's: with 16-bit parameters every term and the result are rounded,
so they are recorded, not a yardstick.  `adapterv2_filter.npz` holds a list of state-dict key names (in `meta`) with
adapter_filter's answers.

File names start with `adapterv2_`, which no earlier test's prefix picks up.
"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn

from make_golden_neighbours import REF, rand, save

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
IN_FEATURES = 16
KEYS = ["lm_head.linear.weight", "lm_head.linear.bias", "lm_head.adapter_bias", "lm_head.adapter_scale", "transformer.wte.weight",
        "transformer.h.0.norm_1.weight", "transformer.h.0.norm_1.bias", "transformer.h.0.norm_2.weight",
        "transformer.h.0.attn.attn.linear.weight", "transformer.h.0.attn.attn.adapter_bias", "transformer.h.0.attn.attn.adapter_scale",
        "transformer.h.0.attn.proj.linear.bias", "transformer.h.1.attn.adapter_wte.weight", "transformer.h.1.attn.gating_factor",
        "transformer.h.0.mlp.fc_1.linear.weight", "transformer.h.0.mlp.fc_2.adapter_scale", "transformer.h.0.mlp.proj.adapter_bias",
        "transformer.ln_f.weight", "transformer.ln_f.bias", "transformer.h.0.attn.attn.lora_A", "blocks.0.norm_1.weight",
        "blocks.0.attn.linear.weight", "1.ln_f.weight", "0.mlp.fc.adapter_scale"]


def extract():
    path = os.path.join(REF, "adapter_v2.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    names = ("AdapterV2Linear", "adapter_filter")
    picked = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    if sorted(n.name for n in picked) != sorted(names):
        raise RuntimeError(f"{path}: {names} not found")
    ns = {"torch": torch, "nn": nn, "Any": object}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns["AdapterV2Linear"], ns["adapter_filter"]


def linear_cases(AdapterV2Linear):
    pairs = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32")]
    i = 0
    for dt, pdt in pairs:
        for M, N in ((5, 24), (3, 7)):
            for bias in (True, False):
                seed = 700 + 10 * i
                i += 1
                m = AdapterV2Linear(IN_FEATURES, N, bias=bias)
                with torch.no_grad():
                    m.linear.weight.copy_(rand((N, IN_FEATURES), seed, 0.4))
                    if bias:
                        m.linear.bias.copy_(rand((N,), seed + 1, 0.3))
                    m.adapter_scale.copy_(1.0 + rand((N,), seed + 2, 0.5))
                    m.adapter_scale[N // 3] = 0.0                           # a zero scale is legal
                    m.adapter_bias.copy_(rand((N,), seed + 3, 0.5))
                m.to(DT[dt])
                m.adapter_scale.data = m.adapter_scale.data.to(DT[pdt])
                m.adapter_bias.data = m.adapter_bias.data.to(DT[pdt])
                if pdt != dt:                                               # float32 values that no 16-bit number holds
                    with torch.no_grad():
                        m.adapter_scale.mul_(1.0 + 2.0 ** -12)
                        m.adapter_bias.add_(2.0 ** -13)
                m.adapter_scale.requires_grad_(True)
                m.adapter_bias.requires_grad_(True)
                caught = {}

                def hook(mod, inp, out, caught=caught):
                    out.retain_grad()
                    caught["z"] = out

                m.linear.register_forward_hook(hook)
                x = rand((M, IN_FEATURES), seed + 4, 1.5, DT[dt]).requires_grad_(True)
                y = m(x)
                dy = rand((M, N), seed + 5, 1.0, y.dtype)
                y.backward(dy)
                arrays = dict(x=x.detach(), weight=m.linear.weight.detach(), adapter_scale=m.adapter_scale.detach(),
                              adapter_bias=m.adapter_bias.detach(), z=caught["z"].detach(), y=y.detach(), dy=dy, dz=caught["z"].grad,
                              dscale=m.adapter_scale.grad, dbias=m.adapter_bias.grad)
                if bias:
                    arrays["bias"] = m.linear.bias.detach()
                save(f"adapterv2_{dt}_p{pdt}_m{M}n{N}_{'bias' if bias else 'nobias'}",
                     dict(fn="AdapterV2Linear", in_features=IN_FEATURES, out_features=N, rows=M, bias=bias, dtype=dt, param_dtype=pdt,
                          out_dtype=str(y.dtype), zero_scale_column=N // 3, seed=seed), **arrays)


def filter_case(adapter_filter):
    answers = [bool(adapter_filter(k, None)) for k in KEYS]
    save("adapterv2_filter", dict(fn="adapter_filter", keys=KEYS), answers=np.array(answers, dtype=np.uint8))


def main():
    torch.set_num_threads(4)
    torch.manual_seed(0)
    AdapterV2Linear, adapter_filter = extract()
    linear_cases(AdapterV2Linear)
    filter_case(adapter_filter)


if __name__ == "__main__":
    main()
