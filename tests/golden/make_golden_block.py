#!/usr/bin/env python3
"""Golden vectors for the decoder block's neighbours of the attention sub-layer, by RUNNING THE REFERENCE's own pure-torch code.

    python tests/golden/make_golden_block.py          (where make_golden_neighbours.py runs: it needs the reference's tree)

Like make_golden_neighbours.py: each definition is located by name in the file's syntax tree and executed, as it stands in the
file, in a namespace that holds nothing but torch and the typing names -- no package import, no edited or copied source:

  * lit_gpt/rmsnorm.py   RMSNorm (6-34)
  * lit_gpt/model.py     LLaMAMLP (622-633), GemmaMLP (636-641), with a plain namespace object for `config`

Only inputs, parameters, outputs and the gradients of backward() on a seeded cotangent are stored (.npz, the call arguments in
`meta`; 16-bit tensors as the float32 values they hold exactly).  The MLP fixtures also hold the activations inside the module
(a = fc_1(x), b = fc_2(x), g = act(a) * b, caught by forward hooks), which is what the gated-activation kernel is checked on.

The reference's whole `Block` cannot be executed this way: its `CausalSelfAttention.fastmax` moves the operator's result with
`.cuda()` (lit_gpt/model.py:482-486) and its operator modules import packages that are not installed, so there is no
block_llama_*.npz; the block is checked by composition (kernels on against the tensor-op restatement).
"""
import ast
import os
import types

import torch
import torch.nn as nn

from make_golden_neighbours import REF, extract, rand, save

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def rmsnorm_cases():
    (RMSNorm,) = extract(os.path.join(REF, "rmsnorm.py"), ["RMSNorm"])
    shape, C = (2, 9, 72), 72
    cases = [("f32", 1e-5, False, "f32"), ("f32", 1e-6, True, "f32")]
    for dt in ("bf16", "f16"):
        cases += [(dt, 1e-5, False, dt), (dt, 1e-6, True, dt), (dt, 1e-6, False, "f32"), (dt, 1e-5, True, "f32")]
    for i, (dt, eps, offset, wdt) in enumerate(cases):
        norm = RMSNorm(C, eps=eps, add_unit_offset=offset)
        with torch.no_grad():
            norm.weight.copy_((0.0 if offset else 1.0) + rand((C,), 300 + i, 0.3))
        norm.to(DT[wdt])
        x = rand(shape, 310 + i, 1.5, DT[dt]).requires_grad_(True)
        y = norm(x)
        gy = rand(shape, 320 + i, 1.0, y.dtype)
        y.backward(gy)
        name = f"rmsnorm_{dt}_eps{'5' if eps == 1e-5 else '6'}_w{wdt}" + ("_offset" if offset else "")
        save(name, dict(fn="RMSNorm", size=C, eps=eps, add_unit_offset=offset, x_dtype=dt, weight_dtype=wdt,
                        out_dtype=str(y.dtype), seed=300 + i),
             x=x.detach(), weight=norm.weight.detach(), y=y.detach(), gy=gy, dx=x.grad, dweight=norm.weight.grad)


def extract_mlps():
    """LLaMAMLP and GemmaMLP of lit_gpt/model.py, executed as they stand; their `config: Config` annotation is evaluated when
    the class body runs, so the name is bound to the plain namespace type the cases pass in"""
    path = os.path.join(REF, "model.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    names = ["LLaMAMLP", "GemmaMLP"]
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    if [n.name for n in picked] != names:
        raise RuntimeError(f"{path}: {names} not found")
    ns = {"torch": torch, "nn": nn, "Config": types.SimpleNamespace}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def mlp_cases():
    LLaMAMLP, GemmaMLP = extract_mlps()
    # (class, dtype, rows, n_embd, intermediate_size, bias)
    cases = [(cls, dt, 3, 16, 88, False) for cls in (LLaMAMLP, GemmaMLP) for dt in ("f32", "bf16", "f16")]
    cases += [(LLaMAMLP, "f32", 2, 16, 7, True), (GemmaMLP, "f32", 2, 16, 7, True), (LLaMAMLP, "bf16", 2, 16, 7, True),
              (GemmaMLP, "f16", 2, 16, 7, False)]
    for i, (cls, dt, M, n_embd, inter, bias) in enumerate(cases):
        config = types.SimpleNamespace(n_embd=n_embd, intermediate_size=inter, bias=bias)
        mlp = cls(config)
        g = torch.Generator().manual_seed(400 + i)
        with torch.no_grad():
            for p in mlp.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 2 and p.shape[1] == n_embd else 0.2))
        mlp.to(DT[dt])
        caught = {}
        mlp.fc_1.register_forward_hook(lambda m, inp, out: caught.__setitem__("a", out.detach().clone()))
        mlp.fc_2.register_forward_hook(lambda m, inp, out: caught.__setitem__("b", out.detach().clone()))
        mlp.proj.register_forward_hook(lambda m, inp, out: caught.__setitem__("g", inp[0].detach().clone()))
        x = rand((1, M, n_embd), 410 + i, 1.5, DT[dt]).requires_grad_(True)
        y = mlp(x)
        gy = rand(tuple(y.shape), 420 + i, 1.0, y.dtype)
        y.backward(gy)
        arrays = dict(x=x.detach(), y=y.detach(), gy=gy, dx=x.grad, **caught)
        for n, p in mlp.named_parameters():
            arrays[n.replace(".", "_")] = p.detach()
            arrays["d_" + n.replace(".", "_")] = p.grad
        act = "silu" if cls is LLaMAMLP else "gelu"
        save(f"mlp_{cls.__name__.lower()}_{dt}_i{inter}", dict(fn=cls.__name__, act=act, n_embd=n_embd, intermediate_size=inter,
                                                               bias=bias, dtype=dt, rows=M, seed=400 + i), **arrays)


def main():
    torch.set_num_threads(4)
    torch.manual_seed(0)
    rmsnorm_cases()
    mlp_cases()


if __name__ == "__main__":
    main()
