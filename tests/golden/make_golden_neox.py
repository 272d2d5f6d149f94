#!/usr/bin/env python3
"""Golden vectors for the NeoX (pythia) block's neighbours of the attention sub-layer, in the manner of make_golden_block.py.

    python tests/golden/make_golden_neox.py          (where make_golden_neighbours.py runs: it needs the reference's tree)

  * lit_gpt/model.py     GptNeoxMLP (608-619), located by name in the file's syntax tree and executed as it stands, with a plain
                         namespace object for `config` (n_embd, intermediate_size, bias, gelu_approximate="none")
  * torch.nn.LayerNorm   what `Config.norm_class` resolves to for the pythia configs (lit_gpt/config.py:55, 143-147): there is
                         no reference source to execute, the class is torch's own

Only inputs, parameters, outputs and the gradients of backward() on a seeded cotangent are stored (.npz, the call arguments in
`meta`; 16-bit tensors as the float32 values they hold exactly).  The MLP fixtures also hold the activations inside the module
(a = fc(x), g = gelu(a), caught by forward hooks), which is what the activation kernel is checked on.

File names start with `layernorm_` and `neox_mlp_`, which no earlier test's prefix (`rmsnorm_`, `mlp_`) picks up.
"""
import ast
import os
import types

import torch
import torch.nn as nn

from make_golden_neighbours import REF, rand, save

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def layernorm_cases():
    shape, C, eps = (2, 9, 72), 72, 1e-5
    for i, (dt, wdt) in enumerate([("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32")]):
        norm = nn.LayerNorm(C, eps=eps)
        with torch.no_grad():
            norm.weight.copy_(1.0 + rand((C,), 500 + i, 0.3))
            norm.bias.copy_(rand((C,), 505 + i, 0.2))
        norm.to(DT[wdt])
        x = (rand(shape, 510 + i, 1.5) + 0.4).to(DT[dt]).requires_grad_(True)        # a mean away from zero
        y = norm(x)
        gy = rand(shape, 520 + i, 1.0, y.dtype)
        y.backward(gy)
        save(f"layernorm_{dt}_w{wdt}", dict(fn="LayerNorm", size=C, eps=eps, x_dtype=dt, weight_dtype=wdt, out_dtype=str(y.dtype),
                                            seed=500 + i),
             x=x.detach(), weight=norm.weight.detach(), bias=norm.bias.detach(), y=y.detach(), gy=gy, dx=x.grad,
             dweight=norm.weight.grad, dbias=norm.bias.grad)


def extract_neox_mlp():
    """GptNeoxMLP of lit_gpt/model.py, executed as it stands; its `config: Config` annotation is evaluated when the class body
    runs, so the name is bound to the plain namespace type the cases pass in"""
    path = os.path.join(REF, "model.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GptNeoxMLP"]
    if len(picked) != 1:
        raise RuntimeError(f"{path}: GptNeoxMLP not found")
    ns = {"torch": torch, "nn": nn, "Config": types.SimpleNamespace}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns["GptNeoxMLP"]


def mlp_cases():
    GptNeoxMLP = extract_neox_mlp()
    # (dtype, rows, n_embd, intermediate_size, bias)
    cases = [(dt, 3, 16, 88, False) for dt in ("f32", "bf16", "f16")] + [("f32", 2, 16, 7, True), ("bf16", 2, 16, 7, True)]
    for i, (dt, M, n_embd, inter, bias) in enumerate(cases):
        config = types.SimpleNamespace(n_embd=n_embd, intermediate_size=inter, bias=bias, gelu_approximate="none")
        mlp = GptNeoxMLP(config)
        g = torch.Generator().manual_seed(600 + i)
        with torch.no_grad():
            for p in mlp.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 2 and p.shape[1] == n_embd else 0.2))
        mlp.to(DT[dt])
        caught = {}
        mlp.fc.register_forward_hook(lambda m, inp, out: caught.__setitem__("a", out.detach().clone()))
        mlp.proj.register_forward_hook(lambda m, inp, out: caught.__setitem__("g", inp[0].detach().clone()))
        x = rand((1, M, n_embd), 610 + i, 1.5, DT[dt]).requires_grad_(True)
        y = mlp(x)
        gy = rand(tuple(y.shape), 620 + i, 1.0, y.dtype)
        y.backward(gy)
        arrays = dict(x=x.detach(), y=y.detach(), gy=gy, dx=x.grad, **caught)
        for n, p in mlp.named_parameters():
            arrays[n.replace(".", "_")] = p.detach()
            arrays["d_" + n.replace(".", "_")] = p.grad
        save(f"neox_mlp_{dt}_i{inter}", dict(fn="GptNeoxMLP", act="gelu", n_embd=n_embd, intermediate_size=inter, bias=bias,
                                             dtype=dt, rows=M, seed=600 + i), **arrays)


def main():
    torch.set_num_threads(4)
    torch.manual_seed(0)
    layernorm_cases()
    mlp_cases()


if __name__ == "__main__":
    main()
