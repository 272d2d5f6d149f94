#!/usr/bin/env python3
"""The bits of the dense last-row logits, recorded from a build of this library on an MI355X.

    PYTHONPATH=. python tests/golden/make_golden_last_logits.py          (needs the built library and the device)

Unlike the other make_golden_*.py this one runs no reference: it goes through the public ``generate.last_logits`` only and stores
what it returns, so that a change which is meant to leave the kernel's plan alone (rows per wave, the unroll rule, the piece
order, the short last piece) can be held to the bits of the commit before it.  tests/test_next_token_gpu.py compares with
``torch.equal``.  Regenerate only with a change that is meant to move the bits, and say so.

One file per dtype, last_logits_{f32,bf16,f16}.npz, 16-bit tensors as int16 bit patterns.  Two cases each, the smallest shapes
that reach every branch of the plan (16 rows of W per workgroup, lanes take pieces l, l + 64, ..., two pieces per trip at G <= 2):
    vec    V = 37: three workgroups, the last with one wave that has a single valid row and two waves that leave.  C = 130 pieces
           of 16 bytes (520 float32, 1040 16-bit): lanes make two or three trips, the unrolled loop has a remainder.
    elem   V = 37, C = 101: the element route with a short last piece.  W starts at column 1 of a (39, 120) tensor, x is the last
           position of a (9, 5, C) tensor.
Each is scored at B = 1, 2, 3, 9 (G = 1, 2, 4, and 8 followed by a second pass of 1), into float32 and into the input dtype,
with and without a bias of V + 5 elements.  Outputs: ``{case}_B{B}_{f32|same}_{bias|nobias}``.
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SEED = 20
V, PIECES, C_ELEM = 37, 130, 101
BATCHES = (1, 2, 3, 9)


def operands(d, case):
    """(x, W) of a case as the views the kernel is to see, from the tensors a file holds"""
    if case == "vec":
        return d["vec_x"], d["vec_w"]
    return d["elem_hidden"][:, -1], d["elem_wide"][1:V + 1, 1:1 + C_ELEM]


def bits(t):
    t = t.detach().cpu()
    return (t.view(torch.int16) if t.element_size() == 2 else t).numpy()


def main():
    from fastmax_experiments_amd.generate import last_logits
    for name, dt in DT.items():
        g = torch.Generator().manual_seed(SEED)
        C = PIECES * 16 // torch.empty(0, dtype=dt).element_size()
        d = {"vec_x": torch.randn(max(BATCHES), C, generator=g), "vec_w": torch.randn(V, C, generator=g),
             "elem_hidden": torch.randn(max(BATCHES), 5, C_ELEM, generator=g), "elem_wide": torch.randn(V + 2, 120, generator=g),
             "bias": torch.randn(V + 5, generator=g)}
        d = {k: t.to(dt).cuda() for k, t in d.items()}
        out = {k: bits(t) for k, t in d.items()}
        for case in ("vec", "elem"):
            x, w = operands(d, case)
            for B in BATCHES:
                for out_name, out_dt in dict(f32=torch.float32, same=dt).items():
                    for bias_name, bias in dict(bias=d["bias"], nobias=None).items():
                        out[f"{case}_B{B}_{out_name}_{bias_name}"] = bits(last_logits(x[:B], w, out_dt, bias=bias))
        meta = dict(fn="generate.last_logits", dtype=name, seed=SEED, V=V, C_vec=C, C_elem=C_ELEM, batches=list(BATCHES),
                    device=torch.cuda.get_device_name(0))
        out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(HERE, f"last_logits_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
