"""Softmax attention's backward without a GPU: the float64 reference against torch's, a torch emulation of the kernels' rounding
points against the allowance (and a planted fault outside it), and the C ABI's host-side refusals."""
import ctypes

import pytest
import torch

import softmax_bwd_ref as br
from fastmax_experiments_amd import _lib

P = 0x1000          # a non-null, 16-byte aligned address: nothing below dereferences it on the host
SMALLEST, LARGEST = (2, 2, 2, 1, 40), (2, 8, 2, 300, 128)          # (B, H, Hkv, N, D) of tests/test_softmax_bwd_gpu.py


def test_reference_agrees_with_torch():
    q, k, v, dO = br.inputs(2, 4, 2, 37, 16, torch.bfloat16, 0)
    ref = br.reference(q, k, v, dO)
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    kx, vx = (t.repeat_interleave(2, dim=1) for t in leaves[1:])
    o = torch.nn.functional.scaled_dot_product_attention(leaves[0], kx, vx, is_causal=True)
    for want, key in zip(torch.autograd.grad(o, leaves, dO.double()), ("dq", "dk", "dv")):
        assert (ref[key] - want).abs().max() < 1e-12 and (ref["allow_" + key] > 0).all(), key


def emulate(q, k, v, dO, fault=None):
    """the kernels' rounding points: float32 scores, lse and o of a float32 / 16-bit forward, P and dS in the dtype, float32 sums"""
    dt, (B, H, N, D), Hkv = q.dtype, q.shape, k.shape[1]
    scale, f = D ** -0.5, lambda t: t.to(dt).float()
    q, k, v, dO = (t.float() for t in (q, k, v, dO))
    kx, vx = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    keep = torch.ones(N, N, dtype=torch.bool).tril(-1 if fault == "mask" else 0)          # the fault: the diagonal masked too
    x = (scale * (q @ kx.transpose(-1, -2))).masked_fill(~torch.ones(N, N, dtype=torch.bool).tril(), float("-inf"))
    e = (x - x.max(-1, keepdim=True).values).exp()
    lse, o = x.max(-1, keepdim=True).values + e.sum(-1, keepdim=True).log(), f(f(e) @ vx / e.sum(-1, keepdim=True))
    p = (x - lse).exp().masked_fill(~keep, 0.0)
    delta = 0.0 if fault == "delta" else (dO * o).sum(-1, keepdim=True)
    dS = p * (dO @ vx.transpose(-1, -2) - delta)
    group = lambda t: t.view(B, Hkv, H // Hkv, N, D).sum(2)          # noqa: E731
    return (f(scale * (f(dS) @ kx)), f(scale * group(f(dS).transpose(-1, -2) @ q)), f(group(f(p).transpose(-1, -2) @ dO)))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [SMALLEST, LARGEST], ids=["smallest", "largest"])
def test_emulated_rounding_points_stay_inside_the_undoubled_allowance(shape, dt):
    q, k, v, dO = br.inputs(*shape, dt, 3)
    ref = br.reference(q, k, v, dO)
    fr = br.fractions(emulate(q, k, v, dO), ref)
    print(f"emulation {shape} {dt}: fractions of the doubled allowance dq {fr[0]:.3f} dk {fr[1]:.3f} dv {fr[2]:.3f}")
    assert max(fr) <= 0.5
    if shape == LARGEST:
        for fault in ("delta", "mask"):
            assert max(br.fractions(emulate(q, k, v, dO, fault), ref)) > 1.0, fault


def _call(kw):
    a = {**dict(q=P, k=P, v=P, o=P, lse=P, go=P, dq=P, B=1, H=2, Hkv=1, T=3, D=64, dtype=_lib.BF16, ws_bytes=1 << 20, st=(640, 640, 64)), **kw}
    s = (ctypes.c_int64 * 3)(*a["st"])
    return _lib.lib().fastmax_hip_softmax_backward(a["q"], s, a["k"], s, a["v"], s, a["o"], a["lse"], a["go"], s, a["dq"], P, P, a["B"],
                                                   a["H"], a["Hkv"], a["T"], a["D"], a["dtype"], 0.125, P, a["ws_bytes"], None)


@pytest.mark.parametrize("kw, code", [
    (dict(dtype=_lib.F32), _lib.E_BAD_DTYPE), (dict(dtype=_lib.F64), _lib.E_BAD_DTYPE), (dict(D=12), _lib.E_BAD_SHAPE),
    (dict(D=264), _lib.E_BAD_SHAPE), (dict(T=0), _lib.E_BAD_SHAPE), (dict(Hkv=3), _lib.E_BAD_SHAPE), (dict(q=None), _lib.E_NULL),
    (dict(o=None), _lib.E_NULL), (dict(k=P + 2), _lib.E_ALIGNMENT), (dict(st=(640, 640, 68)), _lib.E_ALIGNMENT),
    (dict(D=136), _lib.E_BAD_SHAPE), (dict(lse=None), _lib.E_NULL), (dict(go=None, dtype=_lib.F32, D=136), _lib.E_NULL),
    (dict(ws_bytes=2 * 3 * 4 - 1), _lib.E_WORKSPACE), (dict(dq=P + 8, ws_bytes=0), _lib.E_ALIGNMENT)])
def test_host_side_refusals(kw, code):
    assert _call(kw) == code


def test_workspace_sizes():
    ws = _lib.lib().fastmax_hip_softmax_backward_workspace
    assert ws(2, 8, 300, 128) == 2 * 8 * 300 * 4 and ws(1, 2, 1, 8) == 8
    assert ws(1, 2, 3, 136) == 0 and ws(1, 2, 3, 12) == 0 and ws(1, 2, 0, 64) == 0 and ws(0, 2, 3, 64) == 0
