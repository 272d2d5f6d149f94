"""Float64 reference of LLaMA-Adapter's gated prefix attention, out = y + gate * softmax(scale q ak^T) av, and of its gradients
(autograd over the float64 formula on the exact 16-bit inputs), with the first-order allowance its tests grant, per element: the
formulas of DESIGN.md 4.6c, doubled.  u is the unit roundoff, ``tiny`` the half spacing below the dtype's normal range, n_i = aT
(no mask), M = B r N the rows behind each dak / dav element."""
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
EPS = 2.0 ** -24
KEYS = ("out", "dq", "dak", "dav", "dgate")


def inputs(B, H, Hkv, N, D, aT, dt, seed, zero_head=None):
    """y, q, dO as the block's transposed views (B,N,H,D) -> (B,H,N,D); ak, av (Hkv,aT,D); gate float32 (1,1,H,1), random in
    +-[0.25, 1] with ``zero_head`` exactly 0"""
    g = torch.Generator().manual_seed(seed)
    y, q, dO = (torch.randn(B, N, H, D, generator=g).to(dt).transpose(1, 2) for _ in range(3))
    ak, av = (torch.randn(Hkv, aT, D, generator=g).to(dt) for _ in range(2))
    gate = (torch.rand(H, generator=g) * 0.75 + 0.25) * (torch.randint(0, 2, (H,), generator=g) * 2 - 1)
    if zero_head is not None:
        gate[zero_head] = 0.0
    return y, q, ak, av, gate.view(1, 1, H, 1), dO


def formula(y, q, ak, av, gate, scale):
    """-> (P, ay, out) with ak, av (Hkv,aT,D) repeated per query head and gate of H elements, in the inputs' dtype"""
    r = q.shape[1] // ak.shape[0]
    akx, avx = (t.repeat_interleave(r, dim=0) for t in (ak, av))
    p = (scale * q @ akx.transpose(-1, -2)).softmax(-1)
    ay = p @ avx
    return p, ay, y + gate.reshape(1, -1, 1, 1) * ay


def reference(y, q, ak, av, gate, dO, scale=None):
    """-> dict(out, dq, dak, dav, dgate, allow_*), float64, the allowances doubled; dgate as H values"""
    u, tiny, (B, H, N, D), (Hkv, aT, _) = U[q.dtype], TINY[q.dtype], q.shape, ak.shape
    r, scale = H // Hkv, D ** -0.5 if scale is None else scale
    y, q, ak, av, gate, dO = (t.detach().double().cpu() for t in (y, q, ak, av, gate, dO))
    leaves = [t.clone().requires_grad_(True) for t in (q, ak, av, gate)]
    dq, dak, dav, dgate = torch.autograd.grad(formula(y, leaves[0], leaves[1], leaves[2], leaves[3], scale)[2], leaves, dO)
    p, ay, out = formula(y, q, ak, av, gate, scale)
    akx, avx = (t.repeat_interleave(r, dim=0) for t in (ak, av))
    gt = gate.reshape(1, H, 1, 1).abs()
    dd = (dO * ay).sum(-1, keepdim=True)
    core = p * (dO @ avx.transpose(-1, -2) - dd)
    dS = gt * core.abs()

    def group(t):          # (B,H,aT,D) -> summed over the batch and each KV head's group
        return t.sum(0).view(Hkv, r, aT, D).sum(1)

    M = B * r * N
    delta = (D + 2) * EPS * scale * (q.abs() @ akx.abs().transpose(-1, -2)).max(-1, keepdim=True).values
    eps = 2 * delta + (aT + 12) * EPS
    a = ((aT + D + 8) * EPS + u + 2 * delta) * (p @ avx.abs())
    derr = (dO.abs() * a).sum(-1, keepdim=True) + (D + 2) * EPS * (dO * ay).abs().sum(-1, keepdim=True)
    E = gt * ((eps + u + 4 * EPS) * core.abs() + p * ((D + 2) * EPS * dO.abs() @ avx.abs().transpose(-1, -2) + derr)) + tiny
    Et, dSt = (t.transpose(-1, -2) for t in (E, dS))
    allow = dict(out=u * out.abs() + tiny + gt * a + 2 * EPS * (y.abs() + (gt * ay).abs()),
                 dq=u * dq.abs() + tiny + scale * (E @ akx.abs() + (aT + 2) * EPS * (dS @ akx.abs())),
                 dak=u * dak.abs() + tiny + scale * group(Et @ q.abs() + (M + 2) * EPS * (dSt @ q.abs())),
                 dav=u * dav.abs() + tiny + group(gt * (((eps + u + (M + 2) * EPS) * p + tiny).transpose(-1, -2) @ dO.abs())),
                 dgate=(derr.sum((0, 2, 3)) + (B * N + 2) * EPS * dd.abs().sum((0, 2, 3))))
    res = dict(out=out, dq=dq, dak=dak, dav=dav, dgate=dgate.reshape(H))
    return dict(res, **{"allow_" + key: 2 * val for key, val in allow.items()})


def fractions(got, ref):
    """the largest |error| / allowance per tensor of ``got`` (a dict over a subset of KEYS); finite values only"""
    assert all(torch.isfinite(t.float()).all() for t in got.values())
    return {key: ((t.double().cpu().reshape(ref[key].shape) - ref[key]).abs() / ref["allow_" + key]).max().item() for key, t in got.items()}
