"""Drop-in for the reference's ``attention_mechanisms/fastmax_hack.py`` ("linearmax").

Reference: fastmax_hack.py:5-60.  Masked branch (36-60): mean-centre / max-norm Q and K, then
first- or second-order fastmax with normalize_term = 1.  Unmasked branch (6-33): same prologue,
first order only (``p`` is ignored there), denominator constant N_k (line 21), float32 ``ones``
promote low-precision inputs to a float32 result.
The prologue and the attention both run in libfastmax_hip.so -- float64 inputs excepted: they are float64 end to end, the
O(N D) prologue as differentiable float64 tensor ops on the device and the attention behind it in the float64 kernels
(csrc/fastmax_f64.hip; ``fastmax.FP64_KERNELS`` off restores the float32-arithmetic route).  Which autograd nodes a call becomes is decided once, by
``linearmax_plan``; ``fastmax_hack``, ``fastmax_hack_grouped`` and the nodes below only read its record.
"""
import functools
import os
from typing import NamedTuple

import torch

from .. import ops
from .fastmax import MAX_HEADS_PER_LAUNCH, _KERNEL_DTYPES, fastattention_einops, fp64_kernels

# A/B switches, read once: 0 runs linearmax with gradients as two autograd nodes instead of one / hands the block's K to the
# prologue per query head instead of per key head (tests use the routes behind them as references)
FUSED_TRAINING = os.environ.get("FASTMAX_LINEARMAX_FUSED_TRAIN", "1") != "0"
GROUPED_K = os.environ.get("FASTMAX_GROUPED_K", "1") != "0"


class LinearmaxPlan(NamedTuple):
    operator: str      # "fused_forward" (one pass over q, k, v, no autograd node), "one_node" (_LinearmaxP1), "two_node" (two
    #                    _NormalizeQK nodes + fastattention_einops), "unmasked" (two _NormalizeQK nodes + _UnmaskedNk)
    prologue: str      # where q, k are normalised: "in_scan" (by the scan kernels while they stage their tiles), "cast" (the
    #                    kernels of fastmax_normalize.hip, in the input dtype) or "tensor_ops" (float64: differentiable float64
    #                    tensor ops on the device, in front of the float64 kernels)
    prologue_bwd: str  # the sides whose prologue backward the scan kernels finish themselves: "both", "q" (grouped heads: the
    #                    group's dk' are summed by the prologue's own backward pass) or "none" (off the one-node route)
    k_layout: str      # "per_head", or K at its G key heads: "group_copies" (the prologue's store writes the G * rep normalised
    #                    copies) / "group_views" (q, v are (B*G, rep, N, D), K is viewed the same way: nothing is copied)
    slices: int        # batch slices the call is cut into (heads are independent; a launch takes 65535 of them)


def linearmax_plan(dtype, B, H, Nq, Nk, D, p=1, mask=True, needs_grad=False, rep=1, views=False, train_supported=None,
                   fp64_kernels=False):
    """The one decision "which nodes and kernels run for this linearmax call", from plain data (no tensor is touched).
    dtype: of q (anything but bf16 / fp16 computes in fp32); B, H: batch and heads of q AS LAUNCHED ((B*G, rep) beside group
    views); needs_grad: grad mode is on and one of q, k, v asks for a gradient; rep: query heads per key head when K arrives at
    its G groups (fastmax_hack_grouped: the training route, masked, whatever needs_grad says), else 1; views: q, v arrive as
    (B*G, rep, N, D) group views; train_supported: fastmax_hip_linearmax_train_supported's answer (host arithmetic) -- None asks
    the library, and only where the answer is needed.  Where the inputs live is not an argument: CPU tensors are moved to the
    device and take the same route.  A plan the library then rejects raises (_lib.check).  Launch-bound calls pay for every host
    instruction, so the answer is kept per argument tuple; the two things it reads besides its arguments are part of that tuple.
    fp64_kernels: float64 inputs run float64 end to end ("two_node" / "unmasked" with the "tensor_ops" prologue).  fastmax_hack
    passes fastmax.FP64_KERNELS; a caller that does not ask (the attention block) keeps the float32-arithmetic route for float64."""
    return _plan(dtype, B, H, Nq, Nk, D, p, mask, needs_grad, rep, views, train_supported, FUSED_TRAINING, ops._force_path,
                 bool(fp64_kernels))


@functools.lru_cache(maxsize=4096)
def _plan(dtype, B, H, Nq, Nk, D, p, mask, needs_grad, rep, views, train_supported, fused_training, forced_path, fp64_kernels):
    """linearmax_plan's rules (forced_path: the kernel family ops.set_forced_path forces, which the library's answer reads;
    fp64_kernels: fastmax.FP64_KERNELS)"""
    if D > ops.MAX_HEAD_SIZE:
        raise NotImplementedError(f"head size {D} > {ops.MAX_HEAD_SIZE} is not supported by the HIP kernels")
    if dtype == torch.float64 and fp64_kernels and rep == 1:
        slices = 1 if B * H <= MAX_HEADS_PER_LAUNCH or B == 1 else -(-B // max(1, MAX_HEADS_PER_LAUNCH // H))
        return LinearmaxPlan("two_node" if mask else "unmasked", "tensor_ops", "none", "per_head", slices)
    kdt = dtype if dtype in _KERNEL_DTYPES else torch.float32
    k_layout = "per_head" if rep == 1 else ("group_views" if views else "group_copies")
    slices = 1
    if rep == 1 and B * H > MAX_HEADS_PER_LAUNCH and B > 1:
        step = max(1, MAX_HEADS_PER_LAUNCH // H)
        slices, B = -(-B // step), step
    # the scan kernels with the prologue inside: first order, masked, D <= 128 in whole 16-byte pieces (what the library's
    # linearmax_fwd_check comes to once ops._prep has aligned the operands)
    in_scan = mask and p == 1 and D <= 128 and (D * kdt.itemsize) % 16 == 0 and B * H <= MAX_HEADS_PER_LAUNCH
    if in_scan and rep == 1 and not needs_grad:
        return LinearmaxPlan("fused_forward", "in_scan", "none", k_layout, slices)
    if in_scan and fused_training and k_layout != "group_copies":
        if ops.linearmax_train_supported(kdt, B, H, Nq, D) if train_supported is None else train_supported:
            return LinearmaxPlan("one_node", "in_scan", "both" if rep == 1 else "q", k_layout, slices)
    return LinearmaxPlan("two_node" if mask else "unmasked", "cast", "none", k_layout, slices)


class _NormalizeQK(torch.autograd.Function):
    """y = (x - mean_D x) / max_n ||x_n - mean_D x_n||   (fastmax_hack.py:38-43), in x's dtype; forward and backward
    in libfastmax_hip.so (fastmax_normalize.hip): the plan's "cast" prologue."""

    @staticmethod
    def forward(ctx, x, rep=1, view=False):
        """rep > 1 (x holds the G key heads of grouped-query attention): the result serves the G * rep query heads -- as
        copies (B, G*rep, N, D) written by the prologue's store, or with ``view`` as a stride-0 view (B*G, rep, N, D) of
        the G normalised heads (nothing is copied; the attention kernels' strides do the group indexing).  Either way the
        gradient arrives per query head and the backward pass sums a group while it reads."""
        y, inv = ops.normalize_cast(x, 1 if view else rep)
        ctx.save_for_backward(x, inv)
        ctx.rep = rep
        return _group_view(y, rep) if view else y

    @staticmethod
    def backward(ctx, gy):
        x, inv = ctx.saved_tensors
        return ops.normalize_backward(x, gy, inv, ctx.rep), None, None


class _LinearmaxP1(torch.autograd.Function):
    """Masked first-order linearmax (fastmax_hack.py:36-60) as ONE autograd node on the raw q, k, v: the prologue is applied by
    the scan kernels while they stage their tiles, forwards and backwards, so no normalised copy of q or k is written or kept
    (the two normalize_cast passes and the separate statistics passes of the two-node route disappear); its gradient is the
    one-pass prologue backward on the scans' dq, dk.  ``rep`` > 1 (grouped-query heads): k holds the G key heads, q and v are
    (B*G, rep, N, D) (v a stride-0 group view): K is viewed the same way, every query head of a group computes the group's
    statistics from the same rows, and the prologue backward sums the group's gradients while it reads them."""

    @staticmethod
    def forward(ctx, q, k, v, rep, prologue_bwd):
        q, k, v = (ops._prep(t, t.device) for t in (q, k, v))
        o, g, inv_q, inv_k, states, nstar = ops.linearmax_forward_fused(q, _group_view(k, rep), v, train=True)
        ctx.save_for_backward(q, k, v, o, g, inv_q, inv_k)
        ctx.states, ctx.nstar, ctx.rep = states, nstar, rep
        ctx.fuse = {"both": 3, "q": 2}[prologue_bwd]          # the C entry point's flags: bit 1 the dQ kernel, bit 0 the dK/dV kernel
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, g, inv_q, inv_k = ctx.saved_tensors
        rep = ctx.rep
        go = ops._prep(go.to(q.dtype), q.device)
        # dq leaves the dQ kernel as the gradient wrt the raw q; so does dk unless the group's dk' still have to be summed
        dq, dk, dv = ops.linearmax_backward(q, _group_view(k, rep), v, o, g, go, inv_q, inv_k, ctx.states, nstar=ctx.nstar,
                                            fuse=ctx.fuse)
        ctx.states = ctx.nstar = None
        if not ctx.fuse & 1:
            B, G, N, D = k.shape
            inv_g = inv_k.view(B * G, rep)[:, 0].contiguous().view(B, G)
            dk = ops.normalize_backward(k, dk.view(B, G * rep, N, D), inv_g, rep)
        return dq, dk, dv, None, None


def _group_view(k, rep):
    """k (B, G, N, D) as the stride-0 view (B*G, rep, N, D) the kernels read beside grouped queries"""
    if rep == 1:
        return k
    B, G, N, D = k.shape
    return k.view(B * G, 1, N, D).expand(B * G, rep, N, D)


def fastmax_hack(q, k, v, p=1, mask=True):
    """linearmax (reference: fastmax_hack.py:5)."""
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    B, H, Nq, D = q.shape
    return linearmax(q, k, v, _plan(q.dtype, B, H, Nq, k.shape[2], D, p, mask, needs_grad, 1, False, None, FUSED_TRAINING,
                                    ops._force_path, fp64_kernels()), p, mask)


def linearmax(q, k, v, plan, p=1, mask=True):
    """fastmax_hack for a caller that holds the call's linearmax_plan record (k_layout "per_head")"""
    if plan.slices > 1:
        step = max(1, MAX_HEADS_PER_LAUNCH // q.shape[1])          # heads are independent: run the batch in slices
        return torch.cat([linearmax(q[i:i + step], k[i:i + step], v[i:i + step], plan._replace(slices=1), p, mask)
                          for i in range(0, q.shape[0], step)], dim=0)
    dev = ops._device() if q.device.type != "cuda" else q.device
    home, in_dtype = q.device, q.dtype
    if plan.prologue == "tensor_ops":
        assert fp64_kernels(), "a float64 prologue in front of float32 kernels: the plan was made with fp64_kernels=True while fastmax.FP64_KERNELS is off"
        # float64 end to end: the prologue as tensor ops autograd differentiates, the attention in the float64 kernels
        qn, kn = _normalize_tensor_ops(q.to(dev)), _normalize_tensor_ops(k.to(dev))
        if plan.operator == "unmasked":
            return _UnmaskedNk.apply(qn, kn, v.to(dev), float(k.shape[2])).to(home)
        return fastattention_einops.apply(qn, kn, v.to(dev), True, 1, True, p, 0.0, False).to(home)
    kdt = in_dtype if in_dtype in _KERNEL_DTYPES else torch.float32
    qd, kd, vd = (ops._prep(t.to(kdt), dev) for t in (q, k, v))
    if plan.operator == "fused_forward":
        # inference / forward-only: prologue fused into the matrix-core kernel, one pass over Q, K, V
        return ops.linearmax_forward_fused(qd, kd, vd).to(device=home, dtype=in_dtype)
    if plan.operator == "one_node":
        return _LinearmaxP1.apply(qd, kd, vd, 1, plan.prologue_bwd).to(device=home, dtype=in_dtype)
    # prologue and attention as separate autograd nodes; 16-bit inputs keep their dtype between the two, like the reference
    qn, kn = _NormalizeQK.apply(qd), _NormalizeQK.apply(kd)
    if plan.operator == "unmasked":
        # fastmax_hack.py:6-33: first order whatever p is; constant term N_k; result float32 for
        # low-precision inputs (float32 ones at line 21), float64 stays float64
        o = _UnmaskedNk.apply(qn, kn, vd, float(k.shape[2]))
        out_dt = torch.float64 if in_dtype == torch.float64 else torch.float32
    else:
        o = fastattention_einops.apply(qn, kn, vd, True, 1, True, p, 0.0, False)
        out_dt = in_dtype
    return o.to(device=home, dtype=out_dt)


def fastmax_hack_grouped(q, k_groups, v, rep, p=1, plan=None):
    """Masked linearmax for grouped-query attention on the training route: k_groups (B,G,N,D) with H = G * rep query heads.
    Same values as fastmax_hack(q, expand(k_groups), v, p, mask=True): the max-norm statistics of identical head copies
    are identical, so the prologue runs once per key head (the reference expands first, model.py:404-411, and normalises
    every copy, fastmax_hack.py:38-43).  Two layouts (the plan's k_layout; without ``plan`` it is read off q's shape):
      q, v (B,H,N,D) with v already repeated         -> the prologue's store writes the H normalised copies of K
      q, v (B*G, rep, N, D) (v a stride-0 group view) -> K is normalised at its G heads and handed on as a stride-0 view too:
                                                        no per-query-head copy of K or V exists anywhere"""
    if plan is None:
        views = rep > 1 and q.shape[:2] == (k_groups.shape[0] * k_groups.shape[1], rep)
        plan = linearmax_plan(q.dtype, *q.shape[:3], k_groups.shape[2], q.shape[3], p, True, True, rep, views)
    if plan.operator == "one_node":
        return _LinearmaxP1.apply(q, k_groups, v, rep, plan.prologue_bwd).to(q.dtype)
    qn = _NormalizeQK.apply(q)
    kn = _NormalizeQK.apply(k_groups, rep, plan.k_layout == "group_views")
    return fastattention_einops.apply(qn, kn, v, True, 1, True, p, 0.0, False).to(q.dtype)


def _normalize_tensor_ops(x):
    """the prologue (fastmax_hack.py:38-43 / 10-15) as differentiable tensor ops in x's dtype: the float64 route"""
    x = x - x.mean(-1, keepdim=True)
    return x / torch.linalg.norm(x, dim=3).max(dim=2).values[..., None, None]


class _UnmaskedNk(torch.autograd.Function):
    """Unmasked p=1 fastmax with nt=1 and the denominator constant g0 = N_k (fastmax_hack.py:17-31); float64 inputs (the
    plan's "tensor_ops" prologue) stay float64, everything else computes in float32."""

    @staticmethod
    def forward(ctx, q, k, v, g0):
        cdt = torch.float64 if q.dtype == torch.float64 else torch.float32
        q, k, v = (ops._prep(t.detach().to(cdt), q.device) for t in (q, k, v))
        o, g = ops.forward(q, k, v, 1, False, 1.0, g0, cdt)
        ctx.save_for_backward(q, k, v, o, g)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, g = ctx.saved_tensors
        dq, dk, dv = ops.backward(q, k, v, o, g, ops._prep(go.to(q.dtype), q.device), 1, False, 1.0)
        return dq, dk, dv, None
