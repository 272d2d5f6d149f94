"""The mixture-of-experts MLP (lit_gpt/model.py:644-674, LoRA wiring lit_gpt/lora.py:711-730): top-k routing, token dispatch
and combine in HIP around the expert MLPs.

The reference routes with a ``topk``, a softmax and an (E, M, k) boolean mask, then per expert a ``torch.where`` (one host
synchronisation each), two fancy-index gathers and an indexed read-modify-write of ``y``.  Here csrc/moe.hip (C ABI:
include/fastmax_hip_moe.h, bound by ``_lib.MOE_ABI``) does the routing and a stable counting sort of the (token, expert) pairs in
one to three launches, gathers the tokens into per-expert runs of rows, and combines the experts' outputs with the reference's
rounding points.  The experts are ``block.LLaMAMLP`` (three ``LoRALinear``, NF4 after ``quantize_base``, the gated activation
kernel), each run on its slice of the gathered rows.

    route                  -> expert, prob, prob32 (M, k), offsets (E + 1), row_of (S), slot_of (M, k); a token's k entries in
                              ascending expert id, expert e owning slots offsets[e] .. offsets[e + 1], its tokens ascending
    gather                 xs[s] = x[row_of[s]]
    combine                y[t] = sum_j prob[t, j] ys[slot_of[t, j]], every product and every add rounded to the dtype
and the backward pass of each.  There is no CPU path through the kernels; ``fused_neighbours = False`` on the module selects the
reference's loop restated in tensor ops (A/B runs, parity tests, CPU).
"""
import torch
import torch.nn as nn

from . import _lib, block, ops
from .block import _need_device, _rows
from .lora import LoRALinear


def _check_sizes(what: str, n_expert: int, n_expert_per_token: int) -> None:
    if not 1 <= n_expert_per_token <= _lib.MOE_MAX_PER_TOKEN:
        raise ValueError(f"{what}: n_expert_per_token should be in 1 .. {_lib.MOE_MAX_PER_TOKEN}, got {n_expert_per_token}")
    if n_expert > _lib.MOE_MAX_EXPERTS:
        raise ValueError(f"{what}: n_expert should be at most {_lib.MOE_MAX_EXPERTS}, got {n_expert}")
    if n_expert_per_token > n_expert:
        raise ValueError(f"{what}: n_expert_per_token ({n_expert_per_token}) exceeds n_expert ({n_expert})")


# ---- kernel calls -------------------------------------------------------------------------------------------------------------
def route(router: torch.Tensor, k: int):
    """router (M, E) -> (expert, prob, prob32, offsets, row_of, slot_of); see the module's docstring.  Nothing is read back."""
    if router.dim() != 2 or router.numel() == 0:
        raise ValueError(f"moe.route: router should be (M, E), got {tuple(router.shape)}")
    M, E = router.shape
    _check_sizes("moe.route", E, k)
    _need_device(router, "moe.route")
    r2, dev = _rows(router, E), router.device
    ints = dict(dtype=torch.int32, device=dev)
    expert, slot_of = torch.empty((M, k), **ints), torch.empty((M, k), **ints)
    offsets, row_of = torch.empty(E + 1, **ints), torch.empty(M * k, **ints)
    prob = torch.empty((M, k), dtype=router.dtype, device=dev)
    prob32 = torch.empty((M, k), dtype=torch.float32, device=dev)
    ops._call("fastmax_hip_moe_route", dev,
              (r2.data_ptr(), r2.stride(0), expert.data_ptr(), prob.data_ptr(), prob32.data_ptr(), offsets.data_ptr(),
               row_of.data_ptr(), slot_of.data_ptr(), M, E, k, ops._DT[router.dtype]),
              ws=int(_lib.lib().fastmax_hip_moe_route_workspace(M, E)))
    return expert, prob, prob32, offsets, row_of, slot_of


def gather(x: torch.Tensor, row_of: torch.Tensor) -> torch.Tensor:
    """x (M, C), row_of (S,) int32 -> xs (S, C) = x[row_of], bit for bit"""
    _need_device(x, "moe.gather")
    M, C = x.shape
    x2, S = _rows(x, C), row_of.shape[0]
    xs = torch.empty((S, C), dtype=x.dtype, device=x.device)
    ops._call("fastmax_hip_moe_gather", x.device,
              (x2.data_ptr(), x2.stride(0), row_of.data_ptr(), xs.data_ptr(), xs.stride(0), M, S, C, ops._DT[x.dtype]))
    return xs


def _slot_sum(name: str, src, prob, slot_of) -> torch.Tensor:
    _need_device(src, "moe." + name)
    C, (M, k) = src.shape[1], slot_of.shape
    s2 = _rows(src, C)
    out = torch.empty((M, C), dtype=src.dtype, device=src.device)
    weights = () if prob is None else (prob.data_ptr(),)
    ops._call("fastmax_hip_moe_" + name, src.device,
              (s2.data_ptr(), s2.stride(0), *weights, slot_of.data_ptr(), out.data_ptr(), out.stride(0), M, k, C, ops._DT[src.dtype]))
    return out


def combine(ys: torch.Tensor, prob: torch.Tensor, slot_of: torch.Tensor) -> torch.Tensor:
    """ys (S, C), prob (M, k) in ys's dtype, slot_of (M, k) int32 -> y (M, C)"""
    if prob.dtype != ys.dtype or prob.shape != slot_of.shape:
        raise ValueError(f"moe.combine: prob should be {tuple(slot_of.shape)} {ys.dtype}, got {tuple(prob.shape)} {prob.dtype}")
    return _slot_sum("combine", ys, prob.contiguous(), slot_of)


def gather_backward(dxs: torch.Tensor, slot_of: torch.Tensor) -> torch.Tensor:
    """dxs (S, C) -> dx (M, C): the float32 sum of a token's k slots, j ascending, rounded once"""
    return _slot_sum("gather_backward", dxs, None, slot_of)


def combine_backward(dy: torch.Tensor, ys: torch.Tensor, prob: torch.Tensor, slot_of: torch.Tensor):
    """-> (dys (S, C), dprob (M, k)) in one pass over dy and ys"""
    _need_device(dy, "moe.combine_backward")
    C, (M, k) = ys.shape[1], slot_of.shape
    dy2, ys2, p = _rows(dy, C), _rows(ys, C), prob.contiguous()
    dys = torch.empty((ys.shape[0], C), dtype=ys.dtype, device=ys.device)
    dprob = torch.empty((M, k), dtype=ys.dtype, device=ys.device)
    ops._call("fastmax_hip_moe_combine_backward", ys.device,
              (dy2.data_ptr(), dy2.stride(0), ys2.data_ptr(), ys2.stride(0), p.data_ptr(), slot_of.data_ptr(), dys.data_ptr(),
               dys.stride(0), dprob.data_ptr(), M, k, C, ops._DT[ys.dtype]))
    return dys, dprob


def route_backward(dprob: torch.Tensor, prob32: torch.Tensor, expert: torch.Tensor, E: int) -> torch.Tensor:
    """the softmax's backward over the k selected values, scattered into an otherwise zero drouter (M, E)"""
    _need_device(dprob, "moe.route_backward")
    M, k = expert.shape
    g = dprob.contiguous()
    drouter = torch.empty((M, E), dtype=dprob.dtype, device=dprob.device)
    ops._call("fastmax_hip_moe_route_backward", dprob.device,
              (g.data_ptr(), prob32.data_ptr(), expert.data_ptr(), drouter.data_ptr(), drouter.stride(0), M, E, k,
               ops._DT[dprob.dtype]))
    return drouter


def _read_offsets(offsets: torch.Tensor) -> list:
    """the forward's one device-to-host copy: E + 1 integers"""
    return offsets.tolist()


# ---- autograd -------------------------------------------------------------------------------------------------------------------
class _RouteFn(torch.autograd.Function):
    """router -> (prob, expert, prob32, offsets, row_of, slot_of); only prob carries a gradient"""

    @staticmethod
    def forward(ctx, router, k):
        expert, prob, prob32, offsets, row_of, slot_of = route(router, k)
        ctx.save_for_backward(prob32, expert)
        ctx.E = router.shape[1]
        ctx.mark_non_differentiable(expert, prob32, offsets, row_of, slot_of)
        return prob, expert, prob32, offsets, row_of, slot_of

    @staticmethod
    def backward(ctx, dprob, *_):
        prob32, expert = ctx.saved_tensors
        return route_backward(dprob, prob32, expert, ctx.E), None


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, row_of, slot_of):
        ctx.save_for_backward(slot_of)
        return gather(x, row_of)

    @staticmethod
    def backward(ctx, dxs):
        (slot_of,) = ctx.saved_tensors
        return gather_backward(dxs, slot_of), None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ys, prob, slot_of):
        ctx.save_for_backward(ys, prob, slot_of)
        return combine(ys, prob, slot_of)

    @staticmethod
    def backward(ctx, dy):
        ys, prob, slot_of = ctx.saved_tensors
        dys, dprob = combine_backward(dy, ys, prob, slot_of)
        return dys, dprob, None


# ---- module ---------------------------------------------------------------------------------------------------------------------
class LLaMAMoE(nn.Module):
    """lit_gpt/model.py:644-674 with the LoRA wiring of lit_gpt/lora.py:711-730.  Members ``gate`` and ``experts`` as in the
    reference, so its state dict keys carry over (``gate.linear.weight``, ``experts.3.fc_1.linear.weight``, ...).

    With ``fused_neighbours`` the forward pass reads E + 1 integers back from the device ONCE per call (the experts' row counts,
    which size the experts' matrix products); the reference pays one ``torch.where`` read per expert, E per call.  The backward
    pass reads nothing back.  An expert without tokens is not called, and its parameters get no gradient from that call."""

    def __init__(self, n_embd: int, intermediate_size: int, n_expert: int, n_expert_per_token: int, bias: bool = False, r: int = 0,
                 alpha: int = 1, dropout: float = 0.0, to_mlp: bool = False) -> None:
        super().__init__()
        _check_sizes("LLaMAMoE", n_expert, n_expert_per_token)
        self.gate = LoRALinear(n_embd, n_expert, bias=False, r=(r if to_mlp else 0), lora_alpha=alpha, lora_dropout=dropout)
        self.experts = nn.ModuleList(block.LLaMAMLP(n_embd, intermediate_size, bias=bias, r=r, alpha=alpha, dropout=dropout,
                                                    to_mlp=to_mlp) for _ in range(n_expert))
        self.n_expert, self.n_expert_per_token = n_expert, n_expert_per_token
        self._fused = True

    @property
    def fused_neighbours(self) -> bool:
        return self._fused

    @fused_neighbours.setter
    def fused_neighbours(self, on: bool) -> None:
        """the routing kernels and the experts' gated-activation kernel on or off together"""
        self._fused = bool(on)
        for expert in self.experts:
            expert.fused_neighbours = self._fused

    def quantize_base(self, double_quant: bool = False):
        """NF4 for the experts' linears.  The gate stays dense: its n_expert output columns are fewer than the NF4 kernels take
        (bitsandbytes would quantize it with the rest)."""
        for expert in self.experts:
            expert.quantize_base(double_quant)
        return self

    def _eager(self, x2: torch.Tensor) -> torch.Tensor:
        """model.py:661-673 in tensor ops: one ``torch.where`` read per expert.  As on the fused route an expert without tokens is
        not called (the reference calls it on no rows, for zero gradients; the NF4 kernels take no empty batch)"""
        top, chosen = torch.topk(self.gate(x2), self.n_expert_per_token)
        prob = top.softmax(dim=1, dtype=torch.float).to(x2.dtype)
        y = torch.zeros_like(x2)
        for e, expert in enumerate(self.experts):
            t, j = torch.where(chosen == e)                              # tokens ascending: the order of the kernels' slots
            if t.numel():
                y[t] += prob[t, j, None] * expert(x2[t])
        return y

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not self._fused:
            return self._eager(x2).view(x.shape)
        _need_device(x, "LLaMAMoE")
        prob, _, _, offsets, row_of, slot_of = _RouteFn.apply(self.gate(x2), self.n_expert_per_token)
        bounds = _read_offsets(offsets)
        xs = _GatherFn.apply(x2, row_of, slot_of)
        runs = torch.split(xs, [b - a for a, b in zip(bounds, bounds[1:])])
        ys = torch.cat([expert(rows) for expert, rows in zip(self.experts, runs) if rows.shape[0]])
        return _CombineFn.apply(ys, prob, slot_of).view(x.shape)
