"""The mixture-of-experts MLP (lit_gpt/model.py:644-674, LoRA wiring lit_gpt/lora.py:711-730): top-k routing, token dispatch
and combine in HIP around the expert MLPs.

The reference routes with a ``topk``, a softmax and an (E, M, k) boolean mask, then per expert a ``torch.where`` (one host
synchronisation each), two fancy-index gathers and an indexed read-modify-write of ``y``.  Here csrc/moe.hip (C ABI:
include/fastmax_hip_moe.h, bound by ``_lib.ABI``) does the routing and a stable counting sort of the (token, expert) pairs in
one to three launches, gathers the tokens into per-expert runs of rows, and combines the experts' outputs with the reference's
rounding points.  The experts are ``block.LLaMAMLP`` (three ``LoRALinear``, NF4 after ``quantize_base``, the gated activation
kernel), each run on its slice of the gathered rows.

    route                  -> expert, prob, prob32 (M, k), offsets (E + 1), row_of (S), slot_of (M, k); a token's k entries in
                              ascending expert id, expert e owning slots offsets[e] .. offsets[e + 1], its tokens ascending
    gather                 xs[s] = x[row_of[s]]
    combine                y[t] = sum_j prob[t, j] ys[slot_of[t, j]], every product and every add rounded to the dtype
and the backward pass of each.  There is no CPU path through the kernels; ``fused_neighbours = False`` on the module selects the
reference's loop restated in tensor ops (A/B runs, parity tests, CPU).

At decode size (M <= 16 tokens, NF4 experts, no gradient) ``LLaMAMoE.device_routed = True`` replaces gather, the per-expert
calls and the ``cat`` by two launches that take their runs from ``offsets`` / ``row_of`` ON THE DEVICE (csrc/moe_decode.hip, C ABI
include/fastmax_hip_moe_decode.h, bound by ``_lib.ABI``), with the same bits:
    experts_up             h[s] = round(silu(fc_1_e(x[row_of[s]]))) * fc_2_e(x[row_of[s]])   for s in expert e's run
    experts_down           ys[s] = proj_e(h[s])
The experts' NF4 operands reach the kernels through a device table (``expert_table``).  Nothing is read back, so the layer can
be recorded in a graph (``generate.GraphedDecoder``).
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, block, lora, ops
from .block import _need_device, _rows
from .lora import LoRALinear, NF4Linear


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


# ---- the decode-size expert kernels on device-side row counts -----------------------------------------------------------------
class _LinearEntry(ctypes.Structure):
    """struct fastmax_moe_linear"""
    _fields_ = [("wq", ctypes.c_void_p), ("scales", lora.NF4Scales._C), ("bias", ctypes.c_void_p)]


class _ExpertEntry(ctypes.Structure):
    """struct fastmax_moe_expert_entry"""
    _fields_ = [("fc_1", _LinearEntry), ("fc_2", _LinearEntry), ("proj", _LinearEntry)]


ENTRY_BYTES = ctypes.sizeof(_ExpertEntry)
_DECODE_DTYPES = (torch.bfloat16, torch.float32)
_EXPERT_LINEARS = ("fc_1", "fc_2", "proj")


def _expert_bases(experts):
    """the experts' frozen layers in the table's order; a layer that is not an NF4Linear raises"""
    bases = [getattr(expert, n).linear for expert in experts for n in _EXPERT_LINEARS]
    for b in bases:
        if not isinstance(b, NF4Linear):
            raise RuntimeError("moe.expert_table: every expert linear should be an NF4Linear (quantize_base()), got "
                               f"{type(b).__name__}")
    return bases


def _table_tag(bases) -> tuple:
    """what the table's addresses depend on: every weight's (address, version, device), its scales' and its bias's address"""
    return tuple((b.weight.data_ptr(), b.weight._version, b.weight.device, b.weight.quant_state[0].data_ptr(),
                  None if b.bias is None else (b.bias.data_ptr(), b.bias.dtype)) for b in bases)


def expert_table(experts):
    """-> (table, keep): a uint8 device tensor of len(experts) ``fastmax_moe_expert_entry`` (fc_1, fc_2, proj of each expert: the
    codes' address, the ``scales_of(base)`` fields, the float32 bias or null) and the tensors its addresses point into.  Copies
    to the device (and, for double-quantised scales, may read one scalar back), so it cannot run while a stream is capturing."""
    bases = _expert_bases(experts)
    dev = bases[0].weight.device
    if dev.type != "cuda":
        raise RuntimeError("moe.expert_table runs on an MI355X only; there is no CPU path through the kernels")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("moe.expert_table: the experts' device table cannot be built while a stream is capturing (it is copied "
                           "from the host); run the layer once eagerly before the recording")
    if _lib.lib().fastmax_hip_moe_expert_entry_bytes() != ENTRY_BYTES:
        raise RuntimeError(f"moe.expert_table: the library's fastmax_moe_expert_entry has "
                           f"{_lib.lib().fastmax_hip_moe_expert_entry_bytes()} bytes, the packer's {ENTRY_BYTES}")
    keep, linears = [], []
    for b in bases:
        if b.weight.device != dev or b.weight.data_ptr() % 16:
            raise RuntimeError("moe.expert_table: the experts' codes should sit on one device, 16-byte aligned")
        sc, bias = lora.scales_of(b), lora._bias32(b)
        if bias is not None and bias.data_ptr() % 16:
            bias = bias.clone()
        keep += [b.weight.data, sc, bias]
        linears.append(_LinearEntry(b.weight.data_ptr(), sc.c, None if bias is None else bias.data_ptr()))
    host = (_ExpertEntry * len(experts))(*(_ExpertEntry(*linears[3 * e:3 * e + 3]) for e in range(len(experts))))
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    return table, keep


def _check_decode(what: str, x2: torch.Tensor, table: torch.Tensor, offsets: torch.Tensor, k: int, row_of=None, slots=0) -> int:
    _need_device(x2, what)
    for name, t, n in (("offsets", offsets, None), ("row_of", row_of, slots)):
        if t is not None and (t.dim() != 1 or t.dtype != torch.int32 or t.device != x2.device or not t.is_contiguous()
                              or (n is not None and t.shape[0] != n)):
            raise ValueError(f"{what}: {name} should be a dense int32 vector{'' if n is None else f' of {n} slots'} on {x2.device}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    E = offsets.shape[0] - 1
    if x2.dtype not in _DECODE_DTYPES:
        raise TypeError(f"{what}: dtype {x2.dtype} is not bfloat16 or float32")
    if table.dtype != torch.uint8 or table.numel() != E * ENTRY_BYTES or table.device != x2.device:
        raise ValueError(f"{what}: table should hold {E} entries of {ENTRY_BYTES} bytes on {x2.device}, got {table.numel()} bytes "
                         f"on {table.device}")
    _check_sizes(what, E, k)
    return E


def _decode_out(what: str, out, shape, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous():
        raise ValueError(f"{what}: out should be a contiguous {tuple(shape)} {like.dtype} tensor on {like.device}, got "
                         f"{tuple(out.shape)} {out.dtype} on {out.device}")
    return out


def experts_up(x2: torch.Tensor, table: torch.Tensor, offsets: torch.Tensor, row_of: torch.Tensor, k: int,
               intermediate_size: int, out: torch.Tensor = None) -> torch.Tensor:
    """x2 (M, C), M <= 16; table from ``expert_table``; offsets (E + 1), row_of (M k) from ``route`` ->
    h (M k, I): h[s] = round(silu(fc_1_e(x2[row_of[s]]))) * fc_2_e(x2[row_of[s]]) for the slots s of expert e.  Nothing is read back."""
    M, C = x2.shape
    E = _check_decode("moe.experts_up", x2, table, offsets, k, row_of, M * k)
    x2 = lora._rows(x2, C)
    h = _decode_out("moe.experts_up", out, (M * k, intermediate_size), x2)
    ops._call("fastmax_hip_moe_experts_up", x2.device,
              (x2.data_ptr(), x2.stride(0), table.data_ptr(), offsets.data_ptr(), row_of.data_ptr(), h.data_ptr(), h.stride(0), M, E, k,
               C, intermediate_size, ops._DT[x2.dtype]))
    return h


def experts_down(h: torch.Tensor, table: torch.Tensor, offsets: torch.Tensor, k: int, n_embd: int,
                 out: torch.Tensor = None) -> torch.Tensor:
    """h (M k, I) from ``experts_up`` -> ys (M k, C): ys[s] = proj_e(h[s]) over the same runs"""
    E = _check_decode("moe.experts_down", h, table, offsets, k)
    S, I = h.shape
    if S % k:
        raise ValueError(f"moe.experts_down: h should have M k rows, got {S} with k = {k}")
    h = lora._rows(h, I)
    ys = _decode_out("moe.experts_down", out, (S, n_embd), h)
    ops._call("fastmax_hip_moe_experts_down", h.device,
              (h.data_ptr(), h.stride(0), table.data_ptr(), offsets.data_ptr(), ys.data_ptr(), ys.stride(0), S // k, E, k, n_embd, I,
               ops._DT[h.dtype]))
    return ys


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
    pass reads nothing back.  An expert without tokens is not called, and its parameters get no gradient from that call.

    ``device_routed`` (default off): a call of at most 16 tokens in bfloat16 or float32 that needs no gradient runs
    gate -> route -> experts_up -> experts_down -> combine, five launches behind the gate product with nothing read back, and
    gives the bits of the route above.  It reads the experts' NF4 codes whatever ``cache_dense`` copies they hold.  Every other
    call goes the way it went."""

    def __init__(self, n_embd: int, intermediate_size: int, n_expert: int, n_expert_per_token: int, bias: bool = False, r: int = 0,
                 alpha: int = 1, dropout: float = 0.0, to_mlp: bool = False) -> None:
        super().__init__()
        _check_sizes("LLaMAMoE", n_expert, n_expert_per_token)
        self.gate = LoRALinear(n_embd, n_expert, bias=False, r=(r if to_mlp else 0), lora_alpha=alpha, lora_dropout=dropout)
        self.experts = nn.ModuleList(block.LLaMAMLP(n_embd, intermediate_size, bias=bias, r=r, alpha=alpha, dropout=dropout,
                                                    to_mlp=to_mlp) for _ in range(n_expert))
        self.n_expert, self.n_expert_per_token = n_expert, n_expert_per_token
        self.n_embd, self.intermediate_size = n_embd, intermediate_size
        self._fused = True
        self._device_routed = False
        self._table = None                           # (tag, table, the tensors it points into)

    @property
    def fused_neighbours(self) -> bool:
        return self._fused

    @fused_neighbours.setter
    def fused_neighbours(self, on: bool) -> None:
        """the routing kernels and the experts' gated-activation kernel on or off together"""
        self._fused = bool(on)
        for expert in self.experts:
            expert.fused_neighbours = self._fused

    @property
    def device_routed(self) -> bool:
        return self._device_routed

    @device_routed.setter
    def device_routed(self, on: bool) -> None:
        """the decode-size route on device-side row counts; refused unless the experts are what its kernels compute"""
        if on:
            linears = [getattr(expert, n) for expert in self.experts for n in _EXPERT_LINEARS]
            if not all(isinstance(lin.linear, NF4Linear) for lin in linears):
                raise ValueError("LLaMAMoE.device_routed: the experts are dense; the decode kernels read NF4 weights, so call "
                                 "quantize_base() first")
            if any(lin.r > 0 for lin in linears):
                raise ValueError("LLaMAMoE.device_routed: the experts carry an active LoRA branch (r > 0 with to_mlp=True), "
                                 "which the decode kernels do not compute")
            if self.n_embd % 128 or self.intermediate_size % 128:
                raise ValueError(f"LLaMAMoE.device_routed: n_embd and intermediate_size should be multiples of 128, got "
                                 f"{self.n_embd} and {self.intermediate_size}")
        self._device_routed = bool(on)

    def expert_table(self) -> torch.Tensor:
        """the experts' device table, rebuilt when a weight moved or was written (never during a stream capture)"""
        tag = _table_tag(_expert_bases(self.experts))
        if self._table is None or self._table[0] != tag:
            table, keep = expert_table(self.experts)
            self._table = (tag, table, keep)
        return self._table[1]

    def _takes_device_route(self, x2: torch.Tensor) -> bool:
        if not (self._device_routed and self._fused) or x2.shape[0] > _lib.MOE_DECODE_MAX_ROWS or x2.dtype not in _DECODE_DTYPES:
            return False
        return not (torch.is_grad_enabled() and (x2.requires_grad or any(p.requires_grad for p in self.parameters())))

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
        if self._takes_device_route(x2):
            k = self.n_expert_per_token
            _, prob, _, offsets, row_of, slot_of = route(self.gate(x2), k)
            table = self.expert_table()
            h = experts_up(x2, table, offsets, row_of, k, self.intermediate_size)
            return combine(experts_down(h, table, offsets, k, C), prob, slot_of).view(x.shape)
        prob, _, _, offsets, row_of, slot_of = _RouteFn.apply(self.gate(x2), self.n_expert_per_token)
        bounds = _read_offsets(offsets)
        xs = _GatherFn.apply(x2, row_of, slot_of)
        runs = torch.split(xs, [b - a for a, b in zip(bounds, bounds[1:])])
        ys = torch.cat([expert(rows) for expert, rows in zip(self.experts, runs) if rows.shape[0]])
        return _CombineFn.apply(ys, prob, slot_of).view(x.shape)
