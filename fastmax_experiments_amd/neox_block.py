"""The GPT-NeoX (pythia) decoder block around the attention sub-layer: the LayerNorm pair, the three-way residual add and the
ungated GELU MLP in HIP.

The reference's ``Block.forward`` (lit_gpt/model.py:340-361), parallel-residual form -- its ``Config`` defaults
(config.py:30-91: ``parallel_residual=True``, ``LayerNorm``, ``GptNeoxMLP``) and what the pythia checkpoints are:
    n_1 = norm_1(x);  h = attn(n_1);  n_2 = n_1 if shared_attention_norm else norm_2(x)
    x = mlp(n_2) + h + x
with ``torch.nn.LayerNorm`` and ``GptNeoxMLP`` (model.py:608-619: proj(gelu(fc(x)))).  ``CausalSelfAttention`` is
attention_block.py's; ``fc`` and ``proj`` are ``LoRALinear`` (NF4 base after ``quantize_base``).
What this file adds runs in csrc/neox_block.hip (C ABI: include/fastmax_hip_neox.h, bound by ``_lib.ABI``):
    layer_norm_pair    norm_1 and norm_2 of one block normalise the SAME row with the same eps: one pass computes mean and
                       rstd once and writes both outputs, optionally with the hand-over  s = mlp + h + x  of the block before
                       in front of it (3 row reads and 3 row writes where tensor ops take 6 and 4)
    gelu               exact GELU forward and a one-pass backward that recomputes it
Rounding points are the reference's: each add is rounded to the activation dtype, statistics are float32, the normalised and
scaled row is rounded ONCE (torch's LayerNorm).  There is no CPU path through the kernels; ``fused_neighbours = False`` on a
module selects the tensor-op restatement (A/B runs, parity tests).

The kernels are OPT-IN (``block.fused_neighbours = True``, or ``FUSED_NEIGHBOURS_DEFAULT`` for modules built afterwards): on an
MI355X they are ahead of the tensor ops at the pythia-1b width and behind them at pythia-70m, where the step is bound by the
host's time per call (profiles/r13_neox_block.md).

``NeoXStack`` / ``run_neox_blocks`` own the hand-over between blocks; only the last three-way add runs alone.  ``block.Block``
stays the sequential-residual form and keeps refusing this one: the two forms share no code path around the attention.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .attention_block import CausalSelfAttention
from .block import DecoderBlock, _act_operands, _need_device, _rows
from .lora import LoRALinear

FUSED_NEIGHBOURS_DEFAULT = False          # what ``fused_neighbours`` of a newly built module starts as

# ---- kernel calls -------------------------------------------------------------------------------------------------------------
def _check_ln_shapes(x, params, residuals):
    C = x.shape[-1] if x.dim() else 0
    if C == 0 or x.numel() == 0:
        raise ValueError(f"layer_norm: empty input of shape {tuple(x.shape)} (C = 0 or no rows)")
    wdt = params[0].dtype
    for name, t in zip(("weight", "bias", "weight2", "bias2"), params):
        if t is None:
            continue
        if t.dim() != 1 or t.shape[0] != C:
            raise ValueError(f"layer_norm: {name} should have {C} elements, got shape {tuple(t.shape)}")
        if t.dtype != wdt or (wdt != x.dtype and wdt != torch.float32):
            raise ValueError(f"layer_norm: the parameters should share {x.dtype} or float32, {name} is {t.dtype}")
    for name, r in zip(("r1", "r2"), residuals):
        if r is not None and (r.shape != x.shape or r.dtype != x.dtype):
            raise ValueError(f"layer_norm: {name} should match x ({tuple(x.shape)}, {x.dtype}), got {tuple(r.shape)}, {r.dtype}")
    if residuals[1] is not None and residuals[0] is None:
        raise ValueError("layer_norm: r2 needs r1")
    if params[3] is not None and params[2] is None:
        raise ValueError("layer_norm: bias2 needs weight2")


def layer_norm_forward(x, weight, bias=None, eps: float = 1e-5, r1=None, r2=None, weight2=None, bias2=None):
    """-> (s, y1, y2, mean, rstd): s = x, x + r1 or (r1 + r2) + x, each add rounded to x's dtype (x itself without r1);
    y_k = LayerNorm(s) under (weight_k, bias_k) in x's dtype (y2 is None without weight2); mean, rstd (M,) float32"""
    _check_ln_shapes(x, (weight, bias, weight2, bias2), (r1, r2))
    _need_device(x, "layer_norm")
    C, dev = x.shape[-1], x.device
    x2 = _rows(x, C)
    ra, rb = (None if r is None else _rows(r, C) for r in (r1, r2))
    w1, b1, w2, b2 = (None if t is None else t.contiguous() for t in (weight, bias, weight2, bias2))
    M = x2.shape[0]
    s2 = x2 if r1 is None else torch.empty((M, C), dtype=x.dtype, device=dev)
    y1 = torch.empty((M, C), dtype=x.dtype, device=dev)
    y2 = None if w2 is None else torch.empty((M, C), dtype=x.dtype, device=dev)
    mean, rstd = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(2))
    ops._call("fastmax_hip_layernorm_forward", dev,
              (x2.data_ptr(), x2.stride(0), ops._ptr(ra), 0 if ra is None else ra.stride(0), ops._ptr(rb),
               0 if rb is None else rb.stride(0), w1.data_ptr(), ops._ptr(b1), ops._ptr(w2), ops._ptr(b2),
               None if r1 is None else s2.data_ptr(), s2.stride(0), y1.data_ptr(), C, ops._ptr(y2), C, mean.data_ptr(),
               rstd.data_ptr(), M, C, float(eps), ops._DT[x.dtype], ops._DT[w1.dtype]))
    return (x if r1 is None else s2.view(x.shape)), y1.view(x.shape), None if y2 is None else y2.view(x.shape), mean, rstd


def layer_norm_backward_workspace(M: int, C: int, dtype, pair: bool, want_param_grads: bool) -> int:
    return int(_lib.lib().fastmax_hip_layernorm_backward_workspace(M, C, ops._DT[dtype], int(bool(pair)),
                                                                   int(bool(want_param_grads))))


def layer_norm_backward(dy1, s, weight, mean, rstd, dy2=None, weight2=None, ds_in=None, want=(False, False, False, False)):
    """-> (ds, dweight, dbias, dweight2, dbias2): ds in s's dtype, with ``ds_in`` (the incoming gradient of the residual
    stream) added; the parameter gradients asked for in ``want`` as (C,) float32, bitwise reproducible, the others None"""
    if (dy2 is None) != (weight2 is None):
        raise ValueError("layer_norm backward: dy2 and weight2 come together")
    if dy2 is None and (want[2] or want[3]):
        raise ValueError("layer_norm backward: the second norm's gradients need dy2 and weight2")
    _need_device(s, "layer_norm backward")
    C, dev = s.shape[-1], s.device
    s2 = _rows(s, C)
    d1 = _rows(dy1.to(s.dtype), C)
    d2 = None if dy2 is None else _rows(dy2.to(s.dtype), C)
    di = None if ds_in is None else _rows(ds_in.to(s.dtype), C)
    w1 = weight.contiguous()
    w2 = None if weight2 is None else weight2.contiguous()
    M = s2.shape[0]
    ds = torch.empty((M, C), dtype=s.dtype, device=dev)
    grads = [torch.empty(C, dtype=torch.float32, device=dev) if w else None for w in want]
    ws = layer_norm_backward_workspace(M, C, s.dtype, d2 is not None, any(want))
    ops._call("fastmax_hip_layernorm_backward", dev,
              (d1.data_ptr(), d1.stride(0), ops._ptr(d2), 0 if d2 is None else d2.stride(0), s2.data_ptr(), s2.stride(0),
               w1.data_ptr(), ops._ptr(w2), mean.data_ptr(), rstd.data_ptr(), ops._ptr(di), 0 if di is None else di.stride(0),
               ds.data_ptr(), C, *(ops._ptr(g) for g in grads), M, C, ops._DT[s.dtype], ops._DT[w1.dtype]), ws=ws)
    return (ds.view(s.shape), *grads)


def gelu_forward(a):
    """exact GELU a (1 + erf(a / sqrt 2)) / 2, rounded to a's dtype; a (..., I), any row stride"""
    I = a.shape[-1] if a.dim() else 0
    if I == 0 or a.numel() == 0:
        raise ValueError(f"gelu: empty input of shape {tuple(a.shape)}")
    (a2,) = _act_operands("gelu", I, a)
    y = torch.empty((a2.shape[0], I), dtype=a.dtype, device=a.device)
    ops._call("fastmax_hip_act_forward", a.device,
              (a2.data_ptr(), a2.stride(0), y.data_ptr(), I, a2.shape[0], I, _lib.NEOX_ACT_GELU, ops._DT[a.dtype]))
    return y.view(a.shape)


def gelu_backward(a, dy):
    """-> da = dy gelu'(a) in one pass over a and dy; gelu is recomputed"""
    I = a.shape[-1] if a.dim() else 0
    if I == 0 or a.numel() == 0:
        raise ValueError(f"gelu: empty input of shape {tuple(a.shape)}")
    a2, dy2 = _act_operands("gelu", I, a, dy)
    da = torch.empty((a2.shape[0], I), dtype=a.dtype, device=a.device)
    ops._call("fastmax_hip_act_backward", a.device,
              (a2.data_ptr(), a2.stride(0), dy2.data_ptr(), dy2.stride(0), da.data_ptr(), I, a2.shape[0], I, _lib.NEOX_ACT_GELU,
               ops._DT[a.dtype]))
    return da.view(a.shape)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
class _LayerNormPairFn(torch.autograd.Function):
    """(x, r1, r2, w1, b1, w2, b2) -> (y1[, y2][, s]): y2 with w2, s with r1.  Backward: ds = the LayerNorm backward of dy1
    and dy2 plus the gradient arriving at s (the fused adds' backward); it is the gradient of x, r1 and r2 alike.  Parameter
    gradients only for the parameters that ask (in LoRA fine-tuning the norms are frozen)."""

    @staticmethod
    def forward(ctx, x, r1, r2, w1, b1, w2, b2, eps):
        s, y1, y2, mean, rstd = layer_norm_forward(x, w1, b1, eps, r1, r2, w2, b2)
        ctx.save_for_backward(s, w1, w2, mean, rstd)
        ctx.pair, ctx.summed = w2 is not None, r1 is not None
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (w1, b1, w2, b2))
        return (y1,) + ((y2,) if ctx.pair else ()) + ((s,) if ctx.summed else ())

    @staticmethod
    def backward(ctx, *grads):
        s, w1, w2, mean, rstd = ctx.saved_tensors
        grads = list(grads)
        gy1 = grads.pop(0)
        gy2 = grads.pop(0) if ctx.pair else None
        gs = grads.pop(0) if ctx.summed else None
        if gy1 is None:
            gy1 = torch.zeros_like(s)
        if ctx.pair and gy2 is None:
            gy2 = torch.zeros_like(s)
        want = tuple(bool(ctx.needs_input_grad[i]) and ctx.dtypes[i - 3] is not None for i in (3, 4, 5, 6))
        ds, *pg = layer_norm_backward(gy1, s, w1, mean, rstd, gy2, w2, gs, want)
        pg = [None if g is None else g.to(dt) for g, dt in zip(pg, ctx.dtypes)]
        return (ds, ds if ctx.summed else None, ds if ctx.needs_input_grad[2] else None, *pg, None)


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return gelu_forward(a)

    @staticmethod
    def backward(ctx, dy):
        (a,) = ctx.saved_tensors
        return gelu_backward(a, dy)


def gelu(a):
    return _GeluFn.apply(a)


# ---- modules -----------------------------------------------------------------------------------------------------------------
class LayerNorm(nn.Module):
    """``torch.nn.LayerNorm(size, eps=eps)`` (what ``Config.norm_class`` resolves to): same parameter names (``weight``,
    ``bias``), so its checkpoints load."""

    def __init__(self, size: int, eps: float = 1e-5) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(size))
        self.bias = nn.Parameter(torch.zeros(size))
        self.eps = eps
        self.fused_neighbours = FUSED_NEIGHBOURS_DEFAULT          # False: F.layer_norm

    def _eager(self, x: torch.Tensor) -> torch.Tensor:
        if x.device.type != "cpu" and self.weight.dtype != x.dtype:
            # torch's device LayerNorm wants one dtype; float32 arithmetic and one rounding is what its CPU kernel computes
            return F.layer_norm(x.float(), x.shape[-1:], self.weight.float(), self.bias.float(), self.eps).to(x.dtype)
        return F.layer_norm(x, x.shape[-1:], self.weight, self.bias, self.eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.fused_neighbours:
            return self._eager(x)
        return _LayerNormPairFn.apply(x, None, None, self.weight, self.bias, None, None, self.eps)[0]

    def reset_parameters(self) -> None:
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)


def layer_norm_pair(x: torch.Tensor, norm_1: LayerNorm, norm_2: LayerNorm = None, r1=None, r2=None):
    """-> (s, y1, y2) as one autograd node: s = x, x + r1 or (r1 + r2) + x (the residual stream, in the tensors' dtype),
    y1 = norm_1(s), y2 = norm_2(s) from the same statistics (``norm_2 = None``, the shared attention norm: y2 is y1 and a
    single output is written)"""
    if r2 is not None and r1 is None:
        raise ValueError("layer_norm_pair: r2 needs r1")
    if norm_2 is not None and norm_2.eps != norm_1.eps:
        raise ValueError(f"layer_norm_pair: the two norms share their statistics, eps differs ({norm_1.eps}, {norm_2.eps})")
    if not norm_1.fused_neighbours:
        s = x if r1 is None else (x + r1 if r2 is None else r1 + r2 + x)
        y1 = norm_1._eager(s)
        return s, y1, (y1 if norm_2 is None else norm_2._eager(s))
    w2, b2 = (None, None) if norm_2 is None else (norm_2.weight, norm_2.bias)
    out = list(_LayerNormPairFn.apply(x, r1, r2, norm_1.weight, norm_1.bias, w2, b2, norm_1.eps))
    y1 = out.pop(0)
    y2 = y1 if norm_2 is None else out.pop(0)
    return (x if r1 is None else out.pop(0)), y1, y2


class GptNeoxMLP(nn.Module):
    """proj(gelu(fc(x))), exact GELU -- lit_gpt/model.py:608-619 with the LoRA wiring of lit_gpt/lora.py (``fc`` and ``proj``
    are ``LoRALinear``: state-dict keys ``fc.linear.weight``, ``fc.lora_A`` ...).  The bias of ``fc`` stays in the linear."""

    def __init__(self, n_embd: int, intermediate_size: int, bias: bool = True, r: int = 0, alpha: int = 1, dropout: float = 0.0,
                 to_mlp: bool = False, gelu_approximate: str = "none") -> None:
        super().__init__()
        if gelu_approximate != "none":
            raise NotImplementedError(f"GptNeoxMLP: gelu_approximate={gelu_approximate!r} is not built; only the exact GELU "
                                      "(\"none\") has kernels")
        kw = dict(bias=bias, r=(r if to_mlp else 0), lora_alpha=alpha, lora_dropout=dropout)
        self.fc = LoRALinear(n_embd, intermediate_size, **kw)
        self.proj = LoRALinear(intermediate_size, n_embd, **kw)
        self.fused_neighbours = FUSED_NEIGHBOURS_DEFAULT

    def quantize_base(self, double_quant: bool = False):
        for lin in (self.fc, self.proj):
            lin.quantize_base(double_quant)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a = self.fc(x)
        return self.proj(gelu(a) if self.fused_neighbours else F.gelu(a))


class NeoXBlock(DecoderBlock):
    """One decoder block in the parallel-residual form (model.py:350-352).  Members ``norm_1``, ``attn``, ``norm_2``, ``mlp``
    as in the reference, so its state dict keys carry over (``norm_1.bias``, ``attn.attn.linear.weight``,
    ``mlp.fc.linear.weight`` ...); ``norm_2`` is absent with ``shared_attention_norm``."""

    def __init__(self, n_embd: int, n_head: int, n_query_groups: int = None, head_size: int = None, bias: bool = True,
                 rotary_percentage: float = 0.25, intermediate_size: int = None, norm_eps: float = 1e-5,
                 shared_attention_norm: bool = False, gelu_approximate: str = "none", attn_alg: str = "fastmax", r: int = 8,
                 alpha: int = 16, dropout: float = 0.0, to_query: bool = True, to_key: bool = False, to_value: bool = True,
                 to_projection: bool = False, to_mlp: bool = False) -> None:
        super().__init__()
        if intermediate_size is None:
            raise ValueError("NeoXBlock needs intermediate_size")
        self.norm_1 = LayerNorm(n_embd, eps=norm_eps)
        self.attn = CausalSelfAttention(n_embd, n_head, n_query_groups=n_query_groups, head_size=head_size, bias=bias,
                                        rotary_percentage=rotary_percentage, attn_alg=attn_alg, r=r, alpha=alpha, dropout=dropout,
                                        to_query=to_query, to_key=to_key, to_value=to_value, to_projection=to_projection)
        self.norm_2 = None if shared_attention_norm else LayerNorm(n_embd, eps=norm_eps)
        self.mlp = GptNeoxMLP(n_embd, intermediate_size, bias=bias, r=r, alpha=alpha, dropout=dropout, to_mlp=to_mlp,
                              gelu_approximate=gelu_approximate)
        self._fused = FUSED_NEIGHBOURS_DEFAULT

    def run_open(self, n_1, n_2, cos, sin, input_pos=None, state=None):
        """both branches after the norms, without the three-way add: -> (m, h) with the block's output m + h + x"""
        h = self.attn(n_1, cos, sin, input_pos, state)
        return self.mlp(n_2), h

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, input_pos=None, state=None) -> torch.Tensor:
        """``state``: the attention's decode state cache (``FastmaxDecodeState(p=2)`` / ``LinearmaxDecodeState``), passed through"""
        _, n_1, n_2 = layer_norm_pair(x, self.norm_1, self.norm_2)
        m, h = self.run_open(n_1, n_2, cos, sin, input_pos, state)
        return m + h + x


def run_neox_blocks(blocks, x, cos, sin, input_pos=None, states=None):
    """the blocks in sequence with the hand-over fused: the three-way add after block i and both norms of block i + 1 are one
    ``layer_norm_pair``; the last add runs on its own.  ``states``: one decode state cache per block, or None"""
    m = h = None
    for i, blk in enumerate(blocks):
        x, n_1, n_2 = layer_norm_pair(x, blk.norm_1, blk.norm_2, m, h)
        m, h = blk.run_open(n_1, n_2, cos, sin, input_pos, None if states is None else states[i])
    return m + h + x


NeoXBlock.run_sequence = staticmethod(run_neox_blocks)


class NeoXStack(nn.Module):
    """NeoX blocks in sequence, owning the hand-over between them (``run_neox_blocks``).  With the kernels on, the result is
    bitwise that of calling the blocks one after the other."""

    def __init__(self, blocks) -> None:
        super().__init__()
        self.blocks = nn.ModuleList(blocks)

    @property
    def fused_neighbours(self) -> bool:
        return all(b.fused_neighbours for b in self.blocks)

    @fused_neighbours.setter
    def fused_neighbours(self, on: bool) -> None:
        for b in self.blocks:
            b.fused_neighbours = on

    def forward(self, x, cos, sin, input_pos=None, states=None):
        return run_neox_blocks(self.blocks, x, cos, sin, input_pos, states)
