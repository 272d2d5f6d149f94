"""The whole decoder block around the attention sub-layer: RMSNorm, both residual adds and the gated MLP in HIP.

The reference's ``Block.forward`` (lit_gpt/model.py:340-361), sequential-residual form:
    x = attn(norm_1(x)) + x
    x = mlp(norm_2(x)) + x
with ``RMSNorm`` (lit_gpt/rmsnorm.py:20-31) and ``LLaMAMLP`` / ``GemmaMLP`` (model.py:622-641, LoRA wiring lora.py:661-709).
``CausalSelfAttention`` is attention_block.py's; the three MLP linears are ``LoRALinear`` (NF4 base after ``quantize_base``).
``mlp_class="LLaMAMoE"`` puts moe.py's mixture of ``LLaMAMLP`` experts in the MLP's place.
What this file adds runs in csrc/block_neighbours.hip (C ABI: include/fastmax_hip_block.h, bound by ``_lib.ABI``):
    rms_norm / rms_norm_add    the norm, optionally with the residual add in front of it as ONE pass that also writes the sum
    gated_act                  act(fc_1(x)) * fc_2(x), forward and a one-pass backward that recomputes act
Rounding points are the reference's: the add and the normalised row are rounded to the activation dtype, statistics are
float32, act(a) is rounded before the product.  There is no CPU path through the kernels; ``fused_neighbours = False`` on a
module selects an eager restatement in tensor ops (A/B runs, parity tests).

Inside ``Block`` the add after the attention and ``norm_2`` are one ``rms_norm_add``.  ``BlockStack`` owns the hand-over
between blocks: the add after one block's MLP and the next block's ``norm_1`` fuse the same way; only the last add runs alone.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .attention_block import CONFIG_SHAPES, CausalSelfAttention
from .lora import LoRALinear

# intermediate_size of the CONFIG_SHAPES entries (lit_gpt/config.py).  Sizes only: the pythia configs name LayerNorm and
# GptNeoxMLP there, which Block refuses and neox_block.NeoXBlock builds; here their widths also serve tests and the step with
# RMSNorm and the gated MLP
CONFIG_INTERMEDIATE = {"pythia-14m": 512, "tiny-llama-1.1b": 5632, "Llama-2-7b-hf": 11008, "pythia-1b": 8192, "Gemma-2b": 16384,
                       "pythia-70m": 2048, "Mixtral-8x7B-v0.1": 14336}
# what the mixture-of-experts configs add to Block's arguments (config.py:1344-1362); kept out of CONFIG_SHAPES, whose entries
# are CausalSelfAttention's arguments
CONFIG_MOE = {"Mixtral-8x7B-v0.1": dict(mlp_class="LLaMAMoE", n_expert=8, n_expert_per_token=2)}

_ACT = {"silu": _lib.ACT_SILU, "gelu": _lib.ACT_GELU}


# ---- kernel calls -------------------------------------------------------------------------------------------------------------
def _need_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on an MI355X only; there is no CPU path through the kernels "
                           "(fused_neighbours = False selects the tensor-op restatement)")
    if t.dtype not in ops._DT:
        raise TypeError(f"{what}: dtype {t.dtype} is not float32, bfloat16 or float16")


def _rows(t: torch.Tensor, C: int) -> torch.Tensor:
    """(..., C) -> (M, C) with unit stride along the row (a view whenever the layout allows)"""
    t2 = t.reshape(-1, C)
    return t2 if t2.stride(1) == 1 and t2.stride(0) >= C else t2.contiguous()


def _check_norm_shapes(x: torch.Tensor, weight: torch.Tensor, r=None):
    C = x.shape[-1] if x.dim() else 0
    if C == 0 or x.numel() == 0:
        raise ValueError(f"rms_norm: empty input of shape {tuple(x.shape)} (C = 0 or no rows)")
    if weight.dim() != 1 or weight.shape[0] != C:
        raise ValueError(f"rms_norm: weight should have {C} elements, got shape {tuple(weight.shape)}")
    if r is not None and (r.shape != x.shape or r.dtype != x.dtype):
        raise ValueError(f"rms_norm_add: r should match x ({tuple(x.shape)}, {x.dtype}), got {tuple(r.shape)}, {r.dtype}")
    if weight.dtype != x.dtype and weight.dtype != torch.float32:
        raise ValueError(f"rms_norm: weight should be {x.dtype} or float32, got {weight.dtype}")


def rms_norm_forward(x, r, weight, eps: float, add_unit_offset: bool):
    """-> (s, y, rstd): s = x + r rounded to x's dtype (x itself without r), y the normalised rows times the weight in the
    promoted dtype of the two, rstd (M,) float32"""
    _check_norm_shapes(x, weight, r)
    _need_device(x, "rms_norm")
    C, dev = x.shape[-1], x.device
    x2 = _rows(x, C)
    r2 = None if r is None else _rows(r, C)
    w = weight.contiguous()
    M = x2.shape[0]
    s2 = x2 if r is None else torch.empty((M, C), dtype=x.dtype, device=dev)
    y2 = torch.empty((M, C), dtype=torch.promote_types(x.dtype, w.dtype), device=dev)
    rstd = torch.empty(M, dtype=torch.float32, device=dev)
    ops._call("fastmax_hip_rmsnorm_forward", dev,
              (x2.data_ptr(), x2.stride(0), ops._ptr(r2), 0 if r2 is None else r2.stride(0), w.data_ptr(),
               None if r is None else s2.data_ptr(), s2.stride(0), y2.data_ptr(), y2.stride(0), rstd.data_ptr(), M, C,
               float(eps), int(bool(add_unit_offset)), ops._DT[x.dtype], ops._DT[w.dtype]))
    return s2.view(x.shape), y2.view(x.shape), rstd


def rms_norm_backward_workspace(M: int, C: int, dtype, want_dweight: bool) -> int:
    return int(_lib.lib().fastmax_hip_rmsnorm_backward_workspace(M, C, ops._DT[dtype], int(bool(want_dweight))))


def rms_norm_backward(dy, s, weight, rstd, ds_in=None, add_unit_offset: bool = False, want_dweight: bool = False):
    """-> (ds, dweight or None): ds in s's dtype, with ``ds_in`` (the incoming gradient of the residual stream) added;
    dweight (C,) float32, bitwise reproducible"""
    _need_device(s, "rms_norm backward")
    C, dev = s.shape[-1], s.device
    s2, dy2 = _rows(s, C), _rows(dy, C)
    w = weight.contiguous()
    if dy2.dtype != torch.promote_types(s.dtype, w.dtype):
        dy2 = dy2.to(torch.promote_types(s.dtype, w.dtype))
    di2 = None if ds_in is None else _rows(ds_in.to(s.dtype), C)
    M = s2.shape[0]
    ds = torch.empty((M, C), dtype=s.dtype, device=dev)
    dw = torch.empty(C, dtype=torch.float32, device=dev) if want_dweight else None
    ws = rms_norm_backward_workspace(M, C, s.dtype, want_dweight)
    ops._call("fastmax_hip_rmsnorm_backward", dev,
              (dy2.data_ptr(), dy2.stride(0), s2.data_ptr(), s2.stride(0), w.data_ptr(), rstd.data_ptr(), ops._ptr(di2),
               0 if di2 is None else di2.stride(0), ds.data_ptr(), ds.stride(0), ops._ptr(dw), M, C,
               int(bool(add_unit_offset)), ops._DT[s.dtype], ops._DT[w.dtype]), ws=ws)
    return ds.view(s.shape), dw


def _act_operands(what: str, I: int, *tensors):
    """the operands of an element-wise operator (``what`` names it in the messages) as (M, I) rows"""
    for t in tensors[1:]:
        if t.shape != tensors[0].shape or t.dtype != tensors[0].dtype:
            raise ValueError(f"{what}: operands should agree in shape and dtype, got {tuple(t.shape)} {t.dtype} "
                             f"and {tuple(tensors[0].shape)} {tensors[0].dtype}")
    for t in tensors:
        _need_device(t, what)
    return [_rows(t, I) for t in tensors]


def gated_act_forward(a, b, act: str = "silu"):
    """act(a) * b with act(a) rounded to the tensors' dtype first; a, b (..., I), any row stride (halves of one buffer)"""
    I = a.shape[-1]
    if I == 0 or a.numel() == 0:
        raise ValueError(f"gated_act: empty input of shape {tuple(a.shape)}")
    a2, b2 = _act_operands("gated_act", I, a, b)
    y = torch.empty((a2.shape[0], I), dtype=a.dtype, device=a.device)
    ops._call("fastmax_hip_gated_act_forward", a.device,
              (a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), y.data_ptr(), y.stride(0), a2.shape[0], I, _ACT[act],
               ops._DT[a.dtype]))
    return y.view(a.shape)


def gated_act_backward(a, b, dy, act: str = "silu"):
    """-> (da, db) in one pass over a, b, dy; act is recomputed"""
    I = a.shape[-1]
    a2, b2, dy2 = _act_operands("gated_act", I, a, b, dy)
    da, db = (torch.empty((a2.shape[0], I), dtype=a.dtype, device=a.device) for _ in range(2))
    ops._call("fastmax_hip_gated_act_backward", a.device,
              (a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), dy2.data_ptr(), dy2.stride(0), da.data_ptr(),
               da.stride(0), db.data_ptr(), db.stride(0), a2.shape[0], I, _ACT[act], ops._DT[a.dtype]))
    return da.view(a.shape), db.view(a.shape)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
class _RMSNormFn(torch.autograd.Function):
    """(x, weight) -> y.  dweight only when the weight asks for it (in LoRA fine-tuning the norms are frozen)."""

    @staticmethod
    def forward(ctx, x, weight, eps, add_unit_offset):
        _, y, rstd = rms_norm_forward(x, None, weight, eps, add_unit_offset)
        ctx.save_for_backward(x, weight, rstd)
        ctx.unit_offset = add_unit_offset
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, rstd = ctx.saved_tensors
        ds, dw = rms_norm_backward(gy, x, weight, rstd, None, ctx.unit_offset, ctx.needs_input_grad[1])
        return ds, (None if dw is None else dw.to(weight.dtype)), None, None


class _RMSNormAddFn(torch.autograd.Function):
    """(x, r, weight) -> (s, y).  Backward: ds = rmsnorm backward of dy plus the gradient arriving at s (the fused add's
    backward); it is the gradient of x and of r alike."""

    @staticmethod
    def forward(ctx, x, r, weight, eps, add_unit_offset):
        s, y, rstd = rms_norm_forward(x, r, weight, eps, add_unit_offset)
        ctx.save_for_backward(s, weight, rstd)
        ctx.unit_offset = add_unit_offset
        return s, y

    @staticmethod
    def backward(ctx, gs, gy):
        s, weight, rstd = ctx.saved_tensors
        if gy is None:
            gy = torch.zeros(s.shape, dtype=torch.promote_types(s.dtype, weight.dtype), device=s.device)
        ds, dw = rms_norm_backward(gy, s, weight, rstd, gs, ctx.unit_offset, ctx.needs_input_grad[2])
        return ds, ds, (None if dw is None else dw.to(weight.dtype)), None, None


class _GatedActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, act):
        ctx.save_for_backward(a, b)
        ctx.act = act
        return gated_act_forward(a, b, act)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        da, db = gated_act_backward(a, b, dy, ctx.act)
        return da, db, None


def gated_act(a, b, act: str = "silu"):
    return _GatedActFn.apply(a, b, act)


def _eager_act(a, act: str):
    return F.silu(a) if act == "silu" else F.gelu(a)


# ---- modules -----------------------------------------------------------------------------------------------------------------
class RMSNorm(nn.Module):
    """lit_gpt/rmsnorm.py: same constructor, same parameter name (``weight``), so its checkpoints load."""

    def __init__(self, size: int, dim: int = -1, eps: float = 1e-6, add_unit_offset: bool = False) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(size))
        self.eps = eps
        self.dim = dim
        self.add_unit_offset = add_unit_offset
        self.fused_neighbours = True          # False: the tensor-op restatement below

    def _eager(self, x: torch.Tensor) -> torch.Tensor:
        dtype = x.dtype
        xf = x.float()
        norm_x = torch.mean(xf * xf, dim=self.dim, keepdim=True)
        x_normed = (xf * torch.rsqrt(norm_x + self.eps)).to(dtype=dtype)
        return x_normed * (1 + self.weight) if self.add_unit_offset else x_normed * self.weight

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.fused_neighbours:
            return self._eager(x)
        if self.dim not in (-1, x.dim() - 1):
            raise NotImplementedError(f"RMSNorm kernels normalise over the last dimension, got dim={self.dim}")
        return _RMSNormFn.apply(x, self.weight, self.eps, self.add_unit_offset)

    def reset_parameters(self) -> None:
        nn.init.ones_(self.weight)


def rms_norm_add(x: torch.Tensor, r: torch.Tensor, norm: RMSNorm):
    """-> (s, n): s = x + r (the residual stream, in the tensors' dtype) and n = norm(s), as one pass over x and r"""
    if not norm.fused_neighbours:
        s = x + r
        return s, norm._eager(s)
    if norm.dim not in (-1, x.dim() - 1):
        raise NotImplementedError(f"RMSNorm kernels normalise over the last dimension, got dim={norm.dim}")
    return _RMSNormAddFn.apply(x, r, norm.weight, norm.eps, norm.add_unit_offset)


class LLaMAMLP(nn.Module):
    """proj(silu(fc_1(x)) * fc_2(x)) -- lit_gpt/model.py:622-633 with the LoRA wiring of lit_gpt/lora.py:661-709"""
    act = "silu"

    def __init__(self, n_embd: int, intermediate_size: int, bias: bool = False, r: int = 0, alpha: int = 1, dropout: float = 0.0,
                 to_mlp: bool = False) -> None:
        super().__init__()
        kw = dict(bias=bias, r=(r if to_mlp else 0), lora_alpha=alpha, lora_dropout=dropout)
        self.fc_1 = LoRALinear(n_embd, intermediate_size, **kw)
        self.fc_2 = LoRALinear(n_embd, intermediate_size, **kw)
        self.proj = LoRALinear(intermediate_size, n_embd, **kw)
        self.fused_neighbours = True

    def quantize_base(self, double_quant: bool = False):
        for lin in (self.fc_1, self.fc_2, self.proj):
            lin.quantize_base(double_quant)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a, b = self.fc_1(x), self.fc_2(x)
        g = gated_act(a, b, self.act) if self.fused_neighbours else _eager_act(a, self.act) * b
        return self.proj(g)


class GemmaMLP(LLaMAMLP):
    """proj(gelu(fc_1(x)) * fc_2(x)), exact GELU -- lit_gpt/model.py:636-641"""
    act = "gelu"


_MLP_CLASSES = {"LLaMAMLP": LLaMAMLP, "GemmaMLP": GemmaMLP}


class DecoderBlock(nn.Module):
    """What the two block forms share.  A subclass builds ``norm_1``, ``attn``, ``norm_2`` (or None) and ``mlp``, starts
    ``_fused`` at its own default, and names in ``run_sequence`` the function that runs a sequence of its kind."""
    run_sequence = None

    @classmethod
    def from_config(cls, config: str, **kw):
        """a block at the head and MLP shapes of a CONFIG_SHAPES entry"""
        kw = {**CONFIG_MOE.get(config, {}), **kw}
        return cls(intermediate_size=kw.pop("intermediate_size", CONFIG_INTERMEDIATE[config]), **CONFIG_SHAPES[config], **kw)

    @property
    def fused_neighbours(self) -> bool:
        return self._fused

    @fused_neighbours.setter
    def fused_neighbours(self, on: bool) -> None:
        """the norm and MLP kernels on or off; the attention sub-layer's own switch (``attn.fused_neighbours``) is separate"""
        self._fused = bool(on)
        for m in (self.norm_1, self.norm_2, self.mlp):
            if m is not None:
                m.fused_neighbours = self._fused

    def quantize_base(self, double_quant: bool = False):
        self.attn.quantize_base(double_quant)
        self.mlp.quantize_base(double_quant)
        return self


class Block(DecoderBlock):
    """One decoder block in the sequential-residual form (model.py:356-360).  Members ``norm_1``, ``attn``, ``norm_2``,
    ``mlp`` as in the reference, so its state dict keys carry over (``attn.attn.linear.weight``, ``mlp.fc_1.linear.weight``...)."""

    def __init__(self, n_embd: int, n_head: int, n_query_groups: int = None, head_size: int = None, bias: bool = False,
                 rotary_percentage: float = 1.0, intermediate_size: int = None, norm_eps: float = 1e-5,
                 mlp_class="LLaMAMLP", norm_class="RMSNorm", parallel_residual: bool = False, shared_attention_norm: bool = False,
                 attn_alg: str = "fastmax", r: int = 8, alpha: int = 16, dropout: float = 0.0, to_query: bool = True,
                 to_key: bool = False, to_value: bool = True, to_projection: bool = False, to_mlp: bool = False,
                 add_unit_offset: bool = False, n_expert: int = 0, n_expert_per_token: int = 0) -> None:
        super().__init__()
        if parallel_residual:
            raise NotImplementedError("Block: parallel_residual=True (x = mlp(norm_2(x)) + attn(norm_1(x)) + x, the pythia form) "
                                      "is not built; only the sequential-residual form is")
        if shared_attention_norm:
            raise NotImplementedError("Block: shared_attention_norm=True is not built (the reference refuses it too without "
                                      "parallel_residual)")
        norm_name = norm_class if isinstance(norm_class, str) else getattr(norm_class, "__name__", str(norm_class))
        if norm_name != "RMSNorm":
            raise NotImplementedError(f"Block: norm class {norm_name} is not built; only RMSNorm has kernels (LayerNorm is missing)")
        mlp_name = mlp_class if isinstance(mlp_class, str) else getattr(mlp_class, "__name__", str(mlp_class))
        if mlp_name not in _MLP_CLASSES and mlp_name != "LLaMAMoE":
            raise NotImplementedError(f"Block: MLP class {mlp_name} is not built; only LLaMAMLP, GemmaMLP (gated) and LLaMAMoE "
                                      "are (GptNeoxMLP is neox_block.NeoXBlock's)")
        if intermediate_size is None:
            raise ValueError("Block needs intermediate_size")
        self.norm_1 = RMSNorm(n_embd, eps=norm_eps, add_unit_offset=add_unit_offset)
        self.attn = CausalSelfAttention(n_embd, n_head, n_query_groups=n_query_groups, head_size=head_size, bias=bias,
                                        rotary_percentage=rotary_percentage, attn_alg=attn_alg, r=r, alpha=alpha, dropout=dropout,
                                        to_query=to_query, to_key=to_key, to_value=to_value, to_projection=to_projection)
        self.norm_2 = RMSNorm(n_embd, eps=norm_eps, add_unit_offset=add_unit_offset)
        mlp_kw = dict(bias=bias, r=r, alpha=alpha, dropout=dropout, to_mlp=to_mlp)
        if mlp_name == "LLaMAMoE":
            from .moe import LLaMAMoE                                # moe.py builds its experts from this file's LLaMAMLP
            self.mlp = LLaMAMoE(n_embd, intermediate_size, n_expert, n_expert_per_token, **mlp_kw)
        else:
            self.mlp = _MLP_CLASSES[mlp_name](n_embd, intermediate_size, **mlp_kw)
        self._fused = True

    def run_open(self, x, n_1, cos, sin, input_pos=None, state=None):
        """everything after ``norm_1`` up to, but without, the last add: -> (m, s) with the block's output m + s"""
        h = self.attn(n_1, cos, sin, input_pos, state)
        s, n_2 = rms_norm_add(h, x, self.norm_2)                 # x = h + x; norm_2(x): one pass
        return self.mlp(n_2), s

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, input_pos=None, state=None) -> torch.Tensor:
        """``state``: the attention's decode state cache (``FastmaxDecodeState(p=2)`` / ``LinearmaxDecodeState``), passed through"""
        m, s = self.run_open(x, self.norm_1(x), cos, sin, input_pos, state)
        return m + s


def run_blocks(blocks, x, cos, sin, input_pos=None, states=None):
    """the blocks in sequence with the hand-over fused: the add after block i's MLP and block i + 1's ``norm_1`` are one
    ``rms_norm_add``; the last add runs on its own.  ``states``: one decode state cache per block, or None"""
    m = s = None
    for i, blk in enumerate(blocks):
        if i == 0:
            n_1 = blk.norm_1(x)
        else:
            x, n_1 = rms_norm_add(m, s, blk.norm_1)
        m, s = blk.run_open(x, n_1, cos, sin, input_pos, None if states is None else states[i])
    return m + s


Block.run_sequence = staticmethod(run_blocks)


class BlockStack(nn.Module):
    """Blocks in sequence, owning the hand-over between them (``run_blocks``).  The result is bitwise that of calling the
    blocks one after the other."""

    def __init__(self, blocks) -> None:
        super().__init__()
        self.blocks = nn.ModuleList(blocks)

    def forward(self, x, cos, sin, input_pos=None, states=None):
        return run_blocks(self.blocks, x, cos, sin, input_pos, states)
