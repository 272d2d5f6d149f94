"""From the last hidden state to the next token in HIP, and the generation loop around it.

The last stretch of the reference's loop (generate/base.py:30-47 after lit_gpt/model.py's ``ln_f`` + ``lm_head``) computes a
(B, T, V) head GEMM of which one row is used, then ``topk``, ``scatter_``, ``softmax`` and ``multinomial`` with a host read per
token.  Here (csrc/last_logits.hip and csrc/next_token.hip, C ABI: include/fastmax_hip_next_token.h, bound by ``_lib.ABI``):
    last_logits    the head over the LAST position only; the weight is read once for up to 8 rows
    Sampler        exact top-k (ties: the lowest indices are kept) and a draw from softmax(logits / temperature) as the argmax of
                   logit / temperature - log(-log u), u from Philox-4x32-10 under (seed, draw number): the token stays on the device.
                   ``top_p`` adds the nucleus filter behind the top-k, inside the same kernel (include/fastmax_hip_nucleus.h):
                   the shortest prefix of the kept entries, largest first, whose softmax mass reaches top_p
    NextTokenHead  ``ln_f`` (the RMSNorm or LayerNorm kernel on the B last rows) + ``lm_head`` + the sampler.  ``lm_head_bias=True``
                   and ``quantize_base()`` (``lm_head`` as NF4 codes) go through the other two entry points of
                   csrc/last_logits.hip (include/fastmax_hip_head.h): the same kernel with a bias, and straight from the codes
    generate       prompt -> tokens through decoder blocks (``Block`` or ``NeoXBlock``) on their decode state caches
    DecodeCursor, GraphedDecoder   the same loop as ONE graph replay per token: position, draw number and output column live in a
                   device record (csrc/decode_cursor.hip, include/fastmax_hip_cursor.h) that the step's first
                   and last kernel read and advance, so every replay takes the same arguments
What differs from the reference: logits are float32 by default (``dtype=`` gives the reference's), and the random stream is the
sampler's own seeded one instead of torch's generator, so a (seed, draw) pair reproduces a token on any batch.  There is no CPU
path through the kernels; ``NextTokenHead.fused = False`` selects the tensor-op restatement for A/B runs.
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .adapter_v2 import AdapterV2Linear, adapter_forward
from .block import BlockStack, RMSNorm, rms_norm_forward
from .lora import NF4Linear, Params4bit, scales_cached, scales_of
from .neox_block import LayerNorm, NeoXStack, layer_norm_forward

_MASK64 = (1 << 64) - 1


def _signed64(v: int) -> int:
    """the 64-bit pattern of v as the int64 the C ABI carries"""
    v &= _MASK64
    return v - (1 << 64) if v >> 63 else v


def _need_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on an MI355X only; there is no CPU path through the kernels")


def _unit_rows(t: torch.Tensor) -> torch.Tensor:
    return t if t.stride(1) == 1 and t.stride(0) >= 0 else t.contiguous()


def _head_scales(base: NF4Linear):
    """``scales_of(base)``; building it copies nothing to the device but, for double-quantised scales, reads one scalar back, so
    it has to exist before a stream starts capturing"""
    if not scales_cached(base) and base.weight.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("last_logits: the NF4 head's block scales have not been handed to the library yet, which cannot happen "
                           "while a stream is capturing (a double-quantised offset is read back from the device); score once "
                           "eagerly before the recording")
    return scales_of(base)


def _nf4_base(weight):
    """the NF4Linear behind ``weight``: itself, or a holder kept on a bare ``Params4bit`` so that its scales are built once"""
    if isinstance(weight, NF4Linear):
        return weight
    if isinstance(weight, Params4bit) and weight.quant_state is not None:
        base = weight.__dict__.get("_head_base")
        if base is None:
            base = weight.__dict__["_head_base"] = _BareNF4(weight)
        return base
    return None


class _BareNF4:
    """what ``scales_of`` reads of an NF4Linear, around a ``Params4bit`` alone (held weakly: the holder lives on the parameter)"""

    def __init__(self, weight):
        self._weight = weakref.ref(weight)

    @property
    def weight(self):
        return self._weight()


def last_logits(x: torch.Tensor, weight, dtype=torch.float32, bias=None, rows=None) -> torch.Tensor:
    """x (B, C) with unit stride along C and any row stride (a last-position view), weight (V, C) -> logits (B, V) in ``dtype``
    (float32 or the inputs' dtype), accumulated in float32.  A row's logits do not depend on the batch it is computed in.
    ``weight``: a tensor of x's dtype, or an ``NF4Linear`` (or its ``Params4bit`` with a quant state) over C inputs with
    C % 64 == 0: the logits of its dequantised weight ``weight.dequantize(x.dtype)``, straight from the codes.  ``bias`` (>= V
    elements of x's dtype) is added in float32 before the logits are rounded.  ``rows``: score the first ``rows`` rows of the
    weight only (``vocab_size`` of a padded vocabulary)."""
    base = _nf4_base(weight)
    shape = tuple(weight.shape) if base is None else tuple(base.weight.quant_state[1])
    if x.dim() != 2 or len(shape) != 2 or x.shape[1] != shape[1] or 0 in x.shape or 0 in shape:
        raise ValueError(f"last_logits: x should be (B, C) and weight (V, C), got {tuple(x.shape)} and {shape}")
    V = shape[0] if rows is None else int(rows)
    if not 1 <= V <= shape[0]:
        raise ValueError(f"last_logits: rows should lie in 1 .. {shape[0]}, got {rows}")
    if x.dtype not in ops._DT or (base is None and x.dtype != weight.dtype):
        raise TypeError(f"last_logits: x and weight should share float32, bfloat16 or float16, got {x.dtype} and "
                        f"{'NF4 codes' if base is not None else weight.dtype}")
    if dtype not in (torch.float32, x.dtype):
        raise TypeError(f"last_logits: dtype should be float32 or {x.dtype}, got {dtype}")
    if bias is not None and (bias.dim() != 1 or bias.shape[0] < V or bias.dtype != x.dtype or bias.device != x.device):
        raise ValueError(f"last_logits: bias should hold {V} elements of {x.dtype} on x's device, got {tuple(bias.shape)} {bias.dtype}")
    if base is not None and shape[1] % 64:
        raise ValueError(f"last_logits: an NF4 weight needs C % 64 == 0 (a 64-weight block inside one row), got C = {shape[1]}")
    _need_device(x, "last_logits")
    x2 = _unit_rows(x)
    B, C = x2.shape
    out = torch.empty((B, V), dtype=dtype, device=x.device)
    bs = None if bias is None else bias.contiguous()
    if base is not None:
        codes = base.weight.data
        if codes.device != x.device:
            raise ValueError(f"last_logits: x is on {x.device}, the NF4 codes on {codes.device}")
        ops._call("fastmax_hip_last_logits_nf4", x.device,
                  (x2.data_ptr(), x2.stride(0), codes.data_ptr(), _head_scales(base).ref, ops._ptr(bs), out.data_ptr(), out.stride(0),
                   B, V, C, ops._DT[x.dtype], ops._DT[dtype]))
        return out
    weight = weight[:V]
    w = weight if weight.stride(1) == 1 and weight.stride(0) >= weight.shape[1] else weight.contiguous()
    if bs is None:
        ops._call("fastmax_hip_last_logits", x.device,
                  (x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), B, V, C, ops._DT[x.dtype],
                   ops._DT[dtype]))
    else:
        ops._call("fastmax_hip_last_logits_bias", x.device,
                  (x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), bs.data_ptr(), out.data_ptr(), out.stride(0), B, V, C,
                   ops._DT[x.dtype], ops._DT[dtype]))
    return out


def _check_sampling(temperature, top_k, top_p=None):
    if not (temperature >= 0.0) or temperature == float("inf"):
        raise ValueError(f"temperature should be a finite number >= 0, got {temperature}")
    if top_k is not None and (int(top_k) != top_k or top_k < 1):
        raise ValueError(f"top_k should be None or an integer >= 1, got {top_k}")
    if top_p is not None and not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p should be None or a number in (0, 1], got {top_p}")


def _nucleus(top_p):
    """the top_p the nucleus entry points receive, or None where there is no nucleus filter (None or 1.0): those calls go to
    the entry points without one and keep their bits"""
    return None if top_p is None or float(top_p) == 1.0 else float(top_p)


def _logit_rows(logits: torch.Tensor, what: str) -> torch.Tensor:
    if logits.dim() != 2 or 0 in logits.shape:
        raise ValueError(f"{what}: logits should be (B, V), got {tuple(logits.shape)}")
    _need_device(logits, what)
    logits = logits.float()
    return logits if logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1] else logits.contiguous()


class Sampler:
    """A seeded stream of draws.  ``seed`` and ``draws`` (the number of ``sample`` calls so far) are all its state: row b of
    call number d takes the Philox block at counter (i / 4, b, d) under the seed.  ``seed=None`` takes one from torch's CPU
    generator, so ``torch.manual_seed`` reproduces a run."""

    def __init__(self, seed=None) -> None:
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self.seed = int(seed) & _MASK64
        self.draws = 0

    def sample(self, logits: torch.Tensor, temperature: float = 1.0, top_k=None, top_p=None) -> torch.Tensor:
        """logits (B, V) -> (B,) int64 tokens on the device; nothing is read back.  ``temperature == 0`` is the argmax (and
        ``top_p`` is ignored).  ``top_p`` in (0, 1): after temperature and top-k, only the smallest set of the largest entries
        whose softmax mass reaches top_p is drawn from (at least one); None or 1.0: no such filter."""
        _check_sampling(temperature, top_k, top_p)
        rows = _logit_rows(logits, "Sampler.sample")
        B, V = rows.shape
        tokens = torch.empty(B, dtype=torch.int64, device=rows.device)
        k, p = 0 if top_k is None else min(int(top_k), V), _nucleus(top_p)
        if p is None:
            ops._call("fastmax_hip_sample", rows.device,
                      (rows.data_ptr(), rows.stride(0), tokens.data_ptr(), B, V, k, float(temperature), _signed64(self.seed),
                       _signed64(self.draws)))
        else:
            ops._call("fastmax_hip_sample_nucleus", rows.device,
                      (rows.data_ptr(), rows.stride(0), tokens.data_ptr(), B, V, k, p, float(temperature), _signed64(self.seed),
                       _signed64(self.draws)))
        self.draws += 1
        return tokens

    def keep_mask(self, logits: torch.Tensor, top_k, top_p=None, temperature: float = 1.0) -> torch.Tensor:
        """bool (B, V): the entries ``sample`` would choose among.  Without ``top_p`` exactly ``top_k`` per row (all of them for
        None or ``top_k >= V``): those above the k-th largest value and, of those equal to it, the lowest indices.  With ``top_p``
        the nucleus of those at ``temperature``: a prefix of them, largest first, lowest index first among equals."""
        _check_sampling(temperature, top_k, top_p)
        rows = _logit_rows(logits, "Sampler.keep_mask")
        B, V = rows.shape
        mask = torch.empty((B, V), dtype=torch.uint8, device=rows.device)
        k, p = 0 if top_k is None else min(int(top_k), V), _nucleus(top_p)
        if p is None:
            ops._call("fastmax_hip_topk_mask", rows.device, (rows.data_ptr(), rows.stride(0), mask.data_ptr(), mask.stride(0), B, V, k))
        else:
            ops._call("fastmax_hip_nucleus_mask", rows.device,
                      (rows.data_ptr(), rows.stride(0), mask.data_ptr(), mask.stride(0), B, V, k, p, float(temperature)))
        return mask.bool()


def _nucleus_keep(probs: torch.Tensor, top_p: float) -> torch.Tensor:
    """bool like probs: largest first (a stable sort: the lowest index first among equals), an entry stays while the mass
    before it is < top_p"""
    p, order = torch.sort(probs, dim=-1, descending=True, stable=True)
    return torch.zeros_like(probs, dtype=torch.bool).scatter_(-1, order, p.cumsum(-1) - p < top_p)


def _sample_tensor_ops(logits: torch.Tensor, temperature: float, top_k, top_p=None) -> torch.Tensor:
    """generate/base.py:30-41 for a batch of rows, drawing from torch's generator; top-p as upstream lit-gpt applies it, after
    temperature and top-k"""
    if top_k is not None:
        v, i = torch.topk(logits, min(int(top_k), logits.size(-1)))
        logits = torch.full_like(logits, float("-inf")).scatter_(-1, i, v)
    if temperature > 0.0:
        probs = torch.softmax(logits / temperature, dim=-1)
        if _nucleus(top_p) is not None:
            probs = probs * _nucleus_keep(probs, float(top_p))
        return torch.multinomial(probs, num_samples=1).squeeze(-1)
    return torch.argmax(logits, dim=-1)


class NextTokenHead(nn.Module):
    """``ln_f`` + ``lm_head`` (the reference's names, so its state-dict keys load) + the sampler.  ``vocab_size`` rows of the
    ``padded_vocab_size`` rows of the weight are scored; the default is all of them, which is what the reference samples over.
    ``norm_class``: "RMSNorm", or "LayerNorm" (the pythia models; state-dict keys ``ln_f.weight`` and ``ln_f.bias``).
    ``lm_head_bias``: the reference's ``config.lm_head_bias`` (the Phi models; state-dict key ``lm_head.bias``).
    ``quantize_base()`` stores ``lm_head`` as NF4 codes, as the reference's quantised runs do with every linear of the model.
    After ``adapter_v2.adapt`` ``lm_head`` is an ``AdapterV2Linear`` (state-dict keys ``lm_head.linear.weight``,
    ``lm_head.adapter_scale`` ...): the score comes from its ``linear`` as before, then one pass of csrc/adapter_v2.hip scales
    and shifts the float32 logits."""

    def __init__(self, n_embd: int, padded_vocab_size: int, vocab_size: int = None, norm_eps: float = 1e-5,
                 add_unit_offset: bool = False, norm_class: str = "RMSNorm", lm_head_bias: bool = False) -> None:
        super().__init__()
        vocab_size = padded_vocab_size if vocab_size is None else vocab_size
        if not 1 <= vocab_size <= padded_vocab_size:
            raise ValueError(f"vocab_size should lie in 1 .. {padded_vocab_size}, got {vocab_size}")
        if norm_class not in ("RMSNorm", "LayerNorm"):
            raise ValueError(f"norm_class should be 'RMSNorm' or 'LayerNorm', got {norm_class!r}")
        if norm_class == "LayerNorm" and add_unit_offset:
            raise ValueError("add_unit_offset belongs to RMSNorm")
        self.ln_f = (LayerNorm(n_embd, eps=norm_eps) if norm_class == "LayerNorm"
                     else RMSNorm(n_embd, eps=norm_eps, add_unit_offset=add_unit_offset))
        self.lm_head = nn.Linear(n_embd, padded_vocab_size, bias=bool(lm_head_bias))
        self.vocab_size = vocab_size
        self.fused = True                     # False: the tensor-op restatement (whole (B, T, V) head, topk + softmax + multinomial)

    def quantize_base(self, double_quant: bool = False) -> "NextTokenHead":
        """``lm_head`` becomes an ``NF4Linear`` of the same weight (block 64; ``double_quant``: 8-bit block scales), the bias
        stays; the state-dict keys are ``NF4Linear``'s.  Called again, nothing happens; the other scale form is refused."""
        lin = self._linear()
        if isinstance(lin, NF4Linear):
            if lin.double_quant != bool(double_quant):
                raise ValueError(f"NextTokenHead.quantize_base: lm_head is already quantised with double_quant="
                                 f"{lin.double_quant}")
            return self
        if lin.in_features % 64:
            raise ValueError(f"NextTokenHead.quantize_base: n_embd should be a multiple of 64 (one NF4 block lies inside one row "
                             f"of the weight), got {lin.in_features}")
        if isinstance(self.lm_head, AdapterV2Linear):
            self.lm_head.linear = NF4Linear.from_linear(lin, double_quant=bool(double_quant))
        else:
            self.lm_head = NF4Linear.from_linear(lin, double_quant=bool(double_quant))
        return self

    def _linear(self):
        """the layer that scores: ``lm_head``, or the ``linear`` inside an adapted one"""
        return self.lm_head.linear if isinstance(self.lm_head, AdapterV2Linear) else self.lm_head

    def _adapter(self):
        """the first ``vocab_size`` entries of an adapted lm_head's (scale, bias) in float32, the logits' dtype; a cast is
        kept until a parameter changes, and refused while a stream is capturing, exactly as ``_bias`` is"""
        ps = (self.lm_head.adapter_scale, self.lm_head.adapter_bias)
        if all(p.dtype == torch.float32 for p in ps):
            return tuple(p.detach()[:self.vocab_size] for p in ps)
        key = tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in ps) + (self.vocab_size,)
        hit = self.__dict__.get("_adapter_cast")
        if hit is None or hit[0] != key:
            if ps[0].is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NextTokenHead: the adapter's scale and bias have not been cast to float32 yet, and a copy made "
                                   "while a stream is capturing would belong to that graph; score once eagerly before the recording")
            hit = self.__dict__["_adapter_cast"] = (key, tuple(p.detach()[:self.vocab_size].float() for p in ps))
        return hit[1]

    def _bias(self, dtype):
        """lm_head's bias in ``dtype`` (an NF4Linear keeps it in float32), or None; the cast is kept until the bias changes"""
        b = self._linear().bias
        if b is None or b.dtype == dtype:
            return None if b is None else b.detach()
        key = (b.data_ptr(), b._version, dtype, b.device)
        hit = self.__dict__.get("_bias_cast")
        if hit is None or hit[0] != key:
            if b.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NextTokenHead: the bias has not been cast to the activations' dtype yet, and a copy made while "
                                   "a stream is capturing would belong to that graph; score once eagerly before the recording")
            hit = self.__dict__["_bias_cast"] = (key, b.detach().to(dtype))
        return hit[1]

    def logits(self, x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        """x (B, T, C) or (B, C) -> the logits (B, vocab_size) of the last position"""
        if x.dim() not in (2, 3):
            raise ValueError(f"NextTokenHead: x should be (B, T, C) or (B, C), got {tuple(x.shape)}")
        lin = self._linear()
        nf4, adapted = isinstance(lin, NF4Linear), lin is not self.lm_head
        if not self.fused:
            n = self.ln_f._eager(x)
            y = F.linear(n, lin.dequantize(n.dtype), self._bias(n.dtype)) if nf4 else lin(n)
            if adapted:
                y = self.lm_head.adapter_scale * (y + self.lm_head.adapter_bias)
            return (y[:, -1] if x.dim() == 3 else y)[:, :self.vocab_size].to(dtype)
        if adapted:
            if dtype != torch.float32:
                raise TypeError(f"NextTokenHead: an adapted lm_head gives float32 logits, got dtype={dtype}")
            return adapter_forward(self._scores(x, lin, nf4, dtype), *self._adapter())
        return self._scores(x, lin, nf4, dtype)

    def _scores(self, x, lin, nf4, dtype):
        """the last position's scores of ``lin`` through the last_logits entry points"""
        last = x[:, -1] if x.dim() == 3 else x
        if isinstance(self.ln_f, LayerNorm):
            _, n, _, _, _ = layer_norm_forward(last, self.ln_f.weight.detach(), self.ln_f.bias.detach(), self.ln_f.eps)
        else:
            _, n, _ = rms_norm_forward(last, None, self.ln_f.weight.detach(), self.ln_f.eps, self.ln_f.add_unit_offset)
        if nf4:
            return last_logits(n, lin, dtype, bias=self._bias(n.dtype), rows=self.vocab_size)
        if lin.bias is not None:
            return last_logits(n, lin.weight.detach(), dtype, bias=self._bias(n.dtype), rows=self.vocab_size)
        return last_logits(n, lin.weight.detach()[:self.vocab_size], dtype)

    def forward(self, x: torch.Tensor, sampler: Sampler, temperature: float = 1.0, top_k=None, top_p=None) -> torch.Tensor:
        """-> (B,) int64 tokens"""
        _check_sampling(temperature, top_k, top_p)
        logits = self.logits(x)
        if not self.fused:
            return _sample_tensor_ops(logits, temperature, top_k, top_p)
        return sampler.sample(logits, temperature, top_k, top_p)


def _check_prompt(prompt, max_returned_tokens, cos, sin):
    if prompt.dim() != 2 or prompt.dtype != torch.int64:
        raise ValueError(f"generate: prompt should be (B, T) int64, got {tuple(prompt.shape)} {prompt.dtype}")
    B, T = prompt.shape
    if T < 1 or max_returned_tokens <= T:
        raise ValueError(f"generate: max_returned_tokens ({max_returned_tokens}) should exceed the prompt's length ({T} >= 1)")
    if cos.shape[0] < max_returned_tokens - 1 or sin.shape[0] < max_returned_tokens - 1:
        raise ValueError(f"generate: the rope cache has {cos.shape[0]} rows, {max_returned_tokens - 1} positions are fed")
    return B, T


def _layers_and_run(blocks, states):
    """the blocks as a sequence and what runs a sequence of their kind over the decode state caches"""
    layers = blocks.blocks if isinstance(blocks, (BlockStack, NeoXStack)) else blocks
    runs = {type(b).run_sequence for b in layers}                      # a block's class names what runs a sequence of its kind
    if len(runs) > 1:
        raise ValueError("generate: the blocks mix NeoXBlock with another kind; a sequence holds one kind")
    if len(states) != len(layers):
        raise ValueError(f"generate: {len(layers)} blocks need as many decode state caches, got {len(states)}")
    (run,) = runs
    return layers, run


_RECORDING_STEPS = 3          # GraphedDecoder._capture: two eager steps, then the recorded one


class DecodeCursor:
    """The device record of include/fastmax_hip_cursor.h (csrc/decode_cursor.hip): the position of the next token to feed, the
    sampler's seed and draw number and a sticky overflow flag, advanced by the kernels themselves.  ``feed`` starts a decode step
    and ``sample`` ends it; both take the same arguments every token, so a step between them can be recorded as a graph."""

    def __init__(self, device) -> None:
        self.words = torch.zeros(_lib.lib().fastmax_hip_cursor_bytes() // 8, dtype=torch.int64, device=device)
        _need_device(self.words, "DecodeCursor")

    def arm(self, pos: int, draw: int, seed: int) -> None:
        """the next feed takes position ``pos``; the sample after it is draw number ``draw`` under ``seed`` and fills column
        ``pos + 1``.  One small copy; the overflow flag is cleared."""
        if pos < 0:
            raise ValueError(f"DecodeCursor.arm: pos should be >= 0, got {pos}")
        host = torch.zeros(self.words.numel(), dtype=torch.int64)
        host[_lib.CURSOR_POS], host[_lib.CURSOR_NEXT] = int(pos), -1
        host[_lib.CURSOR_DRAW_BASE], host[_lib.CURSOR_SEED] = _signed64(int(draw) - (int(pos) + 1)), _signed64(int(seed))
        self.words.copy_(host)

    def read(self) -> dict:
        """the record on the host (this synchronises): pos, next, overflow"""
        w = self.words.tolist()
        return dict(pos=w[_lib.CURSOR_POS], next=w[_lib.CURSOR_NEXT], overflow=bool(w[_lib.CURSOR_OVERFLOW]))

    def feed(self, tok, wte, x, cos, sin, cos_row, sin_row) -> None:
        """x[b] = wte[tok[b]]; cos_row, sin_row (1, n) = the first n columns of row ``pos`` of cos, sin.  tok (B,) int64,
        wte (N, C), x (B, C) in wte's dtype, cos and sin (R, >= n) with shared strides; everything with unit stride along a row."""
        if tok.dim() != 1 or tok.dtype != torch.int64 or not tok.is_contiguous():
            raise ValueError(f"DecodeCursor.feed: tok should be (B,) int64, got {tuple(tok.shape)} {tok.dtype}")
        B = tok.shape[0]
        if wte.dim() != 2 or tuple(x.shape) != (B, wte.shape[1]) or B < 1 or x.stride(1) != 1 or wte.stride(1) != 1:
            raise ValueError(f"DecodeCursor.feed: wte (N, C) and x ({B}, C) with unit stride along C, got {tuple(wte.shape)}, {tuple(x.shape)}")
        if x.dtype != wte.dtype or wte.dtype not in ops._DT:
            raise TypeError(f"DecodeCursor.feed: x and wte should share float32, bfloat16 or float16, got {x.dtype} and {wte.dtype}")
        n = cos_row.shape[-1]
        if (cos.dim() != 2 or cos.shape != sin.shape or cos.stride() != sin.stride() or cos.stride(1) != 1 or cos.shape[1] < n
                or cos_row.numel() != n or sin_row.numel() != n or not (cos_row.is_contiguous() and sin_row.is_contiguous())):
            raise ValueError(f"DecodeCursor.feed: cos, sin (R, >= n) alike and one-row buffers of n columns, got {tuple(cos.shape)}, "
                             f"{tuple(sin.shape)}, {tuple(cos_row.shape)}, {tuple(sin_row.shape)}")
        if len({cos.dtype, sin.dtype, cos_row.dtype, sin_row.dtype}) != 1 or cos.dtype not in ops._DT:
            raise TypeError(f"DecodeCursor.feed: the rope cache and its row buffers should share one dtype, got {cos.dtype}, {cos_row.dtype}")
        ops._call("fastmax_hip_cursor_feed", self.words.device,
                  (self.words.data_ptr(), tok.data_ptr(), wte.data_ptr(), wte.stride(0), wte.shape[0], x.data_ptr(), x.stride(0), B,
                   wte.shape[1], ops._DT[wte.dtype], cos.data_ptr(), sin.data_ptr(), cos.stride(0), cos.shape[0], cos_row.data_ptr(),
                   sin_row.data_ptr(), n, ops._DT[cos.dtype]))

    def sample(self, logits, tok, out, done=None, eos_id=None, temperature: float = 1.0, top_k=None, top_p=None) -> None:
        """``Sampler(seed).sample`` at the cursor's draw number: the tokens go to tok (B,) and to column ``next`` of out (B, L)
        int64, ``token == eos_id`` is ORed into done (B,) uint8, and the cursor moves on by one."""
        _check_sampling(temperature, top_k, top_p)
        rows = _logit_rows(logits, "DecodeCursor.sample")
        B, V = rows.shape
        if tuple(tok.shape) != (B,) or tok.dtype != torch.int64 or not tok.is_contiguous():
            raise ValueError(f"DecodeCursor.sample: tok should be ({B},) int64, got {tuple(tok.shape)} {tok.dtype}")
        if out.dim() != 2 or out.shape[0] != B or out.dtype != torch.int64 or out.stride(1) != 1:
            raise ValueError(f"DecodeCursor.sample: out should be ({B}, L) int64, got {tuple(out.shape)} {out.dtype}")
        if eos_id is not None and (done is None or tuple(done.shape) != (B,) or done.dtype != torch.uint8 or not done.is_contiguous()):
            raise ValueError(f"DecodeCursor.sample: eos_id needs done ({B},) uint8")
        args = (rows.data_ptr(), rows.stride(0), self.words.data_ptr(), tok.data_ptr(), out.data_ptr(), out.stride(0), out.shape[1],
                ops._ptr(done), -1 if eos_id is None else int(eos_id), B, V, 0 if top_k is None else min(int(top_k), V),
                float(temperature))
        p = _nucleus(top_p)
        if p is None:
            ops._call("fastmax_hip_sample_cursor", rows.device, args)
        else:
            ops._call("fastmax_hip_sample_cursor_nucleus", rows.device, args + (p,))


class GraphedDecoder:
    """``generate`` with one graph replay per token after the first.

    Owns the static buffers of a decode step (the token, its embedding, the rope row of its position, the output and the eos
    flags), the ``DecodeCursor`` and ONE recorded graph of a whole step: feed -> the blocks on their state caches -> the head ->
    the cursor's sampler.  The graph is recorded on first use, on the states as the first prompt left them, and serves every later
    prompt, prompt length, ``max_returned_tokens <= max_len`` and seed: what differs between them sits in device memory.
    ``temperature``, ``top_k``, ``top_p`` and ``eos_id`` are recorded by value.  Takes what ``generate`` takes, except a first-order
    ``FastmaxDecodeState``, whose step receives the token count as a kernel argument, blocks whose MLP is a ``moe.LLaMAMoE`` that
    would read its experts' row counts back in every layer, and ``head.fused = False``, whose sampler reads torch's generator on
    the host.  An ``LLaMAMoE`` is taken with ``device_routed`` set on every one of them (quantized experts) and a batch of at most
    16 in bfloat16 or float32: its decode step then runs on device-side row counts; the two eager warm-up steps before the
    recording build each layer's expert table, which cannot be built inside it.  The prompt (B T > 16 rows) runs on the eager route.
    A ``FastmaxKVDecodeState`` keeps its length in its own header, which every step's kernels read and the last one advances; it
    needs room for ``max_len - 1`` tokens.

    ``captures``: graphs recorded so far (1 after the first call); ``replays``: graph launches so far, one per generated token
    after each call's first; ``poll``: with ``eos_id``, ``done`` is read back every ``poll`` replays instead of every token."""

    poll = 16

    def __init__(self, wte: torch.Tensor, blocks, head: NextTokenHead, states, *, cos, sin, max_len: int, temperature: float = 1.0,
                 top_k=None, eos_id=None, top_p=None) -> None:
        _check_sampling(temperature, top_k, top_p)
        self._layers, self._run = _layers_and_run(blocks, states)
        if not len(states):
            raise ValueError("GraphedDecoder: no blocks")
        for s in states:
            s.check_capacity(max_len - 1, "GraphedDecoder")
        for s in states:
            s.check_recordable(_RECORDING_STEPS)
        from .moe import LLaMAMoE
        moes = [b.mlp for b in self._layers if isinstance(getattr(b, "mlp", None), LLaMAMoE)]
        if moes and not all(m.device_routed and m.fused_neighbours for m in moes):
            raise NotImplementedError("GraphedDecoder: an LLaMAMoE reads its experts' row counts back from the device in every "
                                      "layer, which a recorded graph cannot do; generate() runs these blocks eagerly; set "
                                      "`mlp.device_routed = True` on quantized experts")
        if moes and (states[0].B > _lib.MOE_DECODE_MAX_ROWS or wte.dtype not in (torch.bfloat16, torch.float32)):
            raise NotImplementedError(f"GraphedDecoder: a device-routed LLaMAMoE takes at most {_lib.MOE_DECODE_MAX_ROWS} rows in "
                                      f"bfloat16 or float32 without reading its experts' row counts back, got batch {states[0].B} "
                                      f"in {wte.dtype}")
        if not head.fused:
            raise ValueError("GraphedDecoder: head.fused = False samples through torch's generator, whose state a recorded graph "
                             "does not advance; the graphed route needs the HIP sampler")
        if wte.dim() != 2 or wte.dtype not in ops._DT:
            raise ValueError(f"GraphedDecoder: wte should be (rows, C) in float32, bfloat16 or float16, got {tuple(wte.shape)} {wte.dtype}")
        if cos.dim() != 2 or cos.shape != sin.shape or cos.dtype != sin.dtype or cos.dtype not in ops._DT:
            raise ValueError(f"GraphedDecoder: cos and sin should be one (rows, n) shape and dtype, got {tuple(cos.shape)}, {tuple(sin.shape)}")
        if max_len < 2 or cos.shape[0] < max_len - 1:
            raise ValueError(f"GraphedDecoder: max_len ({max_len}) should be >= 2 and the rope cache ({cos.shape[0]} rows) hold "
                             f"max_len - 1 positions")
        _need_device(wte, "GraphedDecoder")
        self.given = dict(wte=wte, blocks=blocks, head=head, states=states, cos=cos, sin=sin)
        self.wte, self.head, self.states = _unit_rows(wte.detach()), head, list(states)
        self.cos, self.sin = cos.contiguous(), sin.contiguous()
        self.max_len, self.temperature, self.top_k, self.eos_id = int(max_len), float(temperature), top_k, eos_id
        self.top_p = _nucleus(top_p)
        dev, B, C = wte.device, states[0].B, wte.shape[1]
        self.B = B
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)
        self.x = torch.zeros((B, C), dtype=wte.dtype, device=dev)
        self.cos_row, self.sin_row = (torch.zeros((1, cos.shape[1]), dtype=cos.dtype, device=dev) for _ in range(2))
        self.out = torch.zeros((B, self.max_len), dtype=torch.int64, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self._pos = torch.zeros(1, dtype=torch.int64, device=dev)          # the blocks never read input_pos on a state cache
        self.cursor = DecodeCursor(dev)
        self._graph, self._stream = None, None
        self.captures = self.replays = 0

    def _step(self) -> None:
        B, C = self.x.shape
        self.cursor.feed(self.tok, self.wte, self.x, self.cos, self.sin, self.cos_row, self.sin_row)
        h = self._run(self._layers, self.x.view(B, 1, C), self.cos_row, self.sin_row, self._pos, self.states)
        self.cursor.sample(self.head.logits(h), self.tok, self.out, self.done, self.eos_id, self.temperature, self.top_k, self.top_p)

    def _capture(self) -> None:
        """Record ``_step`` on the states as they are (non-empty: the blocks pick the single-token route from ``count > 0``).
        Two eager steps on a side stream first, so that every lazy initialisation of the step's own shapes happens outside the
        recording; then the recording on that same stream, one straight chain.  The warm-up advances the states and the recording
        the host's counts: both are put back.  A KV cache with less room than the recording's steps is taken back by that many
        tokens first; the graph does not depend on the length, which its kernels read from the cache's header."""
        dev = self.tok.device
        saved = [(s.state.clone(), s.count) for s in self.states]
        for s in self.states:
            if s.max_len is not None and s.count + _RECORDING_STEPS > s.max_len:
                s.count = s.max_len - _RECORDING_STEPS
        self.tok.zero_()
        self.cursor.arm(0, 0, 0)
        self._stream = torch.cuda.Stream(device=dev)
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._stream):
            for _ in range(2):
                self._step()
        self._stream.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, stream=self._stream):
            self._step()
        torch.cuda.current_stream(dev).wait_stream(self._stream)
        for s, (state, count) in zip(self.states, saved):
            s._restore(state, count)
        self.captures += 1

    @torch.no_grad()
    def generate(self, prompt: torch.Tensor, max_returned_tokens: int, sampler: Sampler = None) -> torch.Tensor:
        """``generate(...)`` of the module, token for token: prompt (B, T) int64 -> (B, n), the prompt included.  The prompt and the
        first draw run eagerly, every further token is one replay.  Afterwards every ``state.count`` and ``sampler.draws`` are what
        the eager loop leaves; with ``eos_id`` the state caches themselves may have run up to ``poll - 1`` tokens past that."""
        B, T = _check_prompt(prompt, max_returned_tokens, self.cos, self.sin)
        if B != self.B or max_returned_tokens > self.max_len:
            raise ValueError(f"GraphedDecoder: built for batch {self.B} and max_len {self.max_len}, got batch {B} and "
                             f"max_returned_tokens {max_returned_tokens}")
        if not self.head.fused:
            raise ValueError("GraphedDecoder: head.fused = False samples through torch's generator; the graphed route needs the HIP sampler")
        _need_device(prompt, "GraphedDecoder.generate")
        for s in self.states:
            s.check_capacity(max_returned_tokens - 1, "GraphedDecoder.generate")
        sampler = Sampler() if sampler is None else sampler
        eos = self.eos_id
        pos = torch.arange(T, device=prompt.device)
        h = self._run(self._layers, F.embedding(prompt, self.wte), self.cos[:T], self.sin[:T], pos, self.states)
        first_draw = sampler.draws
        token = self.head(h, sampler, self.temperature, self.top_k, self.top_p)
        if self._graph is None:
            self._capture()
        self.out[:, :T] = prompt
        self.out[:, T] = token
        self.tok.copy_(token)
        if eos is None:
            self.done.zero_()
        else:
            self.done.copy_(token == eos)
        self.cursor.arm(T, first_draw + 1, sampler.seed)
        steps, ran = max_returned_tokens - T - 1, 0
        finished = eos is not None and bool(self.done.all())
        while ran < steps and not finished:
            k = steps - ran if eos is None else min(max(1, int(self.poll)), steps - ran)
            for _ in range(k):
                self._graph.replay()
            ran += k
            self.replays += k
            finished = eos is not None and bool(self.done.all())
        n = T + 1 + ran
        if eos is not None:
            if self.cursor.read()["overflow"]:
                raise RuntimeError("GraphedDecoder: the decode cursor reports an overflow (a position outside the rope cache or a "
                                   "token outside the embedding table)")
            # what the eager loop returns: the first length at which every row has produced eos_id
            every = (self.out[:, T:n] == eos).to(torch.uint8).cummax(dim=1).values.all(dim=0)
            at = torch.nonzero(every).flatten()[:1].tolist()
            if at:
                n = T + 1 + at[0]
        for s in self.states:
            s._replayed(ran)                                               # the mirror of what the replays fed ...
            s.count = n - 1                                                # ... back to what the eager loop has fed (a KV cache is cut)
        sampler.draws = first_draw + n - T
        return self.out[:, :n].clone()

    def serves(self, wte, blocks, head, states, cos, sin, temperature, top_k, eos_id, top_p=None) -> bool:
        """whether ``generate(...)`` with these arguments is the loop this decoder recorded"""
        g = self.given
        same = (wte is g["wte"] and blocks is g["blocks"] and head is g["head"] and cos is g["cos"] and sin is g["sin"]
                and len(states) == len(self.states) and all(a is b for a, b in zip(states, self.states)))
        return (same and float(temperature) == self.temperature and top_k == self.top_k and eos_id == self.eos_id
                and _nucleus(top_p) == self.top_p)


@torch.no_grad()
def generate(wte: torch.Tensor, blocks, head: NextTokenHead, states, prompt: torch.Tensor, max_returned_tokens: int, *, cos, sin,
             temperature: float = 1.0, top_k=None, eos_id=None, sampler: Sampler = None, graphed: GraphedDecoder = None,
             top_p=None) -> torch.Tensor:
    """prompt (B, T) int64 -> (B, n) tokens, the prompt included, n <= max_returned_tokens.

    ``wte`` is the embedding weight, ``blocks`` a ``BlockStack`` or a sequence of ``Block`` (a ``NeoXStack`` or a sequence of
    ``NeoXBlock`` for the parallel-residual form; one kind per call), ``states`` one EMPTY decode state
    cache per block (``FastmaxDecodeState(p=2)`` / ``LinearmaxDecodeState``, or a ``FastmaxKVDecodeState`` with room for
    ``max_returned_tokens - 1`` tokens), ``cos`` / ``sin`` the rope cache with a row for
    every position fed.  The prompt goes through the blocks in one call, then one token per call with the rope rows of its
    position.  Nothing is read back per token unless ``eos_id`` is given; then the loop ends once every row has produced it.
    ``graphed``: a ``GraphedDecoder`` built from these same arguments runs the loop as one graph replay per token; the default is
    the loop below.  ``top_p``: nucleus sampling behind the top-k (``Sampler.sample``)."""
    if graphed is not None:
        if not graphed.serves(wte, blocks, head, states, cos, sin, temperature, top_k, eos_id, top_p):
            raise ValueError("generate: graphed was built from other tensors, blocks, states or sampling settings than this call's")
        return graphed.generate(prompt, max_returned_tokens, sampler)
    B, T = _check_prompt(prompt, max_returned_tokens, cos, sin)
    _check_sampling(temperature, top_k, top_p)
    layers, run = _layers_and_run(blocks, states)
    for s in states:
        s.check_capacity(max_returned_tokens - 1, "generate")
    sampler = Sampler() if sampler is None else sampler
    dev = prompt.device
    pos = torch.arange(max_returned_tokens, device=dev)
    out = torch.empty((B, max_returned_tokens), dtype=torch.int64, device=dev)
    out[:, :T] = prompt
    h = run(layers, F.embedding(prompt, wte), cos[:T], sin[:T], pos[:T], states)
    n, done = T, None
    while True:
        token = head(h, sampler, temperature, top_k, top_p)
        out[:, n] = token
        n += 1
        if eos_id is not None:
            hit = token == eos_id
            done = hit if done is None else done | hit
            if bool(done.all()):
                break
        if n == max_returned_tokens:
            break
        t = n - 1                                                      # the position of the token just produced
        h = run(layers, F.embedding(token.view(B, 1), wte), cos[t:t + 1], sin[t:t + 1], pos[t:t + 1], states)
    return out[:, :n]
