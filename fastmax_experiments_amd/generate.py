"""From the last hidden state to the next token in HIP, and the generation loop around it.

The last stretch of the reference's loop (generate/base.py:30-47 after lit_gpt/model.py's ``ln_f`` + ``lm_head``) computes a
(B, T, V) head GEMM of which one row is used, then ``topk``, ``scatter_``, ``softmax`` and ``multinomial`` with a host read per
token.  Here (csrc/next_token.hip, C ABI: include/fastmax_hip_next_token.h, bound by ``_lib.NEXT_TOKEN_ABI``):
    last_logits    the head over the LAST position only; the weight is read once for up to 8 rows
    Sampler        exact top-k (ties: the lowest indices are kept) and a draw from softmax(logits / temperature) as the argmax of
                   logit / temperature - log(-log u), u from Philox-4x32-10 under (seed, draw number): the token stays on the device
    NextTokenHead  ``ln_f`` (the RMSNorm or LayerNorm kernel on the B last rows) + ``lm_head`` + the sampler
    generate       prompt -> tokens through decoder blocks (``Block`` or ``NeoXBlock``) on their decode state caches
What differs from the reference: logits are float32 by default (``dtype=`` gives the reference's), and the random stream is the
sampler's own seeded one instead of torch's generator, so a (seed, draw) pair reproduces a token on any batch.  There is no CPU
path through the kernels; ``NextTokenHead.fused = False`` selects the tensor-op restatement for A/B runs.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .block import BlockStack, RMSNorm, rms_norm_forward
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


def last_logits(x: torch.Tensor, weight: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """x (B, C) with unit stride along C and any row stride (a last-position view), weight (V, C) -> logits (B, V) in ``dtype``
    (float32 or the inputs' dtype), accumulated in float32.  A row's logits do not depend on the batch it is computed in."""
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or 0 in x.shape or 0 in weight.shape:
        raise ValueError(f"last_logits: x should be (B, C) and weight (V, C), got {tuple(x.shape)} and {tuple(weight.shape)}")
    if x.dtype != weight.dtype or x.dtype not in ops._DT:
        raise TypeError(f"last_logits: x and weight should share float32, bfloat16 or float16, got {x.dtype} and {weight.dtype}")
    if dtype not in (torch.float32, x.dtype):
        raise TypeError(f"last_logits: dtype should be float32 or {x.dtype}, got {dtype}")
    _need_device(x, "last_logits")
    x2 = _unit_rows(x)
    w = weight if weight.stride(1) == 1 and weight.stride(0) >= weight.shape[1] else weight.contiguous()
    B, C = x2.shape
    V = w.shape[0]
    out = torch.empty((B, V), dtype=dtype, device=x.device)
    ops._call("fastmax_hip_last_logits", x.device,
              (x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), B, V, C, ops._DT[x.dtype],
               ops._DT[dtype]))
    return out


def _check_sampling(temperature, top_k):
    if not (temperature >= 0.0) or temperature == float("inf"):
        raise ValueError(f"temperature should be a finite number >= 0, got {temperature}")
    if top_k is not None and (int(top_k) != top_k or top_k < 1):
        raise ValueError(f"top_k should be None or an integer >= 1, got {top_k}")


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

    def sample(self, logits: torch.Tensor, temperature: float = 1.0, top_k=None) -> torch.Tensor:
        """logits (B, V) -> (B,) int64 tokens on the device; nothing is read back.  ``temperature == 0`` is the argmax."""
        _check_sampling(temperature, top_k)
        rows = _logit_rows(logits, "Sampler.sample")
        B, V = rows.shape
        tokens = torch.empty(B, dtype=torch.int64, device=rows.device)
        ops._call("fastmax_hip_sample", rows.device,
                  (rows.data_ptr(), rows.stride(0), tokens.data_ptr(), B, V, 0 if top_k is None else min(int(top_k), V),
                   float(temperature), _signed64(self.seed), _signed64(self.draws)))
        self.draws += 1
        return tokens

    def keep_mask(self, logits: torch.Tensor, top_k) -> torch.Tensor:
        """bool (B, V): the entries ``sample`` would choose among.  Exactly ``top_k`` per row (all of them for None or
        ``top_k >= V``): those above the k-th largest value and, of those equal to it, the lowest indices."""
        _check_sampling(0.0, top_k)
        rows = _logit_rows(logits, "Sampler.keep_mask")
        B, V = rows.shape
        mask = torch.empty((B, V), dtype=torch.uint8, device=rows.device)
        ops._call("fastmax_hip_topk_mask", rows.device,
                  (rows.data_ptr(), rows.stride(0), mask.data_ptr(), mask.stride(0), B, V, 0 if top_k is None else min(int(top_k), V)))
        return mask.bool()


def _sample_tensor_ops(logits: torch.Tensor, temperature: float, top_k) -> torch.Tensor:
    """generate/base.py:30-41 for a batch of rows, drawing from torch's generator"""
    if top_k is not None:
        v, i = torch.topk(logits, min(int(top_k), logits.size(-1)))
        logits = torch.full_like(logits, float("-inf")).scatter_(-1, i, v)
    if temperature > 0.0:
        probs = torch.softmax(logits / temperature, dim=-1)
        return torch.multinomial(probs, num_samples=1).squeeze(-1)
    return torch.argmax(logits, dim=-1)


class NextTokenHead(nn.Module):
    """``ln_f`` + ``lm_head`` (the reference's names, so its state-dict keys load) + the sampler.  ``vocab_size`` rows of the
    ``padded_vocab_size`` rows of the weight are scored; the default is all of them, which is what the reference samples over.
    ``norm_class``: "RMSNorm", or "LayerNorm" (the pythia models; state-dict keys ``ln_f.weight`` and ``ln_f.bias``)."""

    def __init__(self, n_embd: int, padded_vocab_size: int, vocab_size: int = None, norm_eps: float = 1e-5,
                 add_unit_offset: bool = False, norm_class: str = "RMSNorm") -> None:
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
        self.lm_head = nn.Linear(n_embd, padded_vocab_size, bias=False)
        self.vocab_size = vocab_size
        self.fused = True                     # False: the tensor-op restatement (whole (B, T, V) head, topk + softmax + multinomial)

    def logits(self, x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        """x (B, T, C) or (B, C) -> the logits (B, vocab_size) of the last position"""
        if x.dim() not in (2, 3):
            raise ValueError(f"NextTokenHead: x should be (B, T, C) or (B, C), got {tuple(x.shape)}")
        if not self.fused:
            n = self.ln_f._eager(x)
            y = self.lm_head(n)
            return (y[:, -1] if x.dim() == 3 else y)[:, :self.vocab_size].to(dtype)
        last = x[:, -1] if x.dim() == 3 else x
        if isinstance(self.ln_f, LayerNorm):
            _, n, _, _, _ = layer_norm_forward(last, self.ln_f.weight.detach(), self.ln_f.bias.detach(), self.ln_f.eps)
        else:
            _, n, _ = rms_norm_forward(last, None, self.ln_f.weight.detach(), self.ln_f.eps, self.ln_f.add_unit_offset)
        return last_logits(n, self.lm_head.weight.detach()[:self.vocab_size], dtype)

    def forward(self, x: torch.Tensor, sampler: Sampler, temperature: float = 1.0, top_k=None) -> torch.Tensor:
        """-> (B,) int64 tokens"""
        _check_sampling(temperature, top_k)
        logits = self.logits(x)
        if not self.fused:
            return _sample_tensor_ops(logits, temperature, top_k)
        return sampler.sample(logits, temperature, top_k)


@torch.no_grad()
def generate(wte: torch.Tensor, blocks, head: NextTokenHead, states, prompt: torch.Tensor, max_returned_tokens: int, *, cos, sin,
             temperature: float = 1.0, top_k=None, eos_id=None, sampler: Sampler = None) -> torch.Tensor:
    """prompt (B, T) int64 -> (B, n) tokens, the prompt included, n <= max_returned_tokens.

    ``wte`` is the embedding weight, ``blocks`` a ``BlockStack`` or a sequence of ``Block`` (a ``NeoXStack`` or a sequence of
    ``NeoXBlock`` for the parallel-residual form; one kind per call), ``states`` one EMPTY decode state
    cache per block (``FastmaxDecodeState(p=2)`` / ``LinearmaxDecodeState``), ``cos`` / ``sin`` the rope cache with a row for
    every position fed.  The prompt goes through the blocks in one call, then one token per call with the rope rows of its
    position.  Nothing is read back per token unless ``eos_id`` is given; then the loop ends once every row has produced it."""
    if prompt.dim() != 2 or prompt.dtype != torch.int64:
        raise ValueError(f"generate: prompt should be (B, T) int64, got {tuple(prompt.shape)} {prompt.dtype}")
    B, T = prompt.shape
    if T < 1 or max_returned_tokens <= T:
        raise ValueError(f"generate: max_returned_tokens ({max_returned_tokens}) should exceed the prompt's length ({T} >= 1)")
    if cos.shape[0] < max_returned_tokens - 1 or sin.shape[0] < max_returned_tokens - 1:
        raise ValueError(f"generate: the rope cache has {cos.shape[0]} rows, {max_returned_tokens - 1} positions are fed")
    _check_sampling(temperature, top_k)
    layers = blocks.blocks if isinstance(blocks, (BlockStack, NeoXStack)) else blocks
    runs = {type(b).run_sequence for b in layers}                      # a block's class names what runs a sequence of its kind
    if len(runs) > 1:
        raise ValueError("generate: the blocks mix NeoXBlock with another kind; a sequence holds one kind")
    if len(states) != len(layers):
        raise ValueError(f"generate: {len(layers)} blocks need as many decode state caches, got {len(states)}")
    (run,) = runs
    sampler = Sampler() if sampler is None else sampler
    dev = prompt.device
    pos = torch.arange(max_returned_tokens, device=dev)
    out = torch.empty((B, max_returned_tokens), dtype=torch.int64, device=dev)
    out[:, :T] = prompt
    h = run(layers, F.embedding(prompt, wte), cos[:T], sin[:T], pos[:T], states)
    n, done = T, None
    while True:
        token = head(h, sampler, temperature, top_k)
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
