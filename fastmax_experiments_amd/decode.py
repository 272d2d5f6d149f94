"""Opt-in decode-time state caches: fastmax first order (p=1) and second order (p=2), and first-order
linearmax (`LinearmaxDecodeState`).

The reference generates with a zero-padded KV cache and re-runs UNMASKED attention over the whole cache for every
new token (lit_gpt/model.py:427-430, 464-466; generate/base.py:85-92): O(N D) per token and, by quirk Q4, not the
same function as masked attention over the real sequence.  Here a carried state lives in HBM: `prefill` builds it from
the prompt and `step` returns masked fastmax at the new last position for a fixed cost per token.  Because it changes
the decode semantics it is a separate class, not a silent replacement of `fastmax(mask=False)`.

  p=1  state (S2 = sum k v^T, S1 = sum v, ksum = sum k, count) per head; O(D^2) per token (csrc/fastmax_decode.hip).
  p=2  the model's `fastmax(q, k, v, p=2)` (attention_block.py).  With k~ = [1, k] and v' = [v, 1] the state is
       S~[(m,l)][j] = sum_n k~_m k~_l v'_j over the pairs m <= l, (D+1)(D+2)/2 rows of D+1 floats (0.58 MB per head at
       D = 64, 4.4 MB at D = 128); O(D^3) per token (csrc/fastmax_decode_p2.hip).  It depends on K and V only, so it
       is kept per KV head: with grouped-query attention (`n_query_groups` < H) one pass over a group's state serves
       its H / n_query_groups query heads.  The token count inside the state is an fp32 sum of ones: exact up to 2^24
       tokens.  The prompt's own outputs come from the masked p=2 forward (`fastmax(..., mask=True, p=2)`).
       `extend` continues a state of any length by T >= 1 tokens at once (a second turn, a block of draft tokens, a long
       prompt in pieces): the cached tokens are read out of the state for all T queries in one matrix-core pass, the
       chunk's own masked part comes from the p=2 tile kernels, and the state is then advanced by the T tokens: about
       three passes over the state instead of the 2 T of T single steps.  `prefill(..., chunk=C)` feeds a prompt as
       `extend` calls of C tokens: masked p=2 attention in time linear in N (forward only).
       `step_qkv` / `extend_qkv` take the attention block's QKV projection output (B,T,G,q_per_kv+2,hs) and the rope rows
       of the new positions instead of split, rotated q, k, v: what `CausalSelfAttention.forward(..., state=...)` calls.
       For one token the step kernel can de-interleave and rotate while it loads (csrc/fastmax_decode_qkv.hip): bit-identical
       to the split + RoPE pass followed by `step`, one launch less (`fused_step`, off by default: FUSED_STEP_DEFAULT).

  linearmax  the model's `fastmax_hack(q, k, v, p=1, mask=True)`: `LinearmaxDecodeState` (csrc/linearmax_decode.hip).  The
       prologue centres every q and k row over D and divides ALL of q by one scalar per (b, h), Mq = the largest centred-row
       norm of q over the sequence, and all of k by Mk likewise.  With qc, kc the centred, unscaled rows
           f(q^_i . k^_j) = 1 + (qc_i . kc_j) / (Mq Mk)
           o_i = (S1 + a qc_i^T S2) / (count + a qc_i . ksum),   a = 1 / (Mq Mk)
           S2 = sum_j kc_j v_j^T,  S1 = sum_j v_j,  ksum = sum_j kc_j     (sums over j <= i)
       so the two statistics leave the bilinear sums as one scalar: a state of unscaled centred sums never needs rescaling,
       only a moves as the two running maxima grow.  O(D^2) per token and about 70 KB per KV head at D = 128.

  KV cache  `FastmaxKVDecodeState` (csrc/fastmax_kv_decode.hip): the K and V rows themselves, the length a device word, and masked
       fastmax over the live prefix at every new position: O(N D) per token like the reference's cache, but the masked function,
       grouped-query heads on one K/V read, and head sizes up to 256, where the carried states stop at 128.  Opt-in like the rest.
"""
import ctypes

import torch

from . import _lib, ops
from .attention_mechanisms.fastmax import fastmax
from .attention_mechanisms.fastmax_hack import fastmax_hack


# FastmaxDecodeState.step_qkv: which of the two bit-identical routes a new state takes.  The fused step has not yet been timed
# against split + step on an MI355X (profiles/r07_block_decode.md), so the route made only of previously measured kernels
# stays the default; set `state.fused_step = True` for the single-launch step.
FUSED_STEP_DEFAULT = False


def _kv_heads(H, n_query_groups):
    """the number of KV heads under ``n_query_groups`` (None: one per query head)"""
    Hkv = H if n_query_groups is None else n_query_groups
    if Hkv <= 0 or H % Hkv != 0:
        raise ValueError(f"n_query_groups={n_query_groups} does not divide the {H} query heads")
    return Hkv


class _DecodeState:
    """What the state caches share: the record `state` (float32, zeroed) of `count` tokens for B sequences of H query heads on
    Hkv KV heads of size D, and the entry points that take the attention block's QKV projection output.  A subclass gives
    `prefill`, `step` and `extend` on split, rotated q (B,H,T,D) and k, v (B,Hkv,T,D).

    What the attention block and the generation loop ask of a cache is answered here and nowhere else: `check_block_cache`
    (below the classes) for which block generates on which cache, `max_len` and `check_capacity` for how many tokens it holds,
    `check_recordable` for a loop recorded as a graph.  Those three read `max_len`, `p` and `B` of a cache only."""

    max_len = None          # the most tokens the cache holds; None: a carried state, which never fills up
    _count = 0

    def __init__(self, B, H, Hkv, D, nbytes, device, unsupported):
        if nbytes == 0:
            raise NotImplementedError(unsupported)
        self.B, self.H, self.Hkv, self.D = B, H, Hkv, D
        self.state = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)

    @property
    def count(self):
        """the tokens fed so far, on the host; where the kernels keep a count of their own this is its mirror, never read back"""
        return self._count

    @count.setter
    def count(self, n):
        self._count = n

    def reset(self):
        """Empty sequence again; the allocation is kept (a generation loop resets between prompts)."""
        self.state.zero_()
        self._count = 0

    def _restore(self, state, count):
        """back to a saved (``state.clone()``, ``count``) pair: what a graph recording does after its warm-up steps"""
        self.state.copy_(state)
        self._count = count

    def _replayed(self, steps):
        """``steps`` single-token steps ran from a recorded graph, which moves no host counter: the mirror follows"""
        self._count += steps

    def check_capacity(self, fed, what):
        """refuse, before anything runs, a call of ``what`` that feeds more tokens than the cache holds"""
        if self.max_len is not None and fed > self.max_len:
            raise ValueError(f"{what}: {fed} tokens are fed, a {type(self).__name__} of this call holds at most {self.max_len}")

    def check_recordable(self, steps):
        """refuse a cache that a graph of one decode step cannot be recorded on; the recording itself runs ``steps`` single-token
        steps on the non-empty cache"""
        if self.max_len is not None and self.max_len <= steps:
            raise ValueError(f"GraphedDecoder: the recording runs {steps} steps on a non-empty cache; a "
                             f"{type(self).__name__} needs max_len > {steps}, got {self.max_len}")

    def _fastmax_of(self, D, p, normalize_term, tensors_normalized):
        """a fastmax cache's function: order ``p`` and the scaling, as `fastmax` takes them"""
        if p not in (1, 2):
            raise ValueError(f"p should be 1 or 2, got p={p}")
        self.p = p
        self.nt = ops.effective_normalize_term(D, normalize_term, tensors_normalized)
        self._kw = dict(normalize_term=normalize_term, tensors_normalized=tensors_normalized)

    def _masked_fastmax(self, q, k, v):
        """that function over a whole prompt, masked (the tile kernels) -> o (B,H,T,D)"""
        return self._masked_forward(lambda *qkv: fastmax(*qkv, mask=True, p=self.p, **self._kw), q, k, v)

    @staticmethod
    def _tokens(q, what):
        """T of q (B,H,T,D), one token at least"""
        T = q.shape[2] if q.dim() == 4 else 0
        if T < 1:
            raise ValueError(f"{what} takes q (B,H,T,D) with T >= 1, got {tuple(q.shape)}")
        return T

    def _unit_rows(self, q, k, v):
        """q, k, v on the state's device in q's dtype, as the kernels that take any strides with unit stride in D read them (views
        of the split's output as they are)"""
        dev = self.state.device
        return tuple(t if t.stride(3) == 1 else t.contiguous() for t in (x.to(device=dev, dtype=q.dtype) for x in (q, k, v)))

    # qkv (B,T,G,q_per_kv+2,hs) -> rotated q (B,H,T,hs), rotated k and v (B,G,T,hs): one HIP pass where the split kernel takes
    # the shape, else tensor slicing + apply_rope (model.py:397-425)
    _split_qkv = staticmethod(ops.rope_qkv_split)

    def _check_shapes(self, q, k, v, n):
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        if tuple(q.shape) != (B, H, n, D) or tuple(k.shape) != (B, Hkv, n, D) or tuple(v.shape) != (B, Hkv, n, D):
            raise ValueError(f"expected q {(B, H, n, D)} and k, v {(B, Hkv, n, D)}, got {tuple(q.shape)}, {tuple(k.shape)} "
                             f"and {tuple(v.shape)}")

    def _masked_forward(self, attend, q, k, v):
        """attend(q, k, v) over a whole prompt whose K and V sit at their Hkv heads -> o (B,H,T,D)"""
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        if Hkv == H:
            return attend(q, k, v)
        # each group's query heads as the heads of one batch entry, its K and V as stride-0 views over them
        r, T = H // Hkv, q.shape[2]
        qg = q.reshape(B * Hkv, r, T, D)
        kg, vg = (t.reshape(B * Hkv, 1, T, D).expand(B * Hkv, r, T, D) for t in (k, v))
        return attend(qg, kg, vg).reshape(B, H, T, D)

    def _check_qkv(self, qkv, cos, sin, rope_n_elem, what):
        """the QKV projection's output and the rope rows of its T positions, as step_qkv / extend_qkv take them -> (T, rope_n_elem)"""
        B, H, G, D = self.B, self.H, self.Hkv, self.D
        if qkv.dim() != 5 or tuple(qkv.shape[:1] + qkv.shape[2:]) != (B, G, H // G + 2, D) or qkv.shape[1] < 1:
            raise ValueError(f"expected qkv (B,T,G,q_per_kv+2,hs) = {(B, 'T', G, H // G + 2, D)}, got {tuple(qkv.shape)}")
        T = qkv.shape[1]
        n = int(rope_n_elem)
        for t in (cos, sin):
            if t.dim() != 2 or t.shape[0] != T or t.shape[1] < n:
                raise ValueError(f"expected the rope rows of the {T} new positions, (T, >= {n}), got {tuple(t.shape)}")
        return T, n

    def step_qkv(self, qkv, cos, sin, rope_n_elem):
        """ONE new token from the QKV projection's output, qkv (B,1,G,q_per_kv+2,hs) (slots 0..q_per_kv-1 of a group are its
        query heads, then its key head, then its value head); cos, sin: the rope row of the new position, (1, >= rope_n_elem)
        -> o (B,H,1,hs) in qkv's dtype.  Split + RoPE with K and V left at their G heads, then `step`."""
        T, n = self._check_qkv(qkv, cos, sin, rope_n_elem, "step_qkv")
        if T != 1:
            raise ValueError(f"step_qkv takes one token, got T={T}; use extend_qkv")
        return self._step_qkv(qkv, cos, sin, n)

    def _step_qkv(self, qkv, cos, sin, n):
        return self.step(*self._split_qkv(qkv, cos, sin, n))

    def extend_qkv(self, qkv, cos, sin, rope_n_elem):
        """T >= 1 new tokens from the QKV projection's output, qkv (B,T,G,q_per_kv+2,hs); cos, sin: the rope rows of the T new
        positions -> o (B,H,T,hs).  Split + RoPE with K and V at their G heads, then `extend`; `prefill` on an empty state."""
        _, n = self._check_qkv(qkv, cos, sin, rope_n_elem, "extend_qkv")
        q, k, v = self._split_qkv(qkv, cos, sin, n)
        return self._prefill_qkv(q, k, v) if self.count == 0 else self.extend(q, k, v)

    def _prefill_qkv(self, q, k, v):
        return self.prefill(q, k, v)


class FastmaxDecodeState(_DecodeState):
    def __init__(self, B, H, D, device, normalize_term=8, tensors_normalized=False, p=1, n_query_groups=None):
        self._fastmax_of(D, p, normalize_term, tensors_normalized)
        if p == 1 and n_query_groups not in (None, H):
            raise ValueError("the first-order decode state has one record per head: n_query_groups must be None or H")
        Hkv = _kv_heads(H, n_query_groups)
        L = _lib.lib()
        # the second-order state is kept per KV head
        nbytes = L.fastmax_hip_decode_state_bytes(B, H, D) if p == 1 else L.fastmax_hip_p2_decode_state_bytes(B, Hkv, D)
        super().__init__(B, H, Hkv, D, nbytes, device, f"head size {D} not supported")
        self.prefill_chunk = None   # extend_qkv on an empty state: prefill(..., chunk=prefill_chunk)
        # step_qkv: True = the step kernel rotates q, k while it loads them; False = split + RoPE pass, then step (two
        # launches).  Bit-identical.  See FUSED_STEP_DEFAULT for the measurement behind the default.
        self.fused_step = FUSED_STEP_DEFAULT

    def prefill(self, q, k, v, chunk=None):
        """Masked forward over the prompt; also captures the end-of-prompt state.  Returns o (B,H,N,D).
        p=2: q (B,H,N,D), k and v (B,n_query_groups,N,D).  With `chunk=C` (p=2) the prompt is fed as `extend` calls of C
        tokens, the last one shorter: linear in N, where the default runs the quadratic tile kernels over the whole prompt."""
        if chunk is not None:
            if chunk <= 0:
                raise ValueError(f"chunk should be a positive number of tokens, got chunk={chunk}")
            if self.p != 2:
                raise NotImplementedError("chunked prefill needs the second-order state cache (p=2)")
        assert self.count == 0, "prefill starts a sequence"
        self._check_shapes(q, k, v, q.shape[2])
        if chunk is not None:
            o = torch.empty((self.B, self.H, q.shape[2], self.D), dtype=q.dtype, device=q.device)
            for s in range(0, q.shape[2], chunk):
                o[:, :, s:s + chunk] = self.extend(q[:, :, s:s + chunk], k[:, :, s:s + chunk], v[:, :, s:s + chunk])
            return o
        o = self._masked_fastmax(q, k, v)
        # the state of the whole prompt from its prepared k, v
        kd, vd = ops._prep(k, k.device), ops._prep(v.to(k.dtype), k.device)
        prob = ops._problem(kd, kd, kd.dtype, kd.dtype, self.p, True, self.nt, 0.0)
        ops._call(f"fastmax_hip_p{self.p}_prefill_state", kd.device, (ctypes.byref(prob), *ops._qkv(kd, vd), self.state.data_ptr()))
        self._count = kd.shape[2]
        return o

    def step(self, q, k, v):
        """q,k,v: (B,H,1,D) of the new token -> o (B,H,1,D); O(D^2) per head.
        p=2: k and v are (B,n_query_groups,1,D); O(D^3) per KV head."""
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        if self.p == 2:
            self._check_shapes(q, k, v, 1)
            k, v = k.to(q.dtype), v.to(q.dtype)
        qd, kd, vd = (ops._prep(t, q.device) for t in (q, k, v))
        o = torch.empty((B, H, 1, D), dtype=q.dtype, device=q.device)
        dt = ops._DT[q.dtype]
        args = (*ops._qkv(qd, kd, vd), self.state.data_ptr(), o.data_ptr())
        if self.p == 2:
            ops._call("fastmax_hip_p2_decode_step", q.device, args + (B, H, Hkv, D, dt, dt, 1.0 / self.nt))
        else:
            ops._call("fastmax_hip_p1_decode_step", q.device, args + (B, H, D, dt, dt, 1.0 / self.nt, self.count + 1))
        self._count += 1
        return o

    def extend(self, q, k, v):
        """p=2: T >= 1 new tokens after the `count` cached ones (any count, 0 included).  q (B,H,T,D), k and v
        (B,n_query_groups,T,D) -> o (B,H,T,D) in q's dtype = masked p=2 fastmax at the T new positions over the cached and
        the new tokens; the state advances by T tokens."""
        if self.p != 2:
            raise NotImplementedError("extend needs the second-order state cache (p=2); for linearmax blocks, whose statistics "
                                      "run over the whole sequence, use LinearmaxDecodeState")
        T = self._tokens(q, "extend")
        self._check_shapes(q, k, v, T)
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        qd, kd, vd = (ops._prep(t.to(q.dtype), q.device) for t in (q, k, v))
        o = torch.empty((B, H, T, D), dtype=q.dtype, device=q.device)
        prob = ops._problem(qd, kd, qd.dtype, qd.dtype, 2, True, self.nt, 0.0)
        ops._call("fastmax_hip_p2_extend", q.device, (ctypes.byref(prob), Hkv, *ops._qkv(qd, kd, vd), self.state.data_ptr(), o.data_ptr()),
                  ws=_lib.lib().fastmax_hip_p2_extend_workspace(B, H, Hkv, T, D))
        self._count += T
        return o

    def check_recordable(self, steps):
        if self.p != 2:
            raise NotImplementedError("GraphedDecoder: a first-order FastmaxDecodeState passes its token count to the step kernel "
                                      "by value, which a recorded graph would freeze; use FastmaxDecodeState(p=2) or "
                                      "LinearmaxDecodeState")
        super().check_recordable(steps)

    def _check_qkv(self, qkv, cos, sin, rope_n_elem, what):
        if self.p != 2:
            raise NotImplementedError(f"{what} needs the second-order state cache (p=2); for linearmax blocks, whose statistics "
                                      "run over the whole sequence, use LinearmaxDecodeState")
        return super()._check_qkv(qkv, cos, sin, rope_n_elem, what)

    def _step_qkv(self, qkv, cos, sin, n):
        """`fused_step`: de-interleave + RoPE happen inside the step kernel's loader when
        fastmax_hip_p2_decode_step_qkv_supported says so; else (and with fused_step off) split + RoPE, then `step`."""
        B, H, G, D = self.B, self.H, self.Hkv, self.D
        dt = ops._DT.get(qkv.dtype)
        L = _lib.lib()
        if not (self.fused_step and qkv.is_cuda and dt is not None and
                L.fastmax_hip_p2_decode_step_qkv_supported(G, H // G, D, n, dt)):
            return super()._step_qkv(qkv, cos, sin, n)
        qkv = qkv.contiguous()
        tables16 = int(cos.dtype == qkv.dtype and qkv.dtype in (torch.bfloat16, torch.float16))
        cos32, sin32 = (t[:, :n].float().contiguous() for t in (cos, sin))
        o = torch.empty((B, H, 1, D), dtype=qkv.dtype, device=qkv.device)
        ops._call("fastmax_hip_p2_decode_step_qkv", qkv.device,
                  (qkv.data_ptr(), cos32.data_ptr(), sin32.data_ptr(), self.state.data_ptr(), o.data_ptr(), B, G, H // G, D, n,
                   tables16, dt, dt, 1.0 / self.nt))
        self._count += 1
        return o

    def _prefill_qkv(self, q, k, v):
        return self.prefill(q, k, v, chunk=self.prefill_chunk)     # None: the one-shot masked forward + state capture


class FastmaxKVDecodeState(_DecodeState):
    """KV-cache decode for fastmax blocks (csrc/fastmax_kv_decode.hip, include/fastmax_hip_kv_decode.h): the K and V rows of up to
    ``max_len`` tokens in ``dtype`` (the activations'), and at each new position masked polynomial attention
    o = sum_j f(s_j) v_j / sum_j f(s_j) over the cached rows and the new ones, in float32.  Head sizes 1 .. 256: the two config
    shapes with 256-wide heads (pythia-1b, Gemma-2b) generate on this class only.  Per token it reads the live prefix of the
    cache, 4 D bytes per bf16 position, where the second-order state moves (D+1)(D+2)/2 (D+1) floats whatever the length; the
    measured crossover lengths are in profiles/r23_kv_decode.md.  Opt-in: nothing selects it automatically.

    q (B,H,T,D); k and v (B,n_query_groups,T,D) at their KV heads: one read of a K/V row serves the group's query heads.
    ``state`` is ONE tensor: a 64-byte header (int32 words: the length, a sticky overflow flag) and both caches, so a
    ``clone()`` / ``copy_()`` pair saves and restores everything.  The length the kernels use is the header's; ``count`` is the
    host's mirror of it and nothing is ever read back.  A row's output bits depend on its q row and the cache prefix alone: not on
    B, the batch row, T (a token fed alone or inside an ``extend``), ``max_len``, the inputs' strides or eager / replayed."""

    def __init__(self, B, H, D, device, max_len, dtype, p=2, n_query_groups=None, normalize_term=8, tensors_normalized=False):
        self._fastmax_of(D, p, normalize_term, tensors_normalized)
        Hkv = _kv_heads(H, n_query_groups)
        if dtype not in ops._DT:
            raise ValueError(f"the KV decode cache holds float32, bfloat16 or float16, got {dtype}")
        if int(max_len) != max_len or max_len < 1 or max_len >= 2 ** 31:
            raise ValueError(f"max_len should be a number of tokens in 1 .. 2^31 - 1, got {max_len}")
        self.dtype, self.max_len = dtype, int(max_len)
        nbytes = _lib.lib().fastmax_hip_kv_decode_state_bytes(B, Hkv, D, self.max_len, ops._DT[dtype])
        if nbytes and torch.device(device).type != "cuda":
            raise RuntimeError("the KV decode cache lives on an MI355X (HIP device); there is no CPU path through the kernels")
        super().__init__(B, H, Hkv, D, nbytes, device,
                         f"KV decode cache: batch {B} x {Hkv} KV heads of size {D} not supported (head sizes 1 .. {_lib.KV_MAX_D}, "
                         f"B * n_query_groups <= 65535)")
        self.capacity = -(-self.max_len // _lib.KV_CHUNK) * _lib.KV_CHUNK       # positions allocated: max_len up to a whole chunk

    @classmethod
    def for_attention(cls, attn, B, max_len, device, dtype):
        """the cache of a ``CausalSelfAttention`` (``attn_alg="fastmax"``: the block's p = 2 with its default scaling)"""
        return cls(B, attn.n_head, attn.head_size, device, max_len, dtype, p=2, n_query_groups=attn.n_query_groups)

    @property
    def header(self):
        """the header's int32 words, a view of ``state`` (reading them synchronises)"""
        return self.state[:_lib.KV_HEADER_WORDS].view(torch.int32)

    @_DecodeState.count.setter
    def count(self, n):
        """a smaller value truncates the cache (one small device write; the rows stay and are overwritten); a larger one raises"""
        n = int(n)
        if n < 0 or n > self._count:
            raise ValueError(f"count can only be lowered (a truncation): the cache holds {self._count} tokens, got {n}")
        if n < self._count:
            ops._call("fastmax_hip_kv_decode_set_len", self.state.device, (self.state.data_ptr(), n, self.max_len))
        self._count = n

    def reset(self):
        """Empty sequence again: the header is cleared, the rows stay where they are."""
        self.state[:_lib.KV_HEADER_WORDS].zero_()
        self._count = 0

    def _inputs(self, q, k, v, T):
        self._check_shapes(q, k, v, T)
        if not (q.dtype == k.dtype == v.dtype == self.dtype):
            raise TypeError(f"the cache holds {self.dtype}, got q {q.dtype}, k {k.dtype}, v {v.dtype}")
        if self._count + T > self.max_len:
            raise ValueError(f"the cache holds {self._count} of at most {self.max_len} tokens, {T} more do not fit")
        return self._unit_rows(q, k, v)

    def prefill(self, q, k, v):
        """Masked forward over the prompt (the tile kernels), o (B,H,T,D); the cache then holds the prompt's K and V rows."""
        assert self._count == 0, "prefill starts a sequence"
        T = self._tokens(q, "prefill")
        qd, kd, vd = self._inputs(q, k, v, T)
        with torch.no_grad():
            o = self._masked_fastmax(qd, kd, vd)
        ops._call("fastmax_hip_kv_decode_load", self.state.device,
                  (*ops._qkv(kd, vd), self.state.data_ptr(), self.B, self.Hkv, T, self.D, self.max_len, ops._DT[self.dtype]))
        self._count = T
        return o

    def step(self, q, k, v):
        """q (B,H,1,D), k and v (B,n_query_groups,1,D) of the new token -> o (B,H,1,D): the rows join the cache, one pass over
        its live prefix serves every query head of a group."""
        return self._append_attend(q, k, v, 1)

    def extend(self, q, k, v):
        """T >= 1 new tokens after the ``count`` cached ones (any count, 0 included) -> o (B,H,T,D) = masked attention at the T
        new positions; bit for bit what T single steps give."""
        return self._append_attend(q, k, v, self._tokens(q, "extend"))

    def _append_attend(self, q, k, v, T):
        qd, kd, vd = self._inputs(q, k, v, T)
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        dev = self.state.device
        o = torch.empty((B, H, T, D), dtype=self.dtype, device=dev)
        ops._call("fastmax_hip_kv_decode_append_attend", dev,
                  (*ops._qkv(qd, kd, vd), self.state.data_ptr(), o.data_ptr(), B, H, Hkv, T, D, self.max_len, ops._DT[self.dtype],
                   self.p, 1.0 / self.nt),
                  ws=_lib.lib().fastmax_hip_kv_decode_workspace(B, H, Hkv, T, D, self.max_len))
        self._count += T
        return o


class LinearmaxDecodeState(_DecodeState):
    """Decode state cache of a linearmax block: masked first-order linearmax L(q, k, v) = fastmax_hack(q, k, v, p=1, mask=True)
    at O(D^2) per token (the factorisation is in the module docstring).  q (B,H,T,D); k and v (B,n_query_groups,T,D) at their
    KV heads (default: one per query head), expanded as the model expands them.

    `extend(T)` is NOT T steps, unlike the p=2 cache: every row of L sees the statistics (Mq, Mk) of the whole sequence it was
    computed over -- the reference's own training-time behaviour -- so `extend` folds both maxima over its whole chunk before
    it reads out any row and returns rows count .. count+T-1 of L over all count+T tokens, while `step` returns the last row
    of L over the count+1 tokens seen so far.  Rows whose centred q or k is all zero divide by zero, as in the reference.
    The token count the kernels use lives in the state itself; `count` is the host's copy and nothing is ever read back."""

    def __init__(self, B, H, D, device, n_query_groups=None):
        Hkv = _kv_heads(H, n_query_groups)
        nbytes = _lib.lib().fastmax_hip_linearmax_decode_state_bytes(B, H, Hkv, D)
        super().__init__(B, H, Hkv, D, nbytes, device,
                         f"linearmax decode state: head size {D} with {H // Hkv} query heads per KV head not supported")

    def prefill(self, q, k, v):
        """L over the prompt (the matrix-core masked forward), o (B,H,N,D); the state then holds the prompt."""
        assert self.count == 0, "prefill starts a sequence"
        T = self._tokens(q, "prefill")
        self._check_shapes(q, k, v, T)
        with torch.no_grad():
            o = self._masked_forward(lambda *qkv: fastmax_hack(*qkv, p=1, mask=True), q, k, v)
        self._advance(q, k, v, T, readout=False)
        return o

    def step(self, q, k, v):
        """q (B,H,1,D), k and v (B,n_query_groups,1,D) of the new token -> o (B,H,1,D) in q's dtype: the last row of L over
        the count + 1 tokens; one launch, O(D^2) per KV head."""
        self._check_shapes(q, k, v, 1)
        return self._advance(q, k, v, 1)

    def extend(self, q, k, v):
        """T >= 1 new tokens after the `count` cached ones (any count, 0 included) -> o (B,H,T,D) in q's dtype = rows
        count .. count+T-1 of L over all count + T tokens.  T = 1 is `step`, bit for bit."""
        T = self._tokens(q, "extend")
        self._check_shapes(q, k, v, T)
        return self._advance(q, k, v, T)

    def _check_shapes(self, q, k, v, n):
        super()._check_shapes(q, k, v, n)
        if q.dtype not in ops._DT:
            raise TypeError(f"linearmax decode state takes float32, bfloat16 or float16, got {q.dtype}")

    def _advance(self, q, k, v, T, readout=True):
        """the state moves on by the T tokens; with `readout` -> their rows of L"""
        dev = self.state.device
        if dev.type != "cuda":
            ops._device()          # raises: there is no CPU path
        qd, kd, vd = self._unit_rows(q, k, v)          # k and v are cast to q's dtype
        o = torch.empty((self.B, self.H, T, self.D), dtype=q.dtype, device=dev) if readout else None
        ops._call("fastmax_hip_linearmax_decode_advance", dev,
                  (*ops._qkv(qd, kd, vd), self.state.data_ptr(), ops._ptr(o), self.B, self.H, self.Hkv, T, self.D, ops._DT[q.dtype]))
        self._count += T
        return o


def check_block_cache(attn_alg, state):
    """Which cache a ``CausalSelfAttention`` of ``attn_alg`` generates on: raises unless ``state`` is one."""
    if attn_alg == "linearmax":
        if isinstance(state, FastmaxDecodeState):
            raise NotImplementedError("a linearmax block generates on a LinearmaxDecodeState, not on a FastmaxDecodeState: its "
                                      "statistics run over the whole sequence, which the fastmax state caches do not carry")
        if not isinstance(state, LinearmaxDecodeState):
            raise TypeError(f"a linearmax block generates on a LinearmaxDecodeState, got {type(state).__name__}")
    elif isinstance(state, LinearmaxDecodeState):
        raise TypeError("a fastmax block generates on a FastmaxDecodeState(p=2), not on a LinearmaxDecodeState")
    elif isinstance(state, FastmaxKVDecodeState) and state.p != 2:
        raise ValueError(f"a fastmax block computes p=2 fastmax; the FastmaxKVDecodeState was built with p={state.p}")
