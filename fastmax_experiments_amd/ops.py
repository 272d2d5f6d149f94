"""Host side of the fastmax operator: tensor plumbing around the C ABI (include/fastmax_hip.h).

PyTorch is used for device memory, streams and autograd bookkeeping only; all arithmetic of
the hot path runs in libfastmax_hip.so.
"""
import ctypes
import os
import math

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_force_path = _lib.PATH_AUTO


def set_forced_path(path):
    """Testing / benchmarking hook: force a kernel family (``_lib.PATH_*``); AUTO restores dispatch."""
    global _force_path
    _force_path = int(path)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("fastmax needs an MI355X (HIP device); there is no CPU fallback for this operator")
    return torch.device("cuda", torch.cuda.current_device())


def _prep(t, dev):
    """-> tensor on the HIP device with unit stride in D and 16-byte aligned rows."""
    if t.device.type != "cuda":
        t = t.to(dev, non_blocking=False)
    es = t.element_size()
    ok = t.stride(3) == 1 and all((s * es) % 16 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _strides(t):
    return (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ws(nbytes, dev):
    if nbytes == 0:
        return None, ctypes.c_void_p(0)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf, ctypes.c_void_p(buf.data_ptr())


def _qkv(*tensors):
    """(address, strides) of each tensor, flat: the way the C ABI takes q, k, v and grad_o"""
    return tuple(a for t in tensors for a in (t.data_ptr(), _strides(t)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(name, dev, args, ws=None, tail=(), not_covered=()):
    """``name(*args[, workspace, its size], *tail, stream)`` on ``dev``'s current stream, with ``ws`` bytes of fresh workspace
    when a size is given.  -> (True, the workspace tensor or None), or (False, None) when the library answers with one of the
    codes in ``not_covered``; any other code but 0 raises."""
    wsb, wsargs = None, ()
    if ws is not None:
        wsb, wsp = _ws(ws, dev)
        wsargs = (wsp, ws)
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(*args, *wsargs, *tail, _stream(dev))
    if rc in not_covered:
        return False, None
    _lib.check(rc, name)
    return True, wsb


def _problem(q, k, in_dt, out_dt, p, causal, nt, g0):
    B, H, Nq, D = q.shape
    return _lib.Problem(B, H, Nq, k.shape[2], D, _DT[in_dt], _DT[out_dt], int(p), int(causal), 1.0 / nt,
                        1.0 / (2.0 * nt * nt), float(g0), _force_path)


def selected_path(q, k, p, causal, nt=1.0):
    in_dt = q.dtype if q.dtype in _DT else torch.float32
    out_dt = in_dt if causal else torch.float32          # dtype rule Q1
    prob = _problem(q, k, in_dt, out_dt, p, causal, nt, 0.0)
    return _lib.lib().fastmax_hip_select_path(ctypes.byref(prob))


def planned_kernels(q, k, v, p, causal, o=None, grad_o=None, nt=1.0):
    """What forward() -- and with ``grad_o`` also backward() -- would launch for these tensors (fastmax_hip_plan; nothing runs).
    -> dict(rc, path, fwd_kernel, bwd_kernel, nseg, state_bytes) with the kernels by name (``_lib.FWD_KERNELS`` /
    ``BWD_KERNELS``; None: rejected, or no backward asked for).  Tensors are taken as forward() takes them; o and the
    gradients, which forward() and backward() allocate themselves, count as aligned unless ``o`` is given."""
    dev = q.device
    in_dt = q.dtype if q.dtype in _DT else torch.float32
    out_dt = o.dtype if o is not None else (in_dt if causal else torch.float32)          # dtype rule Q1
    q, k, v = (_prep(t, dev) for t in (q, k, v))
    prob = _problem(q, k, in_dt, out_dt, p, causal, nt, float(q.shape[2]))
    fresh = 256          # stands for a fresh allocation: only the alignment of an address is looked at
    bwd = (None,) * 5 if grad_o is None else (*_qkv(_prep(grad_o, dev)), fresh, fresh, fresh)
    plan = _lib.Plan()
    _lib.lib().fastmax_hip_plan(ctypes.byref(prob), *_qkv(q, k, v), fresh if o is None else o.data_ptr(), *bwd, ctypes.byref(plan))

    def name(names, i):
        return names[i] if i >= 0 else None

    return dict(rc=plan.rc, path=plan.path, fwd_kernel=name(_lib.FWD_KERNELS, plan.fwd_kernel),
                bwd_kernel=name(_lib.BWD_KERNELS, plan.bwd_kernel), nseg=plan.nseg, state_bytes=plan.state_bytes)


KEEP_STATES = os.environ.get("FASTMAX_KEEP_STATES", "1") != "0"


MAX_HEAD_SIZE = 256      # FASTMAX_MAX_D (include/fastmax_hip.h): the largest head size in lit_gpt/config.py (pythia-1b, Gemma-2b)


def forward(q, k, v, p, causal, nt, g0, out_dtype, need_g=True, keep_states=False):
    """q,k,v: device tensors (B,H,N,D) of one dtype in {f32,bf16,f16}. -> (o, g), or (o, g, states) with ``keep_states``:
    the sequence-split prefix states the p=1 masked forward left in its workspace (None when this call has none), for
    ``backward(..., states=...)``"""
    L = _lib.lib()
    if p not in (1, 2):
        raise ValueError(f"p should be 1 or 2, got p={p}")
    dev = q.device
    B, H, Nq, D = q.shape
    if D > MAX_HEAD_SIZE:
        raise NotImplementedError(f"head size {D} > {MAX_HEAD_SIZE} is not supported by the HIP kernels")
    prob = _problem(q, k, q.dtype, out_dtype, p, causal, nt, g0)
    o = torch.empty((B, H, Nq, D), dtype=out_dtype, device=dev)
    g = torch.empty((B, H, Nq), dtype=torch.float32, device=dev) if need_g else None
    _, wsb = _call("fastmax_hip_forward", dev, (ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr(), _ptr(g)),
                   ws=L.fastmax_hip_forward_workspace(ctypes.byref(prob)))
    return (o, g, _kept_states(prob, q, k, v, o, wsb)) if keep_states else (o, g)


def _kept_states(prob, q, k, v, o, wsb):
    """the forward's workspace when it holds the sequence split's prefix states for this call, else None"""
    if not KEEP_STATES or wsb is None:
        return None
    nb = _lib.lib().fastmax_hip_forward_state_bytes(ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr())
    return wsb if 0 < nb <= wsb.numel() else None


def backward(q, k, v, o, g, grad_o, p, causal, nt, states=None):
    L = _lib.lib()
    dev = q.device
    prob = _problem(q, k, q.dtype, o.dtype, p, causal, nt, 0.0)
    dq = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dk = torch.empty(k.shape, dtype=q.dtype, device=dev)
    dv = torch.empty(v.shape, dtype=q.dtype, device=dev)
    _call("fastmax_hip_backward_with_states", dev,
          (ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr(), g.data_ptr(), *_qkv(grad_o), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()),
          ws=L.fastmax_hip_backward_workspace(ctypes.byref(prob)), tail=(_ptr(states), 0 if states is None else states.numel()))
    return dq, dk, dv


def normalize(x):
    """linearmax prologue on the device. x: (B,H,N,D) -> (y float32 contiguous, inv_norm (B,H) float32)."""
    L = _lib.lib()
    dev = x.device
    B, H, N, D = x.shape
    if D > MAX_HEAD_SIZE:
        raise NotImplementedError(f"head size {D} > {MAX_HEAD_SIZE} is not supported by the HIP kernels")
    y = torch.empty((B, H, N, D), dtype=torch.float32, device=dev)
    inv = torch.empty((B, H), dtype=torch.float32, device=dev)
    _call("fastmax_hip_normalize", dev, (*_qkv(x), _DT[x.dtype], y.data_ptr(), inv.data_ptr(), B, H, N, D),
          ws=L.fastmax_hip_normalize_workspace(B, H))
    return y, inv


def normalize_cast(x, rep=1):
    """linearmax prologue written in x's own dtype (training route): -> (y like x, contiguous; inv_norm (B,H) float32),
    or None when the head size is not a whole number of 16-byte pieces (caller falls back to normalize()).
    rep > 1 (grouped-query attention): x holds the G key heads, y the G * rep query-head copies (B, G * rep, N, D)."""
    L = _lib.lib()
    dev = x.device
    B, H, N, D = x.shape
    y = torch.empty((B, H * rep, N, D), dtype=x.dtype, device=dev)
    inv = torch.empty((B, H), dtype=torch.float32, device=dev)
    # room for one word per 256-token block of every head: the two-launch form (see include/fastmax_hip.h)
    ws = max(L.fastmax_hip_normalize_workspace(B, H), 4 * B * H * ((N + 255) // 256))
    args = (*_qkv(x), _DT[x.dtype], y.data_ptr(), inv.data_ptr(), B, H)
    if rep == 1:
        ok, _ = _call("fastmax_hip_normalize_cast", dev, args + (N, D), ws=ws, not_covered=(_lib.E_BAD_SHAPE,))
    else:
        ok, _ = _call("fastmax_hip_normalize_cast_expand", dev, args + (rep, N, D), ws=ws, not_covered=(_lib.E_BAD_SHAPE,))
    return (y, inv) if ok else None


def normalize_backward(x, gy, inv, rep=1):
    """gradient of normalize_cast wrt x; gy like y (made contiguous), inv from the forward."""
    L = _lib.lib()
    dev = x.device
    B, H, N, D = x.shape
    gy = gy.to(x.dtype).contiguous()
    gx = torch.empty((B, H, N, D), dtype=x.dtype, device=dev)
    ws = L.fastmax_hip_normalize_backward_workspace(B, H * rep, N)
    args = (*_qkv(x), _DT[x.dtype], gy.data_ptr(), inv.data_ptr(), gx.data_ptr(), B, H)
    if rep == 1:
        _call("fastmax_hip_normalize_backward", dev, args + (N, D), ws=ws)
    else:
        _call("fastmax_hip_normalize_backward_expand", dev, args + (rep, N, D), ws=ws)
    return gx


def normalize_stats(x):
    """1 / max_n ||x_n - mean_D x_n|| per (b,h) -- the only global quantity of the linearmax prologue."""
    L = _lib.lib()
    dev = x.device
    B, H, N, D = x.shape
    inv = torch.empty((B, H), dtype=torch.float32, device=dev)
    _call("fastmax_hip_normalize_stats", dev, (*_qkv(x), _DT[x.dtype], inv.data_ptr(), B, H, N, D), ws=L.fastmax_hip_normalize_workspace(B, H))
    return inv


def normalize_stats_pair(q, k):
    """normalize_stats of q and of k in two launches in all (per-block maxima of both tensors, one fold)"""
    if q.shape != k.shape or q.dtype != k.dtype or q.device != k.device or q.shape[0] * q.shape[1] > 65535:
        return normalize_stats(q), normalize_stats(k)
    L = _lib.lib()
    dev = q.device
    B, H, N, D = q.shape
    qi = torch.empty((B, H), dtype=torch.float32, device=dev)
    ki = torch.empty((B, H), dtype=torch.float32, device=dev)
    _call("fastmax_hip_normalize_stats2", dev, (*_qkv(q, k), _DT[q.dtype], qi.data_ptr(), ki.data_ptr(), B, H, N, D),
          ws=L.fastmax_hip_normalize_stats2_workspace(B, H, N))
    return qi, ki


def linearmax_forward_fused(q, k, v, return_stats=False, train=False):
    """Masked first-order linearmax with the prologue fused into the matrix-core kernel.
    Returns None when the shape / dtype is not covered (the caller then uses the unfused route).
    ``train``: -> (o, g, inv_q, inv_k, states, k_nstar) for linearmax_backward (states = the forward's workspace when it holds
    the sequence split's prefix states, else None; nstar (2, B*H) = per head the row of q / of k that attains the max-norm)."""
    L = _lib.lib()
    dev = q.device
    B, H, N, D = q.shape
    if q.dtype not in _DT or D > 128:
        return None
    prob = _problem(q, k, q.dtype, q.dtype, 1, True, 1.0, 0.0)
    if B * H > 65535:
        return None
    if train and not L.fastmax_hip_linearmax_train_supported(ctypes.byref(prob)):
        return None
    # statistics + scan in one entry point (with the sequence split the statistics ride on the split's state pass)
    stats = torch.empty((2, B * H), dtype=torch.float32, device=dev)
    nstar = torch.full((2, B * H), -1, dtype=torch.int32, device=dev) if train else None
    o = torch.empty((B, H, N, D), dtype=q.dtype, device=dev)
    g = torch.empty((B, H, N), dtype=torch.float32, device=dev) if train else None
    nq, nk = (nstar[0].data_ptr(), nstar[1].data_ptr()) if train else (None, None)
    ok, wsb = _call("fastmax_hip_linearmax_forward_auto", dev,
                    (ctypes.byref(prob), *_qkv(q, k, v), stats[0].data_ptr(), stats[1].data_ptr(), nq, nk, o.data_ptr(), _ptr(g)),
                    ws=L.fastmax_hip_linearmax_forward_auto_workspace(ctypes.byref(prob)),
                    not_covered=(_lib.E_BAD_SHAPE, _lib.E_ALIGNMENT))          # not covered by the fused kernel
    if not ok:
        return None
    if train:
        return o, g, stats[0], stats[1], _kept_states(prob, q, k, v, o, wsb), nstar
    return (o, stats[0], stats[1]) if return_stats else o


def linearmax_backward(q, k, v, o, g, grad_o, inv_q, inv_k, states=None, nstar=None, fuse=0):
    """backward of linearmax_forward_fused(train=True): q, k RAW, the scans apply the prologue while staging.
    -> (dq_n, dk_n, dv): gradients wrt the NORMALISED q, k (finish with normalize_backward) and wrt v.  With ``nstar`` (from
    the forward) and ``fuse`` bit 0 the dK/dV kernel applies the prologue's backward itself and dk_n is the gradient wrt the raw
    k; bit 1 (with bit 0): the dQ kernel does the same for dq_n."""
    L = _lib.lib()
    dev = q.device
    prob = _problem(q, k, q.dtype, o.dtype, 1, True, 1.0, 0.0)
    dq = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dk = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dv = torch.empty(v.shape, dtype=q.dtype, device=dev)
    nq, nk = (None, None) if nstar is None else (nstar[0].data_ptr(), nstar[1].data_ptr())
    _call("fastmax_hip_linearmax_backward", dev,
          (ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr(), g.data_ptr(), *_qkv(grad_o), inv_q.data_ptr(), inv_k.data_ptr(), nq, nk,
           dq.data_ptr(), dk.data_ptr(), dv.data_ptr()),
          ws=L.fastmax_hip_backward_workspace(ctypes.byref(prob)),
          tail=(_ptr(states), 0 if states is None else states.numel(), 0 if nstar is None else fuse))
    return dq, dk, dv


def effective_normalize_term(D, normalize_term, tensors_normalized):
    # attention_mechanisms/fastmax.py:78-82
    return 1.0 if tensors_normalized is True else normalize_term * math.sqrt(D)


def rope_qkv_supported(dtype, head_size, rope_n_elem):
    e = 4 if dtype == torch.float32 else 8
    return dtype in _DT and rope_n_elem % 2 == 0 and (rope_n_elem // 2) % e == 0 and (head_size - rope_n_elem) % e == 0


def build_rope_cache(seq_len: int, n_elem: int, device=None, base: int = 10000, condense_ratio: int = 1):
    """cos / sin tables of lit_gpt/model.py:676-699 (public RoPE formula)."""
    theta = 1.0 / (base ** (torch.arange(0, n_elem, 2, device=device).float() / n_elem))
    seq_idx = torch.arange(seq_len, device=device) / condense_ratio
    idx_theta = torch.outer(seq_idx, theta).repeat(1, 2)
    return torch.cos(idx_theta), torch.sin(idx_theta)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    half = x.size(-1) // 2
    rotated = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return ((x * cos) + (rotated * sin)).to(dtype=x.dtype)


def eager_rope_qkv_split(qkv, cos, sin, n):
    """tensor slicing + apply_rope (model.py:397-425, without the GQA expand): qkv (B,T,G,q_per_kv+2,hs) -- slots
    0..q_per_kv-1 of a group are its query heads, then its key head, then its value head -> q (B,H,T,hs) and k rotated on
    their first n dims, k and v (B,G,T,hs) at their G heads"""
    B, T, G, total, hs = qkv.shape
    qpk = total - 2
    q = qkv[:, :, :, :qpk].permute(0, 2, 3, 1, 4).reshape(B, G * qpk, T, hs)
    k, v = (qkv[:, :, :, qpk + i].permute(0, 2, 1, 3) for i in (0, 1))
    cos, sin = cos[:, :n], sin[:, :n]
    q = torch.cat((apply_rope(q[..., :n], cos, sin), q[..., n:]), dim=-1)
    k = torch.cat((apply_rope(k[..., :n], cos, sin), k[..., n:]), dim=-1)
    return q, k, v


def rope_qkv_split(qkv, cos, sin, n):
    """qkv (B,T,G,q_per_kv+2,hs) -> rotated q (B,H,T,hs), rotated k and v (B,G,T,hs): K and V stay at their G heads.
    One HIP pass where the split kernel takes the shape, else `eager_rope_qkv_split`."""
    if qkv.is_cuda and rope_qkv_supported(qkv.dtype, qkv.shape[4], n):
        return RopeQKVSplit.apply(qkv, cos, sin, n, 0)
    return eager_rope_qkv_split(qkv, cos, sin, n)


_ROPE_F32 = {}


def _rope_tables_f32(cos, sin, T, n_elem):
    """the kernel's exact float32 copies of the first T rows of the rope cache; every layer of a step asks for the same
    tables, so the last conversion is kept (keyed by storage, version and shape of the cache tensors)"""
    if cos.is_cuda and torch.cuda.is_current_stream_capturing():
        # a recorded HIP graph keeps reading these tables on every replay: allocate them inside the capture, so that they
        # live in the graph's own memory pool (an entry of the one-slot cache below is freed by the next eager call with
        # another sequence length, rope cache or model)
        return cos[:T, :n_elem].float().contiguous(), sin[:T, :n_elem].float().contiguous()
    key = (cos.data_ptr(), sin.data_ptr(), cos._version, sin._version, tuple(cos.shape), cos.dtype, str(cos.device), T, n_elem)
    hit = _ROPE_F32.get("last")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    c = cos[:T, :n_elem].float().contiguous()
    s_ = sin[:T, :n_elem].float().contiguous()
    _ROPE_F32["last"] = (key, c, s_, cos, sin)          # the cache tensors are held so that their addresses cannot be reused
    return c, s_


def rope_qkv_backward(gq, gk, gv, cos32, sin32, B, T, G, qpk, hs, rope_n, kern_expand):
    """gradient of the QKV split + RoPE pass: (B,T,G,qpk+2,hs) from the gradients of q, k, v (inverse rotation, re-interleave;
    kern_expand 1 / 2: k, v (or v) arrive per query head and are summed over their group while they are read)"""
    gq, gk, gv = gq.contiguous(), gk.contiguous(), gv.contiguous()
    gqkv = torch.empty((B, T, G, qpk + 2, hs), dtype=gq.dtype, device=gq.device)
    _call("fastmax_hip_rope_qkv_split_backward", gq.device,
          (gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), cos32.data_ptr(), sin32.data_ptr(), gqkv.data_ptr(), B, T, G, qpk, hs, rope_n,
           kern_expand, _DT[gq.dtype]))
    return gqkv


class RopeQKVSplit(torch.autograd.Function):
    """qkv (B,T,G,q_per_kv+2,hs) -> q (B,H,T,hs), k, v (B,H,T,hs): de-interleave + RoPE + GQA expand in one HIP pass
    (fastmax_rope.hip; lit_gpt/model.py:397-425), and the mirror pass for the gradient."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, rope_n_elem, expand=1):
        """expand: what the key / value heads look like to the attention that follows (H = G * q_per_kv query heads):
          0  k, v stay at their G heads (B,G,T,hs)
          1  k, v COPIED for the query heads of their group (B,H,T,hs) -- the reference's expand + reshape, model.py:404-420
          2  k stays (B,G,T,hs), v copied
          3  nothing is copied: q comes back as (B*G, q_per_kv, T, hs) and k, v as views of the G-head tensors with head
             stride 0, shaped the same -- (batch, group) becomes the batch axis and the kernels' own strides do the
             group indexing, so every query head of a group reads the same K, V rows; the gradients then arrive per
             query head and the backward pass sums them over the group while it reads them
          4  k stays (B,G,T,hs) (for the linearmax prologue, which normalises per key head), q and v as in 3"""
        B, T, G, total, hs = qkv.shape
        qpk = total - 2
        qkv = qkv.contiguous()
        # a rope cache kept in the tensors' own 16-bit dtype ("bf16-true"): model.py:708 then rounds each product to that
        # dtype before the sum -- the kernel reproduces those roundings (tables travel as exact float32 copies)
        tables16 = 16 if (cos.dtype == qkv.dtype and qkv.dtype in (torch.bfloat16, torch.float16)) else 0
        cos, sin = _rope_tables_f32(cos, sin, T, rope_n_elem)
        k_copies, v_copies = expand == 1, expand in (1, 2)
        kern_expand = 1 if (k_copies and v_copies) else (2 if v_copies else 0)          # what the forward pass materialises
        q = torch.empty((B, G * qpk, T, hs), dtype=qkv.dtype, device=qkv.device)
        k = torch.empty((B, G * qpk if k_copies else G, T, hs), dtype=qkv.dtype, device=qkv.device)
        v = torch.empty((B, G * qpk if v_copies else G, T, hs), dtype=qkv.dtype, device=qkv.device)
        _call("fastmax_hip_rope_qkv_split", qkv.device,
              (qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), B, T, G, qpk, hs, rope_n_elem,
               kern_expand | tables16, _DT[qkv.dtype]))
        ctx.save_for_backward(cos, sin)
        ctx.dims = (B, T, G, qpk, hs, rope_n_elem, int(expand))
        if expand in (3, 4):
            def group_view(t):
                return t.view(B * G, 1, T, hs).expand(B * G, qpk, T, hs)
            return q.view(B * G, qpk, T, hs), (group_view(k) if expand == 3 else k), group_view(v)
        return q, k, v

    @staticmethod
    def backward(ctx, gq, gk, gv):
        cos, sin = ctx.saved_tensors
        B, T, G, qpk, hs, rope_n_elem, expand = ctx.dims
        # modes 3 / 4: gradients of the stride-0 views arrive dense, one per query head, laid out (B*G, qpk, T, hs) =
        # (B, H, T, hs): exactly what the kernel's group-summing read expects for copied heads
        kern_expand = {0: 0, 1: 1, 2: 2, 3: 1, 4: 2}[expand]
        gqkv = rope_qkv_backward(gq, gk, gv, cos, sin, B, T, G, qpk, hs, rope_n_elem, kern_expand)
        return gqkv, None, None, None, None
