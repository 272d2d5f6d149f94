"""Host side of the fastmax operator: tensor plumbing around the C ABI (include/fastmax_hip.h).

PyTorch is used for device memory, streams and autograd bookkeeping only; all arithmetic of
the hot path runs in libfastmax_hip.so.
"""
import ctypes
import os
import math
from typing import NamedTuple

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
# float64 is the operator's alone (forward, backward, their plan and sizes): every other entry point keeps looking its dtype up
# in _DT, where a float64 tensor is a KeyError on the host and never reaches the library
_OP_DT = {**_DT, torch.float64: _lib.F64}
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
    if ok:
        return t
    if t.dtype == torch.float64 and t.shape[3] % 2:
        # the float64 kernels have no misaligned fallback: rows of an odd head size are copied to an even row stride
        B, H, N, D = t.shape
        padded = torch.empty((B, H, N, D + 1), dtype=t.dtype, device=t.device)[..., :D]
        return padded.copy_(t)
    return t.contiguous()


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


def _call(name, dev, args, ws=None, tail=()):
    """``name(*args[, workspace, its size], *tail, stream)`` on ``dev``'s current stream, with ``ws`` bytes of fresh workspace
    when a size is given.  -> the workspace tensor or None; any code but 0 raises."""
    wsb, wsargs = None, ()
    if ws is not None:
        wsb, wsp = _ws(ws, dev)
        wsargs = (wsp, ws)
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(*args, *wsargs, *tail, _stream(dev))
    _lib.check(rc, name)
    return wsb


def _problem(q, k, in_dt, out_dt, p, causal, nt, g0):
    B, H, Nq, D = q.shape
    if in_dt == torch.float64:
        # 1/nt as two floats whose double sum the kernels take (struct fastmax_problem, include/fastmax_hip.h)
        a = ctypes.c_float(1.0 / nt).value
        return _lib.Problem(B, H, Nq, k.shape[2], D, _lib.F64, _OP_DT[out_dt], int(p), int(causal), a, 1.0 / nt - a, float(g0), _force_path)
    return _lib.Problem(B, H, Nq, k.shape[2], D, _OP_DT[in_dt], _OP_DT[out_dt], int(p), int(causal), 1.0 / nt,
                        1.0 / (2.0 * nt * nt), float(g0), _force_path)


def selected_path(q, k, p, causal, nt=1.0):
    in_dt = q.dtype if q.dtype in _OP_DT else torch.float32
    out_dt = in_dt if causal or in_dt == torch.float64 else torch.float32          # dtype rule Q1; float64 stays float64
    prob = _problem(q, k, in_dt, out_dt, p, causal, nt, 0.0)
    return _lib.lib().fastmax_hip_select_path(ctypes.byref(prob))


def planned_kernels(q, k, v, p, causal, o=None, grad_o=None, nt=1.0):
    """What forward() -- and with ``grad_o`` also backward() -- would launch for these tensors (fastmax_hip_plan; nothing runs).
    -> dict(rc, path, fwd_kernel, bwd_kernel, nseg, state_bytes) with the kernels by name (``_lib.FWD_KERNELS`` /
    ``BWD_KERNELS``; None: rejected, or no backward asked for).  Tensors are taken as forward() takes them; o and the
    gradients, which forward() and backward() allocate themselves, count as aligned unless ``o`` is given."""
    dev = q.device
    in_dt = q.dtype if q.dtype in _OP_DT else torch.float32
    out_dt = o.dtype if o is not None else (in_dt if causal or in_dt == torch.float64 else torch.float32)          # dtype rule Q1
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
    """q,k,v: device tensors (B,H,N,D) of one dtype in {f32,bf16,f16,f64}; g is float32, float64 for float64 inputs (which
    take out_dtype float64 only and need 16-byte aligned rows: `_prep`). -> (o, g), or (o, g, states) with ``keep_states``:
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
    g = torch.empty((B, H, Nq), dtype=torch.float64 if q.dtype == torch.float64 else torch.float32, device=dev) if need_g else None
    wsb = _call("fastmax_hip_forward", dev, (ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr(), _ptr(g)),
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
    """linearmax prologue written in x's own dtype (training route): -> (y like x, contiguous; inv_norm (B,H) float32).
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
        _call("fastmax_hip_normalize_cast", dev, args + (N, D), ws=ws)
    else:
        _call("fastmax_hip_normalize_cast_expand", dev, args + (rep, N, D), ws=ws)
    return y, inv


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


def linearmax_train_supported(dtype, B, H, N, D) -> bool:
    """the library's host-side answer (nothing is launched, no device is needed): does the linear-time backward behind
    linearmax_forward_fused(train=True) cover this masked first-order problem?"""
    prob = _lib.Problem(B, H, N, N, D, _DT[dtype], _DT[dtype], 1, 1, 1.0, 0.5, 0.0, _force_path)
    return bool(_lib.lib().fastmax_hip_linearmax_train_supported(ctypes.byref(prob)))


def linearmax_forward_fused(q, k, v, return_stats=False, train=False):
    """Masked first-order linearmax with the prologue fused into the matrix-core kernel; which calls it covers is
    fastmax_hack.linearmax_plan's to say (a call it does not cover raises).
    ``train``: -> (o, g, inv_q, inv_k, states, k_nstar) for linearmax_backward (states = the forward's workspace when it holds
    the sequence split's prefix states, else None; nstar (2, B*H) = per head the row of q / of k that attains the max-norm)."""
    L = _lib.lib()
    dev = q.device
    B, H, N, D = q.shape
    prob = _problem(q, k, q.dtype, q.dtype, 1, True, 1.0, 0.0)
    # statistics + scan in one entry point (with the sequence split the statistics ride on the split's state pass)
    stats = torch.empty((2, B * H), dtype=torch.float32, device=dev)
    nstar = torch.full((2, B * H), -1, dtype=torch.int32, device=dev) if train else None
    o = torch.empty((B, H, N, D), dtype=q.dtype, device=dev)
    g = torch.empty((B, H, N), dtype=torch.float32, device=dev) if train else None
    nq, nk = (nstar[0].data_ptr(), nstar[1].data_ptr()) if train else (None, None)
    wsb = _call("fastmax_hip_linearmax_forward_auto", dev,
                (ctypes.byref(prob), *_qkv(q, k, v), stats[0].data_ptr(), stats[1].data_ptr(), nq, nk, o.data_ptr(), _ptr(g)),
                ws=L.fastmax_hip_linearmax_forward_auto_workspace(ctypes.byref(prob)))
    if train:
        return o, g, stats[0], stats[1], _kept_states(prob, q, k, v, o, wsb), nstar
    return (o, stats[0], stats[1]) if return_stats else o


def linearmax_backward(q, k, v, o, g, grad_o, inv_q, inv_k, states, nstar, fuse):
    """backward of linearmax_forward_fused(train=True): q, k RAW, the scans apply the prologue while staging; states, nstar: from
    that forward.  -> (dq, dk, dv).  ``fuse`` bit 1: the dQ kernel applies the prologue's backward itself and dq is the gradient
    wrt the raw q; bit 0: the dK/dV kernel does the same for dk -- without it dk is the gradient wrt the NORMALISED k (finish
    with normalize_backward)."""
    L = _lib.lib()
    dev = q.device
    prob = _problem(q, k, q.dtype, o.dtype, 1, True, 1.0, 0.0)
    dq = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dk = torch.empty(q.shape, dtype=q.dtype, device=dev)
    dv = torch.empty(v.shape, dtype=q.dtype, device=dev)
    _call("fastmax_hip_linearmax_backward", dev,
          (ctypes.byref(prob), *_qkv(q, k, v), o.data_ptr(), g.data_ptr(), *_qkv(grad_o), inv_q.data_ptr(), inv_k.data_ptr(),
           nstar[0].data_ptr(), nstar[1].data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()),
          ws=L.fastmax_hip_backward_workspace(ctypes.byref(prob)), tail=(_ptr(states), 0 if states is None else states.numel(), fuse))
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


class KVLayout(NamedTuple):
    """what the key / value heads look like to the attention that follows the QKV split (H = G * q_per_kv query heads)"""
    k: str            # "groups" (B,G,T,hs), "copies" (B,H,T,hs) written by the kernel, or "views": nothing is copied, q comes back
    v: str            # as (B*G, q_per_kv, T, hs) beside views of the G-head tensors with head stride 0, shaped the same -- (batch,
    #                   group) becomes the batch axis and the kernels' own strides do the group indexing
    fwd: int          # the split kernel's `expand`: what it materialises (0 nothing, 1 k and v, 2 v)
    bwd: int          # the gradient kernel's `expand`: what arrives per query head and is summed over its group while it is read
    #                   (1 k and v, 2 v) -- the dense gradients of views are laid out (B*G, qpk, T, hs) = (B, H, T, hs), like copies'


KV_GROUPS, KV_COPIES, K_GROUPS_V_COPIES, KV_VIEWS, K_GROUPS_V_VIEWS = range(5)
KV_LAYOUTS = {KV_GROUPS: KVLayout("groups", "groups", 0, 0),
              KV_COPIES: KVLayout("copies", "copies", 1, 1),                 # the reference's expand + reshape, model.py:404-420
              KV_VIEWS: KVLayout("views", "views", 0, 1),
              # K left at its groups for the linearmax prologue, which normalises per key head
              K_GROUPS_V_COPIES: KVLayout("groups", "copies", 2, 2), K_GROUPS_V_VIEWS: KVLayout("groups", "views", 0, 2)}


class RopeQKVSplit(torch.autograd.Function):
    """qkv (B,T,G,q_per_kv+2,hs) -> q (B,H,T,hs), k, v (B,H,T,hs): de-interleave + RoPE + GQA expand in one HIP pass
    (fastmax_rope.hip; lit_gpt/model.py:397-425), and the mirror pass for the gradient."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, rope_n_elem, expand=KV_COPIES):
        """expand: one of the KV_LAYOUTS above"""
        layout = KV_LAYOUTS[int(expand)]
        B, T, G, total, hs = qkv.shape
        qpk = total - 2
        qkv = qkv.contiguous()
        # a rope cache kept in the tensors' own 16-bit dtype ("bf16-true"): model.py:708 then rounds each product to that
        # dtype before the sum -- the kernel reproduces those roundings (tables travel as exact float32 copies)
        tables16 = 16 if (cos.dtype == qkv.dtype and qkv.dtype in (torch.bfloat16, torch.float16)) else 0
        cos, sin = _rope_tables_f32(cos, sin, T, rope_n_elem)
        q = torch.empty((B, G * qpk, T, hs), dtype=qkv.dtype, device=qkv.device)
        k = torch.empty((B, G * qpk if layout.k == "copies" else G, T, hs), dtype=qkv.dtype, device=qkv.device)
        v = torch.empty((B, G * qpk if layout.v == "copies" else G, T, hs), dtype=qkv.dtype, device=qkv.device)
        _call("fastmax_hip_rope_qkv_split", qkv.device,
              (qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), B, T, G, qpk, hs, rope_n_elem,
               layout.fwd | tables16, _DT[qkv.dtype]))
        ctx.save_for_backward(cos, sin)
        ctx.dims = (B, T, G, qpk, hs, rope_n_elem, layout.bwd)
        return group_views(q, k, v, layout)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        cos, sin = ctx.saved_tensors
        return rope_qkv_backward(gq, gk, gv, cos, sin, *ctx.dims), None, None, None, None


def group_views(q, k, v, layout):
    """q (B,H,T,hs), k, v (B,G,T,hs) as ``layout`` hands them on: with "views", q as (B*G, qpk, T, hs) beside stride-0 views"""
    if layout.v != "views":
        return q, k, v
    (B, G, T, hs), qpk = v.shape, q.shape[1] // v.shape[1]

    def view(t):
        return t.view(B * G, 1, T, hs).expand(B * G, qpk, T, hs)
    return q.view(B * G, qpk, T, hs), (view(k) if layout.k == "views" else k), view(v)
