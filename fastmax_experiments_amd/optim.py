"""AdamW over the flat LoRA-gradient bucket (`dp.FlatGradBucket`) in hand-written HIP: include/fastmax_hip_optim.h,
csrc/flat_adamw.hip.

The accumulation boundary of a fine-tune step -- divide by the world size, clip by the global norm, decoupled weight decay, both
moments, bias correction, the update, the parameter written in its own dtype, the gradient zeroed -- is one pass over the flat
buffers (two with the norm), in place of the chain `flat.div_`, `clip_grad_norm_`, `torch.optim.AdamW.step()`, `bucket.zero()`.
The step count, the norm and the clip coefficient stay on the device and the launch arguments never change, so a step whose lr
comes from a device tensor can be recorded in a HIP graph.  16-bit parameters ("bf16-true" training) are updated through float32
master weights: an update below one bf16 ulp of the weight is not lost.

On a CPU bucket `step` runs the same formulas as tensor ops over the flat buffers: a rehearsal of the control flow (gloo tests,
`finetune_step.ToyLoRA`), not a second implementation of the hot path -- on a HIP device there is no path but the kernels.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _DT, _call, _ptr

SEGMENT_RECORD = np.dtype([("param", "<u8"), ("offset", "<i8"), ("numel", "<i8"), ("dtype", "<i4"), ("pad", "<i4")])
CHUNK_RECORD = np.dtype([("start", "<i8"), ("segment", "<i4"), ("len", "<i4")])
RECORD_BYTES = 64                     # the scalar record at the head of the workspace (fastmax_hip_optim.h)
_NORM, _COEF = 0, 1                   # float32 words of the record
_FINITE = 2                           # int32 word
_STEP, _SKIPPED = 2, 3                # int64 words


def chunk_elems() -> int:
    """elements per workgroup of the update pass (a host-only query of the library)"""
    return int(_lib.lib().fastmax_hip_adamw_chunk())


def chunk_table(numels: Sequence[int], chunk: int) -> np.ndarray:
    """The chunk records for parameters of `numels` elements packed one after the other: every segment cut into pieces of
    `chunk` elements and a remainder; a chunk never crosses a segment boundary and every flat index is covered exactly once."""
    if chunk <= 0:
        raise ValueError(f"chunk should be positive, got {chunk}")
    parts, off = [], 0
    for s, numel in enumerate(numels):
        if numel <= 0:
            raise ValueError(f"segment {s} has {numel} elements")
        starts = np.arange(0, numel, chunk, dtype=np.int64)
        rec = np.zeros(len(starts), dtype=CHUNK_RECORD)
        rec["start"] = off + starts
        rec["segment"] = s
        rec["len"] = np.minimum(chunk, numel - starts)
        parts.append(rec)
        off += numel
    return np.concatenate(parts)


def segment_table(ptrs: Sequence[int], numels: Sequence[int], dtypes: Sequence[int]) -> np.ndarray:
    rec = np.zeros(len(numels), dtype=SEGMENT_RECORD)
    rec["param"] = np.asarray(ptrs, dtype=np.uint64)
    rec["numel"] = np.asarray(numels, dtype=np.int64)
    rec["offset"] = np.cumsum(rec["numel"]) - rec["numel"]
    rec["dtype"] = np.asarray(dtypes, dtype=np.int32)
    return rec


class FlatAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` (amsgrad=False, maximize=False) over `bucket.params`, reading the gradient from `bucket.flat`.

    One param group, so a `LambdaLR` drives `param_groups[0]["lr"]`.  Owns flat float32 `m`, `v`, `master` (the float32 weights
    behind the 16-bit parameters; a float32 parameter is its own master), the device record (step and skipped counters, norm,
    clip coefficient) and the segment and chunk tables, built and uploaded once."""

    def __init__(self, bucket, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, skip_nonfinite: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"lr should not be negative, got {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas should lie in [0, 1), got {betas}")
        if eps < 0.0 or weight_decay < 0.0:
            raise ValueError(f"eps and weight_decay should not be negative, got {eps}, {weight_decay}")
        params: List[torch.nn.Parameter] = list(bucket.params)
        for i, p in enumerate(params):
            if not p.is_contiguous():
                raise ValueError(f"FlatAdamW needs contiguous parameters: parameter {i} of shape {tuple(p.shape)} is not")
            if p.dtype not in _DT:
                raise ValueError(f"FlatAdamW takes float32, bfloat16 and float16 parameters, got {p.dtype}")
            if p.device != bucket.flat.device:
                raise ValueError("FlatAdamW needs every parameter on the bucket's device")
        if bucket.flat.dtype not in _DT:
            raise ValueError(f"FlatAdamW takes a float32, bfloat16 or float16 bucket, got {bucket.flat.dtype}")
        self.bucket = bucket
        self.skip_nonfinite = bool(skip_nonfinite)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        dev = bucket.flat.device
        self._on_device = dev.type == "cuda"
        n = bucket.flat.numel()
        self._numels = [p.numel() for p in params]
        self._offsets = [int(o) for o in np.cumsum([0] + self._numels[:-1])]
        self._lowp = [p.dtype != torch.float32 for p in params]
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.master = torch.zeros(n, dtype=torch.float32, device=dev) if any(self._lowp) else None
        if self._on_device:
            L = _lib.lib()
            self._chunk = chunk_elems()
            self._ws_bytes = int(L.fastmax_hip_adamw_workspace(n))
            self._ptrs = tuple(p.data_ptr() for p in params)
            segs = segment_table(self._ptrs, self._numels, [_DT[p.dtype] for p in params])
            chunks = chunk_table(self._numels, self._chunk)
            self._n_chunks = len(chunks)
            self._segments = torch.from_numpy(segs.view(np.uint8).copy()).to(dev)
            self._chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        else:
            self._ws_bytes = RECORD_BYTES
        self._ws = torch.zeros(self._ws_bytes, dtype=torch.uint8, device=dev)          # zeroed once: counters, ticket
        self._rec_f32 = self._ws[:RECORD_BYTES].view(torch.float32)
        self._rec_i32 = self._ws[:RECORD_BYTES].view(torch.int32)
        self._rec_i64 = self._ws[:RECORD_BYTES].view(torch.int64)
        self.refresh_master()

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("FlatAdamW has one param group: the flat bucket is one range with one set of hyper-parameters")
        super().add_param_group(param_group)

    def _segments_of(self, flat: torch.Tensor):
        return [flat[o:o + k] for o, k in zip(self._offsets, self._numels)]

    @torch.no_grad()
    def refresh_master(self):
        """Re-read the 16-bit parameters into `master` (after loading a checkpoint into the model)."""
        if self.master is None:
            return
        for p, low, w in zip(self.bucket.params, self._lowp, self._segments_of(self.master)):
            if low:
                w.copy_(p.detach().reshape(-1))

    def zero_grad(self, set_to_none: bool = True):
        """the bucket's zero(): the `.grad` views stay aliased"""
        self.bucket.zero()

    # ---- counters: device reads that synchronise, for logging only ----------------------------------------------------------
    def step_count(self) -> int:
        return int(self._rec_i64[_STEP].item())

    def skipped(self) -> int:
        return int(self._rec_i64[_SKIPPED].item())

    def last_norm(self) -> float:
        """the gradient norm of the last step that computed it (max_norm given or skip_nonfinite on)"""
        return float(self._rec_f32[_NORM].item())

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self):
        g = self.param_groups[0]
        return {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                "master": None if self.master is None else self.master.detach().cpu().clone(),
                "step": self.step_count(), "skipped": self.skipped(),
                "param_groups": [{k: v for k, v in g.items() if k != "params"}]}

    @torch.no_grad()
    def load_state_dict(self, state):
        if state["m"].numel() != self.m.numel() or (state["master"] is None) != (self.master is None):
            raise ValueError("FlatAdamW.load_state_dict: the state belongs to another bucket layout")
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        if self.master is not None:
            self.master.copy_(state["master"])
            for p, low, w in zip(self.bucket.params, self._lowp, self._segments_of(self.master)):
                if low:
                    p.copy_(w.view_as(p))            # the 16-bit parameter is the rounded master, as after every step
        self._rec_i64[_STEP] = int(state["step"])
        self._rec_i64[_SKIPPED] = int(state["skipped"])
        self.param_groups[0].update(state["param_groups"][0])

    # ---- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, max_norm: Optional[float] = None, zero_grad: bool = True,
             lr: Optional[torch.Tensor] = None, closure=None):
        """One AdamW update from `bucket.flat` times `grad_scale` (1 / world after a SUM all-reduce), clipped to `max_norm` by
        the global norm when given; `zero_grad` zeroes the bucket in the same pass.  `lr`: None takes the group's lr by value; a
        0-dim float32 tensor on the bucket's device is read by the kernels, and the call can then be recorded in a graph."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        if lr is not None and (not isinstance(lr, torch.Tensor) or lr.numel() != 1 or lr.dtype != torch.float32 or
                               lr.device != self.bucket.flat.device):
            raise ValueError("lr should be None or a one-element float32 tensor on the bucket's device")
        if self._on_device:
            self._step_device(group, float(grad_scale), max_norm, bool(zero_grad), lr)
        else:
            self._step_rehearsal(group, float(grad_scale), max_norm, bool(zero_grad), lr)
        return loss

    def _step_device(self, group, grad_scale, max_norm, zero_grad, lr):
        params = self.bucket.params
        if tuple(p.data_ptr() for p in params) != self._ptrs:
            raise RuntimeError("a parameter's storage moved since FlatAdamW was built (model.to(...), a re-assigned .data): "
                               "the segment table holds its old address; build the optimizer after the model is in place")
        flat = self.bucket.flat
        dev = flat.device
        b1, b2 = (float(b) for b in group["betas"])
        clip = max_norm is not None
        ws = (self._ws.data_ptr(), self._ws_bytes)          # the optimizer's own: the record at its head lives across steps
        if clip or self.skip_nonfinite:
            _call("fastmax_hip_adamw_norm", dev, (flat.data_ptr(), _DT[flat.dtype], flat.numel(), grad_scale, *ws))
        _call("fastmax_hip_adamw_update", dev,
              (flat.data_ptr(), _DT[flat.dtype], flat.numel(), self.m.data_ptr(), self.v.data_ptr(), _ptr(self.master),
               sum(self._lowp), self._segments.data_ptr(), len(params), self._chunks.data_ptr(), self._n_chunks,
               float(group["lr"]), _ptr(lr), b1, b2, 1.0 - b1, 1.0 - b2, float(group["eps"]), float(group["weight_decay"]),
               grad_scale, float(max_norm) if clip else 0.0, int(clip), int(self.skip_nonfinite), int(zero_grad), *ws))

    def _step_rehearsal(self, group, grad_scale, max_norm, zero_grad, lr):
        """the kernels' formulas as float32 tensor ops over the flat buffers (CPU bucket only)"""
        flat = self.bucket.flat
        b1, b2 = (float(b) for b in group["betas"])
        lr_now = float(group["lr"]) if lr is None else float(lr)
        g = flat.float() * grad_scale
        coef, finite = 1.0, True
        if max_norm is not None or self.skip_nonfinite:
            norm = float(torch.sqrt((g * g).sum()))
            finite = math.isfinite(norm)
            if max_norm is not None:
                c = float(max_norm) / (norm + 1e-6)
                coef = 1.0 if c > 1.0 else c
            self._rec_f32[_NORM], self._rec_f32[_COEF], self._rec_i32[_FINITE] = norm, coef, int(finite)
        if self.skip_nonfinite and not finite:
            self._rec_i64[_SKIPPED] += 1
        else:
            t = self.step_count() + 1
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            g = g * coef
            self.m.mul_(b1).add_(g, alpha=1.0 - b1)
            self.v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            update = (self.m / (self.v.sqrt() / math.sqrt(bc2) + float(group["eps"]))) * (lr_now / bc1)
            decay = 1.0 - lr_now * float(group["weight_decay"])
            masters = self._segments_of(self.master) if self.master is not None else [None] * len(self._numels)
            for p, low, w, u in zip(self.bucket.params, self._lowp, masters, self._segments_of(update)):
                if low:
                    w.mul_(decay).sub_(u)
                    p.copy_(w.view_as(p))
                else:
                    p.mul_(decay).sub_(u.view_as(p))
            self._rec_i64[_STEP] = t
        if zero_grad:
            flat.zero_()

    # ---- what the tests ask about the launch ------------------------------------------------------------------------------------
    def route_counts(self) -> Tuple[int, int]:
        """(chunks that move as 4-element pieces, chunks that move element by element): the rule of fastmax_hip_optim.h applied
        to this optimizer's tables on the host"""
        if not self._on_device:
            raise RuntimeError("route_counts describes the device launch; this FlatAdamW runs the CPU rehearsal")
        gsize = self.bucket.flat.element_size()
        gptr = self.bucket.flat.data_ptr()
        vec = 0
        chunks = chunk_table(self._numels, self._chunk)
        psize = [p.element_size() for p in self.bucket.params]
        for c in chunks:
            s = int(c["segment"])
            start, local = int(c["start"]), int(c["start"]) - self._offsets[s]
            ok = (int(c["len"]) % 4 == 0 and start % 4 == 0 and (gptr + start * gsize) % (4 * gsize) == 0 and
                  (self._ptrs[s] + local * psize[s]) % (4 * psize[s]) == 0)
            vec += int(ok)
        return vec, len(chunks) - vec
