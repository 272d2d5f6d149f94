"""One list of dispatch cases, shared by tests/test_plan_cases_cpu.py (what fastmax_hip_plan answers, host arithmetic only)
and tests/test_plan_kernels_gpu.py (the planned kernels against float64).  Each case is the smallest problem that makes
fwd_plan / bwd_select of csrc/fastmax_api.hip pick one kernel, or one side of a threshold between two of them.

A case: id, (B, H, Nq, Nk, D), in dtype, p, mask, forced path, layout variant, and what the library has to answer: the forward
return code (0, or FASTMAX_E_ALIGNMENT for a forced family with a misaligned operand), the forward kernel, the backward
kernel, and whether the sequence split is active (nseg > 1).  `gpu` = the GPU test runs it; the others are host-only
plan checks (the far side of a threshold whose near side runs, head counts that only change the split, the 20000-token
rule).  `out` = the dtype of o when it is not the Python rule's (masked: the input dtype, unmasked: float32).

Layout variants (all ordinary views into allocated memory on the GPU, made-up addresses on the host):
  aligned  every operand keeps the 16-byte rule
  q_off8, go_off8, o_off8, dq_off8   that operand starts 8 bytes past a 16-byte boundary
  k_rowpad k's row stride is D + 8 bytes of elements: every other row starts 8 bytes off
"""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np

from fastmax_experiments_amd import _lib
from fastmax_experiments_amd._lib import F32, BF16, F16, E_ALIGNMENT, Plan, Problem

Case = namedtuple("Case", "id shape dtype p mask path layout rc fwd bwd split gpu out tune")
LAYOUTS = ("aligned", "q_off8", "go_off8", "o_off8", "dq_off8", "k_rowpad")
DTYPES = {"f32": F32, "bf16": BF16, "f16": F16}
DTYPE_NAMES = {v: k for k, v in DTYPES.items()}
PATHS = {"auto": _lib.PATH_AUTO, "quadratic": _lib.PATH_QUADRATIC, "recurrent": _lib.PATH_RECURRENT, "mfma": _lib.PATH_MFMA,
         "quadratic_mfma": _lib.PATH_QUADRATIC_MFMA}
SCANS = ("FWD_SCAN_V2", "FWD_SCAN_D128_2P", "FWD_SCAN_BF16", "FWD_SCAN_GEN")
GUARD = 64          # elements of NaN on either side of every output on the GPU

CASES = []


def case(shape, dtype, p, mask, fwd, bwd, split=False, path="auto", layout="aligned", rc=0, gpu=True, out=None, tune=None):
    if len(shape) == 4:
        shape = (shape[0], shape[1], shape[2], shape[2], shape[3])
    B, H, Nq, Nk, D = shape
    cid = f"{dtype}-p{p}-{'masked' if mask else 'unmasked'}-{B}x{H}x{Nq}x{Nk}x{D}-{path}-{layout}"
    if out:
        cid += f"-out_{out}"
    if tune:
        cid += "-" + "_".join(f"{k}{v}" for k, v in tune.items())
    assert cid not in {c.id for c in CASES}, cid
    CASES.append(Case(cid, shape, dtype, p, mask, path, layout, rc, fwd, bwd, split, gpu, out, tune))
    return cid


ALL = ("f32", "bf16", "f16")

# ---- forward scans (p = 1 masked), unsplit at N = 130 (three 64-row chunks, a ragged last one), split at N = 520 (nine chunks:
#      two segments of five and four); under 512 rows the backward is the 16-row tiles, from 512 the linear-time kernels
case((1, 2, 130, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUAD_MFMA")
case((1, 2, 520, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_LIN", split=True)
case((1, 2, 130, 32), "f32", 1, True, "FWD_SCAN_GEN", "BWD_QUAD_MFMA")
case((1, 2, 130, 64), "f16", 1, True, "FWD_SCAN_GEN", "BWD_QUAD_MFMA")
case((1, 2, 520, 32), "f32", 1, True, "FWD_SCAN_GEN", "BWD_LIN", split=True)
case((1, 2, 130, 64), "bf16", 1, True, "FWD_SCAN_GEN", "BWD_QUAD_MFMA", tune={"bf16_kernel": 0})
for _d in (64, 72, 128):
    case((1, 2, 130, _d), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_QUAD_MFMA")
case((1, 2, 520, 128), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_LIN", split=True)
case((1, 2, 130, 68), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_QUAD_MFMA")
case((1, 2, 130, 128), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_QUAD_MFMA")
case((1, 2, 130, 72), "f16", 1, True, "FWD_SCAN_D128_2P", "BWD_QUAD_MFMA")
case((1, 2, 520, 128), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_SCAN", split=True)
# ---- the linear-time backwards at N = 520, every dtype
case((1, 2, 520, 64), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_LIN", split=True)
case((1, 2, 520, 32), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_LIN", split=True)
case((1, 2, 520, 64), "f16", 1, True, "FWD_SCAN_GEN", "BWD_LIN", split=True)
case((1, 2, 520, 32), "f16", 1, True, "FWD_SCAN_GEN", "BWD_LIN", split=True)
case((1, 2, 520, 68), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_SCAN", split=True)
case((1, 2, 520, 72), "f16", 1, True, "FWD_SCAN_D128_2P", "BWD_SCAN", split=True)
# ---- the vector-ALU recurrence: forced, and where a p = 1 masked problem loses the matrix cores
for _dt in ALL:
    case((1, 2, 65, 64), _dt, 1, True, "FWD_RECURRENT", "BWD_QUAD_MFMA", path="recurrent")
case((1, 2, 130, 64), "f32", 1, True, "FWD_RECURRENT", "BWD_QUADRATIC", layout="q_off8")
case((1, 2, 130, 64), "bf16", 1, True, "FWD_RECURRENT", "BWD_QUADRATIC", layout="q_off8")
# ---- p = 1 unmasked from totals: N_q >= 64, N_k >= 512; the fp32 / fp16 backward above D = 64 is tiles
for _dt in ALL:
    case((1, 2, 64, 512, 64), _dt, 1, False, "FWD_UNMASKED_LIN", "BWD_UNMASKED_LIN")
case((1, 2, 64, 512, 128), "bf16", 1, False, "FWD_UNMASKED_LIN", "BWD_UNMASKED_LIN")
case((1, 2, 64, 512, 128), "f32", 1, False, "FWD_UNMASKED_LIN", "BWD_QUAD_MFMA")
# ---- 32 x 32 tiles from N_q = 256 (backward: N_k = 256 too); two-part operands above D = 64 stay on the 16-row forward
for _dt in ALL:
    case((1, 2, 256, 64), _dt, 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 256, 128), "bf16", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 256, 300, 64), "f32", 1, False, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 255, 64), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 255, 64), "bf16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 255, 64), "f16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 256, 128), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD32")
case((1, 2, 300, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUAD32")
case((1, 2, 520, 64), "f32", 1, True, "FWD_QUAD32", "BWD_QUAD32", path="quadratic_mfma")
case((1, 2, 520, 64), "f32", 1, True, "FWD_RECURRENT", "BWD_QUAD32", layout="o_off8")
case((1, 2, 64, 300, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 1, 256, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
# ---- head sizes above 128: tiles only; the matrix-core backward is bf16 only
case((1, 2, 70, 136), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUADRATIC")
case((1, 2, 70, 136), "f16", 2, True, "FWD_QUAD_MFMA", "BWD_QUADRATIC")
case((1, 2, 70, 256), "bf16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 70, 256), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUADRATIC")
# ---- the vector-ALU tiles: forced, a handful of queries against a short key range, or a misaligned operand
for _dt in ALL:
    case((1, 2, 70, 64), _dt, 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC", path="quadratic")
case((1, 2, 130, 64), "f32", 1, True, "FWD_QUADRATIC", "BWD_QUADRATIC", path="quadratic")
case((1, 2, 15, 255, 64), "f32", 1, False, "FWD_QUADRATIC", "BWD_QUAD_MFMA")
case((1, 2, 70, 64), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC", layout="k_rowpad")
case((1, 2, 70, 64), "bf16", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC", layout="k_rowpad")
case((1, 2, 130, 64), "f32", 1, True, "FWD_RECURRENT", "BWD_QUADRATIC", layout="k_rowpad")
case((1, 2, 70, 64), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC", layout="q_off8")
case((1, 2, 70, 64), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUAD_MFMA", layout="o_off8")
case((1, 2, 70, 64), "f16", 2, True, "FWD_QUADRATIC", "BWD_QUAD_MFMA", layout="o_off8")
case((1, 2, 70, 64), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC", path="quadratic", layout="o_off8")
# grad_o and dq are not forward operands: the matrix-core forward stays, the backward drops to the vector ALU
for _lay in ("go_off8", "dq_off8"):
    case((1, 2, 130, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUADRATIC", layout=_lay)
    case((1, 2, 70, 64), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUADRATIC", layout=_lay)
case((1, 2, 130, 64), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_QUADRATIC", layout="go_off8")
case((1, 2, 70, 64), "f16", 2, True, "FWD_QUAD_MFMA", "BWD_QUADRATIC", layout="dq_off8")
# a forced matrix-core family with a misaligned forward operand is rejected (the backward would still run on the vector ALU,
# or on the tiles when only o is off)
case((1, 2, 130, 64), "f32", 1, True, None, "BWD_QUADRATIC", path="mfma", layout="q_off8", rc=E_ALIGNMENT)
case((1, 2, 70, 64), "f32", 2, True, None, "BWD_QUADRATIC", path="quadratic_mfma", layout="k_rowpad", rc=E_ALIGNMENT)
case((1, 2, 70, 64), "f32", 2, True, None, "BWD_QUAD_MFMA", path="quadratic_mfma", layout="o_off8", rc=E_ALIGNMENT)
# ---- tile edges (the names are what fastmax_hip_plan answers): 32-row tiles with a ragged end -- N = 257: one row in the last
#      wave of the last workgroup; 289: a full wave and one row; ragged queries and ragged keys independently when unmasked
case((1, 2, 257, 64), "bf16", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 257, 64), "f32", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 289, 64), "bf16", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 300, 128), "bf16", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 300, 32), "f16", 1, True, "FWD_QUAD32", "BWD_QUAD32", path="quadratic_mfma")
case((1, 2, 257, 300, 64), "bf16", 2, False, "FWD_QUAD32", "BWD_QUAD32")
case((1, 2, 300, 257, 64), "bf16", 2, False, "FWD_QUAD32", "BWD_QUAD32")
# the per-XCD workgroup mapping of the 32-row tiles, (BH & 7) == 0 in quad32_block (fastmax_quad32_bwd.hip)
case((1, 8, 257, 64), "bf16", 2, True, "FWD_QUAD32", "BWD_QUAD32")
case((2, 4, 300, 64), "f32", 1, True, "FWD_QUAD32", "BWD_QUAD32", path="quadratic_mfma")
# 16-row tiles one row past one and two tiles, and a head size that is no multiple of 16 (single- and two-part operands)
case((1, 2, 17, 64), "bf16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 33, 64), "bf16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 70, 80), "bf16", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
case((1, 2, 70, 80), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA")
# vector-ALU tiles and the recurrence with more than two heads, a second batch entry and a ragged end
case((2, 3, 70, 50), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC")
case((1, 3, 130, 64), "bf16", 1, True, "FWD_RECURRENT", "BWD_QUAD_MFMA", path="recurrent")

# ---- thresholds: (what it is, the case below, the case at / above, the answer that has to differ).  A side that the table
#      above does not already run on the GPU runs when it is the smaller one; the other side is a host-only plan check.
BOUNDARIES = []


def boundary(what, lo, hi, field):
    BOUNDARIES.append((what, lo, hi, field))



def _have(shape, dtype, p, mask, **kw):
    """id of a case already in the list"""
    if len(shape) == 4:
        shape = (shape[0], shape[1], shape[2], shape[2], shape[3])
    hits = [c.id for c in CASES if c.shape == shape and c.dtype == dtype and c.p == p and c.mask == mask and
            c.path == kw.get("path", "auto") and c.layout == kw.get("layout", "aligned") and c.tune is None and c.out == kw.get("out")]
    assert len(hits) == 1, (shape, dtype, p, mask, kw, hits)
    return hits[0]


boundary("Nq 255/256: 32 x 32 forward tiles", _have((1, 2, 255, 64), "f32", 2, True), _have((1, 2, 256, 64), "f32", 2, True), "fwd")
boundary("Nq 255/256: 32 x 32 backward tiles", _have((1, 2, 255, 64), "f32", 2, True), _have((1, 2, 256, 64), "f32", 2, True), "bwd")
boundary("Nk 255/256 at Nq = 256: 32 x 32 backward tiles",
         case((1, 2, 256, 255, 64), "f32", 2, False, "FWD_QUAD32", "BWD_QUAD_MFMA"),
         case((1, 2, 256, 256, 64), "f32", 2, False, "FWD_QUAD32", "BWD_QUAD32", gpu=False), "bwd")
boundary("Nq 511/512: linear-time backward",
         case((1, 2, 511, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUAD32", split=True),
         case((1, 2, 512, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_LIN", split=True, gpu=False), "bwd")
boundary("Nq 511/512: two-part backward scans",
         case((1, 2, 511, 128), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_QUAD32", split=True),
         case((1, 2, 512, 128), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_SCAN", split=True, gpu=False), "bwd")
boundary("Nk 511/512: unmasked linear forward",
         case((1, 2, 64, 511, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA"), _have((1, 2, 64, 512, 64), "f32", 1, False), "fwd")
boundary("Nk 511/512: unmasked linear backward", _have((1, 2, 64, 511, 64), "f32", 1, False), _have((1, 2, 64, 512, 64), "f32", 1, False), "bwd")
boundary("Nq 63/64: unmasked linear forward",
         case((1, 2, 63, 512, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA"), _have((1, 2, 64, 512, 64), "f32", 1, False), "fwd")
boundary("Nq 63/64: unmasked linear backward", _have((1, 2, 63, 512, 64), "f32", 1, False), _have((1, 2, 64, 512, 64), "f32", 1, False), "bwd")
boundary("Nq 15/16 at Nk = 255: matrix-core tiles against the vector ALU", _have((1, 2, 15, 255, 64), "f32", 1, False),
         case((1, 2, 16, 255, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA", gpu=False), "fwd")
boundary("Nk 255/256 at Nq = 15: matrix-core tiles against the vector ALU", _have((1, 2, 15, 255, 64), "f32", 1, False),
         case((1, 2, 15, 256, 64), "f32", 1, False, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA", gpu=False), "fwd")
boundary("D 64/72: headline scan against two-part operands", _have((1, 2, 130, 64), "f32", 1, True),
         case((1, 2, 130, 72), "f32", 1, True, "FWD_SCAN_D128_2P", "BWD_QUAD_MFMA", gpu=False), "fwd")
boundary("D 64/72: fp32 leaves the 32 x 32 forward tiles", _have((1, 2, 256, 64), "f32", 2, True),
         case((1, 2, 256, 72), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD32", gpu=False), "fwd")
boundary("D 128/136: scans end", _have((1, 2, 130, 128), "bf16", 1, True),
         case((1, 2, 130, 136), "bf16", 1, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA", gpu=False), "fwd")
boundary("D 128/136: fp32 matrix-core backward ends",
         case((1, 2, 70, 128), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA"), _have((1, 2, 70, 136), "f32", 2, True), "bwd")
boundary("D % 4 (fp32): matrix cores need whole 16-byte pieces",
         case((1, 2, 70, 50), "f32", 2, True, "FWD_QUADRATIC", "BWD_QUADRATIC"),
         case((1, 2, 70, 52), "f32", 2, True, "FWD_QUAD_MFMA", "BWD_QUAD_MFMA", gpu=False), "fwd")
boundary("D % 8 (16-bit): matrix cores need whole 16-byte pieces",
         case((1, 2, 130, 68), "bf16", 1, True, "FWD_RECURRENT", "BWD_QUADRATIC"), _have((1, 2, 130, 72), "bf16", 1, True), "fwd")
boundary("N 448/449: seven against eight chunks, the sequence split starts",
         case((1, 2, 448, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUAD32"),
         case((1, 2, 449, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_QUAD32", split=True), "split")
boundary("B*H 383/384 at D <= 64: the sequence split stops",
         case((1, 383, 512, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_LIN", split=True, gpu=False),
         case((1, 384, 512, 64), "f32", 1, True, "FWD_SCAN_V2", "BWD_LIN", gpu=False), "split")
boundary("B*H 191/192 at D > 64: the sequence split stops",
         case((1, 191, 512, 128), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_LIN", split=True, gpu=False),
         case((1, 192, 512, 128), "bf16", 1, True, "FWD_SCAN_BF16", "BWD_LIN", gpu=False), "split")
# select(): p = 1 masked problems no scan covers take the tiles up to 20000 tokens, then the recurrence.  Every scan asks for
# equal in / out dtypes, so this is reachable with a 16-bit input and a float32 output only: host-only
boundary("N 20000/20001: tiles against the recurrence",
         case((1, 2, 20000, 64), "bf16", 1, True, "FWD_QUAD32", "BWD_QUAD32", gpu=False, out="f32"),
         case((1, 2, 20001, 64), "bf16", 1, True, "FWD_RECURRENT", "BWD_QUAD32", gpu=False, out="f32"), "fwd")

BY_ID = {c.id: c for c in CASES}
GPU_CASES = [c for c in CASES if c.gpu]

# per 16-row block, forward (o, g) / gradients: TOL of tests/test_blockwise_gpu.py, restated (tests/test_blockwise_cpu.py
# holds the two tables equal).  None is above the per-tensor tolerance tests/test_plan_kernels_gpu.py applies.
BLOCK = 16
BLOCK_TOL = {"bf16": (8e-3, 1e-2), "f16": (2e-3, 2e-3), "f32": (2e-4, 2e-4)}


# Cases whose gradients exceed BLOCK_TOL in rows 0:16 through a rounding the kernels legitimately perform: the 32-row forward
# tiles divide the rounded P by the sum of the unrounded P and store o in bf16, and the backward reads that o back for
# c_i = G_i . o_i (blockwise.tile_model names the source lines).  Gradient tolerance = 1.5 x the worst block of
# blockwise.tile_model for the case, never above the per-tensor 2.5e-2; shape, dtype, p -> (model, measured on the MI355X):
#   (1, 2, 257, 64) bf16 p = 2: dq rows 0:16 of head 1 -- model 2.050e-2, measured 2.050e-2 (dk 1.43e-2 / 1.435e-2); 1.5 x = 3.1e-2 -> 2.5e-2
#   (1, 8, 257, 64) bf16 p = 2: dq rows 0:16 of head 1 -- model 1.177e-2, measured 1.177e-2 (dk 1.03e-2 / 1.028e-2); 1.5 x = 1.77e-2
BLOCK_TOL_BWD_CASE = {((1, 2, 257, 257, 64), "bf16", 2): 2.5e-2, ((1, 8, 257, 257, 64), "bf16", 2): 1.77e-2}
TILE_FORWARDS = ("FWD_QUAD32", "FWD_QUAD_MFMA")


def block_tol(c):
    """(forward, gradients) tolerance of every 16-row block of the case"""
    tf, tb = BLOCK_TOL[c.dtype]
    return tf, BLOCK_TOL_BWD_CASE.get((c.shape, c.dtype, c.p), tb)


def tile_rows(c):
    """(forward, backward) tile height of the kernels the case names: 32 for the wide tiles, 16 for the narrow ones"""
    return (32 if c.fwd == "FWD_QUAD32" else 16, 32 if c.bwd == "BWD_QUAD32" else 16)


# ---- shared plumbing -------------------------------------------------------------------------------------------------
def out_dtype(c):
    return c.out or (c.dtype if c.mask else "f32")


def nt(D):
    return 8.0 * float(np.sqrt(D))          # the oracle's default normalize term (attention_mechanisms/fastmax.py:78-82)


def problem(c):
    B, H, Nq, Nk, D = c.shape
    return Problem(B, H, Nq, Nk, D, DTYPES[c.dtype], DTYPES[out_dtype(c)], c.p, int(c.mask), 1.0 / nt(D), 1.0 / (2.0 * nt(D) ** 2),
                   float(Nq), PATHS[c.path])


def elem_bytes(dtype):
    return 4 if dtype == "f32" else 2


def fake_operands(prob, layout):
    """made-up addresses and strides with the wanted alignment: (q, qs, k, ks, v, vs, o, go, gos, dq, dk, dv)"""
    es = 4 if prob.in_dtype == F32 else 2
    H, Nq, Nk, D = prob.H, prob.Nq, prob.Nk, prob.D
    addr = {n: (i + 1) << 32 for i, n in enumerate(("q", "k", "v", "o", "go", "dq", "dk", "dv"))}
    if layout.endswith("_off8"):
        addr[layout[:-5]] += 8
    pad = 8 // es if layout == "k_rowpad" else 0

    def st(n, row):
        return (ctypes.c_int64 * 3)(H * n * row, n * row, row)

    return (addr["q"], st(Nq, D), addr["k"], st(Nk, D + pad), addr["v"], st(Nk, D), addr["o"], addr["go"], st(Nq, D), addr["dq"],
            addr["dk"], addr["dv"])


def query(L, prob, operands, forward_only=False):
    """fastmax_hip_plan -> (return value, Plan)"""
    ops = list(operands)
    if forward_only:
        ops[7:] = [None] * 5
    plan = Plan()
    rc = L.fastmax_hip_plan(ctypes.byref(prob), *ops, ctypes.byref(plan))
    return rc, plan


def answer(plan):
    """(rc, forward kernel name or None, backward kernel name, nseg > 1)"""
    return (plan.rc, None if plan.fwd_kernel < 0 else _lib.FWD_KERNELS[plan.fwd_kernel],
            None if plan.bwd_kernel < 0 else _lib.BWD_KERNELS[plan.bwd_kernel], plan.nseg > 1)


def expected(c):
    return (c.rc, c.fwd, c.bwd, c.split)


@contextlib.contextmanager
def tuned(L, c):
    """the case's tuning keys through fastmax_hip_tune, put back afterwards"""
    before = {k: L.fastmax_hip_tune_get(k.encode()) for k in (c.tune or {})}
    try:
        for k, v in (c.tune or {}).items():
            assert L.fastmax_hip_tune(k.encode(), v) == 0
        yield
    finally:
        for k, v in before.items():
            L.fastmax_hip_tune(k.encode(), v)


_INPUTS = {}


def host_inputs(c):
    """(q, k, v, grad_o) float32 torch tensors on the CPU that hold values of the case's dtype exactly; the same tensors for
    every layout variant and forced path of a problem.  Unmasked with fewer than 16 queries: K is scaled by 0.25 so that
    g = Nq + a q . ksum stays away from zero (tests/test_plan_cases_cpu.py checks the margin for every GPU case).  Masked with
    one row in the last 16-row block (N = 16 m + 1): that block of dk is the single product dk_N = a (G_N . (v_N - o_N) / g_N) q_N,
    whose dot product of random signs can cancel to nothing in some head; the last row of grad_o takes the signs of the last
    row of v, so that G_N . v_N = sum |G| |v| (tests/test_blockwise_cpu.py: the rounded model passes every block)."""
    import torch
    B, H, Nq, Nk, D = c.shape
    key = (c.shape, c.dtype, c.mask)
    if key not in _INPUTS:
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c.dtype]
        g = torch.Generator().manual_seed(Nq * 131 + Nk * 17 + D)
        q, go = (torch.randn(B, H, Nq, D, generator=g).to(tdt).float() for _ in range(2))
        k, v = (torch.randn(B, H, Nk, D, generator=g).to(tdt).float() for _ in range(2))
        if not c.mask and Nq < 16:
            k = (k * 0.25).to(tdt).float()
        if c.mask and Nk % BLOCK == 1:
            go[:, :, -1] = go[:, :, -1].abs() * torch.where(v[:, :, -1] < 0, -1.0, 1.0)
        _INPUTS[key] = (q, k, v, go)
    return _INPUTS[key]


_ORACLE = {}


def oracle_fwd(c):
    """(o, g) float64 from oracle.c_oracle on the upcast inputs, computed once per problem"""
    from oracle import c_oracle
    key = ("fwd", c.shape, c.dtype, c.mask, c.p)
    if key not in _ORACLE:
        q, k, v, _ = (t.numpy() for t in host_inputs(c))
        _ORACLE[key] = c_oracle.fwd(q, k, v, mask=c.mask, p=c.p)
    return _ORACLE[key]


def oracle_bwd(c):
    """(dq, dk, dv) float64, computed once per problem"""
    from oracle import c_oracle
    key = ("bwd", c.shape, c.dtype, c.mask, c.p)
    if key not in _ORACLE:
        q, k, v, go = (t.numpy() for t in host_inputs(c))
        _ORACLE[key] = c_oracle.bwd(q, k, v, go, mask=c.mask, p=c.p)
    return _ORACLE[key]
