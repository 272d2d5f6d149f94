"""What the QLoRA kernel tests share (tests/test_qlora_ref_cpu.py on any machine, tests/test_qlora_kernels_gpu.py on an MI355X):
float64 references computed from the exact operand values a kernel sees, the element-wise error bound, the input recipe, the
case lists, and the guarded buffers the outputs are written into.

The bound.  Every kernel of csrc/nf4_gemm.hip, csrc/nf4_lora.hip and csrc/lora_thin.hip forms its result as a sum of products of
bf16 values (exact in float32), accumulated in float32 in SOME order, then rounded once to the result type.  For a sum of
`depth` terms accumulated in float32 in any order the forward error is at most  gamma_depth * S  with  S = sum |term|  and
gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); one more rounding
to the result type adds  u_out |ref|  (u_out = 2^-8 for bfloat16: 8 significant bits; 2^-24 for float32).  With the slack of a
factor two for the second-order terms and the rounding of the error itself:

    bound(ref, S, depth, u_out) = u_out |ref| + 2 (depth + 2) 2^-24 S

No constant in it is measured.  A kernel may get a larger accumulation factor (the 2) with a written reason; u_out never moves.
"""
import math
from typing import NamedTuple, Optional

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
GUARD = 64                      # elements of NaN before and after every guarded buffer
PAD = 8                         # elements a padded leading dimension adds to the row width (16 bytes of bf16, 32 of float32)
BF16, F32 = torch.bfloat16, torch.float32


def u_out(dtype) -> float:
    return U_BF16 if dtype == BF16 else U_F32


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().to(torch.float64)


def bound(ref, S, depth, u, acc=2.0):
    """the largest |got - ref| a float32 accumulation of `depth` terms, rounded once with unit roundoff `u`, can show"""
    return u * ref.abs() + acc * (depth + 2) * U_F32 * S


class Worst(NamedTuple):
    ratio: float
    row: int
    col: int

    def __str__(self):
        return f"worst |err| / bound = {self.ratio:.3f} at ({self.row}, {self.col})"


def check_bound(name, got, ref, S, depth, u, tile=(16, 16), acc=2.0, bnd=None) -> Worst:
    """|got - ref| <= bound at every element of a 2-d result; -> the worst ratio and where it is.  A failure names the element,
    its row and column modulo the kernel's tile, and the ratio."""
    got = f64(got)
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite values in the result"
    b = bound(ref, S, depth, u, acc) if bnd is None else bnd
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    flat = int(ratio.argmax())
    r, c = divmod(flat, ref.shape[1])
    worst = Worst(float(ratio.reshape(-1)[flat]), r, c)
    if worst.ratio > 1.0:
        bad = int((ratio > 1.0).sum())
        raise AssertionError(
            f"{name}: {bad} of {ratio.numel()} elements ({100.0 * bad / ratio.numel():.1f} %) outside the bound; worst at ({r}, {c}) -- "
            f"row % {tile[0]} = {r % tile[0]}, column % {tile[1]} = {c % tile[1]} -- got {float(got[r, c])!r}, want {float(ref[r, c])!r}, "
            f"|err| / bound = {worst.ratio:.3f}")
    return worst


def fraction_outside(got, ref, S, depth, u, acc=2.0) -> float:
    return float(((f64(got) - ref).abs() > bound(ref, S, depth, u, acc)).double().mean())


# ---- references ------------------------------------------------------------------------------------------------------------
def linear_ref(x, w, bias=None, ea=None, eb=None):
    """(ref, S) of  y = x w^T + bias + ea eb^T  in float64 on the operands as given (upcast), S the same sum of absolute values"""
    x, w = f64(x), f64(w)
    ref, S = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        ref, S = ref + f64(bias), S + f64(bias).abs()
    if ea is not None:
        ea, eb = f64(ea), f64(eb)
        ref, S = ref + ea @ eb.t(), S + ea.abs() @ eb.abs().t()
    return ref, S


def linear_emulate(x, w, bias=None, ea=None, eb=None, out_dtype=BF16):
    """what a correct kernel computes, on the CPU: float32 products and sums of the bf16 operands, one rounding of the result"""
    y = x.float() @ w.float().t()
    if ea is not None:
        y = y + ea.float() @ eb.float().t()
    if bias is not None:
        y = y + bias.float()
    return y.to(out_dtype)


def _rope_columns(G, qpk, hs, rope_n):
    """per column of y (G (qpk + 2) hs wide; lit_gpt/model.py:397-403): rotated?, the partner column d +- rope_n / 2, the
    partner's sign, and the column of the cos / sin tables"""
    col = torch.arange(G * (qpk + 2) * hs)
    d, slot = col % hs, (col // hs) % (qpk + 2)
    half = rope_n // 2
    rot = (d < rope_n) & (slot <= qpk)                       # q and k heads, the first rope_n elements
    first = d < half
    partner = torch.where(rot, torch.where(first, col + half, col - half), col)
    sign = torch.where(first, -1.0, 1.0).double()
    return rot, partner, sign, torch.where(rot, d, torch.zeros_like(d))


def rope_apply(y, cos, sin, T, G, qpk, hs, rope_n, tables16=False):
    """y (B T, G (qpk + 2) hs) with the rotation of lit_gpt/model.py:702-708 applied, x[d] cos[d] -+ x[d +- rope_n / 2] sin[d],
    in y's own arithmetic (float64: the reference; float32: what the kernel does, with tables16 the products rounded to bf16)"""
    rot, partner, sign, dd = _rope_columns(G, qpk, hs, rope_n)
    t = torch.arange(y.shape[0]) % T
    c, s = cos.to(y.dtype)[t][:, dd], sin.to(y.dtype)[t][:, dd]
    p0, p1 = y * c, (y[:, partner] * sign.to(y.dtype)) * s
    if tables16:
        p0, p1 = p0.to(BF16).to(y.dtype), p1.to(BF16).to(y.dtype)
    return torch.where(rot, p0 + p1, y)


def split_qkv(y, T, G, qpk, hs):
    """y (B T, G (qpk + 2) hs) -> q (B, G qpk, T, hs), k, v (B, G, T, hs)  (model.py:397-425, k and v at their G heads)"""
    B = y.shape[0] // T
    y5 = y.reshape(B, T, G, qpk + 2, hs)
    q = y5[..., :qpk, :].permute(0, 2, 3, 1, 4).reshape(B, G * qpk, T, hs)
    return q.contiguous(), y5[..., qpk, :].permute(0, 2, 1, 3).contiguous(), y5[..., qpk + 1, :].permute(0, 2, 1, 3).contiguous()


def rope_bound(ref_y, by, cos, sin, T, G, qpk, hs, rope_n, tables16):
    """bound of the rotated tensor (in y's layout) given the bound `by` of the bf16 tensor y the rotation reads: a rotated element
    is bf16(y[d] c + y[p] s) with the two products and their sum rounded in float32 (tables16: the products rounded to bf16), so
        |err| <= 2^-8 |ref| + (1 + 2^-7) (|c| by[d] + |s| by[p]) + 2 u_prod (|y[d] c| + |y[p] s|),   u_prod = 2^-24 or 2^-8;
    the other elements keep by"""
    rot, partner, _, dd = _rope_columns(G, qpk, hs, rope_n)
    t = torch.arange(ref_y.shape[0]) % T
    c, s = f64(cos)[t][:, dd].abs(), f64(sin)[t][:, dd].abs()
    ref = rope_apply(ref_y, f64(cos), f64(sin), T, G, qpk, hs, rope_n)
    up = U_BF16 if tables16 else U_F32
    moved = (U_BF16 * ref.abs() + (1 + 2.0 ** -7) * (c * by + s * by[:, partner])
             + 2 * up * (ref_y.abs() * c + ref_y[:, partner].abs() * s))
    return torch.where(rot, moved, by)


# ---- input recipe ----------------------------------------------------------------------------------------------------------
class LinearCase(NamedTuple):
    x: torch.Tensor                 # (M, K) float32 values (the caller casts to the call's dtype)
    w: torch.Tensor                 # (N, K) float32
    bias: torch.Tensor              # (N,) float32
    ea: Optional[torch.Tensor]      # (M, rank_pad) bf16
    eb: Optional[torch.Tensor]      # (N, rank_pad) bf16


def linear_case(M, N, K, rank_pad, seed=0) -> LinearCase:
    """The three terms of y = x w^T + bias + ea eb^T with the same order of magnitude (standard deviation 1 each), so that a
    missing term shows at nearly every element; a fixed seed on a CPU generator."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 13 * rank_pad)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    ea = eb = None
    if rank_pad:
        ea = torch.randn(M, rank_pad, generator=g).to(BF16)
        eb = (torch.randn(N, rank_pad, generator=g) / math.sqrt(rank_pad)).to(BF16)
    return LinearCase(x, w, bias, ea, eb)


def exact_grid(shape, seed, step=0.125, span=4):
    """values k * step, |k| <= span: sums of a few hundred products of such values are exact in float32 in any order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-span, span + 1, shape, generator=g).float() * step


def quantize(w, double_quant):
    """NF4 codes and quant_state of w through the host codec, and the dequantised float32 weight the kernels must reproduce"""
    from fastmax_experiments_amd import lora
    packed, absmax = lora.nf4_quantize(w)
    qs = [absmax, torch.Size(w.shape), w.dtype, lora.BLOCK, None, "nf4"]
    if double_quant:
        codes, absmax2, offset, code2 = lora.absmax_double_quantize(absmax)
        qs[0], qs[4] = codes, [offset, [absmax2, code2]]
    return packed, qs, lora.nf4_dequantize(packed, qs, w.shape)


# ---- the GPU cases (tests/test_qlora_kernels_gpu.py runs them, tests/test_qlora_ref_cpu.py emulates them) ---------------------
# fastmax_hip_qlora_gemm: (M, N, K).  K step 64 with two LDS stages: 192 = three steps, the ring wraps; 264 = one 256-column
# block + one 8-column chunk; 130 and 257 leave 2 rows and 1 row in the last row block (of 128 or of 256)
GEMM_SHAPES = [(130, 264, 192), (257, 8, 64)]
GEMM_DQ_SHAPE = (130, 320, 192)             # 960 scale blocks: absmax2[blk >> 8] reaches index 3
GEMM_RANKS = (0, 16, 32)
# fastmax_hip_nf4_linear_forward_s: (M, N, K, kernel)
FWD_SHAPES = [(130, 132, 192, "tile"), (1, 48, 256, "gemv"), (3, 48, 256, "gemv"), (16, 48, 256, "gemv"), (3, 132, 192, "tile")]
# fastmax_hip_nf4_linear_backward_input_s: (M, N, K)
DX_SHAPES = [(130, 64, 256), (1, 128, 128)]
# fastmax_hip_qlora_gemm_rope: (B, T, G, qpk, hs, rope_n, K); 256-row tiles cross sequence boundaries in all three
ROPE_SHAPES = [(2, 130, 2, 2, 64, 64, 128), (3, 100, 1, 6, 32, 16, 64), (2, 130, 1, 2, 128, 128, 64)]
# fastmax_hip_lora_down
DOWN_M, DOWN_K, DOWN_RP = (1, 17, 130), (64, 192), (16, 32)
# fastmax_hip_lora_tn: (M, ncols, R, RP)
TN_SHAPES = [(130, 64, 8, 16), (130, 128, 16, 16), (130, 128, 24, 32), (130, 64, 32, 32), (1, 64, 16, 16), (1, 128, 8, 16),
             (2049, 64, 8, 16), (2049, 64, 32, 32)]
# fastmax_hip_lora_up: a wave owns 64 NPL columns, NPL = 8 (R <= 16) or 4
UP_R, UP_N, UP_M = (8, 16, 24, 32), (8, 264, 520), (1, 130)


# ---- guarded buffers -------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded2D:
    """a (rows, cols) tensor `t` inside a (rows, ld) buffer of NaN between two bands of 64 NaN elements: check() wants the bands
    and the gap columns [:, cols:] bit for bit as they were, and no NaN in the payload.  `off` shifts the payload by that many
    elements (an output 8 bytes off a 16-byte boundary)."""

    def __init__(self, rows, cols, ld=None, dtype=BF16, device="cuda", off=0):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lo = rows, cols, ld, GUARD + off
        self.buf = torch.full((self.lo + rows * ld + GUARD,), float("nan"), dtype=dtype, device=device)
        self.full = self.buf[self.lo:self.lo + rows * ld].view(rows, ld)
        self.t = self.full[:, :cols]
        self.before = _bits(self.buf).clone()

    def fill(self, values):
        """payload := values (an in-place kernel's input); the gaps and bands keep their NaN"""
        self.t.copy_(values)
        self.before = _bits(self.buf).clone()
        return self

    def ptr(self):
        return self.t.data_ptr()

    def _outside(self, bits):
        body = bits[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)
        return bits[:self.lo], bits[self.lo + self.rows * self.ld:], body[:, self.cols:]

    def check(self, name, payload_written=True):
        for what, now, was in zip(("before the tensor", "past the tensor", "in the gap columns"), self._outside(_bits(self.buf)),
                                  self._outside(self.before)):
            assert torch.equal(now, was), f"{name}: written {what}"
        if payload_written:
            assert not torch.isnan(self.t).any(), f"{name}: elements left unwritten or NaN"

    def untouched(self):
        return torch.equal(_bits(self.buf), self.before)


def padded(t, pad=PAD, device="cuda"):
    """t (2-d) as a view with a leading dimension `pad` elements wider than its rows, zeros in the gap"""
    buf = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=device)
    buf[:, :t.shape[1]].copy_(t)
    return buf[:, :t.shape[1]]
