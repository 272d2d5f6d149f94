/* fastmax_hip_head.h -- the next-token head on a biased or NF4-quantised lm_head in libfastmax_hip.so (MI355X / gfx950 only;
 * csrc/last_logits.hip).  The dtype and error enums and `fastmax_nf4_scales` are those of fastmax_hip.h; the entry points
 * belong to the same library and FASTMAX_ABI_VERSION and are bound by the table ABI in fastmax_experiments_amd/_lib.py.
 * Everything runs on `stream`; nothing is allocated, nothing is read back, there are no atomics, and a dot product is never
 * split over workgroups.
 *
 *   last_logits_bias  fastmax_hip_last_logits (fastmax_hip_next_token.h) with a bias: logits[b, v] = S + (float)bias[v], where
 *                     S is the float32 sum that entry point produces, bit for bit -- the same 16-byte pieces, lane l taking
 *                     pieces l, l + 64, ..., one fused multiply-add per product in index order from +0, the same xor
 *                     butterfly over the 64 lanes.  Then ONE float32 add of the bias, then the store's rounding to out_dtype.
 *                     bias: V elements of `dtype`, or NULL: fastmax_hip_last_logits itself, which is this entry point with no
 *                     bias (one kernel, csrc/last_logits.hip).
 *
 *   last_logits_nf4   logits[b, v] = sum_c x[b, c] w^[v, c] (+ (float)bias[v]),  w^[v, c] = round_to_dtype(code * scale):
 *                     `codes` holds V C / 2 bytes (or more: further rows are not read), row-major with no row padding, two
 *                     4-bit indices into the NF4 codebook per byte, the first weight in the high nibble; the scale of weight
 *                     (v, c) is entry (v C + c) / 64 of `scales` (plain float32, or double-quantised:
 *                     code2[absmax_q[i]] * absmax2[i / 256] + offset with the product and the sum rounded separately).  The
 *                     float32 product code * scale is rounded to `dtype` (to nearest even): w^ is what
 *                     fastmax_hip_nf4_dequantize_s returns.  x: B rows of C elements of `dtype`, unit stride along a row, ANY
 *                     row stride ldx (elements).  out_dtype is FASTMAX_F32 or `dtype`; logits (B, V), row stride ldo >= V.
 *                     Every product x w^ enters a float32 fused multiply-add unrounded; nothing is rounded to bfloat16 unless
 *                     `dtype` is bfloat16.
 *                     Order of one sum, FASTMAX_F32 and FASTMAX_F16: a row of w^ is cut into pieces of 8 weights (one 32-bit word
 *                     of codes); lane l of the wave that owns the row takes pieces l, l + 64, ... and adds their 8 products each
 *                     in index order with one fused multiply-add per product, into ONE accumulator that starts from +0; the 64
 *                     lanes are then added by an xor butterfly (offsets 32, 16, ..., 1).  One wave owns four rows of w^ and reads
 *                     them once for up to 8 rows of x; a larger B is further passes over the codes.
 *                     FASTMAX_BF16 (x and w^ are both bfloat16: the 16x16x32 bf16 matrix instruction multiplies them exactly and
 *                     adds in float32): a row is cut into blocks of 128 weights, the last one of 64 when C % 128 == 64, filled up
 *                     with zeros.  Block j belongs to wave j % 4 of the workgroup that owns the row; a wave adds its blocks in
 *                     index order into one accumulator that starts from +0, each block as four matrix instructions (the first
 *                     takes weights 0..7, 32..39, 64..71, 96..103 of the block, the second 8..15, 40..47, ..., and so on); the
 *                     four waves' sums s0 .. s3 are added as (s0 + s1) + (s2 + s3).  A workgroup owns 16 rows of w^ and reads
 *                     them once for up to 16 rows of x; a larger B is further passes.
 *                     Either way, then one float32 add of the bias, where there is one; then the store's rounding.  The order
 *                     depends on C and the dtype alone: a row's logits have the same bits alone or inside any batch, for any
 *                     ldx, and whether x moves as 16-byte loads (x and ldx on 16-byte boundaries) or element by element.
 *
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing x, w / codes, scales or logits or a scales
 * struct with neither `absmax` nor all of `absmax_q`, `absmax2`, `code2`; FASTMAX_E_BAD_DTYPE for a dtype outside the enum or
 * an out_dtype that is neither FASTMAX_F32 nor dtype; FASTMAX_E_BAD_SHAPE for B, V or C <= 0, ldx < 0, ldo < V, and for
 * last_logits_bias C above 2^30 or ldw < C, for last_logits_nf4 C % 64 != 0 or V C >= 2^40; FASTMAX_E_ALIGNMENT for x, w,
 * bias or logits not aligned to its element, codes not on a 16-byte boundary, or a scale pointer not aligned to its element. */
#ifndef FASTMAX_HIP_HEAD_H
#define FASTMAX_HIP_HEAD_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_last_logits_bias(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* logits, int64_t ldo,
                                 int B, int V, int C, int dtype, int out_dtype, void* stream);
int fastmax_hip_last_logits_nf4(const void* x, int64_t ldx, const uint8_t* codes, const fastmax_nf4_scales* scales, const void* bias,
                                void* logits, int64_t ldo, int B, int V, int C, int dtype, int out_dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_HEAD_H */
