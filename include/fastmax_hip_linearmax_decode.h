/* fastmax_hip_linearmax_decode.h -- decode-time state cache for masked first-order linearmax
 * (fastmax_hack(q, k, v, p=1, mask=True)) in libfastmax_hip.so (MI355X / gfx950 only; csrc/linearmax_decode.hip).
 * The conventions and the dtype and error enums are those of fastmax_hip.h; the entry points here belong to the same
 * library and FASTMAX_ABI_VERSION and are bound by the one table ABI in fastmax_experiments_amd/_lib.py.
 *
 * linearmax centres every q and k row over D and divides all of q by ONE scalar per (b, h), Mq = the largest centred-row norm
 * of q over the sequence, and all of k by Mk in the same way.  With qc, kc the centred, unscaled rows
 *     f(q^_i . k^_j) = 1 + (qc_i . kc_j) / (Mq Mk)
 *     o_i = (S1 + a qc_i^T S2) / (count + a qc_i . ksum),   a = 1 / (Mq Mk)
 *     S2 = sum_j kc_j v_j^T,  S1 = sum_j v_j,  ksum = sum_j kc_j     (sums over j <= i)
 * so a state of unscaled centred sums never needs rescaling: only a moves, as the two running maxima grow.
 *
 * State: float32, one record per (b, kv head), records in (b, kv head) order, 16-byte aligned, all zero for an empty sequence.
 * With DP = 64 for D <= 64, else 128, a record is cut by columns of S2 into 8 slabs of W = DP / 8 columns, one workgroup each,
 * and holds the 8 slab blocks one after the other.  A slab block is
 *     S2 part   DP * W floats: thread (mg, d) of the slab's workgroup (16 row groups x W columns, thread = mg W + d) owns rows
 *               mg R .. mg R + R - 1 (R = DP / 16) of column slab W + d, stored as R consecutive floats at thread R
 *     S1 part   W floats, the slab's columns
 *     ksum      DP floats     -- the slab's OWN copy
 *     stats     count, Mk, Mq of each of the H / Hkv query heads of the group, padded to a multiple of 4 floats -- own copy
 * = DP W + W + DP + 4 ceil((2 + H / Hkv) / 4) floats; 8 of them make a record.  Every slab computes its copies of ksum, the
 * count and the maxima from the same rows in the same order, so all copies hold the same bits and no workgroup of a launch
 * reads what another one writes.  Rows and columns >= D stay zero.  The count is a float32 sum of ones (exact up to 2^24
 * tokens); because it lives in the record, the arguments of a step do not change from token to token and nothing is read back.
 *
 *   linearmax_decode_state_bytes (host only): the size of the state for B sequences, H query heads over Hkv key / value heads
 *       of size D; 0 when the shape is not supported: a non-positive argument, D > 128, H not a multiple of Hkv, or
 *       H / Hkv > 64.
 *   linearmax_decode_advance: append T >= 1 tokens to every sequence and read them out.
 *       q (B,H,T,D); k, v (B,Hkv,T,D) at their Hkv heads; element strides {batch, head, token}, unit stride in D, any
 *       alignment; query heads g H / Hkv .. (g + 1) H / Hkv - 1 belong to kv head g.  dtype: q, k, v and o (FASTMAX_F32 /
 *       BF16 / F16); arithmetic is float32.  Rows are centred by their mean over the D real elements; both maxima are folded
 *       over all T tokens BEFORE any of them is read out, then per token in order the sums advance and
 *       o (contiguous (B,H,T,D)) receives rows count .. count + T - 1 of masked linearmax over the count + T tokens with the
 *       statistics as they stand after this call.  o == NULL: no read-out; the state and both maxima still advance (state
 *       capture after a prefill by the matrix-core forward).  An all-zero centred row divides by zero, as the reference does.
 *       One launch; no float atomics; bitwise reproducible.
 *       Returns FASTMAX_E_NULL for a null q, k, v, state or stride array, FASTMAX_E_BAD_DTYPE for a dtype outside the enum,
 *       FASTMAX_E_BAD_SHAPE for T <= 0, for every shape linearmax_decode_state_bytes refuses and for B Hkv > INT_MAX / 8,
 *       FASTMAX_E_ALIGNMENT for a state that is not 16-byte aligned; every rejection happens before anything is launched. */
#ifndef FASTMAX_HIP_LINEARMAX_DECODE_H
#define FASTMAX_HIP_LINEARMAX_DECODE_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fastmax_hip_linearmax_decode_state_bytes(int B, int H, int Hkv, int D);
int fastmax_hip_linearmax_decode_advance(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                         const void* v, const int64_t* v_strides, float* state, void* o,
                                         int B, int H, int Hkv, int T, int D, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_LINEARMAX_DECODE_H */
