/* fastmax_hip_int8.h -- the LLM.int8 linear ("bnb.int8") in libfastmax_hip.so (MI355X / gfx950 only; csrc/int8_linear.hip):
 * an inference-only linear layer on int8 weight codes, with the products on the int8 matrix cores.  The dtype and error enums
 * are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION (additions only) and are bound
 * by their rows of ABI_EXT in fastmax_experiments_amd/_lib.py.
 *
 * The codec (defined here from the public description of LLM.int8, arXiv 2208.07339; parity with bitsandbytes is UNPINNED):
 *   weight W (N, K):     SCB[n] = max_k |W[n,k]| (float32);  CB[n,k] = rint(W[n,k] * (127.0f / SCB[n])), the division a correctly
 *                        rounded float32 division, the product float32, rint half-to-even; a row with SCB = 0 has codes 0.
 *   activation x (M, K): column c is an OUTLIER iff |x[m,c]| >= threshold for any row m.  SCA[m] = max |x[m,c]| over the other
 *                        columns; CA[m,c] = rint(x[m,c] * (127.0f / SCA[m])) there, 0 on outlier columns and where SCA = 0.
 *   result:              y[m,n] = acc[m,n] * (SCA[m] * SCB[n]) / 16129 + sum_{c outlier} x[m,c] * (CB[n,c] * (SCB[n] / 127))
 *                        + bias[n];  acc = sum_c CA CB is an exact int32, the rest is float32 on the unrounded x, and the result
 *                        is rounded once to x's dtype.
 *
 * Conventions: matrices are row-major with a row stride in ELEMENTS and unit stride along the row; `dtype` is FASTMAX_BF16 or
 * FASTMAX_F16 for activations and results (quantize_weight / dequantize_weight also take FASTMAX_F32); every kernel runs on
 * `stream`, nothing synchronises with the host and nothing is read back: the outlier list and its count stay in device memory,
 * so a captured graph replays correctly when the outlier set changes.  No atomics, no order-dependent reduction: results are
 * bitwise reproducible.  Shapes: K % 64 == 0, N % 16 == 0, M >= 1, K * 16129 < 2^31.  Rows move as 16-byte pieces: x, y, w and
 * the workspace are 16-byte aligned and their row strides are whole 16-byte pieces.
 * Every rejection happens before anything is launched: FASTMAX_E_NULL (a missing required pointer; bias may be NULL),
 * FASTMAX_E_BAD_DTYPE, FASTMAX_E_BAD_SHAPE (the shapes above, a row stride shorter than the row), FASTMAX_E_ALIGNMENT,
 * FASTMAX_E_WORKSPACE (smaller than fastmax_hip_int8_linear_workspace's answer).
 *
 * fastmax_hip_int8_linear: the activation pass (two launches: column flags; row scales + codes + the ascending outlier list) and
 * then one product launch: M <= FASTMAX_INT8_FEW_ROWS the few-rows kernel (16 output columns per workgroup, four waves split K,
 * weight bytes straight from global memory into 16x16x64 i8 MFMA operands), above it the 128 x 128-tile kernel. */
#ifndef FASTMAX_HIP_INT8_H
#define FASTMAX_HIP_INT8_H

#include "fastmax_hip.h"

#define FASTMAX_INT8_FEW_ROWS 16

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_int8_quantize_weight(const void* w, int64_t w_stride, int dtype, int8_t* cb, float* scb, int N, int K, void* stream);
int fastmax_hip_int8_dequantize_weight(const int8_t* cb, const float* scb, void* w, int64_t w_stride, int dtype, int N, int K,
                                       void* stream);
/* ca (M, K) int8 dense; sca M floats; flags K bytes (1 = outlier column); list K int32 of which the first *count are the outlier
 * columns in ascending order (the rest is not written); count one int32 */
int fastmax_hip_int8_quantize_rows(const void* x, int64_t x_stride, int dtype, float threshold, int8_t* ca, float* sca,
                                   uint8_t* flags, int32_t* list, int32_t* count, int M, int K, void* stream);
/* bytes of workspace fastmax_hip_int8_linear needs (0 for a shape it rejects): ca, sca, flags, list, count, 16-byte pieces each */
size_t fastmax_hip_int8_linear_workspace(int M, int K);
int fastmax_hip_int8_linear(const void* x, int64_t x_stride, const int8_t* cb, const float* scb, const float* bias, void* y,
                            int64_t y_stride, int M, int N, int K, int dtype, float threshold, void* workspace,
                            size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_INT8_H */
