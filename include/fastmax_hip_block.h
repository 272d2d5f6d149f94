/* fastmax_hip_block.h -- the decoder block's neighbours of the attention sub-layer in libfastmax_hip.so (MI355X / gfx950 only;
 * csrc/block_neighbours.hip): RMSNorm with an optional residual add in front, its backward pass, and the gated activation of
 * the LLaMA / Gemma MLP with its backward pass.  The dtype and error enums are those of fastmax_hip.h; the entry points here
 * belong to the same library and FASTMAX_ABI_VERSION and are bound by the one table ABI in fastmax_experiments_amd/_lib.py.
 *
 * Conventions: every matrix operand is (M rows, C or I columns) with a row stride in ELEMENTS and unit stride along the row;
 * `dtype` (FASTMAX_F32 / BF16 / F16) is the activation dtype; arithmetic is float32; every kernel runs on `stream`, nothing
 * synchronises with the host, there are no atomics and every reduction has a fixed order (lanes of a wave, then waves through
 * LDS), so all results are bitwise reproducible.  Rows whose length and addresses are whole 16-byte pieces move as 16-byte
 * accesses and (RMSNorm: up to 2048 pieces per row) are read from memory once and kept in registers; any other C, I >= 1 takes
 * a scalar path.  Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing required pointer,
 * FASTMAX_E_BAD_DTYPE for a dtype outside the enum (weight_dtype: `dtype` or FASTMAX_F32), FASTMAX_E_BAD_SHAPE for
 * M <= 0, C <= 0, a row stride shorter than the row or M so large that the grid does not fit, FASTMAX_E_ALIGNMENT for an
 * rstd / dweight / workspace pointer that is not 4-byte aligned or a matrix pointer not aligned to its element,
 * FASTMAX_E_WORKSPACE for a workspace smaller than the query function's answer.
 *
 *   rmsnorm_forward: s = r ? round(x + r) : x   (rounded to `dtype`; written to s_out when r is given -- s_out is then required)
 *       rstd[m] = 1 / sqrt(mean_c(s^2) + eps)   (float32 statistics over the row; rstd may be NULL)
 *       y = round_out(round(s rstd) * w')       w' = weight, or round_w(1 + weight) with add_unit_offset
 *       weight (C) has `weight_dtype`; y has `dtype` when weight_dtype == dtype, else float32 (torch's promotion).
 *   rmsnorm_backward: with n = s rstd, g = w' dy:   ds = round(rstd (g - n mean_c(g n))) [+ ds_in]    (ds, ds_in: `dtype`;
 *       ds_in is added to the rounded result, as accumulating the two gradients would)
 *       dy has y's dtype.  dweight (C floats, may be NULL) = sum_m dy round(n): workgroups leave partial sums over fixed blocks
 *       of rows in the workspace, a second kernel adds them per column in block order.  rmsnorm_backward_workspace is the size
 *       that needs: 0 when want_dweight == 0, and then nothing but ds is written.
 *   gated_act_forward: y = round(round(act(a)) * b), act = FASTMAX_ACT_SILU (a / (1 + exp(-a))) or FASTMAX_ACT_GELU
 *       (a (1 + erf(a / sqrt 2)) / 2); a, b, y (M, I) with their own row strides, so the halves of one (M, 2I) buffer are valid.
 *   gated_act_backward: da = round(dy b act'(a)), db = round(dy round(act(a))), act recomputed; one pass. */
#ifndef FASTMAX_HIP_BLOCK_H
#define FASTMAX_HIP_BLOCK_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fastmax_gated_act { FASTMAX_ACT_SILU = 0, FASTMAX_ACT_GELU = 1 };

int fastmax_hip_rmsnorm_forward(const void* x, int64_t x_stride, const void* r, int64_t r_stride, const void* weight,
                                void* s_out, int64_t s_stride, void* y, int64_t y_stride, float* rstd, int M, int C, float eps,
                                int add_unit_offset, int dtype, int weight_dtype, void* stream);
size_t fastmax_hip_rmsnorm_backward_workspace(int M, int C, int dtype, int want_dweight);
int fastmax_hip_rmsnorm_backward(const void* dy, int64_t dy_stride, const void* s, int64_t s_stride, const void* weight,
                                 const float* rstd, const void* ds_in, int64_t ds_in_stride, void* ds, int64_t ds_stride,
                                 float* dweight, int M, int C, int add_unit_offset, int dtype, int weight_dtype,
                                 void* workspace, size_t workspace_bytes, void* stream);
int fastmax_hip_gated_act_forward(const void* a, int64_t a_stride, const void* b, int64_t b_stride, void* y, int64_t y_stride,
                                  int M, int I, int act, int dtype, void* stream);
int fastmax_hip_gated_act_backward(const void* a, int64_t a_stride, const void* b, int64_t b_stride, const void* dy,
                                   int64_t dy_stride, void* da, int64_t da_stride, void* db, int64_t db_stride, int M, int I,
                                   int act, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_BLOCK_H */
