/* fastmax_hip_neox.h -- the GPT-NeoX (pythia) decoder block's neighbours of the attention sub-layer in libfastmax_hip.so
 * (MI355X / gfx950 only; csrc/neox_block.hip): LayerNorm as a PAIR over one row (norm_1 and norm_2 of the parallel-residual
 * block normalise the same row with the same eps, so they share mean and rstd) with the three-way residual add in front, its
 * backward pass, and the ungated exact-GELU activation of GptNeoxMLP with its backward pass.  The dtype and error enums are
 * those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION (additions only) and are bound by
 * the table ABI in fastmax_experiments_amd/_lib.py.
 *
 * Conventions (those of fastmax_hip_block.h): every matrix operand is (M rows, C or I columns) with a row stride in ELEMENTS
 * and unit stride along the row; `dtype` (FASTMAX_F32 / BF16 / F16) is the activation dtype; arithmetic is float32; every kernel
 * runs on `stream`, nothing synchronises with the host, there are no atomics and every reduction has a fixed order (lanes of a
 * wave, then waves through LDS), so all results are bitwise reproducible.  Rows whose length and addresses are whole 16-byte
 * pieces (LayerNorm: up to 1024 pieces per row) move as 16-byte accesses, are read from memory once and kept in registers; any
 * other C, I >= 1 takes a scalar path.  Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing
 * required pointer (r2 without r1, a residual without s_out, w2 without y2 / dy2 and the reverse, a wanted parameter gradient
 * without a workspace), FASTMAX_E_BAD_DTYPE for a dtype outside the enum (weight_dtype: `dtype` or FASTMAX_F32),
 * FASTMAX_E_BAD_SHAPE for M <= 0, C <= 0, a row stride shorter than the row, an `act` that is not FASTMAX_NEOX_ACT_GELU or M
 * so large that the grid does not fit, FASTMAX_E_ALIGNMENT for a mean / rstd / parameter-gradient pointer that is not 4-byte
 * aligned, a workspace that is not 16-byte aligned or a matrix pointer not aligned to its element, FASTMAX_E_WORKSPACE for a
 * workspace smaller than the query function's answer.
 *
 *   layernorm_forward: s = x;  with r1: s = round(x + r1);  with r1 and r2: s = round(round(r1 + r2) + x)   (the block's
 *       mlp(n_2) + h + x, left to right, every add rounded to `dtype`; s is written to s_out when r1 is given -- s_out is then
 *       required)
 *       mean[m] = mean_c(s), rstd[m] = 1 / sqrt(mean_c((s - mean)^2) + eps)   (float32, the deviations taken from the row in
 *       registers; (M) floats each, either may be NULL)
 *       y1 = round((s - mean) rstd w1 + b1)       ONE rounding, to `dtype`, whatever weight_dtype is (torch's LayerNorm)
 *       y2 = round((s - mean) rstd w2 + b2)       when w2 is given (y2 is then required); same statistics
 *       w1, b1, w2, b2 (C) share `weight_dtype`; b1 and b2 may be NULL.
 *   layernorm_backward: with n = (s - mean) rstd and g = w1 dy1 [+ w2 dy2]:
 *       ds = round(rstd (g - mean_c(g) - n mean_c(g n))) [+ ds_in]     (ds, ds_in, dy1, dy2: `dtype`; ds_in is added to the
 *       rounded result, as accumulating the two gradients would); one pass over dy1, dy2, s
 *       dw_k = sum_m dy_k n, db_k = sum_m dy_k   ((C) floats each, each may be NULL): workgroups leave partial sums over fixed
 *       blocks of rows in the workspace, a second kernel adds them per column in block order.  layernorm_backward_workspace is
 *       the size that needs (`pair`: w2 / dy2 are given): 0 when want_param_grads == 0, and then nothing but ds is written.
 *   act_forward: y = round(gelu(a)), gelu(a) = a (1 + erf(a / sqrt 2)) / 2; a, y (M, I) with their own row strides.
 *   act_backward: da = round(dy gelu'(a)), gelu recomputed from a; one pass. */
#ifndef FASTMAX_HIP_NEOX_H
#define FASTMAX_HIP_NEOX_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fastmax_neox_act { FASTMAX_NEOX_ACT_GELU = 0 };

int fastmax_hip_layernorm_forward(const void* x, int64_t x_stride, const void* r1, int64_t r1_stride, const void* r2,
                                  int64_t r2_stride, const void* w1, const void* b1, const void* w2, const void* b2,
                                  void* s_out, int64_t s_stride, void* y1, int64_t y1_stride, void* y2, int64_t y2_stride,
                                  float* mean, float* rstd, int M, int C, float eps, int dtype, int weight_dtype, void* stream);
size_t fastmax_hip_layernorm_backward_workspace(int M, int C, int dtype, int pair, int want_param_grads);
int fastmax_hip_layernorm_backward(const void* dy1, int64_t dy1_stride, const void* dy2, int64_t dy2_stride, const void* s,
                                   int64_t s_stride, const void* w1, const void* w2, const float* mean, const float* rstd,
                                   const void* ds_in, int64_t ds_in_stride, void* ds, int64_t ds_stride, float* dw1, float* db1,
                                   float* dw2, float* db2, int M, int C, int dtype, int weight_dtype, void* workspace,
                                   size_t workspace_bytes, void* stream);
int fastmax_hip_act_forward(const void* a, int64_t a_stride, void* y, int64_t y_stride, int M, int I, int act, int dtype,
                            void* stream);
int fastmax_hip_act_backward(const void* a, int64_t a_stride, const void* dy, int64_t dy_stride, void* da, int64_t da_stride,
                             int M, int I, int act, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_NEOX_H */
