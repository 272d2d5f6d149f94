/* fastmax_hip_adapter.h -- adapter-v2 fine-tuning in libfastmax_hip.so (MI355X / gfx950 only; csrc/adapter_v2.hip): the per-column
 * scale and bias that lit_gpt/adapter_v2.py:50-62 puts behind every linear of the model, y = adapter_scale * (linear(x) +
 * adapter_bias), as one pass forward and one pass backward that also leaves both parameter gradients.  The dtype and error enums
 * are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION (additions only) and are bound
 * by their rows of the one table ABI in fastmax_experiments_amd/_lib.py.
 *
 * Conventions (those of fastmax_hip_block.h): every matrix operand is (M rows, N columns) with a row stride in ELEMENTS and unit
 * stride along the row; `dtype` (FASTMAX_F32 / BF16 / F16) is the activation dtype, `param_dtype` (that of scale and bias, N
 * elements each) is `dtype` or FASTMAX_F32; arithmetic is float32; every kernel runs on `stream`, nothing synchronises with the
 * host, there are no atomics and every reduction has a fixed order, so all results are bitwise reproducible.  Rows whose length,
 * stride and addresses (the parameters' and the partial sums' too) are whole 16-byte pieces move as 16-byte accesses; anything
 * else with N >= 1 takes a scalar path, and both paths give the same bits.  Every rejection happens before anything is launched:
 * FASTMAX_E_NULL for a missing required pointer (backward: also for one of dscale / dbias without the other, for a call that
 * asks for nothing -- dz, dscale and dbias all NULL -- and for a missing workspace when the sums are wanted),
 * FASTMAX_E_BAD_DTYPE for a dtype outside the enum or a param_dtype that is neither `dtype` nor FASTMAX_F32, FASTMAX_E_BAD_SHAPE
 * for M <= 0, N <= 0, a row stride shorter than the row or M, N so large that the grid does not fit, FASTMAX_E_ALIGNMENT for a
 * matrix or parameter pointer not aligned to its element, a dscale / dbias pointer that is not 4-byte aligned or a workspace
 * that is not 16-byte aligned, FASTMAX_E_WORKSPACE for a workspace smaller than the query function's answer.
 *
 * Rounding points (what torch does with the reference's expression; round = to `dtype`):
 *   adapter_forward, z -> y:
 *       param_dtype == dtype:            t = round(z + bias),  y = round(scale * t),  y has `dtype`
 *       float32 parameters, 16-bit z:    t = float(z) + bias,  y = scale * t,         y is float32 (torch's promotion)
 *       Two operations, two results: nothing is contracted across them.
 *   adapter_backward, (dy, z) -> (dz, dscale, dbias); dy has y's dtype:
 *       dz = round(dy * scale)           one product rounded once; dz (`dtype`) may be NULL
 *       dscale[n] = sum_m dy[m,n] t[m,n] t recomputed from z and bias with the forward's rounding (never y / scale: a zero
 *                                        scale is legal)
 *       dbias[n]  = sum_m dy[m,n] scale[n]
 *       Both sums are N floats, float32 sums of the unrounded float32 products.  They may be NULL together, and then no
 *       workspace is needed and nothing but dz is written.  A workgroup walks a fixed block of
 *       FASTMAX_ADAPTER_ROWS_PER_BLOCK rows (wave w of its four takes rows w, w + 4, ... in order; the four sums are added in
 *       wave order) and leaves one partial row per sum in the workspace, laid out (row blocks, 2, N); a second kernel adds the
 *       partial rows per column in block order.  One pass over dy and z.
 *   adapter_backward_workspace: ceil(M / FASTMAX_ADAPTER_ROWS_PER_BLOCK) * 2 * N * 4 bytes, or 0 when want_param_grads == 0
 *       (or the shape or dtype is one the backward rejects). */
#ifndef FASTMAX_HIP_ADAPTER_H
#define FASTMAX_HIP_ADAPTER_H

#include "fastmax_hip.h"

#define FASTMAX_ADAPTER_ROWS_PER_BLOCK 64

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_adapter_forward(const void* z, int64_t z_stride, const void* scale, const void* bias, void* y, int64_t y_stride,
                                int M, int N, int dtype, int param_dtype, void* stream);
size_t fastmax_hip_adapter_backward_workspace(int M, int N, int dtype, int want_param_grads);
int fastmax_hip_adapter_backward(const void* dy, int64_t dy_stride, const void* z, int64_t z_stride, const void* scale,
                                 const void* bias, void* dz, int64_t dz_stride, float* dscale, float* dbias, int M, int N,
                                 int dtype, int param_dtype, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_ADAPTER_H */
