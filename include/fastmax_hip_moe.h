/* fastmax_hip_moe.h -- the mixture-of-experts MLP's routing, token dispatch and combine in libfastmax_hip.so (MI355X / gfx950
 * only; csrc/moe.hip): what lit_gpt/model.py:644-674 (LLaMAMoE) does around its expert MLPs with a topk, a softmax, a boolean
 * mask and, per expert, a torch.where, two gathers and an indexed read-modify-write.  The dtype and error enums are those of
 * fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION (additions only) and are bound by the
 * table ABI in fastmax_experiments_amd/_lib.py.
 *
 * Notation: M tokens (rows), E experts, k experts per token, S = M k slots, C = n_embd; `dtype` (FASTMAX_F32 / BF16 / F16) is
 * the activation dtype dt.  Limits: 1 <= k <= 8, k <= E <= 64, S < 2^31, M >= 1, C >= 1.
 *
 * Conventions (those of fastmax_hip_block.h): a matrix operand of E or C columns (router, drouter, x, xs, ys, y, dy, dys, dxs,
 * dx) has a row stride in ELEMENTS of its own and unit stride along the row; the per-slot arrays expert, prob, prob32, slot_of,
 * dprob (M, k), row_of (S) and offsets (E + 1) are dense.  Arithmetic is float32 unless said otherwise; every kernel runs on
 * `stream`, allocates nothing and reads nothing back; there are NO atomics and every sum has a fixed order, so all results are
 * bitwise reproducible and do not depend on the launch geometry.  Rows move as 16-byte pieces where the row length, the
 * addresses and the strides of every operand of the call allow it and element by element otherwise, with equal bits either way.
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing pointer, FASTMAX_E_BAD_DTYPE for a dtype
 * outside the enum, FASTMAX_E_BAD_SHAPE for a size outside the limits above or a row stride below its row, FASTMAX_E_ALIGNMENT
 * for a pointer that is not aligned to its element (4 bytes for the int and float arrays) or a workspace that is not 4-byte
 * aligned, FASTMAX_E_WORKSPACE for a workspace smaller than moe_route_workspace's answer.
 *
 *   moe_route: per row of router (M, E) the k largest entries; ties go to the lowest index and NaN ranks above every number
 *       (as torch.topk ranks it).  A token's k entries are stored in ASCENDING EXPERT ID:
 *         expert (M, k) int     the selected experts
 *         prob32 (M, k) float   softmax over the k selected values (evaluated in double, rounded once to float32: the
 *                               reference's softmax(dim=1, dtype=torch.float))
 *         prob   (M, k) dt      prob32 rounded to dt
 *       and the stable dispatch (a counting sort of the S (token, expert) pairs by expert, tokens ascending -- the order
 *       torch.where yields):
 *         offsets (E + 1) int   expert e owns slots offsets[e] .. offsets[e + 1]
 *         row_of  (S) int       the token of a slot
 *         slot_of (M, k) int    the slot of a token's j-th entry: row_of[slot_of[t][j]] == t
 *       Three launches above 256 tokens (selection with one histogram per 256 tokens and ranks inside them by ballot and
 *       popcount; one scan of the histograms; placement), one launch up to 256.  The workspace holds the histograms.
 *   moe_gather:           xs[s] = x[row_of[s]]  (S, C); a copy, nothing is rounded.
 *   moe_combine:          y[t] = 0; for j ascending: y[t] = round(y[t] + round(prob[t][j] ys[slot_of[t][j]]))  -- the
 *                         reference's rounding points (model.py:670-673), both to dt.
 *   moe_combine_backward: dys[slot_of[t][j]] = round(prob[t][j] dy[t]);  dprob[t][j] = round(sum_c dy[t][c] ys[slot][c])
 *                         (dt; the sum in float32: a thread's columns in order, the lanes of a wave, the four waves in order).
 *                         One read of dy and of ys.
 *   moe_gather_backward:  dx[t] = round(sum_j dxs[slot_of[t][j]]), the sum in float32, j ascending.
 *   moe_route_backward:   g = float(dprob), d = prob32 (g - sum_j prob32 g), rounded to dt and written into drouter (M, E) at the
 *                         selected experts; every other entry of drouter is written as zero. */
#ifndef FASTMAX_HIP_MOE_H
#define FASTMAX_HIP_MOE_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FASTMAX_MOE_MAX_EXPERTS 64
#define FASTMAX_MOE_MAX_PER_TOKEN 8

size_t fastmax_hip_moe_route_workspace(int M, int E);
int fastmax_hip_moe_route(const void* router, int64_t router_stride, int* expert, void* prob, float* prob32, int* offsets,
                          int* row_of, int* slot_of, int M, int E, int k, int dtype, void* workspace, size_t workspace_bytes,
                          void* stream);
int fastmax_hip_moe_gather(const void* x, int64_t x_stride, const int* row_of, void* xs, int64_t xs_stride, int M, int S, int C,
                           int dtype, void* stream);
int fastmax_hip_moe_combine(const void* ys, int64_t ys_stride, const void* prob, const int* slot_of, void* y, int64_t y_stride,
                            int M, int k, int C, int dtype, void* stream);
int fastmax_hip_moe_combine_backward(const void* dy, int64_t dy_stride, const void* ys, int64_t ys_stride, const void* prob,
                                     const int* slot_of, void* dys, int64_t dys_stride, void* dprob, int M, int k, int C,
                                     int dtype, void* stream);
int fastmax_hip_moe_gather_backward(const void* dxs, int64_t dxs_stride, const int* slot_of, void* dx, int64_t dx_stride, int M,
                                    int k, int C, int dtype, void* stream);
int fastmax_hip_moe_route_backward(const void* dprob, const float* prob32, const int* expert, void* drouter,
                                   int64_t drouter_stride, int M, int E, int k, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_MOE_H */
