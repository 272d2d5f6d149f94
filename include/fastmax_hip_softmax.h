/* fastmax_hip_softmax.h -- softmax ("quadratic") attention in libfastmax_hip.so (MI355X / gfx950 only): the causal prefill on the
 * matrix cores (csrc/softmax_attention.hip), its backward (csrc/softmax_attention_bwd.hip) and the KV-cache decode
 * (csrc/softmax_kv_decode.hip).  bf16 and fp16.
 * The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION
 * (additions only) and are bound by their rows of ABI_EXT in fastmax_experiments_amd/_lib.py.  Everything runs on `stream`;
 * nothing is allocated, nothing is read back, there are no atomics, and every sum has a fixed order: two calls give the same bits.
 *
 *   forward       o[b, h, i] = sum_{j <= i} softmax_j(scale * q[b, h, i] . k[b, g, j]) v[b, g, j],   g = h / (H / Hkv)
 *                 q (B, H, N, D); k, v (B, Hkv, N, D) at their KV heads; each with its three element strides (batch, head, row)
 *                 and unit stride along D; o (B, H, N, D) contiguous, in `dtype`; lse (B, H, N) float32 contiguous or NULL:
 *                 lse[b, h, i] = log sum_{j <= i} exp(scale * s_ij).  Any N >= 1; D a multiple of 8 in 8 .. 256.  Scores, the row
 *                 maximum, the row sum and the output accumulator are float32; `scale` multiplies the float32 scores; the
 *                 exponentials are rounded to `dtype` once, as the operand of the product with V.
 *
 *   kv_append_attend   T >= 1 new tokens onto a cache of include/fastmax_hip_kv_decode.h (the same state, header words and
 *                 capacity; its state_bytes, load and set_len serve this route as they are).  With n_i = len + i:
 *                     cache row n_i of (b, g) = k[b, g, i], v[b, g, i]                        exact copies
 *                     o[b, h, i] = sum_{j <= n_i} softmax_j(scale * q[b, h, i] . K_j) V_j      o (B, H, T, D) contiguous
 *                     lse[b, h, i] (B, H, T) float32, when lse is not NULL
 *                 in three kinds of launch: append (cache rows only); attend, one workgroup per (chunk of FASTMAX_KV_CHUNK
 *                 positions, b, g, new token, block of up to 16 query heads), which leaves (m, l, D numerator floats) per query
 *                 head and chunk in the workspace, and for chunk 0 the number of chunks of the row (0: the guard fired); combine,
 *                 which merges the chunk partials in ascending chunk order, rescaled to their common maximum, writes o and lse
 *                 and -- one thread of the call's last combine launch, the only reader of the header in that launch -- advances
 *                 len by T.  Attend and combine repeat per slice of FASTMAX_KV_SLICE new tokens.
 *                 Positions past n_i are kept out by selection (their scores are -inf before the exponential, their V pieces
 *                 are zero), so a truncated cache may hold anything there; nothing at or past the capacity is read.
 *                 A row's bits depend on its q row and the cache prefix 0 .. n_i alone: not on B, the batch row, T, max_len,
 *                 the inputs' strides or eager / replayed.
 *                 Guard: len < 0 or len + T > max_len.  Then append writes nothing, combine writes o = 0 (lse = 0), len is left
 *                 alone and overflow = 1.
 *   kv_workspace  bytes of workspace kv_append_attend needs: B * H * min(T, FASTMAX_KV_SLICE) * ((cap / FASTMAX_KV_CHUNK) *
 *                 (D + 2) + 2) * 4; 0 for a shape it rejects.
 *
 *   backward      from the forward's q, k, v, o and lse (required here) and grad_o (B, H, N, D) through its own three strides (a
 *                 transposed view is not copied), with c = scale log2 e, L_i = lse[b, h, i], r = H / Hkv, for j <= i:
 *                     P_ij  = exp2(c s_ij - L_i log2 e)        s_ij = q_i . k_j, float32 on the matrix cores, never stored
 *                     D_i   = sum_c grad_o_ic o_ic             float32, from the forward's own (rounded) o
 *                     dS_ij = P_ij (grad_o_i . v_j - D_i)
 *                     dq_i  = scale sum_{j <= i} dS_ij k_j
 *                     dk_j  = scale sum_{h in group} sum_{i >= j} dS_ij q_i        dv_j = sum_{h in group} sum_{i >= j} P_ij grad_o_i
 *                 dq (B, H, N, D); dk, dv (B, Hkv, N, D): contiguous, in `dtype`.  Any N >= 1; D a multiple of 8 in 8 .. 128.  Two
 *                 tile kernels, each recomputing S and grad_o V^T: dq per (b, h, 128 query rows) over the key tiles in ascending
 *                 order, which also leaves D_i in the workspace; then dk and dv per (b, KV head, 128 keys) over the group's query
 *                 heads in ascending order and, within a head, the query tiles in ascending order.  P and dS are rounded to
 *                 `dtype` once, as matrix operands; all three sums are float32 in that one order and are rounded once, after
 *                 the sum over the group's heads: no atomics, two calls give the same bits.
 *   backward_workspace   bytes of workspace backward needs: B * H * N * 4; 0 for a shape it rejects.
 *
 * Every rejection happens before anything is launched, in this order: FASTMAX_E_NULL (a missing pointer, strides included; lse
 * may be NULL except for backward, whose workspace is required too), FASTMAX_E_BAD_DTYPE (anything but FASTMAX_BF16 / FASTMAX_F16), FASTMAX_E_BAD_SHAPE (a head size that is not a
 * multiple of 8 in 8 .. 256 -- backward: 8 .. 128 --, a count <= 0, H % Hkv != 0, B * H or B * Hkv above 65535, a shape whose state_bytes is 0, a scale
 * that is not finite), FASTMAX_E_ALIGNMENT (q, k, v, o, grad_o, dq, dk, dv or the state not 16-byte aligned, a stride that is not a whole number of
 * 16-byte pieces, lse not 4-byte aligned), FASTMAX_E_WORKSPACE (smaller than kv_workspace's or
 * backward_workspace's answer). */
#ifndef FASTMAX_HIP_SOFTMAX_H
#define FASTMAX_HIP_SOFTMAX_H

#include "fastmax_hip.h"
#include "fastmax_hip_kv_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_softmax_forward(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                const int64_t* v_strides, void* o, float* lse, int B, int H, int Hkv, int N, int D, int dtype,
                                float scale, void* stream);
size_t fastmax_hip_softmax_kv_workspace(int B, int H, int Hkv, int T, int D, int max_len);
int fastmax_hip_softmax_kv_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                         const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B, int H,
                                         int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                         size_t workspace_bytes, void* stream);
size_t fastmax_hip_softmax_backward_workspace(int B, int H, int N, int D);
int fastmax_hip_softmax_backward(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                 const int64_t* v_strides, const void* o, const float* lse, const void* grad_o,
                                 const int64_t* go_strides, void* dq, void* dk, void* dv, int B, int H, int Hkv, int N, int D, int dtype,
                                 float scale, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_SOFTMAX_H */
