/* fastmax_hip_softmax_block.h -- the many-tokens-at-once route onto the softmax KV cache in libfastmax_hip.so (MI355X / gfx950
 * only; csrc/softmax_kv_block.hip): a second chat turn, a prompt fed in pieces, a block of draft tokens.  bf16 and fp16.
 * The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION
 * (additions only) and are bound by their rows of ABI_EXT5 in fastmax_experiments_amd/_lib.py.  Everything runs on `stream`;
 * nothing is allocated, nothing is read back (len is read from the device header only), there are no atomics, every sum has a
 * fixed order, and the call records into a graph.
 *
 *   kv_append_attend_block   the contract of fastmax_hip_softmax_kv_append_attend (fastmax_hip_softmax.h), on the same cache
 *                 (fastmax_hip_kv_decode.h: header, rows, capacity; its state_bytes, load and set_len serve this route as they
 *                 are).  T >= 1 new tokens, any len >= 0.  With n_i = len + i:
 *                     cache row n_i of (b, g) = k[b, g, i], v[b, g, i]                        exact copies
 *                     o[b, h, i] = sum_{j <= n_i} softmax_j(scale * q[b, h, i] . K_j) V_j      o (B, H, T, D) contiguous
 *                     lse[b, h, i] (B, H, T) float32, when lse is not NULL
 *                 Head sizes are multiples of 8 in 8 .. 256.  Scores, maximum, row sum and accumulator are float32; scale * log2 e
 *                 multiplies the float32 score; P is rounded to `dtype` once, as a matrix operand.
 *                 What differs from kv_append_attend is the work split, made for T = 16 .. 512 where that one is made for T = 1:
 *                     rows      the query rows of a KV group (b, g) are the T * (H / Hkv) (token, head) pairs, token-major; a
 *                               workgroup takes FASTMAX_KV_BLOCK_ROWS of them (FASTMAX_KV_BLOCK_ROWS_D256 for head sizes above
 *                               128), each with its own bound n_i, so one read of a K/V chunk serves all of them.
 *                     keys      a workgroup walks a span of FASTMAX_KV_BLOCK_SPAN consecutive chunks of FASTMAX_KV_CHUNK
 *                               positions with a running maximum per row (the online-softmax rescale) and leaves one partial
 *                               (m, l, D numerator floats) per row and span in the workspace; span 0's workgroups also leave each
 *                               row's number of spans there (0: the guard fired).  Span s is the ABSOLUTE positions
 *                               [s * SPAN * CHUNK, (s + 1) * SPAN * CHUNK), whatever len and T are.  The grid comes from cap; a
 *                               workgroup stops at the largest n_i of its rows and exits if its span starts beyond it.
 *                     combine   the combine kernel of kv_append_attend over the spans of a row in ascending order, rescaled to
 *                               their common maximum; one thread of the call's last combine launch advances len by T (or sets
 *                               overflow): the call's only header write.
 *                     append (cache rows only, first) is kv_append_attend's own kernel.  Attend and combine repeat per slice of
 *                     FASTMAX_KV_BLOCK_TOKENS new tokens, which bounds the workspace.
 *                 Positions past n_i are kept out by selection (their scores are -inf before the exponential, V pieces past the
 *                 workgroup's largest n_i are written as zeros), so a truncated cache may hold anything there, NaN included;
 *                 nothing at or past the capacity is read.  A chunk or span with no live position for a row leaves that row's
 *                 (m, l, numerator) bit for bit as they were.
 *                 A row's bits depend on its q row and the cache prefix 0 .. n_i alone: not on B, the batch row, T or how a run of
 *                 tokens is cut into calls, the row's place among a workgroup's rows, max_len, the inputs' strides or eager /
 *                 replayed.  They are NOT the bits of kv_append_attend: the sums are taken in another order (per span with a
 *                 running maximum, then over spans; there per chunk, then over chunks).
 *                 Guard: len < 0 or len + T > max_len.  Then append writes nothing, combine writes o = 0 (lse = 0), len is left
 *                 alone and overflow = 1.
 *   kv_block_workspace   bytes of workspace kv_append_attend_block needs:
 *                     B * H * min(T, FASTMAX_KV_BLOCK_TOKENS) * (nspan * (D + 2) + 1) * 4,
 *                     nspan = ceil(cap / FASTMAX_KV_CHUNK / FASTMAX_KV_BLOCK_SPAN), cap = max_len up to a whole chunk;
 *                 0 for a shape it rejects.
 *
 * Every rejection happens before anything is launched, in the order of fastmax_hip_softmax.h: FASTMAX_E_NULL (a missing pointer,
 * strides included; lse may be NULL), FASTMAX_E_BAD_DTYPE (anything but FASTMAX_BF16 / FASTMAX_F16), FASTMAX_E_BAD_SHAPE (a head
 * size that is not a multiple of 8 in 8 .. 256, a count <= 0, H % Hkv != 0, B * H above 65535, H / Hkv above 16383, a shape whose state_bytes is 0, a
 * scale that is not finite), FASTMAX_E_ALIGNMENT (q, k, v, o, the state or the workspace not 16-byte aligned, a stride that is not
 * a whole number of 16-byte pieces, lse not 4-byte aligned), FASTMAX_E_WORKSPACE (smaller than kv_block_workspace's answer). */
#ifndef FASTMAX_HIP_SOFTMAX_BLOCK_H
#define FASTMAX_HIP_SOFTMAX_BLOCK_H

#include "fastmax_hip.h"
#include "fastmax_hip_kv_decode.h"

#define FASTMAX_KV_BLOCK_ROWS 64
#define FASTMAX_KV_BLOCK_ROWS_D256 16
#define FASTMAX_KV_BLOCK_SPAN 4
#define FASTMAX_KV_BLOCK_TOKENS 64

#ifdef __cplusplus
extern "C" {
#endif

size_t fastmax_hip_softmax_kv_block_workspace(int B, int H, int Hkv, int T, int D, int max_len);
int fastmax_hip_softmax_kv_append_attend_block(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                               const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B,
                                               int H, int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_SOFTMAX_BLOCK_H */
