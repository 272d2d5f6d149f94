/* fastmax_hip_kv_fp8.h -- the softmax KV-cache decode of libfastmax_hip.so on a cache whose K and V rows are stored in 8 bits
 * (MI355X / gfx950 only; csrc/softmax_kv_fp8.hip): OCP e4m3 codes with one power-of-two float32 scale per row, 2 D + 8 bytes per
 * cached position and KV head where the 16-bit cache of fastmax_hip_kv_decode.h takes 4 D.  q and o are bf16 or fp16.
 * The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION
 * (additions only) and are bound by their rows of ABI_EXT4 in fastmax_experiments_amd/_lib.py.  Everything runs on `stream`;
 * nothing is allocated, nothing is read back, there are no atomics, and every sum has a fixed order: two calls give the same bits.
 *
 *   the state     fastmax_hip_kv_fp8_state_bytes(B, Hkv, D, max_len) bytes of device memory, 16-byte aligned:
 *                     bytes 0 .. 63     the header of fastmax_hip_kv_decode.h (word 0 len, word 1 the sticky overflow flag);
 *                                       fastmax_hip_kv_decode_set_len serves this state as it is
 *                     then the K codes  (B * Hkv, cap, D) bytes, cap = max_len rounded up to a whole FASTMAX_KV_CHUNK
 *                     then the V codes  (B * Hkv, cap, D) bytes
 *                     then the K scales (B * Hkv, cap) float32
 *                     then the V scales (B * Hkv, cap) float32
 *                 each array on a 16-byte boundary (cap is a multiple of 128).  0 for a shape the route does not take: B, Hkv, D
 *                 or max_len <= 0, D not a multiple of 16 or above FASTMAX_KV_MAX_D, B * Hkv above 65535.
 *
 *   a row         the D values of one (b, g, position), of K or of V, quantised on its own, in float32:
 *                     amax = max |x|;  s = 2^e, e the smallest integer with amax <= 448 * 2^e: from frexp(amax) = (m, x),
 *                     e = x - 9 if m <= 0.875, else x - 8, clamped to -126 .. 127; amax = 0 gives s = 1
 *                     code = x / s rounded to nearest-even into e4m3 (OCP: 4 exponent bits, 3 mantissa bits, no infinity)
 *                 The division is exact and no quotient exceeds 448, so a row has one correct byte pattern; code * s is exact
 *                 in float32, and a code is exact as a bf16 or fp16 matrix operand.
 *
 *   load          rows 0 .. T-1 of an EMPTY cache = the quantised k, v (B, Hkv, T, D), then len = T: the prompt, whose own
 *                 outputs come from the masked forward.  The kernel does not read the header.  One launch, the append kernel.
 *
 *   append_attend T >= 1 new tokens, the arguments and the three kinds of launch of fastmax_hip_softmax_kv_append_attend
 *                 (fastmax_hip_softmax.h).  With n_i = len + i, Kq_j = kcode_j * kscale_j and Vq_j likewise:
 *                     cache row n_i of (b, g) = the quantised k[b, g, i], v[b, g, i]
 *                     o[b, h, i] = sum_{j <= n_i} softmax_j(scale * q[b, h, i] . Kq_j) Vq_j       o (B, H, T, D) contiguous
 *                     lse[b, h, i] (B, H, T) float32, when lse is not NULL
 *                 The codes are widened to 16-bit matrix operands in registers (exactly); a key's K scale multiplies its float32
 *                 score, its V scale multiplies its exponential before that is rounded to 16 bits as the operand of the product
 *                 with the V codes.  Positions past n_i are kept out by selection: neither their codes nor their scale words
 *                 reach a product.  A row's bits depend on its q row and the cache prefix 0 .. n_i alone: not on B, the batch
 *                 row, T, max_len, the inputs' strides or eager / replayed.
 *                 Guard: len < 0 or len + T > max_len.  Then append writes nothing, combine writes o = 0 (lse = 0), len is left
 *                 alone and overflow = 1.
 *   workspace     bytes of workspace append_attend needs: B * H * min(T, FASTMAX_KV_SLICE) * ((cap / FASTMAX_KV_CHUNK) *
 *                 (D + 2) + 2) * 4; 0 for a shape it rejects.
 *
 * Every rejection happens before anything is launched, in this order: FASTMAX_E_NULL (a missing pointer, strides included; lse
 * may be NULL), FASTMAX_E_BAD_DTYPE (anything but FASTMAX_BF16 / FASTMAX_F16), FASTMAX_E_BAD_SHAPE (a shape whose state_bytes is
 * 0, T <= 0, T > max_len in load, H <= 0, H % Hkv != 0, B * H above 65535, a scale that is not finite), FASTMAX_E_ALIGNMENT (q, k,
 * v, o, the state or the workspace not 16-byte aligned, a stride that is not a whole number of 16-byte pieces, lse not 4-byte
 * aligned), FASTMAX_E_WORKSPACE (smaller than workspace's answer). */
#ifndef FASTMAX_HIP_KV_FP8_H
#define FASTMAX_HIP_KV_FP8_H

#include "fastmax_hip.h"
#include "fastmax_hip_kv_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fastmax_hip_kv_fp8_state_bytes(int B, int Hkv, int D, int max_len);
int fastmax_hip_kv_fp8_load(const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides, void* state, int B,
                            int Hkv, int T, int D, int max_len, int dtype, void* stream);
size_t fastmax_hip_kv_fp8_workspace(int B, int H, int Hkv, int T, int D, int max_len);
int fastmax_hip_softmax_kv_fp8_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                             const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B, int H,
                                             int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                             size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_KV_FP8_H */
