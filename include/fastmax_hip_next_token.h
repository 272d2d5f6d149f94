/* fastmax_hip_next_token.h -- from a hidden state to the next token in libfastmax_hip.so (MI355X / gfx950 only;
 * csrc/last_logits.hip for the logits, csrc/next_token.hip for the rest): the lm-head over the LAST position only, an exact top-k filter and a seeded sampler that leaves its
 * token in device memory.  The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library
 * and FASTMAX_ABI_VERSION and are bound by the table ABI in fastmax_experiments_amd/_lib.py.  Everything runs on
 * `stream`; nothing is allocated, nothing is read back, there are no float atomics.
 *
 *   last_logits   logits[b, v] = sum_c x[b, c] W[v, c], accumulated in float32.
 *                 x: B rows of C elements, unit stride along a row, ANY row stride ldx (elements): the last position of a
 *                 (B, T, C) tensor is passed as a view.  W: (V, C), row stride ldw >= C.  x and W share `dtype`
 *                 (FASTMAX_F32 / BF16 / F16); `out_dtype` is FASTMAX_F32 or `dtype`; logits: (B, V), row stride ldo >= V.
 *                 One wave owns four rows of W and reads them once for a group of up to 8 rows of x; a larger B is further
 *                 passes over W.  A row is cut into pieces of 16 bytes (4 float32 / 8 sixteen-bit elements; the last piece may
 *                 be short); lane l of the wave takes pieces l, l + 64, ... and adds their products in index order with one
 *                 fused multiply-add each, starting from +0; the 64 lanes are then added by an xor butterfly.  That order
 *                 depends on C and the dtype alone: a row's logits have the same bits alone or inside any batch, and whether
 *                 the pieces move as 16-byte loads (C a whole number of pieces, both base addresses and both row strides on
 *                 16-byte boundaries) or element by element.
 *
 *   topk_mask     mask[b, v] = 1 where entry v of row b survives the top-k filter, else 0 (uint8, row stride ldm >= V).
 *                 top_k = 0 or top_k >= V: no filter, all ones.  Otherwise EXACTLY top_k entries survive: those greater than
 *                 the k-th largest value, and of those equal to it the lowest indices until k are kept.  -0.0 and +0.0 compare
 *                 equal; -inf is an ordinary value.  (torch.topk leaves ties unspecified; this rule is the library's.)
 *
 *   sample        tokens[b] (int64, device memory) from row b of float32 logits (B, V), row stride ld >= V:
 *                     temperature == 0:  the kept entry with the largest logit, lowest index on ties;
 *                     temperature  > 0:  argmax over kept entries of logit_i / temperature + g_i, lowest index on ties, with
 *                                        g_i = -log(-log u_i): distributed as multinomial(softmax(logits / temperature)).
 *                 u_i = ((word >> 9) + 0.5) * 2^-23, exact in float32 and never 0 or 1, where `word` is word i % 4 of
 *                 Philox-4x32-10 at counter (i / 4, b, draw_lo, draw_hi) under key (seed_lo, seed_hi); lo / hi are the two
 *                 32-bit halves of the 64-bit host arguments `draw` and `seed` (passed as int64_t, read as bit patterns).
 *                 One workgroup per row.  NaN logits are outside the contract; the token still lies in [0, V).
 *
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing pointer, FASTMAX_E_BAD_DTYPE for a dtype
 * outside the enum or an out_dtype that is neither FASTMAX_F32 nor dtype, FASTMAX_E_BAD_SHAPE for B, V or C <= 0, C above 2^30
 * (last_logits) or V above 2^30 (topk_mask, sample), a row stride of W, the logits or the mask below its row's length, ldx < 0,
 * top_k < 0, or a temperature that is negative or not finite, FASTMAX_E_ALIGNMENT for a pointer that is not aligned to its
 * element. */
#ifndef FASTMAX_HIP_NEXT_TOKEN_H
#define FASTMAX_HIP_NEXT_TOKEN_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_last_logits(const void* x, int64_t ldx, const void* w, int64_t ldw, void* logits, int64_t ldo, int B, int V, int C,
                            int dtype, int out_dtype, void* stream);
int fastmax_hip_sample(const float* logits, int64_t ld, int64_t* tokens, int B, int V, int top_k, float temperature, int64_t seed,
                       int64_t draw, void* stream);
int fastmax_hip_topk_mask(const float* logits, int64_t ld, void* mask, int64_t ldm, int B, int V, int top_k, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_NEXT_TOKEN_H */
