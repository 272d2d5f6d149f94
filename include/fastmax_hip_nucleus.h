/* fastmax_hip_nucleus.h -- top-p (nucleus) sampling in libfastmax_hip.so (MI355X / gfx950 only; csrc/next_token_sample.h,
 * csrc/next_token.hip, csrc/decode_cursor.hip): the filter behind the exact top-k of fastmax_hip_next_token.h, inside the same
 * sampler kernel.  The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and
 * FASTMAX_ABI_VERSION and are bound by the table ABI in fastmax_experiments_amd/_lib.py.  Everything runs on `stream`;
 * nothing is allocated, nothing is read back, there are no float atomics.
 *
 * Terms, for one row of float32 logits:
 *     the order    by key descending, index ascending among equal keys; the key of a value is order-preserving and -0.0 and +0.0
 *                  share one (the order of topk_mask, fastmax_hip_next_token.h)
 *     K            the candidates: the first top_k entries of the order (topk_mask's rule), all V for top_k = 0 or top_k >= V
 *     z_i          logit_i / temperature, temperature as the float32 received
 *     P_i          exp(z_i - max_K z) / sum_K exp(z - max_K z)
 *     C(j)         the sum of P over the first j candidates; C(0) = 0
 *
 * Rules:
 *     nucleus      the first n candidates, n = min{ j >= 1 : C(j) >= top_p }, top_p as the float32 received: the smallest set whose
 *                  mass reaches top_p, at least one token, applied after temperature and top-k.  The kept set is therefore
 *                  "key above a threshold, or equal to it with index <= a limit", like the top-k's.
 *     ties         among candidates equal to the crossing value the lowest indices are kept until the mass reaches top_p.
 *     draw         unchanged: the argmax of z_i + g_i over the kept set, g_i = -log(-log u_i), u_i from Philox-4x32-10 at counter
 *                  (i / 4, b, draw_lo, draw_hi) under key (seed_lo, seed_hi), lowest index on ties.  A (seed, draw) pair gives the
 *                  token of fastmax_hip_sample / fastmax_hip_sample_cursor whenever the nucleus keeps all of K.
 *     switches     top_p == 1 keeps all of K.  temperature == 0 is the argmax and top_p is ignored (nucleus_mask is then
 *                  topk_mask).
 *     outside      a row that holds a NaN or whose largest candidate is an infinity is outside the contract; the token still lies
 *                  in [0, V).
 *
 * How C(j) is evaluated (one workgroup of 1024 threads per row; the kept set is a function of the row's bits, V, top_k, top_p and
 * temperature alone -- not of the batch, the row stride, the alignment or the call):
 *     weight       w_i = expf((logit_i - m) / temperature) in float32, m the row's largest value; 0 <= w_i <= 1
 *     format       q_i = floor(w_i 2^40), an unsigned 64-bit integer (24.40 fixed point); sums of q are 64-bit integer sums, in any
 *                  order the same
 *     target       with total = sum_K q:  needed = ceil(total * top_p), the product taken in float64 (relative error 2^-52), clamped
 *                  to [1, total];  n = min{ j : sum of q over the first j candidates >= needed }
 *     largest V    2^22 = 4194304 (total <= 2^62)
 *     error        |C(j) as evaluated - C(j)| <= 2 (2^-23 ln V + 2^-22 + V 2^-40): the argument of expf carries two roundings
 *                  (relative 2^-23 of |x_i|, and sum_K P_i |x_i| <= ln V), expf at most 2 ulp, the truncation 2^-40 per entry
 *                  against a total >= 2^40; the factor 2 covers numerator and denominator.  3.2e-6 at V = 50304.
 *
 *   sample_nucleus         fastmax_hip_sample with the nucleus behind the top-k: tokens[b] (int64) from row b of logits (B, V),
 *                          row stride ld >= V.
 *   nucleus_mask           mask[b, v] = 1 where entry v of row b is in the kept set, else 0 (uint8, row stride ldm >= V): what
 *                          sample_nucleus chooses among under the same top_k, top_p and temperature.
 *   sample_cursor_nucleus  fastmax_hip_sample_cursor (fastmax_hip_cursor.h: stream, guards and stores of the decode cursor) with
 *                          the nucleus behind the top-k.
 *
 * Every rejection happens before anything is launched: those of fastmax_hip_sample, fastmax_hip_topk_mask and
 * fastmax_hip_sample_cursor with the same codes, and FASTMAX_E_BAD_SHAPE for V above 2^22, for a top_p that is NaN or outside
 * (0, 1], and for a nucleus_mask temperature that is negative or not finite. */
#ifndef FASTMAX_HIP_NUCLEUS_H
#define FASTMAX_HIP_NUCLEUS_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_sample_nucleus(const float* logits, int64_t ld, int64_t* tokens, int B, int V, int top_k, float top_p,
                               float temperature, int64_t seed, int64_t draw, void* stream);
int fastmax_hip_nucleus_mask(const float* logits, int64_t ld, void* mask, int64_t ldm, int B, int V, int top_k, float top_p,
                             float temperature, void* stream);
int fastmax_hip_sample_cursor_nucleus(const float* logits, int64_t ld, void* cursor, int64_t* tok, int64_t* out, int64_t ldo, int64_t L,
                                      void* done, int64_t eos_id, int B, int V, int top_k, float temperature, float top_p,
                                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_NUCLEUS_H */
