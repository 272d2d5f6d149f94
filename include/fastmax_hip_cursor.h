/* fastmax_hip_cursor.h -- the decode cursor of libfastmax_hip.so (MI355X / gfx950 only; csrc/decode_cursor.hip): what changes from
 * one generated token to the next -- the position fed, the draw number, the column that receives the token -- kept in device
 * memory, so that a whole decode step (feed -> blocks -> head -> sample) takes the same arguments every token and one recorded
 * graph generates a token per replay.  The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same
 * library and FASTMAX_ABI_VERSION and are bound by the table ABI in fastmax_experiments_amd/_lib.py.  Everything runs on
 * `stream`; nothing is allocated, nothing is read back, there are no atomics.
 *
 *   the cursor    fastmax_hip_cursor_bytes() bytes of device memory (a multiple of 8, 8-byte aligned), read as int64 words:
 *                     word 0  pos        the position of the next token to feed (>= 0)
 *                     word 1  next       pos + 1 as the last feed left it, or -1: nothing fed, nothing to sample
 *                     word 2  draw_base  the sampler's draw number is draw_base + next (64-bit wrap-around, read as a bit pattern)
 *                     word 3  seed       the sampler's seed (bit pattern)
 *                     word 4  overflow   0, or 1 once any guard below has fired; no kernel ever clears it
 *                     the rest           reserved, zero
 *                 The host arms it with one small copy before a run: {pos, -1, draw - (pos + 1), seed, 0, ...} makes `draw` the
 *                 number of the first draw.  A step is feed, then whatever turns x into logits, then sample_cursor.  Within one
 *                 launch no word is read by one workgroup and written by another: feed reads `pos` and writes `next`,
 *                 sample_cursor reads `next`, `draw_base` and `seed` and writes `pos` = next; `overflow` is only ever written.
 *                 Every writer of a word stores the same value.
 *
 *   cursor_feed   the start of a step.  With p = pos:
 *                     x[b, :]    = wte[tok[b], :]   b < B, C elements of `dtype`; row strides ldw >= C and ldx >= C (elements)
 *                     cos_row[:] = cos[p, :n_cols], sin_row[:] = sin[p, :n_cols]   `rope_dtype`, row stride ld_rope >= n_cols
 *                     next       = p + 1
 *                 A copy: nothing is rounded.  Rows move as 16-byte pieces where the row's length in bytes, both addresses and
 *                 both row strides are multiples of 16 (decided separately for the embedding and for the rope rows), element by
 *                 element otherwise: equal bits either way.  Guards, none of which touches memory outside its operands:
 *                     p < 0 or p >= n_rope_rows:  nothing is written but next = -1 and overflow = 1.  The sample_cursor that
 *                         follows then writes nothing either and the cursor stays where it is: a replay too many is a no-op.
 *                     tok[b] outside [0, n_wte_rows):  x[b, :] = 0 and overflow = 1; the step goes on.
 *
 *   sample_cursor the end of a step: fastmax_hip_sample (fastmax_hip_next_token.h: same filter, same scores, same kernel
 *                 template) with seed = word 3 and draw = draw_base + next, so a (seed, draw) pair gives the token
 *                 fastmax_hip_sample gives.  With n = next, row b's token goes to tok[b] and to out[b * ldo + n] (out: (B, L)
 *                 int64, row stride ldo >= L); with eos_id >= 0, done[b] (uint8) becomes 1 if the token equals eos_id and is left
 *                 alone otherwise; then pos = n.  n < 0 (the feed refused) or n >= L: nothing is written but overflow = 1.
 *                 `done` may be NULL when eos_id < 0.
 *
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing pointer, FASTMAX_E_BAD_DTYPE for a dtype or
 * rope_dtype outside the enum, FASTMAX_E_BAD_SHAPE for B, C, V, L, n_cols, n_wte_rows or n_rope_rows <= 0, C or V above 2^30, a
 * row stride below its row's length, top_k < 0, or a temperature that is negative or not finite, FASTMAX_E_ALIGNMENT for a
 * pointer that is not aligned to its element (the cursor, tok and out: 8 bytes). */
#ifndef FASTMAX_HIP_CURSOR_H
#define FASTMAX_HIP_CURSOR_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fastmax_cursor_word {
    FASTMAX_CURSOR_POS = 0,
    FASTMAX_CURSOR_NEXT = 1,
    FASTMAX_CURSOR_DRAW_BASE = 2,
    FASTMAX_CURSOR_SEED = 3,
    FASTMAX_CURSOR_OVERFLOW = 4,
    FASTMAX_CURSOR_WORDS = 8
};

size_t fastmax_hip_cursor_bytes(void);
int fastmax_hip_cursor_feed(void* cursor, const int64_t* tok, const void* wte, int64_t ldw, int64_t n_wte_rows, void* x, int64_t ldx,
                            int B, int C, int dtype, const void* cos, const void* sin, int64_t ld_rope, int64_t n_rope_rows,
                            void* cos_row, void* sin_row, int n_cols, int rope_dtype, void* stream);
int fastmax_hip_sample_cursor(const float* logits, int64_t ld, void* cursor, int64_t* tok, int64_t* out, int64_t ldo, int64_t L,
                              void* done, int64_t eos_id, int B, int V, int top_k, float temperature, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_CURSOR_H */
