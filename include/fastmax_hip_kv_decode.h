/* fastmax_hip_kv_decode.h -- the KV-cache decode route of libfastmax_hip.so (MI355X / gfx950 only; csrc/fastmax_kv_decode.hip):
 * masked polynomial attention at each new position over a cache of the K and V rows seen so far, for head sizes 1 .. 256, where
 * the carried-state caches of fastmax_hip.h stop at 128 and move (D+1)(D+2)/2 (D+1) floats per token whatever the length.  The
 * dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION
 * (additions only) and are bound by their rows of the one table ABI in fastmax_experiments_amd/_lib.py.  Everything runs on
 * `stream`; nothing is allocated, nothing is read back, there are no atomics, and every sum has a fixed order.
 *
 *   the state     fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, dtype) bytes of device memory, 16-byte aligned:
 *                     bytes 0 .. 63     the header, FASTMAX_KV_HEADER_WORDS int32 words:
 *                         word 0  len       the number of cached positions, 0 <= len <= max_len
 *                         word 1  overflow  0, or 1 once a guard below has fired; no kernel ever clears it
 *                         the rest          reserved, zero
 *                     then the K cache  (B, Hkv, cap, D) elements of `dtype`, cap = max_len rounded up to a whole
 *                                       FASTMAX_KV_CHUNK, so that slot max_len lies inside the allocation
 *                     then the V cache  the same shape
 *                     (D * cap is a multiple of 128 elements, so both caches start on a 16-byte boundary and the total is a
 *                     multiple of 16.)  0 for a shape or dtype the route does not take: B, Hkv, D or max_len <= 0, D above
 *                     FASTMAX_KV_MAX_D, B * Hkv above 65535 (a grid dimension), a dtype outside the enum.
 *                 An all-zero header is the empty cache.  `max_len` and `dtype` are not stored: every call names them, and the
 *                 caller keeps them the same for the life of a state.
 *
 *   load          rows 0 .. T-1 of both caches = k, v (B, Hkv, T, D), then len = T.  For an EMPTY cache (the prompt, whose own
 *                 outputs come from the masked forward): the kernel does not read the header.  One launch.
 *
 *   append_attend T >= 1 new tokens.  With n_i = len + i the position of new token i (i < T), for every query head h of KV head g:
 *                     cache row n_i of (b, g) = k[b, g, i], v[b, g, i]                   exact copies, nothing is rounded
 *                     s_j  = (q[b, h, i] . K_j) * inv_nt                    j = 0 .. n_i, the new rows included
 *                     f    = 1 + s + s^2 / 2  (p = 2),   1 + s  (p = 1)
 *                     o[b, h, i] = sum_j f(s_j) V_j / sum_j f(s_j)                       float32 sums, o (B, H, T, D) contiguous
 *                 in four kinds of launch, in this order:
 *                     append    reads len; writes the T rows of every (b, g).  Cache rows only: no header word.
 *                     attend    reads len and the caches.  One workgroup per (b, g, chunk of FASTMAX_KV_CHUNK positions,
 *                               new token, block of up to 8 query heads of g): K and V rows of the chunk are loaded once for the
 *                               block of heads; numerator (D floats) and denominator of each head go to the workspace.  The grid
 *                               comes from cap; a workgroup whose chunk starts past n_i exits.  Positions past n_i are never read.
 *                     combine   reads len and the workspace; adds the chunk partials of a row in ascending chunk order, divides,
 *                               writes o in `dtype`.
 *                               (attend and combine repeat per slice of FASTMAX_KV_SLICE new tokens, which bounds the workspace.)
 *                     commit    one thread: reads len, writes len = len + T.  The last kernel of the call and the only writer of
 *                               a header word in it.
 *                 Within one launch no word is read by one workgroup and written by another.  There is no running maximum, so
 *                 the chunk partials simply add.  A row's output bits depend on its q row and on the cache prefix 0 .. n_i alone:
 *                 not on B, on which batch row it is, on T, on max_len or on the inputs' strides.
 *                 Guard: len < 0 or len + T > max_len.  Then append writes nothing, attend exits, combine writes o = 0 and commit
 *                 leaves len alone and sets overflow = 1: a replay too many is a no-op.
 *                 K and V rows move as 16-byte pieces where the row's length in bytes is a multiple of 16 (and, for the input
 *                 rows, the row's address is): element by element otherwise, equal bits either way.
 *
 *   set_len       len = new_len if 0 <= new_len <= len (a truncation: the rows stay, the next append overwrites them); otherwise
 *                 len is left alone and overflow = 1.  One thread.
 *
 *   workspace     fastmax_hip_kv_decode_workspace(B, H, Hkv, T, D, max_len) =
 *                 B * H * min(T, FASTMAX_KV_SLICE) * (cap / FASTMAX_KV_CHUNK) * (D + 1) * 4 bytes, 16-byte aligned; 0 for a shape
 *                 append_attend rejects.
 *
 * Every rejection happens before anything is launched, in this order: FASTMAX_E_NULL for a missing pointer (strides included),
 * FASTMAX_E_BAD_DTYPE for a dtype outside the enum, FASTMAX_E_BAD_P for p outside {1, 2}, FASTMAX_E_BAD_SHAPE for T <= 0, a
 * shape whose state_bytes is 0, H <= 0, H % Hkv != 0, T > max_len in load, new_len < 0 or > max_len in set_len, or inv_nt not
 * finite, FASTMAX_E_ALIGNMENT for a state or workspace that is not 16-byte aligned or a q, k, v or o pointer not aligned to
 * its element, FASTMAX_E_WORKSPACE for a workspace smaller than the query function's answer. */
#ifndef FASTMAX_HIP_KV_DECODE_H
#define FASTMAX_HIP_KV_DECODE_H

#include "fastmax_hip.h"

#define FASTMAX_KV_CHUNK 128
#define FASTMAX_KV_SLICE 8
#define FASTMAX_KV_MAX_D 256

#ifdef __cplusplus
extern "C" {
#endif

enum fastmax_kv_word {
    FASTMAX_KV_LEN = 0,
    FASTMAX_KV_OVERFLOW = 1,
    FASTMAX_KV_HEADER_WORDS = 16
};

size_t fastmax_hip_kv_decode_state_bytes(int B, int Hkv, int D, int max_len, int dtype);
size_t fastmax_hip_kv_decode_workspace(int B, int H, int Hkv, int T, int D, int max_len);
int fastmax_hip_kv_decode_load(const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides, void* state,
                               int B, int Hkv, int T, int D, int max_len, int dtype, void* stream);
int fastmax_hip_kv_decode_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                        const void* v, const int64_t* v_strides, void* state, void* o, int B, int H, int Hkv,
                                        int T, int D, int max_len, int dtype, int p, float inv_nt, void* workspace,
                                        size_t workspace_bytes, void* stream);
int fastmax_hip_kv_decode_set_len(void* state, int new_len, int max_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_KV_DECODE_H */
