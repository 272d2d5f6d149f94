/* fastmax_hip_generate.h -- generation-time entry points of libfastmax_hip.so that take the attention block's QKV
 * projection output as it is (MI355X / gfx950 only).  The conventions, the dtype and error enums and the decode state cache
 * these calls advance are those of fastmax_hip.h; the entry points here belong to the same library and FASTMAX_ABI_VERSION
 * and are bound by the one table ABI in fastmax_experiments_amd/_lib.py.
 */
#ifndef FASTMAX_HIP_GENERATE_H
#define FASTMAX_HIP_GENERATE_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- second-order (p = 2) decode step straight from the QKV projection (csrc/fastmax_decode_qkv.hip): what
 *      fastmax_hip_rope_qkv_split (K, V left at their G heads) followed by fastmax_hip_p2_decode_step computes, bit for bit
 *      in o and in the state, as ONE step launch + the finalize: the step kernel de-interleaves and rotates the new token
 *      while it loads it (lit_gpt/model.py:397-425 for one token, then model.py:485's fastmax(p=2) at the new last position).
 *      qkv:   contiguous (B, G, qpk + 2, D) in in_dtype: one new token per batch entry, the projection's (B,1,G,qpk+2,hs)
 *             view.  Slots 0 .. qpk-1 of a group are its query heads, slot qpk its key head, slot qpk+1 its value head.
 *      cos, sin: ONE row of rope_n float32 each, the new token's position (the same for every batch entry).  The first
 *             rope_n elements of every query head and of the key head become x cos + rot(x) sin, rot(x) = cat(-x[half:],
 *             x[:half]), with the split pass's roundings: two float32 products and their sum unfused; with tables16 != 0
 *             and a 16-bit in_dtype each product is rounded to in_dtype first (a rope cache kept in the tensors' dtype);
 *             the result is rounded to in_dtype before use, as the split pass stores it.
 *      state, o, a, out_dtype: as for fastmax_hip_p2_decode_step with H = G qpk query heads and Hkv = G; o (B,H,1,D).
 *      p2_decode_step_qkv_supported (host only): 1 when in_dtype is one of the three, G > 0, 0 < qpk <= 256,
 *             0 < D <= 128, rope_n is even and 0 <= rope_n <= D; else 0.  These are the step's limits (D, qpk) and the
 *             rotation's (an even rope_n inside the head); the loader works element by element, so unlike the split pass it
 *             asks for no whole 16-byte pieces and no alignment.
 *      p2_decode_step_qkv: FASTMAX_E_NULL for a null pointer, FASTMAX_E_BAD_DTYPE for a dtype outside the enum,
 *             FASTMAX_E_BAD_SHAPE for everything else _supported refuses, for B <= 0, B G > 65535 and B G qpk > INT_MAX;
 *             every rejection happens before anything is launched.  Bitwise reproducible: no float atomics. */
int fastmax_hip_p2_decode_step_qkv_supported(int G, int qpk, int D, int rope_n, int in_dtype);
int fastmax_hip_p2_decode_step_qkv(const void* qkv, const float* cos, const float* sin, float* state, void* o,
                                   int B, int G, int qpk, int D, int rope_n, int tables16,
                                   int in_dtype, int out_dtype, float a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_GENERATE_H */
