/* fastmax_hip_optim.h -- AdamW over the flat LoRA-gradient bucket in libfastmax_hip.so (MI355X / gfx950 only;
 * csrc/flat_adamw.hip): the whole accumulation boundary of a fine-tune step -- division by the world size, global-norm clip,
 * decoupled weight decay, both moments, bias correction, the update, the parameter written in its own dtype, the gradient zeroed
 * -- in at most two launches.  The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library
 * and FASTMAX_ABI_VERSION and are bound by the table ABI in fastmax_experiments_amd/_lib.py.
 *
 * Buffers: `g` is the flat gradient, n elements of `g_dtype` (FASTMAX_F32 / BF16 / F16).  m, v are flat float32 moments (n each).
 * `master` is a flat float32 copy (n) used ONLY at the flat positions of 16-bit parameters: a float32 parameter is updated in
 * place, a 16-bit parameter receives round_to_nearest_even(master).  master may be NULL when n_lowp (the number of 16-bit
 * segments) is 0.  Everything runs on `stream`; nothing is read back to the host; there are no float atomics and every sum has a
 * fixed order, so all results are bitwise reproducible and do not depend on how the flat range is cut into segments.
 *
 * Segment record, 32 bytes, one per parameter, in device memory (`segments`, n_segments of them):
 *     void*   param     the parameter's first element (contiguous)
 *     int64_t offset    its first flat index (the bucket's packed offsets: the running sum of the numels)
 *     int64_t numel
 *     int32_t dtype     FASTMAX_F32 / BF16 / F16
 *     int32_t pad
 * Chunk record, 16 bytes, one per workgroup of the update pass, in device memory (`chunks`, n_chunks of them):
 *     int64_t start     flat index of the chunk's first element
 *     int32_t segment   index into the segment table; a chunk never crosses a segment boundary
 *     int32_t len       1 .. fastmax_hip_adamw_chunk() elements
 * The chunks cover every flat index exactly once.  Both tables are the caller's; the library checks their counts, not their
 * contents.  A chunk moves as pieces of 4 elements (16 bytes of a float32 stream, 8 bytes of a 16-bit one) when its length is a
 * whole number of pieces and the chunk's first address in every stream (g, m, v, master, the parameter) lies on a piece boundary
 * of that stream; any other chunk moves element by element.  Both routes round every operation alike.
 *
 * Workspace: fastmax_hip_adamw_workspace(n) bytes, 16-byte aligned, ZEROED ONCE by the caller before the first step and then
 * left to the library, and used with ONE pair of tables (the tickets count workgroups per launch).  It begins with the scalar
 * record (64 bytes), followed by 64 first-level ticket counters (64 bytes apart: 4096 bytes, internal) and the norm pass's
 * partial sums (one float per workgroup of the norm pass, at most 1024):
 *     float    norm      offset  0   sqrt(sum (grad_scale g)^2) of the last step that asked for it
 *     float    coef      offset  4   min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_), 1 without clipping
 *     int32_t  finite    offset  8   1 when that norm is finite
 *     int64_t  step      offset 16   t: the number of updates applied so far; the update pass reads it, one thread advances it
 *     int64_t  skipped   offset 24   steps left out because of a non-finite norm
 *     uint64_t ticket    offset 32   second-level ticket of the update pass, over all launches (internal)
 * The caller may read and write step and skipped between launches (checkpoints); ticket stays as the library leaves it.
 *
 *   adamw_norm:   partial sums of (grad_scale g)^2 into the workspace.  Needed before adamw_update whenever clip or
 *                 skip_nonfinite is set, with the same g, n and grad_scale.
 *   adamw_update: per element, in float32 (p = the float32 parameter, or master[i] for a 16-bit one; t = step + 1):
 *                     gh = g * grad_scale * coef
 *                     p  = p * (1 - lr * weight_decay)
 *                     m  = beta1 m + (1 - beta1) gh;   v = beta2 v + (1 - beta2) gh^2
 *                     p  = p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),     bc_k = 1 - beta_k^t
 *                 which is torch.optim.AdamW with amsgrad=False, maximize=False.  bc1, bc2, lr / bc1 and 1 - lr * weight_decay
 *                 are computed in double by one thread of each workgroup, from the step counter, never per element and never in
 *                 float32 powf.  The prototypes carry no doubles, so the caller passes beta1, beta2
 *                 AND their complements, each rounded from its own double.  lr is taken from *lr_ptr (device memory) when
 *                 lr_ptr is given, else from `lr`.  zero_grad: the same pass stores 0 to g.  skip_nonfinite with a non-finite
 *                 norm: p, master, m, v and step stay untouched, g is still zeroed (with zero_grad), skipped advances.
 *
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing required pointer, FASTMAX_E_BAD_DTYPE for a
 * g_dtype outside the enum, FASTMAX_E_BAD_SHAPE for n <= 0, a segment count outside 1 .. n, n_lowp outside 0 .. n_segments, a
 * chunk count <= 0, below ceil(n / chunk), above n or above 2^31 - 1 (the grid), FASTMAX_E_ALIGNMENT for m / v / master /
 * workspace not 16-byte aligned (g: its element, the tables: 8 bytes, lr_ptr: 4), FASTMAX_E_WORKSPACE for a workspace smaller
 * than the query's answer. */
#ifndef FASTMAX_HIP_OPTIM_H
#define FASTMAX_HIP_OPTIM_H

#include "fastmax_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fastmax_hip_adamw_workspace(int64_t n);
int fastmax_hip_adamw_chunk(void);
int fastmax_hip_adamw_norm(const void* g, int g_dtype, int64_t n, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream);
int fastmax_hip_adamw_update(void* g, int g_dtype, int64_t n, float* m, float* v, float* master, int64_t n_lowp,
                             const void* segments, int64_t n_segments, const void* chunks, int64_t n_chunks, float lr,
                             const float* lr_ptr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                             float weight_decay, float grad_scale, float max_norm, int clip, int skip_nonfinite, int zero_grad,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_OPTIM_H */
