/* fastmax_hip_prefix.h -- LLaMA-Adapter's gated prefix attention behind a softmax ("quadratic") block in libfastmax_hip.so
 * (MI355X / gfx950 only; csrc/prefix_attention.hip).  bf16 and fp16.
 * The dtype and error enums are those of fastmax_hip.h; the entry points belong to the same library and FASTMAX_ABI_VERSION
 * (additions only) and are bound by their rows of ABI_EXT3 in fastmax_experiments_amd/_lib.py.  Everything runs on `stream`;
 * nothing is allocated, nothing is read back, there are no atomics, and every sum has a fixed order: two calls give the same bits.
 *
 *   forward       out[b, h, i] = y[b, h, i] + gate[h] * sum_{j < aT} softmax_j(scale * q[b, h, i] . ak[g, j]) av[g, j],
 *                 g = h / (H / Hkv).  q, y (B, H, N, D), each with its three element strides (batch, head, row) and unit stride
 *                 along D; ak, av (Hkv, aT, D) contiguous, at their KV heads; gate H floats; out (B, H, N, D) contiguous, in
 *                 `dtype`, and may be y itself.  aT in 1 .. FASTMAX_PREFIX_MAX_ROWS (one key tile, no mask); any N >= 1; D a
 *                 multiple of 8 in 8 .. 256.  Scores, maximum, sum and the accumulator are float32; the exponentials are rounded
 *                 to `dtype` once, as a matrix operand; the float32 sum y + gate * ay is rounded once.  gate[h] == 0: out has y's
 *                 bits.  A row's bits depend on its own q and y rows and the head's ak, av and gate alone.
 *
 *   backward      from q, grad_o (= dO, through its own three strides), ak, av and gate, with r = H / Hkv:
 *                     P_ij  = softmax_j(scale * s_ij)             s_ij = q_i . ak_j, float32 on the matrix cores, recomputed
 *                     D_i   = sum_j P_ij (dO_i . av_j)            float32; equal to sum_c dO_ic ay_ic with ay never rounded
 *                     dS_ij = gate_h P_ij (dO_i . av_j - D_i)     rounded to `dtype` once, as a matrix operand
 *                     dq_i  = scale sum_j dS_ij ak_j
 *                     dak_j = scale sum_{b, h in group, i} dS_ij q_i        dav_j = sum_{b, h in group} gate_h sum_i P_ij dO_i
 *                     dgate_h = sum_{b, i} D_i
 *                 dq (B, H, N, D) contiguous and dak, dav (Hkv, aT, D) contiguous in `dtype`; dgate H floats.  The gradient of y
 *                 is grad_o itself and has no kernel.  One tile kernel per (b, h, chunk of FASTMAX_PREFIX_BWD_CHUNK rows), which
 *                 writes dq and leaves one float32 partial of dak, dav and sum D_i in the workspace, and one reduce kernel that
 *                 sums the partials of each KV head over (b, query head of the group, chunk) in ascending order and rounds once.
 *                 D a multiple of 8 in 8 .. 128.
 *   backward_workspace   bytes of workspace backward needs: B * H * ceil(N / FASTMAX_PREFIX_BWD_CHUNK) *
 *                 (2 * FASTMAX_PREFIX_MAX_ROWS * D + 1) * 4; 0 for a shape it rejects.
 *
 * Every rejection happens before anything is launched, in this order: FASTMAX_E_NULL (a missing pointer, strides and the
 * workspace included), FASTMAX_E_BAD_DTYPE (anything but FASTMAX_BF16 / FASTMAX_F16), FASTMAX_E_BAD_SHAPE (a head size that is not
 * a multiple of 8 in 8 .. 256 -- backward: 8 .. 128 --, a count <= 0, H % Hkv != 0, B * H above 65535, aT outside
 * 1 .. FASTMAX_PREFIX_MAX_ROWS, a scale that is not finite), FASTMAX_E_ALIGNMENT (q, y, grad_o, ak, av, out, dq or the workspace not
 * 16-byte aligned, a stride that is not a whole number of 16-byte pieces, gate or dgate not 4-byte aligned, dak or dav not 2-byte
 * aligned), FASTMAX_E_WORKSPACE (smaller than backward_workspace's answer). */
#ifndef FASTMAX_HIP_PREFIX_H
#define FASTMAX_HIP_PREFIX_H

#include "fastmax_hip.h"

#define FASTMAX_PREFIX_MAX_ROWS 32
#define FASTMAX_PREFIX_BWD_CHUNK 512

#ifdef __cplusplus
extern "C" {
#endif

int fastmax_hip_prefix_forward(const void* q, const int64_t* q_strides, const void* y, const int64_t* y_strides, const void* ak,
                               const void* av, const float* gate, void* out, int B, int H, int Hkv, int N, int D, int aT, int dtype,
                               float scale, void* stream);
size_t fastmax_hip_prefix_backward_workspace(int B, int H, int N, int D);
int fastmax_hip_prefix_backward(const void* q, const int64_t* q_strides, const void* grad_o, const int64_t* go_strides, const void* ak,
                                const void* av, const float* gate, void* dq, void* dak, void* dav, float* dgate, int B, int H, int Hkv,
                                int N, int D, int aT, int dtype, float scale, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_PREFIX_H */
