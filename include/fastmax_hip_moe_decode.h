/* fastmax_hip_moe_decode.h -- the expert MLPs of the mixture-of-experts layer at decode size, on DEVICE-SIDE row counts, in
 * libfastmax_hip.so (MI355X / gfx950 only; csrc/moe_decode.hip).  fastmax_hip_moe_route (fastmax_hip_moe.h) leaves `offsets`
 * (E + 1) and `row_of` (S) on the device; here a workgroup takes its expert's run of rows from those and its expert's NF4 weights
 * from a device table, so that nothing is read back and which weights a workgroup reads is decided by the data, not by the
 * launch: the whole layer can be recorded in a graph.  The dtype and error enums are those of fastmax_hip.h; the entry points
 * belong to the same library and FASTMAX_ABI_VERSION (additions only) and are bound by the table ABI in
 * fastmax_experiments_amd/_lib.py.
 *
 * Notation: M tokens, 1 <= M <= 16; E experts; k experts per token; S = M k slots; C = n_embd, I = intermediate_size, both
 * multiples of 128; dt = FASTMAX_BF16 or FASTMAX_F32.  A token selects an expert at most once, so a run has at most M <= 16 rows.
 *
 *   moe_experts_up:    for every slot s of expert e's run, t = row_of[s]:
 *                        a = round(x[t] . deq(fc_1_e)^T + bias), b = round(x[t] . deq(fc_2_e)^T + bias)          (to dt)
 *                        h[s] = round(round(silu(a)) * b)                                                          (to dt)
 *                      -- the gather is part of the x loads; the two products share one load of x; the rounding points are those
 *                      of the two linears followed by fastmax_hip_gated_act_forward (FASTMAX_ACT_SILU).
 *   moe_experts_down:  ys[s] = round(h[s] . deq(proj_e)^T + bias) over the same runs.  fastmax_hip_moe_combine follows.
 *
 * A product is the few-rows kernel's of fastmax_hip_nf4_linear_forward_s (M <= 16), operation for operation -- K in 128-wide
 * blocks, block j to wave j % 4, the four partial tiles added as (p0 + p1) + (p2 + p3), then the bias -- and a row's result does
 * not depend on which other rows share its run: every row has the bits the expert's own linears give it.
 * Launch: grid (I / 16, E) resp. (C / 16, E), 256 threads; a workgroup whose run is empty returns at once.
 *
 * Operands: x (M, C), h (S, I), ys (S, C) with a row stride in ELEMENTS and unit stride along the row, 16-byte aligned rows;
 * offsets, row_of dense int.  `table`: E entries in DEVICE memory, 8-byte aligned; per linear the packed codes (16-byte aligned,
 * (N, K) row-major), the fastmax_nf4_scales fields (plain or double-quantised) and the float32 bias (16-byte aligned) or NULL.
 * The library cannot inspect the table's pointers: packing it right is the caller's part (moe.py checks its entry size against
 * fastmax_hip_moe_expert_entry_bytes).  Indices READ FROM DEVICE MEMORY are clamped -- a run to 16 rows inside 0 .. S, row_of
 * to 0 .. M - 1 -- so stale or foreign offsets give wrong numbers, never an access outside x, h or ys.
 *
 * Every rejection happens before anything is launched: FASTMAX_E_NULL for a missing pointer, FASTMAX_E_BAD_DTYPE for a dtype
 * other than bf16 / f32, FASTMAX_E_BAD_SHAPE for M outside 1 .. 16, E outside 1 .. FASTMAX_MOE_MAX_EXPERTS, k outside
 * 1 .. min(E, FASTMAX_MOE_MAX_PER_TOKEN), C or I not a positive multiple of 128, or a row stride below its row,
 * FASTMAX_E_ALIGNMENT for a misaligned pointer or stride. */
#ifndef FASTMAX_HIP_MOE_DECODE_H
#define FASTMAX_HIP_MOE_DECODE_H

#include "fastmax_hip.h"
#include "fastmax_hip_moe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FASTMAX_MOE_DECODE_MAX_ROWS 16

typedef struct fastmax_moe_linear {
    const uint8_t* wq;            /* packed NF4 codes of W (N, K) */
    fastmax_nf4_scales scales;    /* its block scales            */
    const float* bias;            /* (N) float32, or NULL        */
} fastmax_moe_linear;

typedef struct fastmax_moe_expert_entry {
    fastmax_moe_linear fc_1, fc_2, proj;
} fastmax_moe_expert_entry;

size_t fastmax_hip_moe_expert_entry_bytes(void);
int fastmax_hip_moe_experts_up(const void* x, int64_t x_stride, const fastmax_moe_expert_entry* table, const int* offsets,
                               const int* row_of, void* h, int64_t h_stride, int M, int E, int k, int C, int I, int dtype,
                               void* stream);
int fastmax_hip_moe_experts_down(const void* h, int64_t h_stride, const fastmax_moe_expert_entry* table, const int* offsets,
                                 void* ys, int64_t ys_stride, int M, int E, int k, int C, int I, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FASTMAX_HIP_MOE_DECODE_H */
