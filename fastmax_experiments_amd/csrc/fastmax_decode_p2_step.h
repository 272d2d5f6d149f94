// The single-token step of the second-order (p = 2) decode state cache, as a template over WHERE the new token's q, k, v
// come from: split (B,heads,1,D) tensors (fastmax_decode_p2.hip) or the QKV projection's interleaved output, rotated
// while it is loaded (fastmax_decode_qkv.hip).  State layout, grid and the fixed order of every sum: fastmax_decode_p2.hip.
#pragma once
#include "fastmax_mfma_common.h"

#include <algorithm>

namespace fastmax {
namespace p2dec {

constexpr int STEP_SLOTS = 256;   // partial-F rows per (b, kv-head) in the scratch slab: G * q_per_kv <= STEP_SLOTS
constexpr int STEP_RMIN = 32;     // at least this many pair rows per step workgroup
constexpr int QCMAX = 8;          // query heads accumulated in registers per pass over the rows

__host__ __device__ __forceinline__ int ncols(int D) { return (D + 4) & ~3; }               // round_up(D + 1, 4)
__host__ __device__ __forceinline__ int npairs(int D) { return (D + 1) * (D + 2) / 2; }
__device__ __forceinline__ int row_start(int m, int D1) { return m * D1 - m * (m - 1) / 2; }

// pair row r -> (m, l)
__device__ __forceinline__ void decode_row(int r, int D, int& m, int& l) {
    const int D1 = D + 1;
    m = 0;
    while (m < D && row_start(m + 1, D1) <= r) ++m;
    l = m + (r - row_start(m, D1));
}

// ---- step: update every pair row with the new token and accumulate the group's partial F -----------------------------
// grid (G, B * Hkv), 256 threads.  Thread (rs, j4) = (tid / J4, tid % J4) handles columns 4 j4 .. 4 j4 + 3 of the rows
// r0 + rs, r0 + rs + RP, ... of this workgroup's range [r0, r1).
// Src gives the new token's elements as float: k(b, kv-head, d), v(b, kv-head, d) and q(b, kv-head, qpk, i, d) for
// query head i of the group.
template <typename T, int QC, typename Src>
__global__ __launch_bounds__(256) void p2_decode_step_kernel(Src src, float* state, float* part, int Hkv, int qpk, int D, int G,
                                                             float a) {
    __shared__ __attribute__((aligned(16))) float kt[132], vq[132], qt[QCMAX][132], red[16][132];
    const int tid = threadIdx.x, g = blockIdx.x, bkv = blockIdx.y, b = bkv / Hkv, hk = bkv % Hkv;
    const int P = npairs(D), DV = ncols(D), J4 = DV / 4;
    const int RP = min(256 / J4, 16), rs = tid / J4, j4 = tid - rs * J4;
    const bool active = rs < RP;
    const int r0 = (int)((int64_t)P * g / G), r1 = (int)((int64_t)P * (g + 1) / G);
    float* rec = state + (int64_t)bkv * P * DV;
    if (tid < DV) {
        kt[tid] = tid == 0 ? 1.f : (tid <= D ? src.k(b, hk, tid - 1) : 0.f);
        vq[tid] = tid < D ? src.v(b, hk, tid) : (tid == D ? 1.f : 0.f);
    }
    int m0 = 0, l0 = 0;
    if (active && r0 + rs < r1) decode_row(r0 + rs, D, m0, l0);
    for (int c0 = 0; c0 < qpk; c0 += QC) {
        __syncthreads();
        for (int idx = tid; idx < QC * DV; idx += 256) {
            const int hh = idx / DV, c = idx - hh * DV;
            float x = 0.f;
            if (c0 + hh < qpk) {
                if (c == 0) x = 1.f;
                else if (c <= D) x = a * src.q(b, hk, qpk, c0 + hh, c - 1);
            }
            qt[hh][c] = x;
        }
        __syncthreads();
        f32x4 acc[QC];
#pragma unroll
        for (int hh = 0; hh < QC; ++hh) acc[hh] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (active) {
            const f32x4 vv = *reinterpret_cast<const f32x4*>(&vq[4 * j4]);
            int m = m0, l = l0;
            for (int r = r0 + rs; r < r1; r += RP) {
                f32x4* rowp = reinterpret_cast<f32x4*>(rec + (int64_t)r * DV) + j4;
                f32x4 s = *rowp;
                if (c0 == 0) {
                    const float kk = kt[m] * kt[l];
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] = fmaf(kk, vv[e], s[e]);
                    *rowp = s;
                }
                const float w = m == l ? 1.f : 2.f;
#pragma unroll
                for (int hh = 0; hh < QC; ++hh) {
                    const float c = w * qt[hh][m] * qt[hh][l];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[hh][e] = fmaf(c, s[e], acc[hh][e]);
                }
                if (r + RP >= r1) break;                          // (past the last row m would run beyond D)
                l += RP;
                while (l > D) { ++m; l = l - (D + 1) + m; }      // (m, D + 1 + x) is (m + 1, m + 1 + x)
            }
        }
        // fixed-order sum over the RP row groups, one query head at a time
        const int nq = min(QC, qpk - c0);
#pragma unroll
        for (int hh = 0; hh < QC; ++hh) {
            if (hh >= nq) break;
            if (active) *reinterpret_cast<f32x4*>(&red[rs][4 * j4]) = acc[hh];
            __syncthreads();
            if (tid < DV) {
                float f = 0.f;
                for (int i = 0; i < RP; ++i) f += red[i][tid];
                part[(((int64_t)bkv * G + g) * qpk + c0 + hh) * DV + tid] = f;
            }
            __syncthreads();
        }
    }
}

// step workgroups per (b, kv-head): as many as the slab holds for this group size, at least STEP_RMIN rows each
static inline int step_groups(int D, int qpk) {
    const int by_rows = (npairs(D) + STEP_RMIN - 1) / STEP_RMIN;
    return std::max(1, std::min(STEP_SLOTS / qpk, by_rows));
}

// per (b, query head): S~[(0,0)] + the G partials in a fixed order, divide, store o (fastmax_decode_p2.hip)
void launch_p2_finalize(const float* state, const float* part, void* o, int out_dtype, int B, int H, int Hkv, int qpk, int D,
                        int G, hipStream_t stream);

// the step and its finalize; the reduction scratch sits behind the B * Hkv state records
template <typename T, typename Src>
static int launch_step_src(const Src& src, float* state, void* o, int out_dtype, int B, int H, int Hkv, int D, float a,
                           hipStream_t stream) {
    const int qpk = H / Hkv, G = step_groups(D, qpk);
    float* part = state + (size_t)B * Hkv * npairs(D) * ncols(D);
    const dim3 grid(G, B * Hkv);
    if (qpk == 1)
        hipLaunchKernelGGL((p2_decode_step_kernel<T, 1, Src>), grid, dim3(256), 0, stream, src, state, part, Hkv, qpk, D, G, a);
    else if (qpk == 2)
        hipLaunchKernelGGL((p2_decode_step_kernel<T, 2, Src>), grid, dim3(256), 0, stream, src, state, part, Hkv, qpk, D, G, a);
    else if (qpk <= 4)
        hipLaunchKernelGGL((p2_decode_step_kernel<T, 4, Src>), grid, dim3(256), 0, stream, src, state, part, Hkv, qpk, D, G, a);
    else
        hipLaunchKernelGGL((p2_decode_step_kernel<T, QCMAX, Src>), grid, dim3(256), 0, stream, src, state, part, Hkv, qpk, D, G, a);
    launch_p2_finalize(state, part, o, out_dtype, B, H, Hkv, qpk, D, G, stream);
    return (int)hipGetLastError();
}

}  // namespace p2dec
}  // namespace fastmax
