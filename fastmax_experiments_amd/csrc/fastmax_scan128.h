// What the three eight-wave causal scans at 64 < D <= 128 share, once.
//
// 512 threads, 64-token chunks.  Wave (qt, dh): output rows of tile qt = w & 3 of the chunk, output columns [64 dh, 64 dh + 64).
// The 128 x 128 state S2 = sum y z^T lives in MFMA accumulators, value-column slab 16 w per wave, and is published to an LDS
// image (NP bf16 parts) once per chunk; S1 = sum alpha z is a row of 128 floats.
// Used by fwd_p1_mfma_bf16_d128_kernel (fastmax_mfma_bf16.hip, NP = 1), fwd_p1_mfma_d128_2p_kernel (fastmax_mfma_d128_2p.hip,
// NP = 2) and scan_d128_2p_kernel (fastmax_scan_d128_2p.hip, NP = 2).
// These kernels sit on the register ceiling, and a force-inlined function is optimised on its own before it is inlined, so
// moving a piece of the chunk step in here can change a kernel's code.  Only pieces that left every kernel using them with the
// instruction stream it had are here; profiles/r21_scan128_shared.md lists them and the ones that had to stay in the kernels.
#pragma once
#include "fastmax_mfma_common.h"

namespace fastmax {
namespace scan128 {

constexpr int DP = 128, C = 64, KS = DP / 32, MT = DP / 16, IMG = C * DP * 2;

// a thread's place in the state: wave w owns value columns [16 w, 16 w + 16), lane = (r, q4)
struct WaveLane { int w, r, q4; };

// row fragments from global memory (two-part kernels): the eight 16-byte pieces of this lane's row, raw, one chunk ahead
template <bool BUF, typename TIN>
__device__ __forceinline__ void load_row_pieces(const RowPieceLoader<BUF, TIN>& rows, int row, int q4, u32x4 (&raw)[KS][8 / InTraits<TIN>::EPL]) {
    constexpr int EPL = InTraits<TIN>::EPL;
    int q4o = q4;                                                  // opaque: the eight piece offsets are re-formed per chunk, not hoisted and spilled
    asm volatile("" : "+v"(q4o));
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int u = 0; u < 8 / EPL; ++u) raw[ks][u] = rows.load(row, (32 * ks + 8 * q4o) / EPL + u);
}

// The two-part state image: hi and lo parts of SIMG bytes at S2I (DP rows, + 16 where row DP carries ksum), S1 as floats behind
// them.  Template constants, so that each offset is a literal in here as it was in the kernels.
// v at (row, 8-byte unit u8) of the image
template <int S2I, int SIMG> __device__ __forceinline__ void put4(char* smem, int row, int u8, const f32x4 v) {
    bf16x4 hi, lo;
    split4(v, hi, lo);
    const int off = img_off<DP>(row, u8 >> 1) + ((u8 & 1) << 3);
    *reinterpret_cast<bf16x4*>(smem + S2I + off) = hi;
    *reinterpret_cast<bf16x4*>(smem + S2I + SIMG + off) = lo;
}
// (scale S2)^T into the image, scale * ksum into its row DP (where it has one), S1
template <int S2I, int SIMG>
__device__ __forceinline__ void publish(char* smem, const WaveLane& g, const f32x4 (&s2acc)[MT], const f32x4& s1acc, const f32x4& ksacc, float scale) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) put4<S2I, SIMG>(smem, 16 * g.w + g.r, 4 * mt + g.q4, s2acc[mt] * scale);
    if constexpr (SIMG > DP * DP * 2) {
        if (g.r == 0) put4<S2I, SIMG>(smem, DP, 4 * g.w + g.q4, ksacc * scale);
    }
    if (g.q4 == 0) reinterpret_cast<float*>(smem + S2I + 2 * SIMG)[16 * g.w + g.r] = s1acc[0];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// 512 threads and LDS bytes of dynamic LDS; the attribute is set on a kernel's first launch
template <auto KERN, int LDS, typename P> int launch512(const P& prm, int nb, hipStream_t stream) {
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    hipLaunchKernelGGL(KERN, dim3(nb), dim3(512), LDS, stream, prm);
    return (int)hipGetLastError();
}
// BUF: tiles and row pieces through buffer descriptors when a (b,h) slab of each of the three tensors fits their 31-bit offsets
template <typename TIN> bool buf_route(const Strides3& s0, const Strides3& s1, const Strides3& s2, int N, int D) {
    return quad32_span_ok(s0.sn, N, D, (int)sizeof(TIN)) && quad32_span_ok(s1.sn, N, D, (int)sizeof(TIN)) && quad32_span_ok(s2.sn, N, D, (int)sizeof(TIN));
}

}  // namespace scan128
}  // namespace fastmax
