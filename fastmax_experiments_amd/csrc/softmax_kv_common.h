// What the softmax KV-cache routes share (softmax_kv_decode.hip: 16-bit rows, a token at a time; softmax_kv_block.hip: the same rows,
// many tokens at once; softmax_kv_fp8.hip: e4m3 rows with a scale per row): the 16-bit matrix-core operand of either dtype, the
// decomposition's constants, the overflow guard, the 16-bit append kernel and the combine kernel.
// Every attend kernel leaves (m, l, D numerator floats) per query head, new token and chunk (the block route: span) in the same
// workspace layout.
#pragma once
#include "../../include/fastmax_hip_kv_decode.h"
#include "fastmax_mfma_common.h"

#include <cmath>

namespace fastmax {
namespace smkv {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

template <typename T> struct Op;
template <> struct Op<bf16_t> {
    typedef bf16x8 v8;
    static __device__ __forceinline__ f32x4 mma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v8 round8(const float* x) {
        v8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (__bf16)x[i];
        return r;
    }
};
template <> struct Op<f16_t> {
    typedef h8 v8;
    static __device__ __forceinline__ f32x4 mma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v8 round8(const float* x) {
        v8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (_Float16)x[i];
        return r;
    }
};

constexpr int CHUNK = FASTMAX_KV_CHUNK, SLICE = FASTMAX_KV_SLICE, HDR_BYTES = FASTMAX_KV_HEADER_WORDS * 4;
constexpr int NT = 256, NW = 4, WPOS = CHUNK / NW, RB = 16;          // threads, waves, positions per wave, query heads per workgroup
static_assert(WPOS == 32, "a wave takes two 16-row operands");

__host__ __device__ inline int64_t cap_of(int max_len) { return ((int64_t)max_len + CHUNK - 1) / CHUNK * CHUNK; }
__device__ __forceinline__ bool overflows(int len, int T, int max_len) { return len < 0 || (int64_t)len + T > (int64_t)max_len; }
template <int DP> constexpr int v_row() { return 2 * DP + 64; }
template <int DP> constexpr int attend_lds() { return CHUNK * v_row<DP>(); }

// grid: (T, B * Hkv, 2 = K / V); block: 64.  Rows len .. len + T - 1, unless that passes max_len; the header is only read.
static __global__ __launch_bounds__(64) void sm_append_kernel(const uint16_t* k, const uint16_t* v, Strides3 ks, Strides3 vs, const int* hdr,
                                                       uint16_t* kc, uint16_t* vc, int Hkv, int Tn, int D, int max_len, int64_t cap) {
    const int len = hdr[FASTMAX_KV_LEN];
    if (overflows(len, Tn, max_len)) return;
    const int t = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv;
    const bool isv = blockIdx.z != 0;
    const Strides3 s = isv ? vs : ks;
    const uint16_t* src = (isv ? v : k) + (int64_t)b * s.sb + (int64_t)g * s.sh + (int64_t)t * s.sn;
    uint16_t* dst = (isv ? vc : kc) + ((int64_t)bg * cap + len + t) * D;
    if ((int)threadIdx.x < D / 8) reinterpret_cast<uint4*>(dst)[threadIdx.x] = reinterpret_cast<const uint4*>(src)[threadIdx.x];
}

// grid: (B * H, ts); block: 64 .. 256 threads over the columns
template <typename T>
__global__ void sm_combine_kernel(int* hdr, const float* __restrict__ part, const int* __restrict__ nchunks, T* __restrict__ o,
                                  float* __restrict__ lse, int D, int max_len, int Tn, int t0, int ts, int nchunk, int last) {
    const int ti = blockIdx.y;
    const int nc = nchunks[(int64_t)blockIdx.x * ts + ti];
    T* orow = o + ((int64_t)blockIdx.x * Tn + t0 + ti) * D;
    if (last && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {          // the call's only header write
        const int len = hdr[FASTMAX_KV_LEN];
        if (overflows(len, Tn, max_len)) hdr[FASTMAX_KV_OVERFLOW] = 1;
        else hdr[FASTMAX_KV_LEN] = len + Tn;
    }
    if (nc == 0) {                                           // the guard fired in attend
        for (int d = threadIdx.x; d < D; d += blockDim.x) orow[d] = from_float<T>(0.f);
        if (lse && threadIdx.x == 0) lse[(int64_t)blockIdx.x * Tn + t0 + ti] = 0.f;
        return;
    }
    const float* base = part + ((int64_t)blockIdx.x * ts + ti) * nchunk * (D + 2);
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, base[(int64_t)c * (D + 2)]);
    float l = 0.f;
    for (int c = 0; c < nc; ++c) l += base[(int64_t)c * (D + 2) + 1] * __builtin_amdgcn_exp2f(base[(int64_t)c * (D + 2)] - M);
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float num = 0.f;
        for (int c = 0; c < nc; ++c) num += base[(int64_t)c * (D + 2) + 2 + d] * __builtin_amdgcn_exp2f(base[(int64_t)c * (D + 2)] - M);
        orow[d] = from_float<T>(num / l);
    }
    if (lse && threadIdx.x == 0) lse[(int64_t)blockIdx.x * Tn + t0 + ti] = (M + __builtin_amdgcn_logf(l)) * 0.69314718055994531f;
}

// a pointer and its three element strides as whole 16-byte pieces of 16-bit elements
static inline bool pieces(const void* p, const int64_t* s) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0;
}

}  // namespace smkv
}  // namespace fastmax
