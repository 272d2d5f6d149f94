// What the row kernels around the attention sub-layer share (block_neighbours.hip: RMSNorm, gated activation; neox_block.hip:
// the LayerNorm pair, ungated GELU): 16-byte accesses, the row reductions, the fixed-order sum of partial rows, the exact GELU,
// and the host side's checks and launch geometry.  Private to csrc; each piece is defined here and nowhere else.
//
// Reductions: the 64 lanes of a wave by xor-butterfly (every lane ends with the same bits), then the four waves through LDS,
// added in wave order by every thread.  No atomics anywhere.
#pragma once
#include "fastmax_common.h"

namespace fastmax {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// E elements of type U (16 or 32 bytes) <-> float registers, as 16-byte accesses
template <typename U, int E> __device__ __forceinline__ void ld_vec(const U* p, float (&x)[E]) {
    constexpr int PER = 16 / sizeof(U), NV = E / PER;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        u32x4 raw = *reinterpret_cast<const u32x4*>(p + v * PER);
        const U* pv = reinterpret_cast<const U*>(&raw);
#pragma unroll
        for (int e = 0; e < PER; ++e) x[v * PER + e] = to_float(pv[e]);
    }
}
template <typename U, int E> __device__ __forceinline__ void st_vec(U* p, const float (&x)[E]) {
    constexpr int PER = 16 / sizeof(U), NV = E / PER;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        u32x4 raw;
        U* pv = reinterpret_cast<U*>(&raw);
#pragma unroll
        for (int e = 0; e < PER; ++e) pv[e] = from_float<U>(x[v * PER + e]);
        *reinterpret_cast<u32x4*>(p + v * PER) = raw;
    }
}
template <typename U> __device__ __forceinline__ float round_to(float f) { return to_float(from_float<U>(f)); }
// a * b rounded on its own: the sum that follows must not contract it into a fused multiply-add (hipcc contracts by default),
// or the float32 backward with ds_in would not be the result without ds_in plus ds_in
__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p;
}

// sum over the threads that share a row: a wave (WAVE_ROW) or the whole 256-thread workgroup (red: 4 floats of LDS)
template <bool WAVE_ROW> __device__ __forceinline__ float row_sum(float x, float* red) {
    x = wave_sum(x);
    if constexpr (WAVE_ROW) return x;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// two sums behind one barrier (red: 2 x 4 floats)
template <bool WAVE_ROW> __device__ __forceinline__ void row_sum2(float& a, float& b, float (*red)[4]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if constexpr (WAVE_ROW) return;
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

// The backward passes leave NS rows of float32 partial sums per row block: part is (row blocks, NS, C).
// out.o[k][c] = sum over the row blocks of part[blk][k][c], in block order: a workgroup takes a slab of 64 columns of partial
// row k = blockIdx.y, its four waves a quarter of the blocks each (contiguous, in order), and the four quarter sums are added
// in wave order.  With NS > 1 a null out.o[k] is skipped.  A template, so that every translation unit that includes this gets its own.
template <int NS> struct PartialSums { float* o[NS]; };
template <int NS>
__global__ __launch_bounds__(256) void partial_row_sum_kernel(const float* part, PartialSums<NS> out, int nblk, int C) {
    __shared__ float q[4][64];
    const int k = NS > 1 ? blockIdx.y : 0;
    float* o = out.o[0];
    if constexpr (NS > 1) {                                // a single row is only ever summed into an output that is there
#pragma unroll
        for (int i = 1; i < NS; ++i) o = k == i ? out.o[i] : o;
        if (!o) return;                                    // the whole workgroup: nothing below is reached by a part of it
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int per = (nblk + 3) / 4;
    const int b0 = wave * per, b1 = min(nblk, b0 + per);
    float acc = 0.f;
    if (c < C)
        for (int b = b0; b < b1; ++b) acc += part[((int64_t)b * NS + k) * C + c];
    q[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < C) o[c] = ((q[0][lane] + q[1][lane]) + q[2][lane]) + q[3][lane];
}
template <int NS>
static inline void launch_partial_row_sum(const float* part, PartialSums<NS> out, int nblk, int C, hipStream_t st) {
    hipLaunchKernelGGL(partial_row_sum_kernel<NS>, dim3((unsigned)((C + 63) / 64), (unsigned)NS), dim3(256), 0, st, part, out, nblk, C);
}

// SiLU a / (1 + exp(-a)); exact GELU a (1 + erf(a / sqrt 2)) / 2 and its derivative
__device__ __forceinline__ float silu_f(float a) { return a / (1.0f + expf(-a)); }
__device__ __forceinline__ float gelu_f(float a) { return 0.5f * a * (1.0f + erff(a * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_prime(float a) {
    return 0.5f * (1.0f + erff(a * 0.70710678118654752440f)) + a * expf(-0.5f * a * a) * 0.39894228040143267794f;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static inline int elem_size(int dtype) { return dtype == FASTMAX_F32 ? 4 : 2; }
static inline bool aligned16(const void* ptr, int64_t stride, int es) {
    return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0 && ((stride * es) & 15) == 0;
}
static inline bool elem_aligned(const void* ptr, int es) { return (reinterpret_cast<uintptr_t>(ptr) & (es - 1)) == 0; }

// pieces per thread on the norms' piece paths: 0 = one wave per row, 1 / 2 / ... / max_np = one workgroup per row, -1 = scalar path
static inline int norm_shape(int C, int dtype, int max_np) {
    const int e = 16 / elem_size(dtype);
    if (C % e) return -1;
    const int pieces = C / e;
    if (pieces <= 64) return 0;
    for (int np = 1; np <= max_np; np *= 2)
        if (pieces <= 256 * np) return np;
    return -1;
}

// (T, W) pairs: the parameters have the activation dtype or are float32.  Reads dtype and weight_dtype where it is used
#define NORM_DISPATCH(FN, ...)                                                                       \
    do {                                                                                             \
        if (dtype == FASTMAX_F32) FN<float, float>(__VA_ARGS__);                                     \
        else if (dtype == FASTMAX_BF16 && weight_dtype == FASTMAX_F32) FN<bf16_t, float>(__VA_ARGS__); \
        else if (dtype == FASTMAX_BF16) FN<bf16_t, bf16_t>(__VA_ARGS__);                             \
        else if (weight_dtype == FASTMAX_F32) FN<f16_t, float>(__VA_ARGS__);                         \
        else FN<f16_t, f16_t>(__VA_ARGS__);                                                          \
    } while (0)

static inline int norm_check(int M, int C, int dtype, int weight_dtype) {
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (weight_dtype != dtype && weight_dtype != FASTMAX_F32) return FASTMAX_E_BAD_DTYPE;
    if (M <= 0 || C <= 0) return FASTMAX_E_BAD_SHAPE;
    return 0;
}

// The element-wise kernels' geometry over n operands of M rows of I elements (dtype, M and I already checked): every stride
// covers a row and every address is element aligned, or an error code.  vec: all of them allow 16-byte pieces, so a thread
// takes one piece of every operand, else one element; blocks: the 256-thread workgroups that cover M * units.
static inline int elementwise_geometry(int n, const void* const* ptrs, const int64_t* strides, int M, int I, int dtype, bool* vec,
                                       unsigned* blocks) {
    const int es = elem_size(dtype), e = 16 / es;
    *vec = I % e == 0;
    for (int i = 0; i < n; ++i) {
        if (strides[i] < I) return FASTMAX_E_BAD_SHAPE;
        if (!elem_aligned(ptrs[i], es)) return FASTMAX_E_ALIGNMENT;
        *vec = *vec && aligned16(ptrs[i], strides[i], es);
    }
    const int64_t units = (int64_t)M * (*vec ? I / e : I);
    const int64_t nb = (units + 255) / 256;
    if (nb > 0x7fffffff) return FASTMAX_E_BAD_SHAPE;
    *blocks = (unsigned)nb;
    return 0;
}

}  // namespace fastmax
