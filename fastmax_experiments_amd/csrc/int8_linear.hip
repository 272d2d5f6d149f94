// The LLM.int8 linear ("bnb.int8", include/fastmax_hip_int8.h): weight and activation quantisers and the two int8 matrix-core
// products, inference only.  The accumulation is an exact int32; the only floating-point arithmetic is the epilogue.
//
//   int8_quantize_weight_kernel   one workgroup per weight row: row absmax, then 16 codes per 16-byte store
//   int8_dequantize_weight_kernel its inverse, CB * SCB / 127 rounded once
//   int8_flags_kernel             one workgroup per 64 columns of x: the OR over all rows of |x| >= threshold, fixed order
//   int8_rows_kernel              one workgroup per row of x (scale over the non-outlier columns, codes, outlier columns zeroed)
//                                 and one more that writes the ascending outlier list and its count
//   int8_few_rows_kernel          M <= 16: 16 output columns per workgroup, four waves split K; a lane's 16 bytes of a weight
//                                 row go from global memory straight into the A operand of v_mfma_i32_16x16x64_i8, the x codes
//                                 are the B operand; the waves' int32 partial tiles meet in LDS and wave 0 runs the epilogue
//   int8_tile_kernel              M > 16: 128 x 128 output tile, K-steps of 128 codes, four waves of 64 x 64 on the same MFMA;
//                                 CB and CA tiles in LDS under a 16-byte XOR swizzle, two stages, global loads one step ahead
//
// Operand layout of the 16x16x64 i8 MFMA as used here: lane l gives row (A) / column (B) l & 15 and the 16 codes at
// k = 16 (l >> 4) ..; both operands use the same assignment, so the sum over k does not depend on how the hardware numbers the
// bytes inside a lane.  C: lane l holds column l & 15 (the row of x) and rows 4 (l >> 4) + i (four consecutive output columns).
#include "fastmax_common.h"
#include "../../include/fastmax_hip_int8.h"

namespace fastmax {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// eight 16-bit elements (16 bytes) as floats
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
    typedef T Tx8 __attribute__((ext_vector_type(8)));
    const Tx8 t = *reinterpret_cast<const Tx8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
// sixteen elements of a weight row as floats
template <typename T> __device__ __forceinline__ void load16(const T* p, float (&v)[16]) {
    float a[8], b[8];
    load8<T>(p, a);
    load8<T>(p + 8, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = a[i]; v[8 + i] = b[i]; }
}
template <> __device__ __forceinline__ void load16<float>(const float* p, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p + 4 * j);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * j + i] = t[i];
    }
}

// the codec's one product: rint(v * inv) as an int8 code, packed little-endian four to a word
__device__ __forceinline__ unsigned int code_byte(float v, float inv) { return (unsigned int)(int)rintf(v * inv) & 0xffu; }

// max over the workgroup's four waves (fmaxf is exact: any order gives the same value)
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- weight quantiser and its inverse ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void int8_quantize_weight_kernel(const T* __restrict__ w, int64_t ldw, int8_t* __restrict__ cb,
                                                                  float* __restrict__ scb, int K) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const T* row = w + (int64_t)n * ldw;
    float amax = 0.0f;
    for (int c = 16 * threadIdx.x; c < K; c += 16 * 256) {
        float v[16];
        load16<T>(row + c, v);
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
    }
    amax = block_max(amax, red);
    if (threadIdx.x == 0) scb[n] = amax;
    const float inv = amax > 0.0f ? 127.0f / amax : 0.0f;
    for (int c = 16 * threadIdx.x; c < K; c += 16 * 256) {          // the row again, out of the cache
        float v[16];
        load16<T>(row + c, v);
        i32x4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[j] = (int)(code_byte(v[4 * j], inv) | (code_byte(v[4 * j + 1], inv) << 8) | (code_byte(v[4 * j + 2], inv) << 16) |
                           (code_byte(v[4 * j + 3], inv) << 24));
        *reinterpret_cast<i32x4*>(cb + (int64_t)n * K + c) = out;
    }
}

// A float64 to T with ONE rounding.  A 16-bit T goes through float32 rounded to odd (the truncated value with its last bit set
// when anything was cut off), which the final round-to-nearest-even cannot tell from the float64 itself: float32 carries more
// than two bits beyond either 16-bit format.  A plain (T)(float)q rounds twice and is off by one unit once in 2^13 (fp16).
template <typename T> __device__ __forceinline__ T round_once(double q) {
    float f = (float)q;
    if constexpr (sizeof(T) == 2) {
        const double back = (double)f;
        if (back != q) {
            unsigned int u = __float_as_uint(f);
            if (fabs(back) > fabs(q)) u -= 1;          // one step toward zero: the truncation
            f = __uint_as_float(u | 1u);
        }
    }
    return (T)f;
}

// CB * SCB / 127 rounded ONCE to T: the product is exact in float64 and the quotient's own rounding to 53 bits is harmless
// (53 >= 2 p + 2 for every result precision p here), so round_once of it is the exact value rounded once
template <typename T>
__global__ __launch_bounds__(256) void int8_dequantize_weight_kernel(const int8_t* __restrict__ cb, const float* __restrict__ scb,
                                                                    T* __restrict__ w, int64_t ldw, int N, int K) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16 codes each
    const int per_row = K / 16;
    if (unit >= (int64_t)N * per_row) return;
    const int n = (int)(unit / per_row), c = 16 * (int)(unit % per_row);
    const i32x4 pk = *reinterpret_cast<const i32x4*>(cb + (int64_t)n * K + c);
    const double s = (double)scb[n];
    T* out = w + (int64_t)n * ldw + c;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[4 * j + i] = round_once<T>((double)(int8_t)(pk[j] >> (8 * i)) * s / 127.0);
}

// ---- activation pass --------------------------------------------------------------------------------------------------------
// flags[c] = 1 iff |x[m,c]| >= threshold for any m.  A workgroup owns 64 columns: thread (rl, cl) = (tid >> 3, tid & 7) walks rows
// rl, rl + 32, ... of the 8 columns at 8 cl; the 32 row lanes are OR-ed (integer OR: order-free) by shuffles and through LDS.
template <typename T>
__global__ __launch_bounds__(256) void int8_flags_kernel(const T* __restrict__ x, int64_t ldx, float threshold,
                                                        uint8_t* __restrict__ flags, int M) {
    __shared__ unsigned int red[4][8];
    const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3, c0 = 64 * blockIdx.x + 8 * cl;
    unsigned int mask = 0;
    for (int m = rl; m < M; m += 32) {
        float v[8];
        load8<T>(x + (int64_t)m * ldx + c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) mask |= (fabsf(v[i]) >= threshold ? 1u : 0u) << i;
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) mask |= (unsigned int)__shfl_xor((int)mask, off, 64);
    if ((threadIdx.x & 63) < 8) red[threadIdx.x >> 6][cl] = mask;
    __syncthreads();
    if (threadIdx.x < 8) {
        const unsigned int m4 = red[0][cl] | red[1][cl] | red[2][cl] | red[3][cl];
        i32x2 out;
        out[0] = (int)((m4 & 1u) | ((m4 >> 1 & 1u) << 8) | ((m4 >> 2 & 1u) << 16) | ((m4 >> 3 & 1u) << 24));
        out[1] = (int)((m4 >> 4 & 1u) | ((m4 >> 5 & 1u) << 8) | ((m4 >> 6 & 1u) << 16) | ((m4 >> 7 & 1u) << 24));
        *reinterpret_cast<i32x2*>(flags + c0) = out;
    }
}

// workgroups 0 .. M-1: one row of x each.  Workgroup M: the ascending list of outlier columns and its count -- thread t owns the
// columns [t per, (t + 1) per), an exclusive prefix sum of the threads' counts (integers) places its columns.
template <typename T>
__global__ __launch_bounds__(256) void int8_rows_kernel(const T* __restrict__ x, int64_t ldx, const uint8_t* __restrict__ flags,
                                                       int8_t* __restrict__ ca, float* __restrict__ sca, int32_t* __restrict__ list,
                                                       int32_t* __restrict__ count, int M, int K) {
    __shared__ float red[4];
    __shared__ int wsum[4];
    const int m = blockIdx.x;
    if (m == M) {
        const int per = (K + 255) / 256, lo = min(K, per * (int)threadIdx.x), hi = min(K, lo + per);
        int mine = 0;
        for (int c = lo; c < hi; ++c) mine += flags[c];
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int at = incl - mine;
        for (int i = 0; i < w; ++i) at += wsum[i];
        for (int c = lo; c < hi; ++c)
            if (flags[c]) list[at++] = c;
        if (threadIdx.x == 255) *count = at;
        return;
    }
    const T* row = x + (int64_t)m * ldx;
    float amax = 0.0f;
    for (int c = 8 * threadIdx.x; c < K; c += 8 * 256) {
        float v[8];
        load8<T>(row + c, v);
        const i32x2 f = *reinterpret_cast<const i32x2*>(flags + c);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (!((f[i >> 2] >> (8 * (i & 3))) & 0xff)) amax = fmaxf(amax, fabsf(v[i]));
    }
    amax = block_max(amax, red);
    if (threadIdx.x == 0) sca[m] = amax;
    const float inv = amax > 0.0f ? 127.0f / amax : 0.0f;
    for (int c = 8 * threadIdx.x; c < K; c += 8 * 256) {
        float v[8];
        load8<T>(row + c, v);
        const i32x2 f = *reinterpret_cast<const i32x2*>(flags + c);
        i32x2 out;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned int wd = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!((f[j] >> (8 * i)) & 0xff)) wd |= code_byte(v[4 * j + i], inv) << (8 * i);
            out[j] = (int)wd;
        }
        *reinterpret_cast<i32x2*>(ca + (int64_t)m * K + c) = out;
    }
}

// ---- the products -----------------------------------------------------------------------------------------------------------
struct Int8LinearArgs {
    const void* x;            // the unrounded activations (outlier term)
    int64_t ldx;
    const int8_t *ca, *cb;    // (M, K), (N, K)
    const float *sca, *scb, *bias;
    const int32_t *list, *count;
    void* y;
    int64_t ldy;
    int M, N, K;
};

// the outlier term of one row of x against four consecutive output columns: sum over the device-side list, in list order
template <typename T>
__device__ __forceinline__ void outlier_term(const Int8LinearArgs& p, int cnt, int m, int n, const float (&s127)[4], float (&o)[4]) {
    const T* xrow = reinterpret_cast<const T*>(p.x) + (int64_t)m * p.ldx;
    for (int t = 0; t < cnt; ++t) {
        const int c = p.list[t];
        const float xv = (float)xrow[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] += xv * ((float)p.cb[(int64_t)(n + i) * p.K + c] * s127[i]);
    }
}

// acc (exact) -> y: the dequantising scale, the outlier term, the bias, one rounding; four consecutive columns n .. n + 3 of row m
template <typename T>
__device__ __forceinline__ void epilogue4(const Int8LinearArgs& p, int cnt, int m, int n, const i32x4 acc) {
    const float sa = p.sca[m];
    float s127[4], o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4_t sb = *reinterpret_cast<const f32x4_t*>(p.scb + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) s127[i] = sb[i] / 127.0f;
    if (cnt > 0) outlier_term<T>(p, cnt, m, n, s127, o);
    typedef T Tx4 __attribute__((ext_vector_type(4)));
    Tx4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v = (float)acc[i] * (sa * sb[i]) / 16129.0f + o[i];
        if (p.bias) v += p.bias[n + i];
        out[i] = (T)v;
    }
    *reinterpret_cast<Tx4*>(reinterpret_cast<T*>(p.y) + (int64_t)m * p.ldy + n) = out;
}

// M <= 16.  grid N / 16; wave w takes the 64-code steps w, w + 4, ...; two steps are requested before either is multiplied.
template <typename T>
__global__ __launch_bounds__(256) void int8_few_rows_kernel(const Int8LinearArgs p) {
    __shared__ int part[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q4 = lane >> 4;
    const int n0 = 16 * blockIdx.x, nk = p.K / 64;
    const bool mrow = r < p.M;
    const int8_t* wrow = p.cb + (int64_t)(n0 + r) * p.K + 16 * q4;
    const int8_t* xrow = p.ca + (int64_t)(mrow ? r : 0) * p.K + 16 * q4;
    const i32x4 zero = {0, 0, 0, 0};
    i32x4 acc = zero;
    int j = w;
    for (; j + 4 < nk; j += 8) {
        const i32x4 a0 = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wrow + 64 * j));
        const i32x4 a1 = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wrow + 64 * (j + 4)));
        const i32x4 b0 = mrow ? *reinterpret_cast<const i32x4*>(xrow + 64 * j) : zero;
        const i32x4 b1 = mrow ? *reinterpret_cast<const i32x4*>(xrow + 64 * (j + 4)) : zero;
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc, 0, 0, 0);
    }
    if (j < nk) {
        const i32x4 a0 = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wrow + 64 * j));
        const i32x4 b0 = mrow ? *reinterpret_cast<const i32x4*>(xrow + 64 * j) : zero;
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[w][(4 * q4 + i) * 16 + r] = acc[i];
    __syncthreads();
    if (w != 0 || !mrow) return;
    i32x4 tot;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = (4 * q4 + i) * 16 + r;
        tot[i] = part[0][e] + part[1][e] + part[2][e] + part[3][e];
    }
    epilogue4<T>(p, *p.count, r, n0 + 4 * q4, tot);
}

// M > 16.  grid (ceil(N / 128), ceil(M / 128)).  LDS images: rows of 128 codes (8 pieces of 16 bytes), piece c of row r at
// 128 r + 16 (c ^ (r & 7)): the 16 lanes that read one piece of 16 consecutive rows touch every bank equally.  Rows past the
// matrix edge re-read its last row; their results are not stored.
constexpr int TILE = 128, TILE_K = 128, TILE_BYTES = TILE * TILE_K;
__device__ __forceinline__ int swz(int row, int piece) { return row * TILE_K + ((piece ^ (row & 7)) << 4); }

template <typename T>
__global__ __launch_bounds__(256) void int8_tile_kernel(const Int8LinearArgs p) {
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];          // [2 stages][CB tile | CA tile]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q4 = lane >> 4;
    const int wn = w & 1, wm = w >> 1;
    const int n0 = TILE * blockIdx.x, m0 = TILE * blockIdx.y, nk = (p.K + TILE_K - 1) / TILE_K;
    const int koff = 16 * (tid & 7);          // K % 128 may be 64: the last step's upper pieces are zeros then
    // this thread's four pieces of each tile: piece index tid + 256 i -> row (idx >> 3), piece (idx & 7)
    const int8_t* gsrc[2][4];
    int ldst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, piece = idx & 7;
        gsrc[0][i] = p.cb + (int64_t)min(n0 + row, p.N - 1) * p.K + 16 * piece;
        gsrc[1][i] = p.ca + (int64_t)min(m0 + row, p.M - 1) * p.K + 16 * piece;
        ldst[i] = swz(row, piece);
    }
    i32x4 stage[2][4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                stage[o][i] = TILE_K * kt + koff < p.K ? *reinterpret_cast<const i32x4*>(gsrc[o][i] + TILE_K * kt) : i32x4{0, 0, 0, 0};
    };
    auto park = [&](int s) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<i32x4*>(lds + (2 * s + o) * TILE_BYTES + ldst[i]) = stage[o][i];
    };
    i32x4 acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = i32x4{0, 0, 0, 0};
    fetch(0);
    park(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int s = kt & 1;
        if (kt + 1 < nk) fetch(kt + 1);
        const int8_t* sa = lds + (2 * s) * TILE_BYTES;
        const int8_t* sb = sa + TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x4 a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = *reinterpret_cast<const i32x4*>(sa + swz(64 * wn + 16 * t + r, 4 * ks + q4));
                b[t] = *reinterpret_cast<const i32x4*>(sb + swz(64 * wm + 16 * t + r, 4 * ks + q4));
            }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
        }
        if (kt + 1 < nk) park(s ^ 1);
        __syncthreads();
    }
    const int cnt = *p.count;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int m = m0 + 64 * wm + 16 * tj + r;
        if (m >= p.M) continue;
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            const int n = n0 + 64 * wn + 16 * ti + 4 * q4;
            if (n < p.N) epilogue4<T>(p, cnt, m, n, acc[ti][tj]);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static bool piece_aligned(const void* p, int64_t stride, int es) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (stride * es) % 16 == 0;
}
static int int8_shape_check(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1 || K % 64 || N % 16 || (int64_t)K * 16129 >= (int64_t)1 << 31) return FASTMAX_E_BAD_SHAPE;
    return FASTMAX_OK;
}
struct Int8Workspace { size_t ca, sca, flags, list, count, total; };
static Int8Workspace int8_workspace(int M, int K) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    Int8Workspace w;
    w.ca = 0;
    w.sca = w.ca + up((size_t)M * K);
    w.flags = w.sca + up((size_t)M * 4);
    w.list = w.flags + up((size_t)K);
    w.count = w.list + up((size_t)K * 4);
    w.total = w.count + 16;
    return w;
}

template <typename T>
static int launch_rows(const void* x, int64_t ldx, float threshold, int8_t* ca, float* sca, uint8_t* flags, int32_t* list,
                       int32_t* count, int M, int K, hipStream_t st) {
    const T* xt = reinterpret_cast<const T*>(x);
    hipLaunchKernelGGL((int8_flags_kernel<T>), dim3(K / 64), dim3(256), 0, st, xt, ldx, threshold, flags, M);
    hipLaunchKernelGGL((int8_rows_kernel<T>), dim3(M + 1), dim3(256), 0, st, xt, ldx, flags, ca, sca, list, count, M, K);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_product(const Int8LinearArgs& p, hipStream_t st) {
    if (p.M <= FASTMAX_INT8_FEW_ROWS) {
        hipLaunchKernelGGL((int8_few_rows_kernel<T>), dim3(p.N / 16), dim3(256), 0, st, p);
    } else {
        const dim3 grid((p.N + TILE - 1) / TILE, (p.M + TILE - 1) / TILE);
        hipLaunchKernelGGL((int8_tile_kernel<T>), grid, dim3(256), 4 * TILE_BYTES, st, p);
    }
    return (int)hipGetLastError();
}

}  // namespace fastmax

using namespace fastmax;

extern "C" {

int fastmax_hip_int8_quantize_weight(const void* w, int64_t w_stride, int dtype, int8_t* cb, float* scb, int N, int K, void* stream) {
    if (!w || !cb || !scb) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_F32 && dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    const int rc = int8_shape_check(1, N, K);
    if (rc) return rc;
    if (w_stride < K) return FASTMAX_E_BAD_SHAPE;
    if (!piece_aligned(w, w_stride, dtype == FASTMAX_F32 ? 4 : 2) || !piece_aligned(cb, 0, 1) || (reinterpret_cast<uintptr_t>(scb) & 3))
        return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(N), blk(256);
    if (dtype == FASTMAX_F32) hipLaunchKernelGGL((int8_quantize_weight_kernel<float>), grid, blk, 0, st, (const float*)w, w_stride, cb, scb, K);
    else if (dtype == FASTMAX_BF16) hipLaunchKernelGGL((int8_quantize_weight_kernel<__bf16>), grid, blk, 0, st, (const __bf16*)w, w_stride, cb, scb, K);
    else hipLaunchKernelGGL((int8_quantize_weight_kernel<_Float16>), grid, blk, 0, st, (const _Float16*)w, w_stride, cb, scb, K);
    return (int)hipGetLastError();
}

int fastmax_hip_int8_dequantize_weight(const int8_t* cb, const float* scb, void* w, int64_t w_stride, int dtype, int N, int K,
                                       void* stream) {
    if (!w || !cb || !scb) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_F32 && dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    const int rc = int8_shape_check(1, N, K);
    if (rc) return rc;
    if (w_stride < K) return FASTMAX_E_BAD_SHAPE;
    if (!piece_aligned(cb, 0, 1) || (reinterpret_cast<uintptr_t>(w) & (dtype == FASTMAX_F32 ? 3 : 1))) return FASTMAX_E_ALIGNMENT;
    const int64_t nb = ((int64_t)N * (K / 16) + 255) / 256;
    if (nb > 0x7fffffff) return FASTMAX_E_BAD_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)nb), blk(256);
    if (dtype == FASTMAX_F32) hipLaunchKernelGGL((int8_dequantize_weight_kernel<float>), grid, blk, 0, st, cb, scb, (float*)w, w_stride, N, K);
    else if (dtype == FASTMAX_BF16) hipLaunchKernelGGL((int8_dequantize_weight_kernel<__bf16>), grid, blk, 0, st, cb, scb, (__bf16*)w, w_stride, N, K);
    else hipLaunchKernelGGL((int8_dequantize_weight_kernel<_Float16>), grid, blk, 0, st, cb, scb, (_Float16*)w, w_stride, N, K);
    return (int)hipGetLastError();
}

int fastmax_hip_int8_quantize_rows(const void* x, int64_t x_stride, int dtype, float threshold, int8_t* ca, float* sca,
                                   uint8_t* flags, int32_t* list, int32_t* count, int M, int K, void* stream) {
    if (!x || !ca || !sca || !flags || !list || !count) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    const int rc = int8_shape_check(M, 16, K);
    if (rc) return rc;
    if (x_stride < K) return FASTMAX_E_BAD_SHAPE;
    if (!piece_aligned(x, x_stride, 2) || (reinterpret_cast<uintptr_t>(ca) & 7) || (reinterpret_cast<uintptr_t>(flags) & 7) ||
        (reinterpret_cast<uintptr_t>(sca) & 3) || (reinterpret_cast<uintptr_t>(list) & 3) || (reinterpret_cast<uintptr_t>(count) & 3))
        return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? launch_rows<__bf16>(x, x_stride, threshold, ca, sca, flags, list, count, M, K, st)
                                 : launch_rows<_Float16>(x, x_stride, threshold, ca, sca, flags, list, count, M, K, st);
}

size_t fastmax_hip_int8_linear_workspace(int M, int K) {
    if (int8_shape_check(M, 16, K)) return 0;
    return int8_workspace(M, K).total;
}

int fastmax_hip_int8_linear(const void* x, int64_t x_stride, const int8_t* cb, const float* scb, const float* bias, void* y,
                            int64_t y_stride, int M, int N, int K, int dtype, float threshold, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!x || !cb || !scb || !y || !workspace) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    const int rc = int8_shape_check(M, N, K);
    if (rc) return rc;
    if (x_stride < K || y_stride < N) return FASTMAX_E_BAD_SHAPE;
    if (!piece_aligned(x, x_stride, 2) || !piece_aligned(y, y_stride, 2) || !piece_aligned(cb, 0, 1) || !piece_aligned(scb, 0, 4) ||
        !piece_aligned(workspace, 0, 1) || (reinterpret_cast<uintptr_t>(bias) & 3))
        return FASTMAX_E_ALIGNMENT;
    const Int8Workspace ws = int8_workspace(M, K);
    if (workspace_bytes < ws.total) return FASTMAX_E_WORKSPACE;
    char* base = reinterpret_cast<char*>(workspace);
    int8_t* ca = reinterpret_cast<int8_t*>(base + ws.ca);
    float* sca = reinterpret_cast<float*>(base + ws.sca);
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + ws.flags);
    int32_t* list = reinterpret_cast<int32_t*>(base + ws.list);
    int32_t* count = reinterpret_cast<int32_t*>(base + ws.count);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Int8LinearArgs p{x, x_stride, ca, cb, sca, scb, bias, list, count, y, y_stride, M, N, K};
    if (dtype == FASTMAX_BF16) {
        const int err = launch_rows<__bf16>(x, x_stride, threshold, ca, sca, flags, list, count, M, K, st);
        return err ? err : launch_product<__bf16>(p, st);
    }
    const int err = launch_rows<_Float16>(x, x_stride, threshold, ca, sca, flags, list, count, M, K, st);
    return err ? err : launch_product<_Float16>(p, st);
}

}  // extern "C"
