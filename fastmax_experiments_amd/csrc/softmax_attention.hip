// Causal softmax attention, forward, on the matrix cores (include/fastmax_hip_softmax.h: fastmax_hip_softmax_forward).
//
//     o_i = sum_{j <= i} p_ij v_j / sum_{j <= i} p_ij,   p_ij = exp(scale q_i . k_j - max_j),   lse_i = log sum_j exp(scale q_i . k_j)
//
// Work split.  A workgroup of 4 waves owns (b, query head h, 128 query rows); a wave owns 32 of the rows.  The grid is
// (B * H, blocks of 128 rows) and the block index counts DOWN with blockIdx.y, so the blocks with the longest key loops are
// issued first and the causal triangle's tail is made of the short ones.  K and V are read at KV head h / (H / Hkv) through their
// own strides: nothing is copied per query head.
//
// Data flow of a wave, per 64-key tile (tiles above the wave's diagonal are never visited):
//   Q    the wave's 32 rows as DP / 16 B-operand fragments (lane: row lane & 31, columns 16 s + 8 (lane >> 5) ..+7), loaded once
//        from global memory, in registers for the whole key loop; never scaled.
//   K,V  64 rows x DP columns each, staged by all 256 threads as 16-byte pieces into LDS; columns D .. DP - 1 and rows >= N are
//        written as zeros.  Two buffers: the next tile's pieces are loaded from global memory into registers before the matrix
//        work on the current buffer and stored into the other buffer after it; one barrier per tile.  K rows are padded to
//        2 DP + 16 bytes (row reads), V rows to 2 DP + 64 bytes (transposed reads).
//   S^T  = K Q^T per 32-key sub-tile: v_mfma_f32_32x32x16 with K as the A operand (ds_read_b128 of a row) and Q as B.  A lane
//        then holds ONE query row (lane & 31) and 16 of the 32 keys, registers 8 s .. 8 s + 7 = keys 16 s + 4 (lane >> 5) + {0..3},
//        16 s + 8 + 4 (lane >> 5) + {0..3}: exactly a B-operand fragment of the next product, so P never goes through LDS.
//   softmax  x = s * (scale * log2 e) in float32; on the diagonal sub-tile (key0 == the wave's first row) keys above the row are
//        SELECTED to -inf; m' = max(m, max x) over the lane's registers and the partner lane ^ 32; the accumulator and the row
//        sum are multiplied by exp2(m - m'); p = exp2(x - m'); the row sum adds the float32 p (per lane, the two halves are
//        added once at the end); p is rounded to the input dtype as the operand of P V only.
//   O^T  += V^T P^T: V^T as the A operand by ds_read_b64_tr_b16 (a 16-lane block reads 4 rows x 16 columns and receives them
//        transposed), P^T as B from the registers.  DP / 32 accumulator tiles of 32 columns x 32 rows, float32.
//   out  the accumulator tiles times 1 / l go out through store_tile32_t (whole 16-byte row segments); lanes 0 .. 31 write lse.
// Instances are padded to DP = 64, 128, 256 columns; D is any multiple of 8 up to DP.  No atomics; every sum has one order.
//
// Resources (hipcc --save-temps, gfx950): DP = 64: 40,960 bytes of LDS; 128: 73,728; 256: 141,312.  Register counts are in
// DESIGN.md 4.6a.
#include "../../include/fastmax_hip_softmax.h"
#include "fastmax_mfma32_common.h"

#include <cmath>

namespace fastmax {
namespace softmax {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

template <typename T> struct Op;
template <> struct Op<bf16_t> {
    typedef bf16x8 v8;
    static constexpr int DTYPE = FASTMAX_BF16;
    static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v8 round8(const float* x) {
        v8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (__bf16)x[i];
        return r;
    }
};
template <> struct Op<f16_t> {
    typedef h8 v8;
    static constexpr int DTYPE = FASTMAX_F16;
    static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v8 round8(const float* x) {
        v8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (_Float16)x[i];
        return r;
    }
};

constexpr int NW = 4, NT = 64 * NW, ROWS = 32 * NW, TK = 64;          // waves, threads, query rows per workgroup, keys per tile
template <int DP> constexpr int k_row() { return 2 * DP + 16; }
template <int DP> constexpr int v_row() { return 2 * DP + 64; }
template <int DP> constexpr int buf_bytes() { return TK * (k_row<DP>() + v_row<DP>()); }
template <int DP> constexpr int lds_bytes() { return 2 * buf_bytes<DP>(); }

struct Args {
    const void *q, *k, *v;
    Strides3 qs, ks, vs;
    void* o;
    float* lse;
    int B, H, Hkv, N, D;
    float c;          // scale * log2(e)
};

// the 16-byte pieces of one K / V tile that a thread moves: PP per matrix
template <int DP> struct Pieces {
    static constexpr int PP = TK * (DP / 8) / NT;
    uint4 k[PP], v[PP];
};

template <typename T, int DP>
__device__ __forceinline__ void load_tile(Pieces<DP>& r, const uint16_t* kb, const uint16_t* vb, int64_t ksn, int64_t vsn, int key0, int N,
                                          int D) {
#pragma unroll
    for (int u = 0; u < Pieces<DP>::PP; ++u) {
        const int i = threadIdx.x + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        const bool live = key0 + row < N && 8 * pc < D;
        r.k[u] = live ? *reinterpret_cast<const uint4*>(kb + (int64_t)(key0 + row) * ksn + 8 * pc) : uint4{0, 0, 0, 0};
        r.v[u] = live ? *reinterpret_cast<const uint4*>(vb + (int64_t)(key0 + row) * vsn + 8 * pc) : uint4{0, 0, 0, 0};
    }
}

template <int DP> __device__ __forceinline__ void store_tile(const Pieces<DP>& r, char* buf) {
    char* vimg = buf + TK * k_row<DP>();
#pragma unroll
    for (int u = 0; u < Pieces<DP>::PP; ++u) {
        const int i = threadIdx.x + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        *reinterpret_cast<uint4*>(buf + row * k_row<DP>() + 16 * pc) = r.k[u];
        *reinterpret_cast<uint4*>(vimg + row * v_row<DP>() + 16 * pc) = r.v[u];
    }
}

// A operand of the 32x32x16 product from the V image, transposed: lane (d = lane & 31, h = lane >> 5) receives rows
// row0 + 4 h + {0..3} and row0 + 8 + 4 h + {0..3} of column col0 + d
template <typename V8, int DP> __device__ __forceinline__ V8 ld_vt(const char* vimg, int row0, int col0, int lane) {
    const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const char* a = vimg + (row0 + 4 * (g >> 1) + qq) * v_row<DP>() + 2 * (col0 + 16 * (g & 1) + 4 * pp);
    union { V8 v; s16x4 h[2]; } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 8 * v_row<DP>()));
    return u.v;
}

// grid: (B * H, ceil(N / ROWS)); block: NT
template <typename T, int DP>
__global__ __launch_bounds__(NT) void softmax_fwd_kernel(const Args a) {
    typedef typename Op<T>::v8 V8;
    constexpr int KS = DP / 16, DT = DP / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H, g = h / (a.H / a.Hkv);
    const int q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * ROWS;          // heaviest blocks first
    const int N = a.N, D = a.D;
    const int row_first = q0 + 32 * w, row = row_first + l31;
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.qs.sb + (int64_t)h * a.qs.sh + (int64_t)row * a.qs.sn;
    const uint16_t* kb = reinterpret_cast<const uint16_t*>(a.k) + (int64_t)b * a.ks.sb + (int64_t)g * a.ks.sh;
    const uint16_t* vb = reinterpret_cast<const uint16_t*>(a.v) + (int64_t)b * a.vs.sb + (int64_t)g * a.vs.sh;

    V8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * hh;
        const uint4 x = (row < N && col < D) ? *reinterpret_cast<const uint4*>(qrow + col) : uint4{0, 0, 0, 0};
        qf[s] = __builtin_bit_cast(V8, x);
    }
    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
    float m = -INFINITY, l = 0.f;

    const int last_row = q0 + ROWS - 1 < N - 1 ? q0 + ROWS - 1 : N - 1;
    const int ntile = last_row / TK + 1;                      // the workgroup's key tiles
    const int my_tiles = row_first < N ? row_first / TK + 1 : 0;          // this wave's: up to its diagonal
    Pieces<DP> pcs;
    load_tile<T, DP>(pcs, kb, vb, a.ks.sn, a.vs.sn, 0, N, D);
    store_tile<DP>(pcs, smem);
    __syncthreads();
    for (int kt = 0; kt < ntile; ++kt) {
        const char* kimg = smem + (kt & 1) * buf_bytes<DP>();
        const char* vimg = kimg + TK * k_row<DP>();
        const bool more = kt + 1 < ntile;
        if (more) load_tile<T, DP>(pcs, kb, vb, a.ks.sn, a.vs.sn, (kt + 1) * TK, N, D);
        if (kt < my_tiles) {
            const int key0 = kt * TK;
            const bool two = key0 + 32 <= row_first;           // the second sub-tile is at or below the diagonal
            f32x16 st[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int i = 0; i < 16; ++i) st[t][i] = 0.f;
                if (t == 0 || two) {
                    const char* krow = kimg + (32 * t + l31) * k_row<DP>() + 16 * hh;
#pragma unroll
                    for (int s = 0; s < KS; ++s) st[t] = Op<T>::mma(*reinterpret_cast<const V8*>(krow + 32 * s), qf[s], st[t]);
                }
            }
            // scale, mask by selection on the diagonal sub-tile, tile maximum
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k0 = key0 + 32 * t;
                const bool diag = k0 == row_first;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                    float x = st[t][i] * a.c;
                    if ((t == 1 && !two) || (diag && key > row)) x = -INFINITY;
                    st[t][i] = x;
                    mx = fmaxf(mx, x);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);                      // finite: key k0 of sub-tile 0 is at or below every row of the wave
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[dt][i] *= alpha;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t == 0 || two) {
                    float p[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        p[i] = __builtin_amdgcn_exp2f(st[t][i] - mn);
                        l += p[i];
                    }
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const V8 pf = Op<T>::round8(p + 8 * s);
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt)
                            acc[dt] = Op<T>::mma(ld_vt<V8, DP>(vimg, 32 * t + 16 * s, 32 * dt, lane), pf, acc[dt]);
                    }
                }
            }
        }
        if (more) store_tile<DP>(pcs, smem + ((kt + 1) & 1) * buf_bytes<DP>());
        __syncthreads();
    }

    l += __shfl_xor(l, 32, 64);
    if (row < N && hh == 0 && a.lse)
        a.lse[((int64_t)b * a.H + h) * N + row] = (m + __builtin_amdgcn_logf(l)) * 0.69314718055994531f;
    // every wave is past the loop's last barrier: the tile buffers are free, a wave takes 4 KiB of them for its store
    store_tile32_t<DT>(smem + 4096 * w, acc, 1.0f / l, lane, a.o, Op<T>::DTYPE, ((int64_t)b * a.H + h) * N, row_first, N, D);
}

template <typename T, int DP> static int launch(const Args& a, hipStream_t stream) {
    auto kern = softmax_fwd_kernel<T, DP>;
    constexpr int lds = lds_bytes<DP>();
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const dim3 grid((unsigned)(a.B * a.H), (unsigned)((a.N + ROWS - 1) / ROWS));
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, stream, a);
    return (int)hipGetLastError();
}

template <typename T> static int launch_dp(const Args& a, hipStream_t stream) {
    if (a.D <= 64) return launch<T, 64>(a, stream);
    if (a.D <= 128) return launch<T, 128>(a, stream);
    return launch<T, 256>(a, stream);
}

static bool pieces(const void* p, const int64_t* s) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0;
}

}  // namespace softmax
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::softmax;

extern "C" int fastmax_hip_softmax_forward(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                           const void* v, const int64_t* v_strides, void* o, float* lse, int B, int H, int Hkv, int N,
                                           int D, int dtype, float scale, void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !o) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || N <= 0 || D < 8 || D > 256 || D % 8 != 0 || (int64_t)B * H > 65535 ||
        ((int64_t)N + ROWS - 1) / ROWS > 65535 || !std::isfinite(scale))
        return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(k, k_strides) || !pieces(v, v_strides) || reinterpret_cast<uintptr_t>(o) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(lse) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    Args a;
    a.q = q, a.k = k, a.v = v, a.o = o, a.lse = lse;
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.B = B, a.H = H, a.Hkv = Hkv, a.N = N, a.D = D;
    a.c = scale * 1.4426950408889634f;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? launch_dp<bf16_t>(a, st) : launch_dp<f16_t>(a, st);
}
