// Causal softmax attention, backward, on the matrix cores (include/fastmax_hip_softmax.h: fastmax_hip_softmax_backward).
//
// With c = scale log2 e, L_i = lse_i of the forward and r = H / Hkv, for j <= i:
//     P_ij = exp2(c s_ij - L_i log2 e)      s_ij = q_i . k_j, float32, never stored
//     D_i  = sum_c dO_ic o_ic               float32, from the forward's own (rounded) o
//     dS_ij = P_ij (dO_i . v_j - D_i)
//     dQ_i = scale sum_{j <= i} dS_ij k_j,   dK_j = scale sum_{h in group} sum_{i >= j} dS_ij q_i,   dV_j = sum_h sum_{i >= j} P_ij dO_i
// Two tile kernels, each of which recomputes S and dP (7 products, not 5): every sum has one order, there are no atomics and two
// calls give the same bits.  Both keep the forward's orientation trick: operand roles are chosen so that the score tile comes out
// of the matrix core in the lane layout of the next product's B operand, so P and dS never pass through LDS.
//
// dQ kernel (the forward's mirror).  A workgroup of 4 waves owns (b, h, 128 query rows), a wave 32 of them; blocks with the longest
// key loops are issued first; tiles above a wave's diagonal are never visited.
//   Q,dO  the wave's rows as DP / 16 B-operand fragments each, in registers for the whole key loop.
//   D_i   from those dO fragments and the matching rows of o: a lane sums its 8-column pieces in ascending order, the two halves
//         of a row are added once; lanes < 32 write it to the workspace (B, H, N), where the dK/dV kernel, launched after this one,
//         reads it.  L_i and D_i are one scalar each per lane.
//   K,V   64-key tiles in LDS, double-buffered through registers, one barrier per tile.  V rows are padded to 2 DP + 16 bytes (row
//         reads), K rows to 2 DP + 64 bytes: the K image is read by rows AND transposed.
//   S^T = K Q^T, dP^T = V dO^T per 32-key sub-tile: A = a row of the K / V image, B = the Q / dO fragments.  A lane holds one
//         query row and 16 keys.  Keys above the row are SELECTED to -inf before the exponential on the diagonal sub-tile.
//   dQ^T += K^T dS^T: dS^T rounded to the input dtype is the B operand, K^T comes from the K image by ds_read_b64_tr_b16.
// dK/dV kernel.  A workgroup of 4 waves owns (b, KV head g, 128 keys), a wave 32 of them; key block 0 has the longest loop and is
// blockIdx.y = 0.  The workgroup walks the r query heads of its group in ascending order and within a head the 64-row query tiles
// from its diagonal to N, as ONE sequence of tiles, so the double buffer runs across heads.
//   K,V   the wave's keys as B-operand fragments, in registers for the whole kernel.
//   Q,dO  64-row tiles in LDS (rows padded to 2 DP + 64 bytes: read by rows and transposed), with the tile's 64 L_i log2 e and 64
//         D_i behind them.  Rows >= N are staged as Q = dO = 0, D = 0, L = +inf: their P is exactly 0 and the forward's lse, which
//         has no such rows, is not read there.
//   S = Q K^T, dP = dO V^T: A = a row of the Q / dO image.  A lane holds one key and 16 queries -- the B-operand layout with the
//         queries as the summed dimension; L and D of those 16 queries are four 16-byte broadcast reads each.
//   dV^T += dO^T P, dK^T += Q^T dS: A by transposed reads of the dO and Q images.  Sub-tiles wholly above the diagonal are skipped;
//         on the diagonal sub-tile queries above the key are selected to P = 0.
//   Both accumulators are float32 and run over all r heads before anything is rounded: one rounding per output element.  dK is
//   multiplied by scale at the store.
// Instances: DP = 64, 128; D any multiple of 8 up to 128; any N >= 1.  LDS: dQ 43,008 / 75,776 bytes, dK/dV 50,176 / 82,944 bytes.
// Register counts are in DESIGN.md 4.6b.
#include "../../include/fastmax_hip_softmax.h"
#include "fastmax_mfma32_common.h"

#include <cmath>

namespace fastmax {
namespace softmax_bwd {

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

constexpr int NW = 4, NT = 64 * NW, ROWS = 32 * NW, TK = 64;          // waves, threads, rows (keys) per workgroup, rows per tile
constexpr int MAX_D = 128;
constexpr float LOG2E = 1.4426950408889634f;
template <int DP> constexpr int row_rd() { return 2 * DP + 16; }          // an image read by rows only
template <int DP> constexpr int row_tr() { return 2 * DP + 64; }          // an image that is also read transposed
template <int DP> constexpr int dq_buf() { return TK * (row_tr<DP>() + row_rd<DP>()); }
template <int DP> constexpr int kv_buf() { return 2 * TK * row_tr<DP>() + 2 * TK * 4; }

struct Args {
    const void *q, *k, *v, *go;
    Strides3 qs, ks, vs, gos;
    const void* o;
    const float* lse;
    void *dq, *dk, *dv;
    float* delta;          // the workspace: D_i, (B, H, N)
    int B, H, Hkv, N, D;
    float c, scale;        // scale * log2(e), scale
};

// the 16-byte pieces of one tile pair that a thread moves: PP per matrix
template <int DP> struct Pieces {
    static constexpr int PP = TK * (DP / 8) / NT;
    uint4 x[PP], y[PP];
};

// rows row0 .. row0 + 63 of two matrices (row strides xsn, ysn); columns >= D and rows >= N come as zeros
template <int DP>
__device__ __forceinline__ void load_pair(Pieces<DP>& r, const uint16_t* xb, const uint16_t* yb, int64_t xsn, int64_t ysn, int row0, int N,
                                          int D) {
#pragma unroll
    for (int u = 0; u < Pieces<DP>::PP; ++u) {
        const int i = threadIdx.x + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        const bool live = row0 + row < N && 8 * pc < D;
        r.x[u] = live ? *reinterpret_cast<const uint4*>(xb + (int64_t)(row0 + row) * xsn + 8 * pc) : uint4{0, 0, 0, 0};
        r.y[u] = live ? *reinterpret_cast<const uint4*>(yb + (int64_t)(row0 + row) * ysn + 8 * pc) : uint4{0, 0, 0, 0};
    }
}

template <int DP, int XROW, int YROW> __device__ __forceinline__ void store_pair(const Pieces<DP>& r, char* buf) {
    char* yimg = buf + TK * XROW;
#pragma unroll
    for (int u = 0; u < Pieces<DP>::PP; ++u) {
        const int i = threadIdx.x + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        *reinterpret_cast<uint4*>(buf + row * XROW + 16 * pc) = r.x[u];
        *reinterpret_cast<uint4*>(yimg + row * YROW + 16 * pc) = r.y[u];
    }
}

// A operand of the 32x32x16 product from an image with RB bytes per row, transposed: lane (d = lane & 31, h = lane >> 5) receives
// rows row0 + 4 h + {0..3} and row0 + 8 + 4 h + {0..3} of column col0 + d
template <typename V8, int RB> __device__ __forceinline__ V8 ld_t(const char* img, int row0, int col0, int lane) {
    const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const char* a = img + (row0 + 4 * (g >> 1) + qq) * RB + 2 * (col0 + 16 * (g & 1) + 4 * pp);
    union { V8 v; s16x4 h[2]; } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 8 * RB));
    return u.v;
}

// the row (register i of an accumulator tile, half hh of the wave) inside a 32-row sub-tile
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// grid: (B * H, ceil(N / ROWS)); block: NT
template <typename T, int DP>
__global__ __launch_bounds__(NT) void softmax_dq_kernel(const Args a) {
    typedef typename Op<T>::v8 V8;
    constexpr int KS = DP / 16, DT = DP / 32, KROW = row_tr<DP>(), VROW = row_rd<DP>(), BUF = dq_buf<DP>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H, g = h / (a.H / a.Hkv);
    const int q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * ROWS;          // heaviest blocks first
    const int N = a.N, D = a.D;
    const int row_first = q0 + 32 * w, row = row_first + l31;
    const int64_t slab = ((int64_t)b * a.H + h) * N;
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.qs.sb + (int64_t)h * a.qs.sh + (int64_t)row * a.qs.sn;
    const uint16_t* grow = reinterpret_cast<const uint16_t*>(a.go) + (int64_t)b * a.gos.sb + (int64_t)h * a.gos.sh + (int64_t)row * a.gos.sn;
    const uint16_t* orow = reinterpret_cast<const uint16_t*>(a.o) + (slab + row) * D;
    const uint16_t* kb = reinterpret_cast<const uint16_t*>(a.k) + (int64_t)b * a.ks.sb + (int64_t)g * a.ks.sh;
    const uint16_t* vb = reinterpret_cast<const uint16_t*>(a.v) + (int64_t)b * a.vs.sb + (int64_t)g * a.vs.sh;

    V8 qf[KS], gf[KS];
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * hh;
        const bool live = row < N && col < D;
        qf[s] = __builtin_bit_cast(V8, live ? *reinterpret_cast<const uint4*>(qrow + col) : uint4{0, 0, 0, 0});
        gf[s] = __builtin_bit_cast(V8, live ? *reinterpret_cast<const uint4*>(grow + col) : uint4{0, 0, 0, 0});
        const V8 of = __builtin_bit_cast(V8, live ? *reinterpret_cast<const uint4*>(orow + col) : uint4{0, 0, 0, 0});
#pragma unroll
        for (int j = 0; j < 8; ++j) delta = fmaf((float)gf[s][j], (float)of[j], delta);
    }
    delta += __shfl_xor(delta, 32, 64);
    const float L2 = row < N ? a.lse[slab + row] * LOG2E : INFINITY;          // rows >= N: P = exp2(-inf) = 0
    if (row < N && hh == 0) a.delta[slab + row] = delta;

    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;

    const int last_row = q0 + ROWS - 1 < N - 1 ? q0 + ROWS - 1 : N - 1;
    const int ntile = last_row / TK + 1;                      // the workgroup's key tiles
    const int my_tiles = row_first < N ? row_first / TK + 1 : 0;          // this wave's: up to its diagonal
    Pieces<DP> pcs;
    load_pair<DP>(pcs, kb, vb, a.ks.sn, a.vs.sn, 0, N, D);
    store_pair<DP, KROW, VROW>(pcs, smem);
    __syncthreads();
    for (int kt = 0; kt < ntile; ++kt) {
        const char* kimg = smem + (kt & 1) * BUF;
        const char* vimg = kimg + TK * KROW;
        const bool more = kt + 1 < ntile;
        if (more) load_pair<DP>(pcs, kb, vb, a.ks.sn, a.vs.sn, (kt + 1) * TK, N, D);
        if (kt < my_tiles) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k0 = kt * TK + 32 * t;
                if (k0 > row_first) continue;                  // wholly above the wave's diagonal
                f32x16 st, dp;
#pragma unroll
                for (int i = 0; i < 16; ++i) st[i] = 0.f, dp[i] = 0.f;
                const char* krow = kimg + (32 * t + l31) * KROW + 16 * hh;
                const char* vrow = vimg + (32 * t + l31) * VROW + 16 * hh;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    st = Op<T>::mma(*reinterpret_cast<const V8*>(krow + 32 * s), qf[s], st);
                    dp = Op<T>::mma(*reinterpret_cast<const V8*>(vrow + 32 * s), gf[s], dp);
                }
                const bool diag = k0 == row_first;
                float ds[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float x = st[i] * a.c - L2;
                    if (diag && k0 + acc_row(i, hh) > row) x = -INFINITY;
                    ds[i] = __builtin_amdgcn_exp2f(x) * (dp[i] - delta);
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const V8 dsf = Op<T>::round8(ds + 8 * s);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        acc[dt] = Op<T>::mma(ld_t<V8, KROW>(kimg, 32 * t + 16 * s, 32 * dt, lane), dsf, acc[dt]);
                }
            }
        }
        if (more) store_pair<DP, KROW, VROW>(pcs, smem + ((kt + 1) & 1) * BUF);
        __syncthreads();
    }
    // every wave is past the loop's last barrier: the tile buffers are free, a wave takes 4 KiB of them for its store
    store_tile32_t<DT>(smem + 4096 * w, acc, a.scale, lane, a.dq, Op<T>::DTYPE, slab, row_first, N, D);
}

// one staged query tile: Q and dO pieces, and for threads 0 .. 63 the row's L log2 e, for threads 64 .. 127 its D
template <int DP> struct QTile {
    Pieces<DP> p;
    float ld;
};

template <int DP>
__device__ __forceinline__ void load_qtile(QTile<DP>& r, const Args& a, int b, int h, int row0) {
    const uint16_t* qb = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.qs.sb + (int64_t)h * a.qs.sh;
    const uint16_t* gb = reinterpret_cast<const uint16_t*>(a.go) + (int64_t)b * a.gos.sb + (int64_t)h * a.gos.sh;
    load_pair<DP>(r.p, qb, gb, a.qs.sn, a.gos.sn, row0, a.N, a.D);
    const int t = threadIdx.x, row = row0 + (t & 63);
    const int64_t idx = ((int64_t)b * a.H + h) * a.N + row;
    r.ld = 0.f;
    if (t < 64) r.ld = row < a.N ? a.lse[idx] * LOG2E : INFINITY;
    else if (t < 128 && row < a.N) r.ld = a.delta[idx];
}

template <int DP> __device__ __forceinline__ void store_qtile(const QTile<DP>& r, char* buf) {
    store_pair<DP, row_tr<DP>(), row_tr<DP>()>(r.p, buf);
    if (threadIdx.x < 128) *reinterpret_cast<float*>(buf + 2 * TK * row_tr<DP>() + 4 * threadIdx.x) = r.ld;
}

// grid: (B * Hkv, ceil(N / ROWS)); block: NT
template <typename T, int DP>
__global__ __launch_bounds__(NT) void softmax_dkdv_kernel(const Args a) {
    typedef typename Op<T>::v8 V8;
    constexpr int KS = DP / 16, DT = DP / 32, QROW = row_tr<DP>(), BUF = kv_buf<DP>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / a.Hkv, g = blockIdx.x % a.Hkv, r = a.H / a.Hkv;
    const int N = a.N, D = a.D;
    const int k0 = (int)blockIdx.y * ROWS;                      // key block 0, the longest loop, first
    const int key_first = k0 + 32 * w, key = key_first + l31;
    const uint16_t* krow = reinterpret_cast<const uint16_t*>(a.k) + (int64_t)b * a.ks.sb + (int64_t)g * a.ks.sh + (int64_t)key * a.ks.sn;
    const uint16_t* vrow = reinterpret_cast<const uint16_t*>(a.v) + (int64_t)b * a.vs.sb + (int64_t)g * a.vs.sh + (int64_t)key * a.vs.sn;

    V8 kf[KS], vf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * hh;
        const bool live = key < N && col < D;
        kf[s] = __builtin_bit_cast(V8, live ? *reinterpret_cast<const uint4*>(krow + col) : uint4{0, 0, 0, 0});
        vf[s] = __builtin_bit_cast(V8, live ? *reinterpret_cast<const uint4*>(vrow + col) : uint4{0, 0, 0, 0});
    }
    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[dt][i] = 0.f, dv[dt][i] = 0.f;

    const int t0 = k0 / TK, nt = (N + TK - 1) / TK - t0;          // the query tiles of one head: from the block's diagonal to N
    const int items = r * nt;                                    // heads ascending, tiles ascending within a head
    const bool wave_live = key_first < N;
    QTile<DP> qt;
    load_qtile<DP>(qt, a, b, g * r, t0 * TK);
    store_qtile<DP>(qt, smem);
    __syncthreads();
    int hq = 0, tile = 0;                                        // of the item being computed
    for (int it = 0; it < items; ++it) {
        const char* qimg = smem + (it & 1) * BUF;
        const char* gimg = qimg + TK * QROW;
        const char* lds = gimg + TK * QROW;                       // 64 x L log2 e, 64 x D
        const bool more = it + 1 < items;
        const int nhq = tile + 1 < nt ? hq : hq + 1, ntile = tile + 1 < nt ? tile + 1 : 0;
        if (more) load_qtile<DP>(qt, a, b, g * r + nhq, (t0 + ntile) * TK);
        if (wave_live) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r0 = (t0 + tile) * TK + 32 * u;          // the sub-tile's first query row
                if (r0 < key_first || r0 >= N) continue;          // wholly above the diagonal, or past the sequence
                f32x16 st, dp;
#pragma unroll
                for (int i = 0; i < 16; ++i) st[i] = 0.f, dp[i] = 0.f;
                const char* qr = qimg + (32 * u + l31) * QROW + 16 * hh;
                const char* gr = gimg + (32 * u + l31) * QROW + 16 * hh;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    st = Op<T>::mma(*reinterpret_cast<const V8*>(qr + 32 * s), kf[s], st);
                    dp = Op<T>::mma(*reinterpret_cast<const V8*>(gr + 32 * s), vf[s], dp);
                }
                const bool diag = r0 == key_first;
                float p[16], ds[16];
#pragma unroll
                for (int ig = 0; ig < 4; ++ig) {
                    const f32x4 L2 = *reinterpret_cast<const f32x4*>(lds + 4 * (32 * u + 8 * ig + 4 * hh));
                    const f32x4 dl = *reinterpret_cast<const f32x4*>(lds + 4 * (TK + 32 * u + 8 * ig + 4 * hh));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = 4 * ig + e;
                        float x = st[i] * a.c - L2[e];
                        if (diag && r0 + acc_row(i, hh) < key) x = -INFINITY;
                        p[i] = __builtin_amdgcn_exp2f(x);
                        ds[i] = p[i] * (dp[i] - dl[e]);
                    }
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const V8 pf = Op<T>::round8(p + 8 * s), dsf = Op<T>::round8(ds + 8 * s);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        dv[dt] = Op<T>::mma(ld_t<V8, QROW>(gimg, 32 * u + 16 * s, 32 * dt, lane), pf, dv[dt]);
                        dk[dt] = Op<T>::mma(ld_t<V8, QROW>(qimg, 32 * u + 16 * s, 32 * dt, lane), dsf, dk[dt]);
                    }
                }
            }
        }
        if (more) store_qtile<DP>(qt, smem + ((it + 1) & 1) * BUF);
        __syncthreads();
        hq = nhq, tile = ntile;
    }
    // every wave is past the loop's last barrier: the tile buffers are free, a wave takes 4 KiB of them for its stores
    const int64_t slab = ((int64_t)b * a.Hkv + g) * N;
    store_tile32_t<DT>(smem + 4096 * w, dk, a.scale, lane, a.dk, Op<T>::DTYPE, slab, key_first, N, D);
    store_tile32_t<DT>(smem + 4096 * w, dv, 1.0f, lane, a.dv, Op<T>::DTYPE, slab, key_first, N, D);
}

template <typename T, int DP> static int launch(const Args& a, hipStream_t stream) {
    auto kq = softmax_dq_kernel<T, DP>;
    auto kkv = softmax_dkdv_kernel<T, DP>;
    constexpr int lds_q = 2 * dq_buf<DP>(), lds_kv = 2 * kv_buf<DP>();
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kq), hipFuncAttributeMaxDynamicSharedMemorySize, lds_q);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kkv), hipFuncAttributeMaxDynamicSharedMemorySize, lds_kv);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const unsigned blocks = (unsigned)((a.N + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(kq, dim3((unsigned)(a.B * a.H), blocks), dim3(NT), lds_q, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kkv, dim3((unsigned)(a.B * a.Hkv), blocks), dim3(NT), lds_kv, stream, a);          // reads the D_i of the first
    return (int)hipGetLastError();
}

template <typename T> static int launch_dp(const Args& a, hipStream_t stream) {
    return a.D <= 64 ? launch<T, 64>(a, stream) : launch<T, 128>(a, stream);
}

static bool pieces(const void* p, const int64_t* s) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0;
}

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace softmax_bwd
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::softmax_bwd;

extern "C" {

size_t fastmax_hip_softmax_backward_workspace(int B, int H, int N, int D) {
    if (B <= 0 || H <= 0 || N <= 0 || D < 8 || D > MAX_D || D % 8 != 0 || (int64_t)B * H > 65535 || ((int64_t)N + ROWS - 1) / ROWS > 65535)
        return 0;
    return (size_t)B * H * N * sizeof(float);
}

int fastmax_hip_softmax_backward(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                 const int64_t* v_strides, const void* o, const float* lse, const void* grad_o,
                                 const int64_t* go_strides, void* dq, void* dk, void* dv, int B, int H, int Hkv, int N, int D, int dtype,
                                 float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !o || !lse || !grad_o || !go_strides || !dq || !dk || !dv || !workspace)
        return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (Hkv <= 0 || H % Hkv != 0 || !std::isfinite(scale) || fastmax_hip_softmax_backward_workspace(B, H, N, D) == 0)
        return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(k, k_strides) || !pieces(v, v_strides) || !pieces(grad_o, go_strides) || !aligned16(o) ||
        !aligned16(dq) || !aligned16(dk) || !aligned16(dv) || reinterpret_cast<uintptr_t>(lse) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(workspace) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_softmax_backward_workspace(B, H, N, D)) return FASTMAX_E_WORKSPACE;
    Args a;
    a.q = q, a.k = k, a.v = v, a.go = grad_o, a.o = o, a.lse = lse, a.dq = dq, a.dk = dk, a.dv = dv;
    a.delta = reinterpret_cast<float*>(workspace);
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.gos = Strides3{go_strides[0], go_strides[1], go_strides[2]};
    a.B = B, a.H = H, a.Hkv = Hkv, a.N = N, a.D = D;
    a.c = scale * LOG2E, a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? launch_dp<bf16_t>(a, st) : launch_dp<f16_t>(a, st);
}

}  // extern "C"
