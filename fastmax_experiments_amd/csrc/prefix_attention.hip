// LLaMA-Adapter's gated prefix attention behind a causal softmax block (include/fastmax_hip_prefix.h).
//
//     out[b, h, i] = y[b, h, i] + gate[h] * sum_{j < aT} softmax_j(scale q[b, h, i] . ak[g, j]) av[g, j],   g = h / (H / Hkv)
//
// aT <= 32 prefix rows: ONE key tile, no mask, no running maximum.  Both kernels are streaming kernels (about 100 flop per byte of
// row traffic): each row tensor is read once and written once, the prefix lives in registers.
//
// Fragments (v_mfma_f32_32x32x16: A row / B column = lane & 31, k = 8 (lane >> 5) + j; C column = lane & 31, row(i) =
// (i & 3) + 8 (i >> 2) + 4 (lane >> 5)).  An A and a B fragment have the same shape, so a "row fragment" of 32 rows x DP columns
// (lane: row lane & 31, columns 16 s + 8 (lane >> 5) ..+7, s < DP / 16) serves as either.
//   akf, avf   row fragments of the head's ak / av; rows >= aT and columns >= D are zeros.
//   akt, avt   the same matrices transposed, as A operands over the keys: element j of fragment (s, dt) is key
//              16 s + 4 (lane >> 5) + (j & 3) + 8 (j >> 2) of column 32 dt + (lane & 31) -- the key order in which a lane holds an
//              S^T tile, so P^T and dS^T feed the next product from the registers they were computed in.
//   All of them are loaded once per workgroup, from global memory, and stay in registers for every tile the workgroup walks.
//
// Forward.  A workgroup of 4 waves owns (b, h, FWD_CHUNK = 256 query rows): a wave walks the chunk's 128-row tiles and owns 32
// rows of each.  Per tile and wave:
//   Q     DP / 16 B fragments straight from global memory through q's strides (16-byte pieces).
//   S^T   = AK Q^T (A = akf).  A lane holds ONE query row and 16 of the 32 keys; keys >= aT are SELECTED to -inf.
//   m, l  per-lane scalars over the 16 registers and the partner lane ^ 32; p = exp2(c s - m) in float32, rounded to the dtype
//         once as the B operand of
//   O^T   = AV^T P^T (A = avt), DP / 32 float32 tiles.
//   out   the tiles go through a wave-private 4 KiB LDS area as float32 (the swizzle of store_tile32_t's float path) and come back
//         as whole 16-byte row pieces: a lane reads the matching piece of y, adds gate * ay / l in float32, rounds ONCE and
//         writes the piece of out.  The lane that reads a piece of y is the one that writes it: out may alias y.
//   gate[h] == 0: the workgroup copies y's pieces (or returns, when out is y): out has y's bits, signed zeros included.
//
// Backward.  A workgroup of 4 waves owns (b, h, BWD_CHUNK = 512 query rows); a wave owns 32 rows of each of the chunk's four
// 128-row tiles.  Per tile and wave, with Q and dO as row fragments qf, gf from global memory (one read serves both orientations,
// as B operands below and as A operands after it; the same registers fill the wave's LDS images):
//   rows as lanes   S^T = AK Q^T, dP^T = AV dO^T (A = akf, avf; B = qf, gf).  P_ij = exp2(c s_ij - m_i) / l_i in float32;
//         D_i = sum_j P_ij dP_ij in float32 -- which IS sum_c dO_ic ay_ic with ay = sum_j P_ij av_j never rounded, without the
//         product that would form ay; dS^T = gate P (dP - D) rounded once is the B operand of dQ^T = AK^T dS^T (A = akt); dq
//         leaves through store_tile32_t times scale.  m_i, 1 / l_i, D_i go to 96 floats of the wave's LDS.
//   keys as lanes   S = Q AK^T, dP = dO AV^T (A = qf, gf; B = akf, avf): a lane holds one key and 16 query rows, whose m, 1 / l
//         and D are 16-byte broadcast reads.  P and dS, rounded once, are the B operands of dAV^T += dO^T P and dAK^T += Q^T dS,
//         whose A operands come by ds_read_b64_tr_b16 from the wave's LDS images of the dO and Q tiles (rows padded to 2 DP + 64
//         bytes).  Rows >= N are staged with m = +inf: their P is exactly 0.
//   The images and statistics are wave-private: the tile loop has no barrier.
// After its tiles a wave holds float32 partial dAK^T, dAV^T and sum_i D_i.  The four waves are merged through LDS in wave order
// (((w0 + w1) + w2) + w3, every lane adding its own registers to its own slots) and the workgroup writes ONE partial to the
// workspace: rows < aT of dak (times scale) and dav (times gate) as (32, D) float32 each, and sum_i D_i.
// The reduce kernel sums the partials of a KV head over (b, query head of the group, chunk) in ascending order, rounds dak and
// dav once and writes dgate[h] = sum_{b, chunk} as float32.  No atomics: two calls give the same bits.
//
// Chunk rule: BWD_CHUNK is 512 rows for every shape (never a function of the device).  A partial is at most 2 * 32 * D * 4 bytes
// against 512 * 3 * 2 D bytes of q, dO and dq: 1 / 12 of the row traffic at aT = 32, 1 / 38 at the reference's aT = 10.
//
// Instances: forward DP = 64, 128, 256; backward DP = 64, 128.  D any multiple of 8 up to DP; any N >= 1.
// LDS: forward 16,384 bytes; backward 67,072 (DP = 64) / 99,840 (DP = 128).  Register counts are in DESIGN.md 4.6c.
#include "../../include/fastmax_hip_prefix.h"
#include "fastmax_mfma32_common.h"

#include <cmath>

namespace fastmax {
namespace prefix {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

template <typename T> struct Op;
template <> struct Op<bf16_t> {
    typedef bf16x8 v8;
    typedef __bf16 elem;
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
    typedef _Float16 elem;
    static constexpr int DTYPE = FASTMAX_F16;
    static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v8 round8(const float* x) {
        v8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (_Float16)x[i];
        return r;
    }
};

constexpr int NW = 4, NT = 64 * NW, ROWS = 32 * NW;          // waves, threads, query rows per workgroup tile
constexpr int FWD_CHUNK = 2 * ROWS, BWD_CHUNK = FASTMAX_PREFIX_BWD_CHUNK, MAX_AT = FASTMAX_PREFIX_MAX_ROWS, BWD_MAX_D = 128;
constexpr float LOG2E = 1.4426950408889634f;
template <int DP> constexpr int img_row() { return 2 * DP + 64; }          // an image that is read transposed
template <int DP> constexpr int wave_lds() { return 2 * 32 * img_row<DP>() + 4096 + 3 * 32 * 4; }          // images, store area, m / 1/l / D

struct Args {
    const void *q, *y, *go, *ak, *av;
    Strides3 qs, ys, gos;
    const float* gate;
    void *out, *dq;
    float* ws;             // backward: partials, then their sums of D_i
    int B, H, Hkv, N, D, aT;
    float c, scale;        // scale * log2(e), scale
};

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

// the key (register i of an S^T tile, half hh of the wave) / the query row of an S tile
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// row fragments of a contiguous (aT, D) matrix; zeros past aT and D
template <typename V8, int KS> __device__ __forceinline__ void load_rows(V8 (&f)[KS], const uint16_t* m, int aT, int D, int l31, int hh) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * hh;
        f[s] = __builtin_bit_cast(V8, (l31 < aT && col < D) ? *reinterpret_cast<const uint4*>(m + l31 * D + col) : uint4{0, 0, 0, 0});
    }
}

// the same matrix transposed, as A operands over the keys (see the file comment)
template <typename V8, int DT> __device__ __forceinline__ void load_transposed(V8 (&f)[2][DT], const uint16_t* m, int aT, int D, int l31, int hh) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            union { V8 v; uint16_t e[8]; } u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = 16 * s + 4 * hh + (j & 3) + 8 * (j >> 2), col = 32 * dt + l31;
                u.e[j] = (key < aT && col < D) ? m[key * D + col] : (uint16_t)0;
            }
            f[s][dt] = u.v;
        }
}

// one tensor row's fragments through its own row pointer; zeros for a row >= N and columns >= D
template <typename V8, int KS> __device__ __forceinline__ void load_row_frags(V8 (&f)[KS], const uint16_t* rowp, bool row_live, int D, int hh) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int col = 16 * s + 8 * hh;
        f[s] = __builtin_bit_cast(V8, (row_live && col < D) ? *reinterpret_cast<const uint4*>(rowp + col) : uint4{0, 0, 0, 0});
    }
}

// grid: (ceil(N / FWD_CHUNK), B * H); block: NT
template <typename T, int DP>
__global__ __launch_bounds__(NT) void prefix_fwd_kernel(const Args a) {
    typedef typename Op<T>::v8 V8;
    typedef typename Op<T>::elem E;
    constexpr int KS = DP / 16, DT = DP / 32;
    __shared__ __attribute__((aligned(16))) char smem[NW * 4096];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H, g = h / (a.H / a.Hkv);
    const int N = a.N, D = a.D, aT = a.aT;
    const int chunk0 = (int)blockIdx.x * FWD_CHUNK;
    const float gate = a.gate[h];
    const int64_t slab = ((int64_t)b * a.H + h) * N;
    const uint16_t* qb = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.qs.sb + (int64_t)h * a.qs.sh;
    const uint16_t* yb = reinterpret_cast<const uint16_t*>(a.y) + (int64_t)b * a.ys.sb + (int64_t)h * a.ys.sh;
    uint16_t* ob = reinterpret_cast<uint16_t*>(a.out) + slab * D;

    if (gate == 0.f) {          // out = y, bit for bit
        const int pr = D / 8, rows = N - chunk0 < FWD_CHUNK ? N - chunk0 : FWD_CHUNK;
        if (ob == yb && a.ys.sn == D) return;
        for (int i = threadIdx.x; i < rows * pr; i += NT) {
            const int row = chunk0 + i / pr, col = 8 * (i % pr);
            *reinterpret_cast<uint4*>(ob + (int64_t)row * D + col) = *reinterpret_cast<const uint4*>(yb + (int64_t)row * a.ys.sn + col);
        }
        return;
    }

    V8 akf[KS], avt[2][DT];
    load_rows<V8, KS>(akf, reinterpret_cast<const uint16_t*>(a.ak) + (int64_t)g * aT * D, aT, D, l31, hh);
    load_transposed<V8, DT>(avt, reinterpret_cast<const uint16_t*>(a.av) + (int64_t)g * aT * D, aT, D, l31, hh);
    char* area = smem + 4096 * w;

    for (int t = 0; t < FWD_CHUNK / ROWS; ++t) {
        const int row_first = chunk0 + ROWS * t + 32 * w, row = row_first + l31;
        if (row_first >= N) break;          // wave-uniform
        V8 qf[KS];
        load_row_frags<V8, KS>(qf, qb + (int64_t)row * a.qs.sn, row < N, D, hh);
        f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) st = Op<T>::mma(akf[s], qf[s], st);
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float x = acc_row(i, hh) < aT ? st[i] * a.c : -INFINITY;
            st[i] = x;
            mx = fmaxf(mx, x);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          // finite: key 0 is live
        float p[16], l = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            p[i] = __builtin_amdgcn_exp2f(st[i] - mx);
            l += p[i];
        }
        l += __shfl_xor(l, 32, 64);
        f32x16 acc[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const V8 pf = Op<T>::round8(p + 8 * s);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc[dt] = Op<T>::mma(avt[s][dt], pf, acc[dt]);
        }
        const float gl = gate / l;
        // acc[dt][i]: column 32 dt + acc_row(i, hh) of row l31.  Through the wave's area as float32, back as 8-column pieces.
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int ig = 0; ig < 4; ++ig)
                *reinterpret_cast<f32x4*>(area + l31 * 128 + ((((2 * ig + hh) ^ l31) & 7) << 4)) =
                    f32x4{acc[dt][4 * ig], acc[dt][4 * ig + 1], acc[dt][4 * ig + 2], acc[dt][4 * ig + 3]} * gl;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = u * 64 + lane, rl = idx >> 2, pc = idx & 3;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(area + rl * 128 + ((((2 * pc) ^ rl) & 7) << 4));
                const f32x4 hi = *reinterpret_cast<const f32x4*>(area + rl * 128 + ((((2 * pc + 1) ^ rl) & 7) << 4));
                const int col = 32 * dt + 8 * pc, r = row_first + rl;
                if (r < N && col < D) {
                    union { uint4 u4; E e[8]; } yv, ov;
                    yv.u4 = *reinterpret_cast<const uint4*>(yb + (int64_t)r * a.ys.sn + col);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ov.e[j] = (E)((float)yv.e[j] + lo[j]);
                        ov.e[4 + j] = (E)((float)yv.e[4 + j] + hi[j]);
                    }
                    *reinterpret_cast<uint4*>(ob + (int64_t)r * D + col) = ov.u4;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// grid: (ceil(N / BWD_CHUNK), B * H); block: NT
template <typename T, int DP>
__global__ __launch_bounds__(NT) void prefix_bwd_kernel(const Args a) {
    typedef typename Op<T>::v8 V8;
    constexpr int KS = DP / 16, DT = DP / 32, IROW = img_row<DP>(), WLDS = wave_lds<DP>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H, g = h / (a.H / a.Hkv);
    const int N = a.N, D = a.D, aT = a.aT;
    const int chunk0 = (int)blockIdx.x * BWD_CHUNK;
    const float gate = a.gate[h];
    const int64_t slab = ((int64_t)b * a.H + h) * N;
    const uint16_t* qb = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.qs.sb + (int64_t)h * a.qs.sh;
    const uint16_t* gb = reinterpret_cast<const uint16_t*>(a.go) + (int64_t)b * a.gos.sb + (int64_t)h * a.gos.sh;
    const uint16_t* akb = reinterpret_cast<const uint16_t*>(a.ak) + (int64_t)g * aT * D;
    const uint16_t* avb = reinterpret_cast<const uint16_t*>(a.av) + (int64_t)g * aT * D;

    V8 akf[KS], avf[KS], akt[2][DT];
    load_rows<V8, KS>(akf, akb, aT, D, l31, hh);
    load_rows<V8, KS>(avf, avb, aT, D, l31, hh);
    load_transposed<V8, DT>(akt, akb, aT, D, l31, hh);

    char* qimg = smem + WLDS * w;
    char* gimg = qimg + 32 * IROW;
    char* area = gimg + 32 * IROW;
    float* stats = reinterpret_cast<float*>(area + 4096);          // m, 1 / l, D of the tile's 32 rows

    f32x16 dak[DT], dav[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dak[dt][i] = 0.f, dav[dt][i] = 0.f;
    float dsum = 0.f;

    for (int t = 0; t < BWD_CHUNK / ROWS; ++t) {
        const int row_first = chunk0 + ROWS * t + 32 * w, row = row_first + l31;
        if (row_first >= N) break;          // wave-uniform; the images are wave-private, so no barrier is skipped
        V8 qf[KS], gf[KS];
        load_row_frags<V8, KS>(qf, qb + (int64_t)row * a.qs.sn, row < N, D, hh);
        load_row_frags<V8, KS>(gf, gb + (int64_t)row * a.gos.sn, row < N, D, hh);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            *reinterpret_cast<V8*>(qimg + l31 * IROW + 32 * s + 16 * hh) = qf[s];
            *reinterpret_cast<V8*>(gimg + l31 * IROW + 32 * s + 16 * hh) = gf[s];
        }
        // rows as lanes
        {
            f32x16 st, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) st[i] = 0.f, dp[i] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                st = Op<T>::mma(akf[s], qf[s], st);
                dp = Op<T>::mma(avf[s], gf[s], dp);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float x = acc_row(i, hh) < aT ? st[i] * a.c : -INFINITY;
                st[i] = x;
                mx = fmaxf(mx, x);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float l = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                st[i] = __builtin_amdgcn_exp2f(st[i] - mx);
                l += st[i];
            }
            l += __shfl_xor(l, 32, 64);
            const float il = 1.0f / l;
            float dd = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                st[i] *= il;
                dd = fmaf(st[i], dp[i], dd);
            }
            dd += __shfl_xor(dd, 32, 64);
            if (hh == 0) {
                stats[l31] = row < N ? mx : INFINITY;
                stats[32 + l31] = il;
                stats[64 + l31] = dd;
                if (row < N) dsum += dd;
            }
            float ds[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) ds[i] = gate * (st[i] * (dp[i] - dd));
            f32x16 acc[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const V8 dsf = Op<T>::round8(ds + 8 * s);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) acc[dt] = Op<T>::mma(akt[s][dt], dsf, acc[dt]);
            }
            store_tile32_t<DT>(area, acc, a.scale, lane, a.dq, Op<T>::DTYPE, slab, row_first, N, D);
        }
        __builtin_amdgcn_wave_barrier();
        // keys as lanes
        {
            f32x16 st, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) st[i] = 0.f, dp[i] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                st = Op<T>::mma(qf[s], akf[s], st);
                dp = Op<T>::mma(gf[s], avf[s], dp);
            }
            float p[16], ds[16];
#pragma unroll
            for (int ig = 0; ig < 4; ++ig) {
                const f32x4 m4 = *reinterpret_cast<const f32x4*>(stats + 8 * ig + 4 * hh);
                const f32x4 il4 = *reinterpret_cast<const f32x4*>(stats + 32 + 8 * ig + 4 * hh);
                const f32x4 dd4 = *reinterpret_cast<const f32x4*>(stats + 64 + 8 * ig + 4 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * ig + e;
                    const float x = l31 < aT ? st[i] * a.c - m4[e] : -INFINITY;
                    p[i] = __builtin_amdgcn_exp2f(x) * il4[e];
                    ds[i] = gate * (p[i] * (dp[i] - dd4[e]));
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const V8 pf = Op<T>::round8(p + 8 * s), dsf = Op<T>::round8(ds + 8 * s);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dav[dt] = Op<T>::mma(ld_t<V8, IROW>(gimg, 16 * s, 32 * dt, lane), pf, dav[dt]);
                    dak[dt] = Op<T>::mma(ld_t<V8, IROW>(qimg, 16 * s, 32 * dt, lane), dsf, dak[dt]);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    // sum_i D_i of the wave: lanes >= 32 hold 0
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) dsum += __shfl_xor(dsum, off, 64);

    // merge the waves in wave order: a lane's register (which, dt, i) has slot ((which DT + dt) 16 + i) 64 + lane
    float* merge = reinterpret_cast<float*>(smem);
    float* msum = merge + 2 * DT * 16 * 64;
    __syncthreads();          // every wave is done with its images
    for (int ww = 0; ww < NW; ++ww) {
        if (w == ww) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float* sk = merge + (dt * 16 + i) * 64 + lane;
                    float* sv = merge + ((DT + dt) * 16 + i) * 64 + lane;
                    *sk = ww == 0 ? dak[dt][i] : *sk + dak[dt][i];
                    *sv = ww == 0 ? dav[dt][i] : *sv + dav[dt][i];
                }
            if (lane == 0) *msum = ww == 0 ? dsum : *msum + dsum;
        }
        __syncthreads();
    }
    // one partial: dak (32, D) times scale, dav (32, D) times gate, rows < aT; then sum_i D_i
    const int64_t pidx = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nparts = (int64_t)gridDim.x * gridDim.y;
    float* part = a.ws + pidx * (2 * 32 * D);
    const int pr = D / 4;
    for (int i = threadIdx.x; i < 2 * aT * pr; i += NT) {
        const int which = i / (aT * pr), rem = i % (aT * pr), key = rem / pr, d = 4 * (rem % pr);
        const int dt = d >> 5, r = d & 31, hq = (r >> 2) & 1, i0 = 4 * (r >> 3);
        const float* s = merge + ((which * DT + dt) * 16 + i0) * 64 + key + 32 * hq;
        const float f = which ? gate : a.scale;
        *reinterpret_cast<f32x4*>(part + (which * 32 + key) * D + d) = f32x4{s[0], s[64], s[128], s[192]} * f;
    }
    if (threadIdx.x == 0) a.ws[nparts * (2 * 32 * D) + pidx] = *msum;
}

struct ReduceArgs {
    const float* ws;
    void *dak, *dav;
    float* dgate;
    int B, H, Hkv, D, aT, nchunk, dtype;
};

// grid: (ceil(aT * D / NT), Hkv); block: NT.  Thread e < aT * D owns dak and dav element e of its KV head; in block x == 0 thread
// t < H / Hkv also owns dgate of the group's query head t.
__global__ __launch_bounds__(NT) void prefix_reduce_kernel(const ReduceArgs a) {
    const int g = blockIdx.y, r = a.H / a.Hkv, e = (int)blockIdx.x * NT + threadIdx.x;
    const int64_t stride = 2 * 32 * a.D, nparts = (int64_t)a.B * a.H * a.nchunk;
    if (e < a.aT * a.D) {
        float sk = 0.f, sv = 0.f;
        for (int b = 0; b < a.B; ++b)
            for (int hq = 0; hq < r; ++hq)
                for (int ck = 0; ck < a.nchunk; ++ck) {
                    const float* part = a.ws + (((int64_t)b * a.H + g * r + hq) * a.nchunk + ck) * stride;
                    sk += part[e];
                    sv += part[32 * a.D + e];
                }
        const int64_t o = (int64_t)g * a.aT * a.D + e;
        if (a.dtype == FASTMAX_BF16) {
            reinterpret_cast<__bf16*>(a.dak)[o] = (__bf16)sk;
            reinterpret_cast<__bf16*>(a.dav)[o] = (__bf16)sv;
        } else {
            reinterpret_cast<_Float16*>(a.dak)[o] = (_Float16)sk;
            reinterpret_cast<_Float16*>(a.dav)[o] = (_Float16)sv;
        }
    }
    if (blockIdx.x == 0)
        for (int hq = threadIdx.x; hq < r; hq += NT) {
            float s = 0.f;
            for (int b = 0; b < a.B; ++b)
                for (int ck = 0; ck < a.nchunk; ++ck) s += a.ws[nparts * stride + ((int64_t)b * a.H + g * r + hq) * a.nchunk + ck];
            a.dgate[g * r + hq] = s;
        }
}

template <typename T> static int launch_fwd(const Args& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.N + FWD_CHUNK - 1) / FWD_CHUNK), (unsigned)(a.B * a.H));
    if (a.D <= 64) hipLaunchKernelGGL((prefix_fwd_kernel<T, 64>), grid, dim3(NT), 0, stream, a);
    else if (a.D <= 128) hipLaunchKernelGGL((prefix_fwd_kernel<T, 128>), grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((prefix_fwd_kernel<T, 256>), grid, dim3(NT), 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T, int DP> static int launch_bwd(const Args& a, hipStream_t stream) {
    auto kern = prefix_bwd_kernel<T, DP>;
    constexpr int lds = NW * wave_lds<DP>();
    static_assert(lds >= (2 * (DP / 32) * 16 * 64 + 1) * 4, "the merge area lies over the waves' images");
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int nchunk = (a.N + BWD_CHUNK - 1) / BWD_CHUNK;
    hipLaunchKernelGGL(kern, dim3((unsigned)nchunk, (unsigned)(a.B * a.H)), dim3(NT), lds, stream, a);
    return (int)hipGetLastError();
}

static bool pieces(const void* p, const int64_t* s) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0;
}

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static bool shape_ok(int B, int H, int Hkv, int N, int D, int aT, int max_d, float scale) {
    return B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && N > 0 && D >= 8 && D <= max_d && D % 8 == 0 && (int64_t)B * H <= 65535 && aT >= 1 &&
           aT <= MAX_AT && std::isfinite(scale);
}

}  // namespace prefix
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::prefix;

extern "C" {

int fastmax_hip_prefix_forward(const void* q, const int64_t* q_strides, const void* y, const int64_t* y_strides, const void* ak,
                               const void* av, const float* gate, void* out, int B, int H, int Hkv, int N, int D, int aT, int dtype,
                               float scale, void* stream) {
    if (!q || !q_strides || !y || !y_strides || !ak || !av || !gate || !out) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!shape_ok(B, H, Hkv, N, D, aT, 256, scale)) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(y, y_strides) || !aligned16(ak) || !aligned16(av) || !aligned16(out) ||
        reinterpret_cast<uintptr_t>(gate) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    Args a{};
    a.q = q, a.y = y, a.ak = ak, a.av = av, a.gate = gate, a.out = out;
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ys = Strides3{y_strides[0], y_strides[1], y_strides[2]};
    a.B = B, a.H = H, a.Hkv = Hkv, a.N = N, a.D = D, a.aT = aT;
    a.c = scale * LOG2E, a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? launch_fwd<bf16_t>(a, st) : launch_fwd<f16_t>(a, st);
}

size_t fastmax_hip_prefix_backward_workspace(int B, int H, int N, int D) {
    if (B <= 0 || H <= 0 || N <= 0 || D < 8 || D > BWD_MAX_D || D % 8 != 0 || (int64_t)B * H > 65535) return 0;
    const size_t nparts = (size_t)B * H * (((size_t)N + BWD_CHUNK - 1) / BWD_CHUNK);
    return nparts * (2 * MAX_AT * (size_t)D + 1) * sizeof(float);
}

int fastmax_hip_prefix_backward(const void* q, const int64_t* q_strides, const void* grad_o, const int64_t* go_strides, const void* ak,
                                const void* av, const float* gate, void* dq, void* dak, void* dav, float* dgate, int B, int H, int Hkv,
                                int N, int D, int aT, int dtype, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !q_strides || !grad_o || !go_strides || !ak || !av || !gate || !dq || !dak || !dav || !dgate || !workspace)
        return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!shape_ok(B, H, Hkv, N, D, aT, BWD_MAX_D, scale)) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(grad_o, go_strides) || !aligned16(ak) || !aligned16(av) || !aligned16(dq) ||
        reinterpret_cast<uintptr_t>(dak) % 2 != 0 || reinterpret_cast<uintptr_t>(dav) % 2 != 0 ||
        reinterpret_cast<uintptr_t>(gate) % 4 != 0 || reinterpret_cast<uintptr_t>(dgate) % 4 != 0 || !aligned16(workspace))
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_prefix_backward_workspace(B, H, N, D)) return FASTMAX_E_WORKSPACE;
    Args a{};
    a.q = q, a.go = grad_o, a.ak = ak, a.av = av, a.gate = gate, a.dq = dq;
    a.ws = reinterpret_cast<float*>(workspace);
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.gos = Strides3{go_strides[0], go_strides[1], go_strides[2]};
    a.B = B, a.H = H, a.Hkv = Hkv, a.N = N, a.D = D, a.aT = aT;
    a.c = scale * LOG2E, a.scale = scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if (dtype == FASTMAX_BF16) rc = D <= 64 ? launch_bwd<bf16_t, 64>(a, st) : launch_bwd<bf16_t, 128>(a, st);
    else rc = D <= 64 ? launch_bwd<f16_t, 64>(a, st) : launch_bwd<f16_t, 128>(a, st);
    if (rc != 0) return rc;
    ReduceArgs r;
    r.ws = a.ws, r.dak = dak, r.dav = dav, r.dgate = dgate;
    r.B = B, r.H = H, r.Hkv = Hkv, r.D = D, r.aT = aT, r.nchunk = (N + BWD_CHUNK - 1) / BWD_CHUNK, r.dtype = dtype;
    hipLaunchKernelGGL(prefix_reduce_kernel, dim3((unsigned)((aT * D + NT - 1) / NT), (unsigned)Hkv), dim3(NT), 0, st, r);
    return (int)hipGetLastError();
}

}  // extern "C"
