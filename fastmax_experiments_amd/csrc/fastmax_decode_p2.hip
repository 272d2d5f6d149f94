// Decode-time state cache for SECOND-order fastmax (opt-in, the p = 2 partner of fastmax_decode.hip).
//
// With a = 1/nt and f(x) = 1 + x + x^2/2 = ((1 + x)^2 + 1) / 2, masked p = 2 fastmax at the last position of a sequence is
//     o = sum_n f(a q.k_n) v_n / sum_n f(a q.k_n).
// Write k~ = [1, k] (D+1 entries), v' = [v, 1] and q~ = [1, a q].  Then (1 + a q.k)^2 = sum_{m,l} q~_m q~_l k~_m k~_l, so the
// per-(b, kv-head) carried state is the symmetric third-order tensor
//     S~[(m,l)][j] = sum_n k~_m k~_l v'_j        (m <= l over the D+1 indices of k~; j over the D+1 of v')
// and a new token is read out as
//     F_j = sum_{m<=l} w q~_m q~_l S~[(m,l)][j] + S~[(0,0)][j]     (w = 2 off the diagonal, 1 on it)
//     o   = F_{:D} / F_D                                           (F is twice the numerator / denominator; the 2 cancels).
// S~ holds the count (S~[(0,0)][D]), S1 = sum v, ksum, S2 = sum k v^T, K2 = sum k k^T and the third-order sum: everything
// the p = 2 polynomial needs.  The count is an fp32 sum of ones: exact up to 2^24 tokens per sequence.
//
// State layout (float32), per (b, kv-head), P = (D+1)(D+2)/2 pair rows of DV = round_up(D+1, 4) floats (16-byte rows):
//     row(m,l) = m (D+1) - m (m-1) / 2 + (l - m),   row[j] = S~[(m,l)][j] for j <= D, 0 for D < j < DV.
// After the B*Hkv records sits the step's reduction scratch: STEP_SLOTS rows of DV floats per (b, kv-head).
// Sizes per kv head: D = 64 -> 2145 x 68 floats (0.58 MB), D = 128 -> 8385 x 132 (4.4 MB).
//
// The state depends on k and v only, so it is kept per KV head: grouped-query attention (H = q_per_kv * Hkv query heads,
// query head h reads kv head h / q_per_kv) reads each pair row once for all q_per_kv query heads of the group.
//
// Kernels
//   p2_prefill_state_kernel   S~ of a whole prompt as one GEMM per (b, kv-head): (pair rows x tokens) . (tokens x (D+1)),
//                             the pair products k~_m k~_l formed on the fly from an LDS image of k~, on the matrix cores
//                             (16x16x32 bf16, fp32 accumulation).  The pair product is split into bf16 hi + lo (exact for
//                             bf16 / f16 inputs), and so is v' for f32 / f16 inputs (bf16 v' is exact as it is).  Each
//                             workgroup owns 128 (D <= 64) or 256 pair rows over ALL tokens, so no cross-workgroup sum is
//                             needed: the pair dimension alone gives 17 (D = 64) to 33 (D = 128) workgroups per head.
//   p2_decode_step_kernel     one token: every pair row read once (16-byte loads), updated by k~_m k~_l v'_j, written back,
//                             and its contribution to F accumulated for the group's query heads; G workgroups per
//                             (b, kv-head) each write their partial F to the scratch slab.
//   p2_decode_finalize_kernel per (b, query head): S~[(0,0)] + the G partials in a fixed order, divide, store o in out_dtype.
//   p2_extend_readout_kernel  T new tokens at once: F of the cached tokens for all T queries of a group as one GEMM
//                             (query rows x pair rows) . (pair rows x (D+1)), the transpose of the prefill GEMM, with the
//                             products w q~_m q~_l formed on the fly; partials per split of the pair dimension.
//   p2_extend_combine_kernel  per new position: (S~[(0,0)] + partials in a fixed order) / 2 + the chunk's own masked sums
//                             (fp32, from the p = 2 tile kernels), divide, store o in out_dtype.
//                             The chunk then enters the state through p2_prefill_state_kernel in accumulate mode.
// No float atomics and no data handed between workgroups of one launch: bitwise reproducible run to run.
#include "fastmax_decode_p2_step.h"

namespace fastmax {
namespace p2dec {

constexpr int PF_KT = 32;         // tokens per MFMA k-step

template <typename T> __device__ __forceinline__ float ld(const void* base, int64_t idx) {
    return to_float(reinterpret_cast<const T*>(base)[idx]);
}

// ---- prefill: S~ over the whole prompt ------------------------------------------------------------------------------
// grid (ceil(P / (64 RT)), B * Hkv), 256 threads; each wave owns RT 16-row tiles of pair rows.  JT = MFMA column tiles
// (16 JT > D + 1, so column 16 JT - 1 is always 0).  With `vec` (rows of whole 16-byte pieces, 16-byte aligned) the next
// k-step's K and V pieces are loaded into registers while the matrix cores work on this one; otherwise element loads.
// ACC: S~ += (the tokens of a chunk that follows the cached ones) instead of S~ =; the old value of each element is read once
// in the epilogue and added last, so the order of the sum stays fixed.
template <typename T, int JT, int RT, bool ACC>
__global__ __launch_bounds__(256) void p2_prefill_state_kernel(const void* k, const void* v, Strides3 ks, Strides3 vs,
                                                               float* state, int Hkv, int N, int D, int vec) {
    constexpr int DVJ = 16 * JT;
    constexpr int KS = PF_KT + 4;                                 // fp32 row stride of the transposed k~ image
    constexpr int VS = PF_KT + 8;                                 // bf16 row stride of the transposed v' images (80 bytes)
    constexpr int NPV = std::is_same<T, bf16_t>::value ? 1 : 2;   // v' parts: bf16 is exact, f32 / f16 are split
    constexpr int EPC = InTraits<T>::EPL;                         // elements per 16-byte piece
    constexpr int NS = (PF_KT * ((DVJ - 16) / EPC) + 255) / 256;  // pieces per thread and tensor at the largest D
    __shared__ __attribute__((aligned(16))) float kt[DVJ][KS];    // kt[c][t] = k~_c of token t
    __shared__ __attribute__((aligned(16))) __bf16 vt[NPV][DVJ][VS];   // vt[p][j][t] = part p of v'_j of token t
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bkv = blockIdx.y, b = bkv / Hkv, h = bkv % Hkv;
    const int P = npairs(D), DV = ncols(D), CPR = D / EPC;
    const T* kb = row_ptr<T>(k, ks.sb, ks.sh, ks.sn, b, h, 0);
    const T* vb = row_ptr<T>(v, vs.sb, vs.sh, vs.sn, b, h, 0);

    // columns past D stay zero for the whole kernel
    for (int idx = tid; idx < (DVJ - D - 1) * PF_KT; idx += 256) {
        const int c = D + 1 + idx / PF_KT, t = idx % PF_KT;
        kt[c][t] = 0.f;
#pragma unroll
        for (int p = 0; p < NPV; ++p) vt[p][c][t] = (__bf16)0.f;
    }
    // this lane's A rows: pair (m, l) of row tile rt; rows past P read the all-zero column DVJ - 1
    int am[RT], al[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = blockIdx.x * (64 * RT) + wave * (16 * RT) + rt * 16 + (lane & 15);
        if (r < P) decode_row(r, D, am[rt], al[rt]);
        else am[rt] = al[rt] = DVJ - 1;
    }
    const int q8 = 8 * (lane >> 4);
    f32x4 acc[RT][JT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) acc[rt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 rk[NS], rv[NS];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int idx = tid + 256 * s, t = idx / CPR, c = idx - t * CPR;
            const bool ok = t < PF_KT && t0 + t < N;
            rk[s] = ok ? *reinterpret_cast<const u32x4*>(kb + (int64_t)(t0 + t) * ks.sn + c * EPC) : u32x4{0, 0, 0, 0};
            rv[s] = ok ? *reinterpret_cast<const u32x4*>(vb + (int64_t)(t0 + t) * vs.sn + c * EPC) : u32x4{0, 0, 0, 0};
        }
    };
    if (vec) fetch(0);
    for (int t0 = 0; t0 < N; t0 += PF_KT) {
        __syncthreads();                                          // the previous step's fragments are read
        if (vec) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int idx = tid + 256 * s, t = idx / CPR, c = idx - t * CPR;
                if (t < PF_KT) {
                    float xk[EPC], xv[EPC];
                    piece_to_float<T>(rk[s], xk);
                    piece_to_float<T>(rv[s], xv);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        kt[c * EPC + e + 1][t] = xk[e];
                        const __bf16 hi = (__bf16)xv[e];
                        vt[0][c * EPC + e][t] = hi;
                        if constexpr (NPV == 2) vt[1][c * EPC + e][t] = (__bf16)(xv[e] - (float)hi);
                    }
                }
            }
            if (t0 + PF_KT < N) fetch(t0 + PF_KT);                // in flight during this step's matrix work
        } else {
            for (int idx = tid; idx < PF_KT * D; idx += 256) {
                const int t = idx / D, d = idx - t * D;
                const bool ok = t0 + t < N;
                const float kx = ok ? ld<T>(kb, (int64_t)(t0 + t) * ks.sn + d) : 0.f;
                const float vx = ok ? ld<T>(vb, (int64_t)(t0 + t) * vs.sn + d) : 0.f;
                kt[d + 1][t] = kx;
                const __bf16 hi = (__bf16)vx;
                vt[0][d][t] = hi;
                if constexpr (NPV == 2) vt[1][d][t] = (__bf16)(vx - (float)hi);
            }
        }
        if (tid < PF_KT) {
            const float one = t0 + tid < N ? 1.f : 0.f;
            kt[0][tid] = one;
            vt[0][D][tid] = (__bf16)one;
            if constexpr (NPV == 2) vt[1][D][tid] = (__bf16)0.f;
        }
        __syncthreads();
        Frag<2> A[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const f32x4 m0 = *reinterpret_cast<const f32x4*>(&kt[am[rt]][q8]), m1 = *reinterpret_cast<const f32x4*>(&kt[am[rt]][q8 + 4]);
            const f32x4 l0 = *reinterpret_cast<const f32x4*>(&kt[al[rt]][q8]), l1 = *reinterpret_cast<const f32x4*>(&kt[al[rt]][q8 + 4]);
            bf16x4 h0, lo0, h1, lo1;
            split4(m0 * l0, h0, lo0);
            split4(m1 * l1, h1, lo1);
            A[rt].p[0] = cat4(h0, h1);
            A[rt].p[1] = cat4(lo0, lo1);
        }
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            Frag<NPV> Bf;
#pragma unroll
            for (int p = 0; p < NPV; ++p) Bf.p[p] = *reinterpret_cast<const bf16x8*>(&vt[p][jt * 16 + (lane & 15)][q8]);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][jt] = mfma_parts<2, NPV>(A[rt], Bf, acc[rt][jt]);
        }
    }
    // C[row 4 (lane >> 4) + e][column lane & 15] of each 16 x 16 tile
    float* rec = state + (int64_t)bkv * P * DV;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int rbase = blockIdx.x * (64 * RT) + wave * (16 * RT) + rt * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j = jt * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (rbase + e < P && j < DV) {
                    float* dst = rec + (int64_t)(rbase + e) * DV + j;
                    if constexpr (ACC) *dst = *dst + acc[rt][jt][e];
                    else *dst = acc[rt][jt][e];
                }
        }
    }
}

// ---- step (p2_decode_step_kernel: fastmax_decode_p2_step.h) from split q (B,H,1,D), k, v (B,Hkv,1,D) ------------------
template <typename T>
struct SplitSrc {
    const void *qp, *kp, *vp;
    Strides3 qs, ks, vs;
    __device__ __forceinline__ float k(int b, int hk, int d) const { return to_float(row_ptr<T>(kp, ks.sb, ks.sh, ks.sn, b, hk, 0)[d]); }
    __device__ __forceinline__ float v(int b, int hk, int d) const { return to_float(row_ptr<T>(vp, vs.sb, vs.sh, vs.sn, b, hk, 0)[d]); }
    __device__ __forceinline__ float q(int b, int hk, int qpk, int i, int d) const {
        return to_float(row_ptr<T>(qp, qs.sb, qs.sh, qs.sn, b, hk * qpk + i, 0)[d]);
    }
};

// grid (B * H), 256 threads
__global__ __launch_bounds__(256) void p2_decode_finalize_kernel(const float* state, const float* part, void* o, int out_dtype,
                                                                 int H, int Hkv, int qpk, int D, int G) {
    __shared__ float den;
    const int tid = threadIdx.x, bh = blockIdx.x, b = bh / H, h = bh % H, bkv = b * Hkv + h / qpk, i = h % qpk;
    const int P = npairs(D), DV = ncols(D);
    float f = 0.f;
    if (tid <= D) {
        f = state[(int64_t)bkv * P * DV + tid];                    // S~[(0,0)][j]
        const float* pp = part + ((int64_t)bkv * G * qpk + i) * DV + tid;
        const int64_t sg = (int64_t)qpk * DV;
        int gg = 0;
        for (; gg + 8 <= G; gg += 8) {                              // 8 loads in flight, then the adds in order
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = pp[(gg + u) * sg];
#pragma unroll
            for (int u = 0; u < 8; ++u) f += x[u];
        }
        for (; gg < G; ++gg) f += pp[gg * sg];
        if (tid == D) den = f;
    }
    __syncthreads();
    if (tid < D) {
        const float val = f / den;
        const int64_t idx = (int64_t)bh * D + tid;
        if (out_dtype == FASTMAX_F32) reinterpret_cast<float*>(o)[idx] = val;
        else if (out_dtype == FASTMAX_BF16) reinterpret_cast<uint16_t*>(o)[idx] = f32_to_bf16_bits(val);
        else reinterpret_cast<_Float16*>(o)[idx] = (_Float16)val;
    }
}

void launch_p2_finalize(const float* state, const float* part, void* o, int out_dtype, int B, int H, int Hkv, int qpk, int D,
                        int G, hipStream_t stream) {
    hipLaunchKernelGGL(p2_decode_finalize_kernel, dim3(B * H), dim3(256), 0, stream, state, part, o, out_dtype, H, Hkv, qpk, D, G);
}

template <typename T, bool ACC = false>
static int launch_prefill_t(const void* k, const void* v, Strides3 ks, Strides3 vs, float* state, int B, int Hkv, int N, int D,
                            hipStream_t stream) {
    const int es = (int)sizeof(T);
    const int vec = (D * es) % 16 == 0 && (reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) % 16 == 0 &&
                    (ks.sb * es | ks.sh * es | ks.sn * es | vs.sb * es | vs.sh * es | vs.sn * es) % 16 == 0;
    const int P = npairs(D);
    if (D <= 64)
        hipLaunchKernelGGL((p2_prefill_state_kernel<T, 5, 2, ACC>), dim3((P + 127) / 128, B * Hkv), dim3(256), 0, stream, k, v, ks, vs,
                           state, Hkv, N, D, vec);
    else
        hipLaunchKernelGGL((p2_prefill_state_kernel<T, 9, 4, ACC>), dim3((P + 255) / 256, B * Hkv), dim3(256), 0, stream, k, v, ks, vs,
                           state, Hkv, N, D, vec);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_step_t(const void* q, const void* k, const void* v, Strides3 qs, Strides3 ks, Strides3 vs, float* state,
                         void* o, int out_dtype, int B, int H, int Hkv, int D, float a, hipStream_t stream) {
    return launch_step_src<T>(SplitSrc<T>{q, k, v, qs, ks, vs}, state, o, out_dtype, B, H, Hkv, D, a, stream);
}


// ---- extend: T new tokens after the cached ones -----------------------------------------------------------------------
// Read-out of the carried state for a block of queries: per (b, kv-head) the GEMM (query rows x pair rows) . (pair rows x DV),
// the transpose of the prefill GEMM.  Query row rho = i T + t (query head i of the group, token t), so all H / Hkv query
// heads of a group are rows of one GEMM and a state row is fetched once per group.  The reduction runs over "chunks" of 8
// pair rows (m, 8 c .. 8 c + 7) with c >= m / 8: aligned in l, so a lane's 8 factors q~_l are two 16-byte LDS reads and the
// pair weight w = 2 (l > m), 1 (l = m), 0 (l < m, or l > D where q~ is zero) is applied while the product is formed.  One
// MFMA k-step takes 4 chunks (one per 8-wide k group of the 16x16x32 instruction).  The product and the fp32 state rows are
// both split into bf16 hi + lo (three matrix instructions per tile, the lo . lo term dropped: ~2^-16 relative).
// grid (KSP, ceil(R / ro_rows), B * Hkv), 256 threads: workgroup x of KSP takes a contiguous range of k-steps and writes its
// partial F for its 128 (D <= 64) or 64 query rows to part[bkv][x][rho][j]; p2_extend_combine_kernel sums them in the order of x.
// 16-row query tiles per wave: 2 at D <= 64 (JT = 5), 1 above (the fp32 q~ image of 128 rows would not fit static LDS)
__host__ __device__ constexpr int ro_mt(int JT) { return JT <= 5 ? 2 : 1; }
static int ro_rows(int D) { return D <= 64 ? 64 * ro_mt(5) : 64 * ro_mt(9); }           // query rows per workgroup
constexpr int RO_TARGET = 512;            // workgroups wanted before the reduction stops being split
constexpr int RO_KSP_MAX = 64;

__host__ __device__ __forceinline__ int ro_nc(int D) { return (D + 8) / 8; }                 // 8-wide l blocks covering D + 1
// chunks before the first one of m-group g (m = 8 g .. 8 g + 7): each m of group g' has nc - g' chunks
__host__ __device__ __forceinline__ int ro_group_start(int g, int nc) { return 8 * (g * nc - g * (g - 1) / 2); }
__host__ __device__ __forceinline__ int ro_nchunks(int D) {
    const int nc = ro_nc(D), gl = D / 8;                                                      // m = D sits in group gl
    return ro_group_start(gl, nc) + (D - 8 * gl + 1) * (nc - gl);
}

template <typename T, int JT>
__global__ __launch_bounds__(256) void p2_extend_readout_kernel(const void* q, Strides3 qs, const float* state, float* part,
                                                                int Hkv, int qpk, int Tn, int D, float a) {
    constexpr int DVJ = 16 * JT, RO_MT = ro_mt(JT), RO_ROWS = 64 * RO_MT;
    constexpr int DQ = DVJ - 8;                                   // 72 / 136: 8 ro_nc(D) <= DQ for D <= 64 / 128
    constexpr int QS = DQ + 4;                                    // fp32 row stride of the q~ image: an odd number of 16-byte pieces
    constexpr int SS = 32 + 8;                                    // bf16 row stride of the transposed state images (80 bytes)
    constexpr int NS = (32 * (DVJ / 4) + 255) / 256;              // 16-byte state pieces per thread and k-step
    __shared__ __attribute__((aligned(16))) float qt[RO_ROWS][QS];          // qt[rho][c] = q~_c of query row rho
    __shared__ __attribute__((aligned(16))) __bf16 sh[2][DVJ][SS];          // sh[p][j][kk] = part p of S~[row kk of the step][j]
    __shared__ unsigned short tab[2][4];                                    // (m << 5 | c) of the 4 chunks of k-step s at tab[s & 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bkv = blockIdx.z, b = bkv / Hkv, hk = bkv % Hkv;
    const int P = npairs(D), DV = ncols(D), J4 = DV / 4, D1 = D + 1, R = qpk * Tn;
    const int nc = ro_nc(D), nch = ro_nchunks(D), nsteps = (nch + 3) / 4;
    const int s0 = (int)((int64_t)nsteps * blockIdx.x / gridDim.x), s1 = (int)((int64_t)nsteps * (blockIdx.x + 1) / gridDim.x);
    const int row0 = blockIdx.y * RO_ROWS;
    const float* rec = state + (int64_t)bkv * P * DV;

    // q~ image of this workgroup's query rows; rows past R and columns past D are zero
    for (int idx = tid; idx < RO_ROWS * QS; idx += 256) {
        const int rl = idx / QS, c = idx - rl * QS, rho = row0 + rl;
        float x = 0.f;
        if (rho < R && c <= D) {
            const int i = rho / Tn, t = rho - i * Tn;
            x = c == 0 ? 1.f : a * to_float(row_ptr<T>(q, qs.sb, qs.sh, qs.sn, b, hk * qpk + i, t)[c - 1]);
        }
        qt[rl][c] = x;
    }
    // state columns past DV stay zero for the whole kernel
    for (int idx = tid; idx < (DVJ - DV) * 32; idx += 256) {
        const int j = DV + idx / 32, kk = idx % 32;
        sh[0][j][kk] = (__bf16)0.f;
        sh[1][j][kk] = (__bf16)0.f;
    }
    // chunk id -> (m, c); ids past the last chunk give m = D + 1, whose q~ column is zero and whose rows are not loaded
    auto chunk_mc = [&](int id, int& m, int& c) {
        if (id >= nch) { m = D1; c = nc - 1; return; }
        int g = 0;
        while (ro_group_start(g + 1, nc) <= id) ++g;
        const int rem = id - ro_group_start(g, nc), w = nc - g;
        m = 8 * g + rem / w;
        c = g + rem % w;
    };
    f32x4 rs[NS];
    auto fetch = [&](int step) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int idx = tid + 256 * s, kk = idx / J4, j4 = idx - kk * J4;
            rs[s] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kk < 32) {
                const int ent = tab[step & 1][kk >> 3], m = ent >> 5, l = 8 * (ent & 31) + (kk & 7);
                if (l >= m && l <= D && m <= D)
                    rs[s] = *reinterpret_cast<const f32x4*>(rec + (int64_t)(row_start(m, D1) + l - m) * DV + 4 * j4);
            }
        }
    };
    f32x4 acc[RO_MT][JT];
#pragma unroll
    for (int mt = 0; mt < RO_MT; ++mt)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) acc[mt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int q8 = 8 * (lane >> 4);
    // a wave's tiles that lie wholly past R do no matrix work (the wave still stages state rows)
    bool live[RO_MT];
#pragma unroll
    for (int mt = 0; mt < RO_MT; ++mt) live[mt] = row0 + wave * (16 * RO_MT) + mt * 16 < R;

    auto put_tab = [&](int step) {
        int m, c;
        chunk_mc(4 * step + tid, m, c);
        tab[step & 1][tid] = (unsigned short)(m << 5 | c);
    };
    if (tid < 4) put_tab(s0);
    __syncthreads();
    fetch(s0);
    for (int step = s0; step < s1; ++step) {
        __syncthreads();                                          // the previous step's fragments are read (and qt is written)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int idx = tid + 256 * s, kk = idx / J4, j4 = idx - kk * J4;
            if (kk < 32) {
                bf16x4 hi, lo;
                split4(rs[s], hi, lo);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sh[0][4 * j4 + e][kk] = hi[e];
                    sh[1][4 * j4 + e][kk] = lo[e];
                }
            }
        }
        if (tid < 4) put_tab(step + 1);
        __syncthreads();
        if (step + 1 < s1) fetch(step + 1);                       // in flight during this step's matrix work
        const int ent = tab[step & 1][lane >> 4], m = ent >> 5, l0 = 8 * (ent & 31);
        Frag<2> A[RO_MT];
#pragma unroll
        for (int mt = 0; mt < RO_MT; ++mt) {
            if (!live[mt]) continue;
            const float* qr = qt[wave * (16 * RO_MT) + mt * 16 + (lane & 15)];
            const float qm = m <= D ? qr[m] : 0.f;
            f32x4 x0 = *reinterpret_cast<const f32x4*>(qr + l0), x1 = *reinterpret_cast<const f32x4*>(qr + l0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int la = l0 + e, lb = l0 + 4 + e;
                x0[e] *= la > m ? 2.f * qm : (la == m ? qm : 0.f);
                x1[e] *= lb > m ? 2.f * qm : (lb == m ? qm : 0.f);
            }
            bf16x4 h0, lo0, h1, lo1;
            split4(x0, h0, lo0);
            split4(x1, h1, lo1);
            A[mt].p[0] = cat4(h0, h1);
            A[mt].p[1] = cat4(lo0, lo1);
        }
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            Frag<2> Bf;
#pragma unroll
            for (int p = 0; p < 2; ++p) Bf.p[p] = *reinterpret_cast<const bf16x8*>(&sh[p][jt * 16 + (lane & 15)][q8]);
#pragma unroll
            for (int mt = 0; mt < RO_MT; ++mt)
                if (live[mt]) acc[mt][jt] = mfma_parts<2, 2>(A[mt], Bf, acc[mt][jt]);
        }
    }
    // C[row 4 (lane >> 4) + e][column lane & 15] of each 16 x 16 tile
    float* out = part + ((int64_t)bkv * gridDim.x + blockIdx.x) * R * DV;
#pragma unroll
    for (int mt = 0; mt < RO_MT; ++mt) {
        const int rbase = row0 + wave * (16 * RO_MT) + mt * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j = jt * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (rbase + e < R && j < DV) out[(int64_t)(rbase + e) * DV + j] = acc[mt][jt][e];
        }
    }
}

// One wave per new position (b, h, t): F = (S~[(0,0)] + the KSP read-out partials, in order) / 2 + the chunk's own masked sum
// [oi g, g] (oi and g in fp32 from the tile kernels), o = F_{:D} / F_D rounded once to out_dtype.  grid ceil(B H T / 4), 256.
__global__ __launch_bounds__(256) void p2_extend_combine_kernel(const float* state, const float* part, const float* oi,
                                                                const float* gi, void* o, int out_dtype, int64_t rows, int H,
                                                                int Hkv, int qpk, int T, int D, int KSP) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = (int)(row % T), bh = (int)(row / T), b = bh / H, h = bh % H, bkv = b * Hkv + h / qpk, i = h % qpk;
    const int P = npairs(D), DV = ncols(D), R = qpk * T;
    const float* s00 = state + (int64_t)bkv * P * DV;
    const float* pp = part + ((int64_t)bkv * KSP * R + (int64_t)i * T + t) * DV;
    const float g = gi[row];
    float f[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int j = lane + 64 * u;
        if (j <= D) {
            float x = s00[j];
            for (int x_ = 0; x_ < KSP; ++x_) x += pp[(int64_t)x_ * R * DV + j];
            f[u] = 0.5f * x + (j < D ? oi[row * D + j] * g : g);
        }
    }
    const int ud = D >> 6, ld_ = D & 63;
    const float den = __shfl(ud == 0 ? f[0] : (ud == 1 ? f[1] : f[2]), ld_, 64);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int j = lane + 64 * u;
        if (j < D) {
            const float val = f[u] / den;
            const int64_t idx = row * D + j;
            if (out_dtype == FASTMAX_F32) reinterpret_cast<float*>(o)[idx] = val;
            else if (out_dtype == FASTMAX_BF16) reinterpret_cast<uint16_t*>(o)[idx] = f32_to_bf16_bits(val);
            else reinterpret_cast<_Float16*>(o)[idx] = (_Float16)val;
        }
    }
}

// how the read-out's reduction is split: KSP workgroups per (b, kv-head, block of ro_rows query rows)
static int extend_ksplit(int B, int Hkv, int64_t mblocks, int D) {
    const int nsteps = (ro_nchunks(D) + 3) / 4;
    const int64_t wg = (int64_t)B * Hkv * mblocks;
    const int64_t want = (RO_TARGET + wg - 1) / wg;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, std::min(nsteps, RO_KSP_MAX)));
}

struct ExtendLayout { size_t oi, g, part, total; int ksp; };
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// workspace: [oi fp32 (B,H,T,D)] [g fp32 (B,H,T)] [partials (B Hkv, KSP, R, DV)] [workspace of the tile forward].
// The partials are sized for the largest KSP * rows of any T' <= T, so the size never shrinks as T grows.
static ExtendLayout extend_layout(int B, int H, int Hkv, int T, int D, size_t fwd_ws) {
    const int qpk = H / Hkv;
    const int64_t R = (int64_t)qpk * T, rows = ro_rows(D), mb = (R + rows - 1) / rows;
    int64_t prow = 0;
    for (int64_t m = 1; m <= mb; ++m) {
        const int ksp = extend_ksplit(B, Hkv, m, D);
        prow = std::max(prow, ksp * std::min<int64_t>(R, m * rows));
        if (ksp == 1) { prow = std::max(prow, R); break; }
    }
    ExtendLayout L;
    L.ksp = extend_ksplit(B, Hkv, mb, D);
    L.oi = 0;
    L.g = up256(sizeof(float) * (size_t)B * H * T * D);
    L.part = L.g + up256(sizeof(float) * (size_t)B * H * T);
    L.total = L.part + up256(sizeof(float) * (size_t)B * Hkv * prow * ncols(D)) + up256(fwd_ws);
    return L;
}

template <typename T>
static int launch_readout_t(const void* q, Strides3 qs, const float* state, float* part, int B, int Hkv, int qpk, int Tn, int D,
                            int ksp, float a, hipStream_t stream) {
    const int64_t R = (int64_t)qpk * Tn;
    const dim3 grid(ksp, (unsigned)((R + ro_rows(D) - 1) / ro_rows(D)), B * Hkv);
    if (D <= 64)
        hipLaunchKernelGGL((p2_extend_readout_kernel<T, 5>), grid, dim3(256), 0, stream, q, qs, state, part, Hkv, qpk, Tn, D, a);
    else
        hipLaunchKernelGGL((p2_extend_readout_kernel<T, 9>), grid, dim3(256), 0, stream, q, qs, state, part, Hkv, qpk, Tn, D, a);
    return (int)hipGetLastError();
}

}  // namespace p2dec
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::p2dec;

extern "C" {

size_t fastmax_hip_p2_decode_state_bytes(int B, int Hkv, int D) {
    if (B <= 0 || Hkv <= 0 || D <= 0 || D > 128) return 0;
    return sizeof(float) * (size_t)B * Hkv * ((size_t)npairs(D) + STEP_SLOTS) * ncols(D);
}

int fastmax_hip_p2_prefill_state(const fastmax_problem* prob, const void* k, const int64_t* k_strides, const void* v,
                                 const int64_t* v_strides, float* state, void* stream) {
    if (!prob || !k || !v || !state || !k_strides || !v_strides) return FASTMAX_E_NULL;
    if (prob->p != 2 || !prob->causal) return FASTMAX_E_BAD_P;
    if (prob->B <= 0 || prob->H <= 0 || prob->Nk <= 0 || prob->Nq != prob->Nk || prob->D <= 0 || prob->D > 128 ||
        (int64_t)prob->B * prob->H > 65535)
        return FASTMAX_E_BAD_SHAPE;
    const Strides3 ks{k_strides[0], k_strides[1], k_strides[2]}, vs{v_strides[0], v_strides[1], v_strides[2]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (prob->in_dtype) {
        case FASTMAX_F32: return launch_prefill_t<float>(k, v, ks, vs, state, prob->B, prob->H, prob->Nk, prob->D, st);
        case FASTMAX_BF16: return launch_prefill_t<bf16_t>(k, v, ks, vs, state, prob->B, prob->H, prob->Nk, prob->D, st);
        case FASTMAX_F16: return launch_prefill_t<f16_t>(k, v, ks, vs, state, prob->B, prob->H, prob->Nk, prob->D, st);
    }
    return FASTMAX_E_BAD_DTYPE;
}

int fastmax_hip_p2_decode_step(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                               const int64_t* v_strides, float* state, void* o, int B, int H, int Hkv, int D, int in_dtype,
                               int out_dtype, float a, void* stream) {
    if (!q || !k || !v || !state || !o || !q_strides || !k_strides || !v_strides) return FASTMAX_E_NULL;
    if (B <= 0 || H <= 0 || Hkv <= 0 || D <= 0 || D > 128 || H % Hkv != 0 || H / Hkv > STEP_SLOTS ||
        (int64_t)B * Hkv > 65535 || (int64_t)B * H > (int64_t)0x7fffffff)
        return FASTMAX_E_BAD_SHAPE;
    if (out_dtype < FASTMAX_F32 || out_dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    const Strides3 qs{q_strides[0], q_strides[1], q_strides[2]}, ks{k_strides[0], k_strides[1], k_strides[2]},
        vs{v_strides[0], v_strides[1], v_strides[2]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (in_dtype) {
        case FASTMAX_F32: return launch_step_t<float>(q, k, v, qs, ks, vs, state, o, out_dtype, B, H, Hkv, D, a, st);
        case FASTMAX_BF16: return launch_step_t<bf16_t>(q, k, v, qs, ks, vs, state, o, out_dtype, B, H, Hkv, D, a, st);
        case FASTMAX_F16: return launch_step_t<f16_t>(q, k, v, qs, ks, vs, state, o, out_dtype, B, H, Hkv, D, a, st);
    }
    return FASTMAX_E_BAD_DTYPE;
}

// the tile forward's workspace for the chunk's own masked p = 2 pass, in either batch decomposition (see p2_extend)
static size_t extend_fwd_workspace(int B, int H, int Hkv, int T, int D) {
    size_t w = 0;
    for (int dt = FASTMAX_F32; dt <= FASTMAX_F16; ++dt) {
        fastmax_problem fp{B, H, T, T, D, dt, FASTMAX_F32, 2, 1, 1.f, 0.5f, 0.f, FASTMAX_PATH_AUTO};
        w = std::max(w, fastmax_hip_forward_workspace(&fp));
        fp.B = B * Hkv, fp.H = H / Hkv;
        w = std::max(w, fastmax_hip_forward_workspace(&fp));
        fp.B = Hkv;
        w = std::max(w, fastmax_hip_forward_workspace(&fp));
    }
    return w;
}

size_t fastmax_hip_p2_extend_workspace(int B, int H, int Hkv, int T, int D) {
    if (B <= 0 || H <= 0 || Hkv <= 0 || T <= 0 || D <= 0 || D > 128 || H % Hkv != 0) return 0;
    return extend_layout(B, H, Hkv, T, D, extend_fwd_workspace(B, H, Hkv, T, D)).total;
}

int fastmax_hip_p2_extend(const fastmax_problem* prob, int Hkv, const void* q, const int64_t* q_strides, const void* k,
                          const int64_t* k_strides, const void* v, const int64_t* v_strides, float* state, void* o,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!prob || !q || !k || !v || !state || !o || !q_strides || !k_strides || !v_strides) return FASTMAX_E_NULL;
    if (prob->p != 2 || !prob->causal) return FASTMAX_E_BAD_P;
    const int B = prob->B, H = prob->H, T = prob->Nk, D = prob->D;
    if (B <= 0 || H <= 0 || Hkv <= 0 || T <= 0 || prob->Nq != T || D <= 0 || D > 128 || H % Hkv != 0 ||
        (int64_t)B * H > 65535 || ((int64_t)(H / Hkv) * T + ro_rows(D) - 1) / ro_rows(D) > 65535 ||
        (int64_t)B * H * T > (int64_t)0x7fffffff)
        return FASTMAX_E_BAD_SHAPE;
    if (prob->in_dtype < FASTMAX_F32 || prob->in_dtype > FASTMAX_F16 || prob->out_dtype < FASTMAX_F32 || prob->out_dtype > FASTMAX_F16)
        return FASTMAX_E_BAD_DTYPE;
    const size_t fwd_ws = extend_fwd_workspace(B, H, Hkv, T, D);
    const ExtendLayout L = extend_layout(B, H, Hkv, T, D, fwd_ws);
    if (!workspace || workspace_bytes < L.total) return FASTMAX_E_WORKSPACE;

    const int qpk = H / Hkv, es = prob->in_dtype == FASTMAX_F32 ? 4 : 2;
    const Strides3 qs{q_strides[0], q_strides[1], q_strides[2]}, ks{k_strides[0], k_strides[1], k_strides[2]},
        vs{v_strides[0], v_strides[1], v_strides[2]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    float *oi = reinterpret_cast<float*>(ws + L.oi), *gi = reinterpret_cast<float*>(ws + L.g), *part = reinterpret_cast<float*>(ws + L.part);
    void* fws = fwd_ws ? ws + (L.total - up256(fwd_ws)) : nullptr;

    // 1. the chunk's own masked p = 2 sums from the tile kernels, numerator kept in fp32: oi = Fi_{:D} / g, g = Fi_D.
    //    Grouped heads: (batch, group) as the batch axis, the group's K and V with head stride 0; when q's batch stride is
    //    not H head strides that view does not exist and the batch entries go one call at a time.
    fastmax_problem fp = *prob;
    fp.out_dtype = FASTMAX_F32;
    fp.path = FASTMAX_PATH_AUTO;
    int rc;
    if (qpk == 1) {
        rc = fastmax_hip_forward(&fp, q, q_strides, k, k_strides, v, v_strides, oi, gi, fws, fwd_ws, stream);
    } else {
        const int64_t gq[3] = {qpk * qs.sh, qs.sh, qs.sn}, gk[3] = {ks.sh, 0, ks.sn}, gv[3] = {vs.sh, 0, vs.sn};
        fp.H = qpk;
        if (qs.sb == H * qs.sh && ks.sb == Hkv * ks.sh && vs.sb == Hkv * vs.sh) {
            fp.B = B * Hkv;
            rc = fastmax_hip_forward(&fp, q, gq, k, gk, v, gv, oi, gi, fws, fwd_ws, stream);
        } else {
            fp.B = Hkv;
            rc = FASTMAX_OK;
            for (int b = 0; b < B && rc == FASTMAX_OK; ++b)
                rc = fastmax_hip_forward(&fp, reinterpret_cast<const char*>(q) + b * qs.sb * es, gq,
                                         reinterpret_cast<const char*>(k) + b * ks.sb * es, gk,
                                         reinterpret_cast<const char*>(v) + b * vs.sb * es, gv, oi + (int64_t)b * H * T * D,
                                         gi + (int64_t)b * H * T, fws, fwd_ws, stream);
        }
    }
    if (rc) return rc;
    // 2. read-out of the cached tokens' state for the T queries, 3. combine, 4. only then S~ += the chunk
    switch (prob->in_dtype) {
        case FASTMAX_F32: rc = launch_readout_t<float>(q, qs, state, part, B, Hkv, qpk, T, D, L.ksp, prob->a, st); break;
        case FASTMAX_BF16: rc = launch_readout_t<bf16_t>(q, qs, state, part, B, Hkv, qpk, T, D, L.ksp, prob->a, st); break;
        default: rc = launch_readout_t<f16_t>(q, qs, state, part, B, Hkv, qpk, T, D, L.ksp, prob->a, st); break;
    }
    if (rc) return rc;
    const int64_t rows = (int64_t)B * H * T;
    hipLaunchKernelGGL(p2_extend_combine_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, state, part, oi, gi, o,
                       prob->out_dtype, rows, H, Hkv, qpk, T, D, L.ksp);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    switch (prob->in_dtype) {
        case FASTMAX_F32: return launch_prefill_t<float, true>(k, v, ks, vs, state, B, Hkv, T, D, st);
        case FASTMAX_BF16: return launch_prefill_t<bf16_t, true>(k, v, ks, vs, state, B, Hkv, T, D, st);
        default: return launch_prefill_t<f16_t, true>(k, v, ks, vs, state, B, Hkv, T, D, st);
    }
}

}  // extern "C"
