// Decode-time state cache for masked first-order linearmax (include/fastmax_hip_linearmax_decode.h).
//
// fastmax_hack(mask=True, p=1) centres every q and k row over D and divides ALL of q by one scalar per (b, h), Mq = the
// largest centred-row norm of q over the sequence, and all of k by Mk in the same way.  With qc, kc the centred, unscaled rows
//     f(q^_i . k^_j) = 1 + (qc_i . kc_j) / (Mq Mk)
//     o_i = (S1 + a qc_i^T S2) / (count + a qc_i . ksum),   a = 1 / (Mq Mk)
//     S2 = sum_j kc_j v_j^T,  S1 = sum_j v_j,  ksum = sum_j kc_j      (j <= i)
// so the two statistics leave the bilinear sums as one scalar: a state of UNSCALED centred sums never needs rescaling, only a
// moves while the two running maxima grow.  One kernel advances the state by T tokens and reads them out.
//
// Parallelism: column d of o needs column d of S2 (plus ksum), so a (b, kv head) record is cut into NS column slabs, one
// workgroup each.  A slab block of the record is self-contained: its columns of S2 and S1, and its OWN copy of ksum, of the
// count and of the maxima, which every slab recomputes from the same rows in the same order (identical bits in every copy).
// Nothing is summed across workgroups, no workgroup reads what another one of the launch writes, there are no atomics, and
// every in-workgroup sum has a fixed order: results are bitwise reproducible.
//
// A workgroup is 16 row groups x W columns: thread (mg, d) owns rows mg R .. mg R + R - 1 of column d0 + d, kept in registers
// for all T tokens and stored in the record in exactly that order (R contiguous floats per thread: read once, written once,
// 16 bytes at a time).  Per token it adds kc_m v_d to its R elements; per query head it dots them with the head's qc rows
// (LDS), and the 16 row groups are summed by wave shuffles and one LDS round per batch of HB heads.
#include "../../include/fastmax_hip_linearmax_decode.h"
#include "fastmax_common.h"

namespace fastmax {
namespace lmdec {

constexpr int NS = 8;                   // column slabs (workgroups) per (b, kv head) record
constexpr int MAX_QPK = 64;             // query heads per kv head
constexpr int HB = 8;                   // query heads per read-out round
constexpr int STAGE_FLOATS = 10240;     // LDS budget of the staged token chunk (floats)
constexpr int MAX_CHUNK = 64;

__host__ __device__ constexpr int round4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr int stat_floats(int qpk) { return round4(2 + qpk); }        // count, Mk, Mq[qpk]
__host__ __device__ constexpr int slab_floats(int dp, int qpk) { return dp * (dp / NS) + dp / NS + dp + stat_floats(qpk); }

__device__ __forceinline__ float group16_sum(float x) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// Centre rows over their D real elements, 16 lanes per row.  Row `row` of the pass is token t_begin + row / nk, kind
// kind0 + row % nk; kind < qpk: query head g qpk + kind, kind == qpk: the key head.  STATS: fold each row's squared norm into
// gm[row group][kind] (every slot has one writer).  WRITE: store the centred row, zero-padded to DP, into kc / qc.
template <typename T, int DP, bool STATS, bool WRITE>
__device__ __forceinline__ void centre_rows(const void* q, const void* k, Strides3 qs, Strides3 ks, int b, int g, int qpk, int D,
                                            int64_t t_begin, int tc, int kind0, int nk, bool write_q, float* kc, float* qc,
                                            float* gm) {
    constexpr int NG = DP * 2 / 16, EPL = DP / 16;
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int nrows = tc * nk;
    const float inv_d = 1.0f / (float)D;
    for (int base = 0; base < nrows; base += NG) {
        const int row = base + grp;
        const bool valid = row < nrows;
        const int t = valid ? row / nk : 0, kind = kind0 + (valid ? row % nk : 0);
        const T* src = kind < qpk ? row_ptr<T>(q, qs.sb, qs.sh, qs.sn, b, g * qpk + kind, 0) + (t_begin + t) * qs.sn
                                  : row_ptr<T>(k, ks.sb, ks.sh, ks.sn, b, g, 0) + (t_begin + t) * ks.sn;
        float x[EPL];
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int idx = l + 16 * e;
            x[e] = (valid && idx < D) ? to_float(src[idx]) : 0.f;
            sum += x[e];
        }
        const float mean = group16_sum(sum) * inv_d;
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            x[e] = (l + 16 * e < D) ? x[e] - mean : 0.f;
            ss = fmaf(x[e], x[e], ss);
        }
        if (STATS) {
            ss = group16_sum(ss);
            if (valid && l == 0) gm[grp * (qpk + 1) + kind] = fmaxf(gm[grp * (qpk + 1) + kind], ss);
        }
        if (WRITE && valid && (kind == qpk || write_q)) {
            float* dst = kind < qpk ? qc + ((int64_t)t * qpk + kind) * DP : kc + t * DP;
#pragma unroll
            for (int e = 0; e < EPL; ++e) dst[l + 16 * e] = x[e];
        }
    }
}

template <typename T>
__device__ __forceinline__ void store_out(void* o, int64_t idx, float val) {
    reinterpret_cast<T*>(o)[idx] = from_float<T>(val);
}

// grid: NS workgroups per (b, kv head); block: 2 DP threads; dynamic LDS: see lds_floats()
template <typename T, int DP>
__global__ __launch_bounds__(DP * 2) void linearmax_advance_kernel(const void* q, const void* k, const void* v, Strides3 qs,
                                                                   Strides3 ks, Strides3 vs, float* state, void* o, int G,
                                                                   int qpk, int D, int Tn, int TC) {
    constexpr int W = DP / NS, NT = DP * 2, R = DP / 16, NW = NT / 64, NG = NT / 16;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.x % NS, bg = blockIdx.x / NS, b = bg / G, g = bg % G;
    const int d = tid % W, mg = tid / W, d0 = slab * W;
    const bool readout = o != nullptr;

    float* rec = state + ((int64_t)bg * NS + slab) * slab_floats(DP, qpk);
    float* rS1 = rec + DP * W;
    float* rK = rS1 + W;
    float* rStat = rK + DP;

    float* kc = lds;                                         // [TC][DP]   centred k rows
    float* vv = kc + TC * DP;                                // [TC][W]    this slab's columns of v
    float* qc = vv + TC * W;                                 // [TC][qpk][DP] centred q rows (read-out only)
    float* gm = qc + (readout ? TC * qpk * DP : 0);          // [NG][qpk + 1] squared-norm maxima per row group
    float* Mx = gm + round4(NG * (qpk + 1));                 // [qpk + 1]  Mq of every head, then Mk
    float* red = Mx + round4(qpk + 1);                       // [2][NW][HB][W][2]

    // the slab's part of the state: on chip until the last token
    float s[R], ksr[R];
#pragma unroll
    for (int j = 0; j < R / 4; ++j) {
        const float4 a = reinterpret_cast<const float4*>(rec + tid * R)[j];
        const float4 c = reinterpret_cast<const float4*>(rK + mg * R)[j];
        s[4 * j] = a.x, s[4 * j + 1] = a.y, s[4 * j + 2] = a.z, s[4 * j + 3] = a.w;
        ksr[4 * j] = c.x, ksr[4 * j + 1] = c.y, ksr[4 * j + 2] = c.z, ksr[4 * j + 3] = c.w;
    }
    float s1 = rS1[d];
    float cnt = rStat[0];

    // both maxima over the WHOLE chunk before any of its rows is read out
    for (int i = tid; i < NG * (qpk + 1); i += NT) gm[i] = 0.f;
    __syncthreads();
    const bool one = Tn <= TC;          // a single staged chunk: statistics and staging in one pass over the rows
    if (one) centre_rows<T, DP, true, true>(q, k, qs, ks, b, g, qpk, D, 0, Tn, 0, qpk + 1, readout, kc, qc, gm);
    else centre_rows<T, DP, true, false>(q, k, qs, ks, b, g, qpk, D, 0, Tn, 0, qpk + 1, false, kc, qc, gm);
    __syncthreads();
    if (tid <= qpk) {
        float m = 0.f;
        for (int i = 0; i < NG; ++i) m = fmaxf(m, gm[i * (qpk + 1) + tid]);
        float* slot = rStat + (tid < qpk ? 2 + tid : 1);
        const float nm = fmaxf(*slot, sqrtf(m));
        Mx[tid] = nm;
        *slot = nm;
    }
    // (Mx is read after the next barrier: every chunk has one before its token loop)

    int buf = 0;
    for (int t0 = 0; t0 < Tn; t0 += TC) {
        const int tc = min(TC, Tn - t0);
        if (!one) {
            __syncthreads();            // the previous chunk's rows are no longer read
            if (readout) centre_rows<T, DP, false, true>(q, k, qs, ks, b, g, qpk, D, t0, tc, 0, qpk + 1, true, kc, qc, gm);
            else centre_rows<T, DP, false, true>(q, k, qs, ks, b, g, qpk, D, t0, tc, qpk, 1, false, kc, qc, gm);
        }
        for (int i = tid; i < tc * W; i += NT) {
            const int t = i / W, c = d0 + i % W;
            vv[i] = c < D ? to_float(row_ptr<T>(v, vs.sb, vs.sh, vs.sn, b, g, 0)[(int64_t)(t0 + t) * vs.sn + c]) : 0.f;
        }
        __syncthreads();
        const float Mk = Mx[qpk];
        for (int t = 0; t < tc; ++t) {
            const float vd = vv[t * W + d];
            const float* kr = kc + t * DP + mg * R;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                s[i] = fmaf(kr[i], vd, s[i]);
                ksr[i] += kr[i];
            }
            s1 += vd;
            cnt += 1.0f;
            if (!readout) continue;
            for (int hb = 0; hb < qpk; hb += HB) {
                const int nh = min(HB, qpk - hb);
                float* rb = red + buf * (NW * HB * W * 2);
                buf ^= 1;
                for (int hh = 0; hh < nh; ++hh) {
                    const float* qr = qc + ((int64_t)t * qpk + hb + hh) * DP + mg * R;
                    float f = 0.f, gg = 0.f;
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        f = fmaf(qr[i], s[i], f);
                        gg = fmaf(qr[i], ksr[i], gg);
                    }
#pragma unroll
                    for (int off = 32; off >= W; off >>= 1) {
                        f += __shfl_xor(f, off, 64);
                        gg += __shfl_xor(gg, off, 64);
                    }
                    if (lane < W) {
                        rb[((wave * HB + hh) * W + d) * 2] = f;
                        rb[((wave * HB + hh) * W + d) * 2 + 1] = gg;
                    }
                }
                // two buffers: the writes of round n + 2 follow barrier n + 1, which every thread reaches after reading round n
                __syncthreads();
                if (mg < nh) {
                    float F = 0.f, Gq = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        F += rb[((w * HB + mg) * W + d) * 2];
                        Gq += rb[((w * HB + mg) * W + d) * 2 + 1];
                    }
                    const float a = 1.0f / (Mx[hb + mg] * Mk);
                    const float val = (s1 + a * F) / (cnt + a * Gq);
                    if (d0 + d < D) {
                        const int64_t h = (int64_t)g * qpk + hb + mg;
                        store_out<T>(o, (((int64_t)b * G * qpk + h) * Tn + t0 + t) * D + d0 + d, val);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < R / 4; ++j) {
        reinterpret_cast<float4*>(rec + tid * R)[j] = make_float4(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3]);
        if (d == 0)
            reinterpret_cast<float4*>(rK + mg * R)[j] = make_float4(ksr[4 * j], ksr[4 * j + 1], ksr[4 * j + 2], ksr[4 * j + 3]);
    }
    if (mg == 0) rS1[d] = s1;
    if (tid == 0) rStat[0] = cnt;
}

static int chunk_tokens(int dp, int qpk, int T, bool readout) {
    const int per = dp + dp / NS + (readout ? qpk * dp : 0);
    int tc = STAGE_FLOATS / per;
    tc = tc < 1 ? 1 : (tc > MAX_CHUNK ? MAX_CHUNK : tc);
    return tc < T ? tc : T;
}

static size_t lds_floats(int dp, int qpk, int tc, bool readout) {
    const int W = dp / NS, NT = dp * 2;
    return (size_t)tc * (dp + W + (readout ? qpk * dp : 0)) + round4(NT / 16 * (qpk + 1)) + round4(qpk + 1) +
           2 * (NT / 64) * HB * W * 2;
}

template <typename T>
static int launch_advance_t(const void* q, const void* k, const void* v, Strides3 qs, Strides3 ks, Strides3 vs, float* state, void* o,
                            int B, int G, int qpk, int Tn, int D, hipStream_t stream) {
    const int dp = D <= 64 ? 64 : 128;
    const int tc = chunk_tokens(dp, qpk, Tn, o != nullptr);
    const size_t lds = sizeof(float) * lds_floats(dp, qpk, tc, o != nullptr);
    const dim3 grid((unsigned)(B * G * NS)), block(dp * 2);
    if (dp == 64)
        hipLaunchKernelGGL((linearmax_advance_kernel<T, 64>), grid, block, lds, stream, q, k, v, qs, ks, vs, state, o, G, qpk, D, Tn, tc);
    else
        hipLaunchKernelGGL((linearmax_advance_kernel<T, 128>), grid, block, lds, stream, q, k, v, qs, ks, vs, state, o, G, qpk, D, Tn, tc);
    return (int)hipGetLastError();
}

}  // namespace lmdec
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::lmdec;

extern "C" {

size_t fastmax_hip_linearmax_decode_state_bytes(int B, int H, int Hkv, int D) {
    if (B <= 0 || H <= 0 || Hkv <= 0 || D <= 0 || D > 128 || H % Hkv != 0 || H / Hkv > MAX_QPK) return 0;
    const int dp = D <= 64 ? 64 : 128;
    return sizeof(float) * (size_t)B * Hkv * NS * slab_floats(dp, H / Hkv);
}

int fastmax_hip_linearmax_decode_advance(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                         const void* v, const int64_t* v_strides, float* state, void* o, int B, int H, int Hkv,
                                         int T, int D, int dtype, void* stream) {
    if (!q || !k || !v || !state || !q_strides || !k_strides || !v_strides) return FASTMAX_E_NULL;
    if (dtype < FASTMAX_F32 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (T <= 0 || fastmax_hip_linearmax_decode_state_bytes(B, H, Hkv, D) == 0 || (int64_t)B * Hkv * NS > (int64_t)0x7fffffff)
        return FASTMAX_E_BAD_SHAPE;
    if (reinterpret_cast<uintptr_t>(state) % 16) return FASTMAX_E_ALIGNMENT;
    const Strides3 qs{q_strides[0], q_strides[1], q_strides[2]}, ks{k_strides[0], k_strides[1], k_strides[2]},
        vs{v_strides[0], v_strides[1], v_strides[2]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (dtype) {
        case FASTMAX_F32: return launch_advance_t<float>(q, k, v, qs, ks, vs, state, o, B, Hkv, H / Hkv, T, D, st);
        case FASTMAX_BF16: return launch_advance_t<bf16_t>(q, k, v, qs, ks, vs, state, o, B, Hkv, H / Hkv, T, D, st);
        default: return launch_advance_t<f16_t>(q, k, v, qs, ks, vs, state, o, B, Hkv, H / Hkv, T, D, st);
    }
}

}  // extern "C"
