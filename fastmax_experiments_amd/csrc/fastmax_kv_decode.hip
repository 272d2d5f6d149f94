// KV-cache decode for fastmax blocks (include/fastmax_hip_kv_decode.h): masked polynomial attention at each new position over
// a cache of K and V rows, head sizes 1 .. 256, the length a device word.
//
//     o_i = sum_{j <= n_i} f(s_j) V_j / sum_{j <= n_i} f(s_j),   s_j = (q_i . K_j) / nt,   f = 1 + s (+ s^2 / 2)
//
// There is no running maximum, so the sums over disjoint ranges of j simply add: a KV head's positions are cut into fixed chunks
// of CHUNK positions, one workgroup per (b, kv head, chunk, new token, block of <= 8 query heads) leaves a numerator row and a
// denominator per query head in the workspace, and a second kernel adds them in ascending chunk order.  A workgroup works for
// ONE new token, so its loop bound is that token's own position: nothing is masked, nothing past the position is read, and a
// row's bits cannot depend on how many tokens the call carries.  Grids come from the cache's capacity; the length is read from
// the state's header by every kernel and written by the call's last one only.
//
// The attend workgroup (256 threads) follows the "M <= 16 rows, stream the operand once" form: K and V go from global memory
// straight to registers, the few q rows sit in LDS as floats.
//   scores   8 lanes share a K row (a wave reads 8 rows = 8 x 128 contiguous bytes at D = 64 bf16 per instruction, 16 bytes per
//            lane); each lane keeps the partial dots of 4 rows x RB query heads, so one q piece read from LDS serves 4 K rows;
//            the 8 lanes are folded by an xor butterfly (fixed order).
//   values   a thread owns one 16-byte piece of the V row (TPR threads per row, NG rows in flight); group g of the NG takes
//            positions g, g + NG, ... in ascending order, f(s_j) comes from LDS as one RB-float read; the NG groups are added in
//            ascending group order through LDS, four query heads per round.
// Vector ALU, not matrix cores.  Measured (profiles/r23_kv_decode.md): with one query head per KV head the attend kernel streams
// the cache at 4.2 - 4.7 TB/s; at 8 query heads per KV head (about 8 flop per cache byte) it is compute-bound at 1.75 TB/s
// (D = 64) to 2.8 TB/s (D = 256).  A matrix-core form of the q_per_kv x chunk scores has not been built or timed.
#include "../../include/fastmax_hip_kv_decode.h"
#include "fastmax_common.h"

#include <cmath>

namespace fastmax {
namespace kvdec {

constexpr int CHUNK = FASTMAX_KV_CHUNK;      // positions per workgroup
constexpr int SLICE = FASTMAX_KV_SLICE;      // new tokens per attend / combine launch
constexpr int MAX_D = FASTMAX_KV_MAX_D;
constexpr int HDR_BYTES = FASTMAX_KV_HEADER_WORDS * 4;
constexpr int NT = 256;                      // threads of an attend workgroup
constexpr int MAX_NG = 32;                   // V rows in flight per workgroup
constexpr int LPR = 8;                       // lanes per K row
constexpr int ROWS_PER_PASS = NT / LPR;      // 32
constexpr int NPASS = CHUNK / ROWS_PER_PASS; // 4
static_assert(CHUNK % ROWS_PER_PASS == 0 && CHUNK % 128 == 0, "cap * D must be a multiple of 128 elements");

__host__ __device__ inline int64_t cap_of(int max_len) { return ((int64_t)max_len + CHUNK - 1) / CHUNK * CHUNK; }
__device__ __forceinline__ bool overflows(int len, int T, int max_len) { return len < 0 || (int64_t)len + T > (int64_t)max_len; }

// ---- row copies ----------------------------------------------------------------------------------------------------------------
// D elements src -> dst by the 64 threads of a workgroup: 16-byte pieces when both rows are whole aligned pieces, else elements
template <typename T>
__device__ __forceinline__ void copy_row(const T* __restrict__ src, T* __restrict__ dst, int D) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const bool vec = D % VEC == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
    if (vec) {
        for (int i = threadIdx.x; i < D / VEC; i += blockDim.x)
            reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = src[i];
    }
}

// row blockIdx.x of (b, g) = blockIdx.y, K (blockIdx.z == 0) or V, to cache position base + blockIdx.x
template <typename T>
__device__ __forceinline__ void put_row(const void* k, const void* v, Strides3 ks, Strides3 vs, T* kc, T* vc, int Hkv, int D,
                                        int64_t cap, int base) {
    const int t = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv;
    const int64_t row = ((int64_t)bg * cap + base + t) * D;
    if (blockIdx.z == 0) copy_row<T>(row_ptr<T>(k, ks.sb, ks.sh, ks.sn, b, g, t), kc + row, D);
    else copy_row<T>(row_ptr<T>(v, vs.sb, vs.sh, vs.sn, b, g, t), vc + row, D);
}

// grid: (T, B * Hkv, 2 = K / V); block: 64.  Rows 0 .. T-1 of an empty cache; one thread writes len = T (no workgroup of this
// launch reads the header).
template <typename T>
__global__ __launch_bounds__(64) void kv_load_kernel(const void* k, const void* v, Strides3 ks, Strides3 vs, int* hdr, T* kc, T* vc,
                                                     int Hkv, int Tn, int D, int64_t cap) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) hdr[FASTMAX_KV_LEN] = Tn;
    put_row<T>(k, v, ks, vs, kc, vc, Hkv, D, cap, 0);
}

// the same grid.  Rows len .. len + T - 1, unless that passes max_len; the header is only read.
template <typename T>
__global__ __launch_bounds__(64) void kv_append_kernel(const void* k, const void* v, Strides3 ks, Strides3 vs, const int* hdr, T* kc,
                                                       T* vc, int Hkv, int Tn, int D, int max_len, int64_t cap) {
    const int len = hdr[FASTMAX_KV_LEN];
    if (overflows(len, Tn, max_len)) return;
    put_row<T>(k, v, ks, vs, kc, vc, Hkv, D, cap, len);
}

// ---- attend ----------------------------------------------------------------------------------------------------------------
// VEC elements of a cache row as floats; VP: one 16-byte load
template <typename T, bool VP>
__device__ __forceinline__ void load_piece(const T* __restrict__ row, int piece, float* x) {
    if constexpr (VP) {
        constexpr int VEC = 16 / (int)sizeof(T);
        union { uint4 u; T e[VEC]; } w;
        w.u = reinterpret_cast<const uint4*>(row)[piece];
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = to_float(w.e[e]);
    } else {
        x[0] = to_float(row[piece]);
    }
}

__device__ __forceinline__ float poly(float s, int p) { return p == 2 ? poly_f<2>(s) : poly_f<1>(s); }

// grid: (cap / CHUNK, B * Hkv, ts * ceil(qpk / RB)); block: NT.  part: (B, H, ts, nchunk, D + 1) floats.
template <typename T, int RB, bool VP>
__global__ __launch_bounds__(NT) void kv_attend_kernel(const void* q, Strides3 qs, const int* __restrict__ hdr,
                                                       const T* __restrict__ kc, const T* __restrict__ vc, float* __restrict__ part,
                                                       int Hkv, int qpk, int D, int max_len, int64_t cap, int Tn, int t0, int ts,
                                                       int p, float inv_nt) {
    constexpr int VEC = VP ? 16 / (int)sizeof(T) : 1;
    constexpr int RR = RB < 4 ? RB : 4;                      // query heads per reduction round
    __shared__ __align__(16) float qf[RB * MAX_D];           // the q rows, zero-padded to whole pieces
    __shared__ __align__(16) float fs[CHUNK * RB];           // f(s_j) of every position, the RB heads of a position together
    __shared__ __align__(16) float red[NT * VEC * RR];       // [group][head of the round][column]
    __shared__ float dred[MAX_NG * RB];                      // [group][head] denominators

    const int len = hdr[FASTMAX_KV_LEN];
    if (overflows(len, Tn, max_len)) return;
    const int nhb = (qpk + RB - 1) / RB;
    const int c = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv, ti = blockIdx.z / nhb, h0 = (blockIdx.z % nhb) * RB;
    const int64_t n = (int64_t)len + t0 + ti;                // this token's position
    const int64_t j0 = (int64_t)c * CHUNK;
    if (j0 > n) return;
    const int jc = (int)(n - j0 + 1 < CHUNK ? n - j0 + 1 : CHUNK);      // positions j0 .. j0 + jc - 1, all <= n
    const int nr = qpk - h0 < RB ? qpk - h0 : RB;            // live query heads of this block
    const int P = (D + VEC - 1) / VEC, Dp = P * VEC;         // pieces per row
    const int tid = threadIdx.x;
    const T* kbase = kc + ((int64_t)bg * cap + j0) * D;
    const T* vbase = vc + ((int64_t)bg * cap + j0) * D;

    for (int i = tid; i < RB * Dp; i += NT) {
        const int r = i / Dp, e = i % Dp;
        qf[i] = (r < nr && e < D) ? to_float(row_ptr<T>(q, qs.sb, qs.sh, qs.sn, b, g * qpk + h0 + r, t0 + ti)[e]) : 0.f;
    }
    __syncthreads();

    // scores: lane (row, sub) of a pass takes pieces sub, sub + 8, ... of its K row
    {
        const int sub = tid & (LPR - 1), rw = tid / LPR;
        float dot[NPASS][RB];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
            for (int r = 0; r < RB; ++r) dot[ps][r] = 0.f;
        for (int i = sub; i < P; i += LPR) {
            float kx[NPASS][VEC];
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const int j = ps * ROWS_PER_PASS + rw;
                if (j < jc) {
                    load_piece<T, VP>(kbase + (int64_t)j * D, i, kx[ps]);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) kx[ps][e] = 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                float qv[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) qv[e] = qf[r * Dp + i * VEC + e];
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) dot[ps][r] = fmaf(kx[ps][e], qv[e], dot[ps][r]);
            }
        }
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int j = ps * ROWS_PER_PASS + rw;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                float d = dot[ps][r];
#pragma unroll
                for (int off = 1; off < LPR; off <<= 1) d += __shfl_xor(d, off, 64);
                if (sub == 0 && j < jc) fs[j * RB + r] = poly(d * inv_nt, p);
            }
        }
    }
    __syncthreads();

    // values: thread (group, piece) adds f(s_j) V_j over its group's positions
    const int TPR = P;
    const int NG = NT / TPR < MAX_NG ? NT / TPR : MAX_NG;
    const int grp = tid / TPR, piece = tid % TPR;
    const bool active = grp < NG;
    float acc[RB][VEC], den[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        den[r] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
    }
    if (active) {
#pragma unroll 4
        for (int j = grp; j < jc; j += NG) {
            float vx[VEC];
            load_piece<T, VP>(vbase + (int64_t)j * D, piece, vx);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float f = fs[j * RB + r];
                den[r] += f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[r][e] = fmaf(f, vx[e], acc[r][e]);
            }
        }
        if (piece == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r) dred[grp * RB + r] = den[r];
        }
    }

    // the NG groups in ascending order, RR heads per round
    float* out = part + ((((int64_t)b * Hkv * qpk + (int64_t)g * qpk + h0) * ts + ti) * gridDim.x + c) * (D + 1);
    const int64_t head_stride = (int64_t)ts * gridDim.x * (D + 1);
#pragma unroll
    for (int r0 = 0; r0 < RB; r0 += RR) {
        __syncthreads();                                     // the previous round's sums are read; first round: fs, dred
        if (active) {
#pragma unroll
            for (int rr = 0; rr < RR; ++rr)
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[(grp * RR + rr) * Dp + piece * VEC + e] = acc[r0 + rr][e];
        }
        __syncthreads();
        for (int i = tid; i < RR * Dp; i += NT) {
            const int rr = i / Dp, col = i % Dp;
            float s = 0.f;
            for (int gi = 0; gi < NG; ++gi) s += red[(gi * RR + rr) * Dp + col];
            if (r0 + rr < nr && col < D) out[(r0 + rr) * head_stride + col] = s;
        }
    }
    if (tid < nr) {
        float s = 0.f;
        for (int gi = 0; gi < NG; ++gi) s += dred[gi * RB + tid];
        out[tid * head_stride + D] = s;
    }
}

// grid: (B * H, ts); block: 64 .. 256 threads over the columns
template <typename T>
__global__ void kv_combine_kernel(const int* __restrict__ hdr, const float* __restrict__ part, T* __restrict__ o, int D, int max_len,
                                  int Tn, int t0, int ts, int nchunk) {
    const int len = hdr[FASTMAX_KV_LEN];
    const int ti = blockIdx.y;
    T* orow = o + ((int64_t)blockIdx.x * Tn + t0 + ti) * D;
    if (overflows(len, Tn, max_len)) {
        for (int d = threadIdx.x; d < D; d += blockDim.x) orow[d] = from_float<T>(0.f);
        return;
    }
    const int nc = (int)(((int64_t)len + t0 + ti) / CHUNK) + 1;
    const float* base = part + ((int64_t)blockIdx.x * ts + ti) * nchunk * (D + 1);
    constexpr int U = 16;          // partials in flight: the loads of a batch are independent, the additions stay in chunk order
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float num = 0.f, den = 0.f;
        for (int c0 = 0; c0 < nc; c0 += U) {
            float a[U], w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u < nc ? c0 + u : nc - 1;
                a[u] = base[(int64_t)c * (D + 1) + d];
                w[u] = base[(int64_t)c * (D + 1) + D];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c0 + u < nc) {
                    num += a[u];
                    den += w[u];
                }
            }
        }
        orow[d] = from_float<T>(num / den);
    }
}

// one thread: the call's only writer of a header word
__global__ void kv_commit_kernel(int* hdr, int Tn, int max_len) {
    const int len = hdr[FASTMAX_KV_LEN];
    if (overflows(len, Tn, max_len)) hdr[FASTMAX_KV_OVERFLOW] = 1;
    else hdr[FASTMAX_KV_LEN] = len + Tn;
}

__global__ void kv_set_len_kernel(int* hdr, int new_len) {
    if (new_len >= 0 && new_len <= hdr[FASTMAX_KV_LEN]) hdr[FASTMAX_KV_LEN] = new_len;
    else hdr[FASTMAX_KV_OVERFLOW] = 1;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct Call {
    const void *q, *k, *v;
    Strides3 qs, ks, vs;
    void *state, *o;
    float* ws;
    int B, H, Hkv, T, D, max_len, p;
    float inv_nt;
    hipStream_t stream;
};

template <typename T, int RB, bool VP>
static void launch_attend(const Call& a, const T* kc, const T* vc, int t0, int ts) {
    const int qpk = a.H / a.Hkv, nhb = (qpk + RB - 1) / RB;
    const int64_t cap = cap_of(a.max_len);
    const dim3 grid((unsigned)(cap / CHUNK), (unsigned)(a.B * a.Hkv), (unsigned)(ts * nhb));
    hipLaunchKernelGGL((kv_attend_kernel<T, RB, VP>), grid, dim3(NT), 0, a.stream, a.q, a.qs, reinterpret_cast<const int*>(a.state),
                       kc, vc, a.ws, a.Hkv, qpk, a.D, a.max_len, cap, a.T, t0, ts, a.p, a.inv_nt);
}

template <typename T, bool VP>
static void launch_attend_rb(const Call& a, const T* kc, const T* vc, int t0, int ts) {
    const int qpk = a.H / a.Hkv;
    if (qpk == 1) launch_attend<T, 1, VP>(a, kc, vc, t0, ts);
    else if (qpk == 2) launch_attend<T, 2, VP>(a, kc, vc, t0, ts);
    else if (qpk <= 4) launch_attend<T, 4, VP>(a, kc, vc, t0, ts);
    else launch_attend<T, 8, VP>(a, kc, vc, t0, ts);
}

template <typename T>
static int append_attend_t(const Call& a) {
    const int64_t cap = cap_of(a.max_len);
    int* hdr = reinterpret_cast<int*>(a.state);
    T* kc = reinterpret_cast<T*>(reinterpret_cast<char*>(a.state) + HDR_BYTES);
    T* vc = kc + (int64_t)a.B * a.Hkv * cap * a.D;
    hipLaunchKernelGGL((kv_append_kernel<T>), dim3((unsigned)a.T, (unsigned)(a.B * a.Hkv), 2), dim3(64), 0, a.stream, a.k, a.v, a.ks,
                       a.vs, hdr, kc, vc, a.Hkv, a.T, a.D, a.max_len, cap);
    const bool vp = a.D % (16 / (int)sizeof(T)) == 0;        // cache rows are whole 16-byte pieces (the caches start on one)
    const int cthreads = a.D <= 64 ? 64 : (a.D <= 128 ? 128 : 256);
    for (int t0 = 0; t0 < a.T; t0 += SLICE) {
        const int ts = a.T - t0 < SLICE ? a.T - t0 : SLICE;
        if (vp) launch_attend_rb<T, true>(a, kc, vc, t0, ts);
        else launch_attend_rb<T, false>(a, kc, vc, t0, ts);
        hipLaunchKernelGGL((kv_combine_kernel<T>), dim3((unsigned)(a.B * a.H), (unsigned)ts), dim3(cthreads), 0, a.stream, hdr, a.ws,
                           reinterpret_cast<T*>(a.o), a.D, a.max_len, a.T, t0, ts, (int)(cap / CHUNK));
    }
    hipLaunchKernelGGL(kv_commit_kernel, dim3(1), dim3(1), 0, a.stream, hdr, a.T, a.max_len);
    return (int)hipGetLastError();
}

template <typename T>
static int load_t(const void* k, Strides3 ks, const void* v, Strides3 vs, void* state, int B, int Hkv, int Tn, int D, int max_len,
                  hipStream_t stream) {
    const int64_t cap = cap_of(max_len);
    T* kc = reinterpret_cast<T*>(reinterpret_cast<char*>(state) + HDR_BYTES);
    T* vc = kc + (int64_t)B * Hkv * cap * D;
    hipLaunchKernelGGL((kv_load_kernel<T>), dim3((unsigned)Tn, (unsigned)(B * Hkv), 2), dim3(64), 0, stream, k, v, ks, vs,
                       reinterpret_cast<int*>(state), kc, vc, Hkv, Tn, D, cap);
    return (int)hipGetLastError();
}

static size_t elem_size(int dtype) { return dtype == FASTMAX_F32 ? 4 : 2; }
static bool aligned(const void* p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace kvdec
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::kvdec;

extern "C" {

size_t fastmax_hip_kv_decode_state_bytes(int B, int Hkv, int D, int max_len, int dtype) {
    if (B <= 0 || Hkv <= 0 || D <= 0 || D > MAX_D || max_len <= 0 || (int64_t)B * Hkv > 65535) return 0;
    if (dtype < FASTMAX_F32 || dtype > FASTMAX_F16) return 0;
    return (size_t)HDR_BYTES + 2 * (size_t)B * Hkv * (size_t)cap_of(max_len) * D * elem_size(dtype);
}

size_t fastmax_hip_kv_decode_workspace(int B, int H, int Hkv, int T, int D, int max_len) {
    if (fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, FASTMAX_F32) == 0 || H <= 0 || H % Hkv != 0 || T <= 0) return 0;
    return sizeof(float) * (size_t)B * H * (size_t)(T < SLICE ? T : SLICE) * (size_t)(cap_of(max_len) / CHUNK) * (D + 1);
}

int fastmax_hip_kv_decode_load(const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides, void* state, int B,
                               int Hkv, int T, int D, int max_len, int dtype, void* stream) {
    if (!k || !v || !k_strides || !v_strides || !state) return FASTMAX_E_NULL;
    if (dtype < FASTMAX_F32 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (T <= 0 || fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, dtype) == 0 || T > max_len) return FASTMAX_E_BAD_SHAPE;
    if (!aligned(state, 16) || !aligned(k, elem_size(dtype)) || !aligned(v, elem_size(dtype))) return FASTMAX_E_ALIGNMENT;
    const Strides3 ks{k_strides[0], k_strides[1], k_strides[2]}, vs{v_strides[0], v_strides[1], v_strides[2]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (dtype) {
        case FASTMAX_F32: return load_t<float>(k, ks, v, vs, state, B, Hkv, T, D, max_len, st);
        case FASTMAX_BF16: return load_t<bf16_t>(k, ks, v, vs, state, B, Hkv, T, D, max_len, st);
        default: return load_t<f16_t>(k, ks, v, vs, state, B, Hkv, T, D, max_len, st);
    }
}

int fastmax_hip_kv_decode_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                        const void* v, const int64_t* v_strides, void* state, void* o, int B, int H, int Hkv, int T,
                                        int D, int max_len, int dtype, int p, float inv_nt, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !state || !o || !workspace) return FASTMAX_E_NULL;
    if (dtype < FASTMAX_F32 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (p != 1 && p != 2) return FASTMAX_E_BAD_P;
    if (T <= 0 || fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, dtype) == 0 || H <= 0 || H % Hkv != 0 || !std::isfinite(inv_nt))
        return FASTMAX_E_BAD_SHAPE;
    const size_t es = elem_size(dtype);
    if (!aligned(state, 16) || !aligned(workspace, 16) || !aligned(q, es) || !aligned(k, es) || !aligned(v, es) || !aligned(o, es))
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_kv_decode_workspace(B, H, Hkv, T, D, max_len)) return FASTMAX_E_WORKSPACE;
    Call a;
    a.q = q, a.k = k, a.v = v;
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.state = state, a.o = o, a.ws = reinterpret_cast<float*>(workspace);
    a.B = B, a.H = H, a.Hkv = Hkv, a.T = T, a.D = D, a.max_len = max_len, a.p = p, a.inv_nt = inv_nt;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    switch (dtype) {
        case FASTMAX_F32: return append_attend_t<float>(a);
        case FASTMAX_BF16: return append_attend_t<bf16_t>(a);
        default: return append_attend_t<f16_t>(a);
    }
}

int fastmax_hip_kv_decode_set_len(void* state, int new_len, int max_len, void* stream) {
    if (!state) return FASTMAX_E_NULL;
    if (max_len <= 0 || new_len < 0 || new_len > max_len) return FASTMAX_E_BAD_SHAPE;
    if (!aligned(state, 16)) return FASTMAX_E_ALIGNMENT;
    hipLaunchKernelGGL(kv_set_len_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<int*>(state),
                       new_len);
    return (int)hipGetLastError();
}

}  // extern "C"
