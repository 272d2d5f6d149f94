// Softmax KV-cache decode (include/fastmax_hip_softmax.h: fastmax_hip_softmax_kv_append_attend) on the cache layout of
// include/fastmax_hip_kv_decode.h: a 64-byte header (length, sticky overflow flag), then the K and the V rows, cap = max_len up to a
// whole chunk of CHUNK positions.
//
//     o_i = sum_{j <= n_i} p_j V_j / sum_{j <= n_i} p_j,   p_j = exp(scale q_i . K_j - max_j),   n_i = len + i
//
// Unlike the polynomial route (fastmax_kv_decode.hip) the sums over disjoint ranges of j do not simply add: every partial carries
// the maximum it was taken against, and a merge rescales to the common maximum first.
//
// append   one workgroup per (new token, (b, g), K / V) copies a row into the cache as 16-byte pieces.  Cache rows only.
// attend   one workgroup (4 waves) per (chunk, (b, g), new token x block of <= 16 query heads of g).  A workgroup works for ONE new
//          token, so its bound is that token's own position n: a row's bits do not depend on T, B, the batch row, max_len, strides.
//          The matrix-core form of the q_per_kv x chunk scores, with v_mfma_f32_16x16x32:
//   Q     the <= 16 query heads are the 16 columns of S^T: B-operand fragments (lane: head lane & 15, columns 32 s + 8 (lane >> 4)
//         ..+7), loaded once from global memory into registers; heads past the group and columns past D are zeros.
//   K     wave w owns positions 32 w .. 32 w + 31 of the chunk as two 16-row A operands; each lane loads its 16-byte pieces of
//         its row straight from the cache in global memory into the operand registers (row lane & 15, the same columns): no LDS.
//   S^T   = K Q^T, float32; a lane then holds one head (lane & 15) and keys 4 (lane >> 4) + {0..3} of each 16-key tile: the
//         B-operand fragment of the next product.  x = s * scale * log2 e; positions past n are SELECTED to -inf.
//   V     the chunk's rows go through LDS (all 256 threads, 16-byte pieces, rows padded to 2 DP + 64 bytes; pieces of positions
//         past n and of columns past D are written as zeros and never loaded: 0 * NaN would be NaN in a matrix product) and
//         come back transposed by ds_read_b64_tr_b16 as the A operand of O^T += V^T P^T.
//   wave  (m, l, O^T) of its 32 positions: m by a butterfly over the four lane groups, l likewise, O^T as DP / 16 tiles.
//   merge the four waves leave m, l in LDS; M = their maximum; each wave scales its O^T by exp2(m - M) and writes it over the
//         (no longer needed) V image; then the 256 threads add the four in wave order and write the workgroup's partial
//         (M, l, D numerator floats) of each query head to the workspace.  Chunk 0's workgroup also leaves the row's number of
//         chunks there (0 when the guard fired), so that combine never reads the header.
// combine  one workgroup per (b * H + h, new token): M = max of the chunk maxima, then numerator and l as sums of the partials
//          times exp2(m_c - M) in ascending chunk order; o = numerator / l, lse = (M + log2 l) ln 2.  Thread 0 of workgroup (0, 0)
//          of the call's LAST combine launch advances the header's length (or sets the overflow flag): the only access to the
//          header in that launch, and the only write to it in the call.
// LDS of attend: 128 (2 DP + 64) + 512 bytes: DP = 32: 16,896; 64: 25,088; 128: 41,472; 256: 74,240.  Registers: 40 / 64 / 104 / 184.
#include "../../include/fastmax_hip_softmax.h"
#include "softmax_kv_common.h"          // Op, the constants, overflows, sm_append_kernel, sm_combine_kernel, pieces: shared

namespace fastmax {
namespace smkv {

// workspace: part (B * H, ts, nchunk, D + 2) floats = (m, l, numerator), then nchunks (B * H, ts) ints
// grid: (cap / CHUNK, B * Hkv, ts * ceil(qpk / RB)); block: NT; dynamic LDS: attend_lds<32 NS>()
template <typename T, int NS>
__global__ __launch_bounds__(NT) void sm_attend_kernel(const uint16_t* __restrict__ q, Strides3 qs, const int* __restrict__ hdr,
                                                       const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                       float* __restrict__ part, int* __restrict__ nchunks, int Hkv, int qpk, int D,
                                                       int max_len, int64_t cap, int Tn, int t0, int ts, float c2) {
    typedef typename Op<T>::v8 V8;
    constexpr int DP = 32 * NS, DT = DP / 16, PPV = CHUNK * (DP / 8) / NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wm[NW][RB], wl[NW][RB];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, gq = lane >> 4;
    const int nhb = (qpk + RB - 1) / RB;
    const int c = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv, ti = blockIdx.z / nhb, h0 = (blockIdx.z % nhb) * RB;
    const int nr = qpk - h0 < RB ? qpk - h0 : RB;            // live query heads of this block
    const int nchunk = gridDim.x;
    const int64_t head0 = (int64_t)bg * qpk + h0;            // b * H + g * qpk + h0
    const int len = hdr[FASTMAX_KV_LEN];
    const bool over = overflows(len, Tn, max_len);
    const int64_t n = (int64_t)len + t0 + ti;                // this token's position
    if (c == 0 && tid < nr) nchunks[(head0 + tid) * ts + ti] = over ? 0 : (int)(n / CHUNK) + 1;
    const int64_t j0 = (int64_t)c * CHUNK;
    if (over || j0 > n) return;
    const uint16_t* kbase = kc + ((int64_t)bg * cap + j0) * D;
    const uint16_t* vbase = vc + ((int64_t)bg * cap + j0) * D;
    const int jn = (int)(n - j0);                            // positions 0 .. jn of the chunk are live (jn may pass CHUNK - 1)

    // K operands of this wave and the Q operands, from global memory
    V8 kf[2][NS], qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int col = 32 * s + 8 * gq;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = WPOS * w + 16 * t + r;
            const uint4 x = (j <= jn && col < D) ? *reinterpret_cast<const uint4*>(kbase + (int64_t)j * D + col) : uint4{0, 0, 0, 0};
            kf[t][s] = __builtin_bit_cast(V8, x);
        }
        const uint4 x = (r < nr && col < D) ? *reinterpret_cast<const uint4*>(q + (int64_t)b * qs.sb + (int64_t)(g * qpk + h0 + r) * qs.sh +
                                                                              (int64_t)(t0 + ti) * qs.sn + col)
                                            : uint4{0, 0, 0, 0};
        qf[s] = __builtin_bit_cast(V8, x);
    }
    // the chunk's V rows into LDS
#pragma unroll
    for (int u = 0; u < PPV; ++u) {
        const int i = tid + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        const uint4 x = (row <= jn && 8 * pc < D) ? *reinterpret_cast<const uint4*>(vbase + (int64_t)row * D + 8 * pc) : uint4{0, 0, 0, 0};
        *reinterpret_cast<uint4*>(smem + row * v_row<DP>() + 16 * pc) = x;
    }

    // S^T of the wave's 32 positions, masked by selection; the wave's maximum per head
    float x[8], mw = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) st = Op<T>::mma(kf[t][s], qf[s], st);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = WPOS * w + 16 * t + 4 * gq + i;
            x[4 * t + i] = j <= jn ? st[i] * c2 : -INFINITY;
            mw = fmaxf(mw, x[4 * t + i]);
        }
    }
    mw = fmaxf(mw, __shfl_xor(mw, 16, 64));
    mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
    const float msafe = mw == -INFINITY ? 0.f : mw;          // a wave with no live position: every p is exp2(-inf) = 0
    float lw = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = __builtin_amdgcn_exp2f(x[i] - msafe);
        lw += x[i];
    }
    lw += __shfl_xor(lw, 16, 64);
    lw += __shfl_xor(lw, 32, 64);
    const V8 pf = Op<T>::round8(x);
    if (gq == 0) wm[w][r] = mw, wl[w][r] = lw;
    __syncthreads();                                         // the V image and the waves' m, l are written

    // O^T = V^T P^T: tile dt holds columns 16 dt + 4 gq + {0..3} of head r
    f32x4 acc[DT];
    {
        const int qq = r >> 2, pp = r & 3;
        const char* va = smem + (WPOS * w + 4 * gq + qq) * v_row<DP>() + 8 * pp;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            union { V8 v; s16x4 h[2]; } u;
            u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt));
            u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt + 16 * v_row<DP>()));
            acc[dt] = Op<T>::mma(u.v, pf, f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    float M = wm[0][r];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) M = fmaxf(M, wm[ww][r]);          // finite: position j0 of wave 0 is live
    const float sc = __builtin_amdgcn_exp2f(mw - M);
    __syncthreads();                                         // every wave has read its V rows: the image becomes the four O^T
    float* red = reinterpret_cast<float*>(smem);             // [wave][head][DP]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<f32x4*>(red + ((w * RB + r) * DP + 16 * dt + 4 * gq)) = acc[dt] * sc;
    __syncthreads();

    float* out = part + (((head0 * ts + ti) * nchunk) + c) * (D + 2);
    const int64_t head_stride = (int64_t)ts * nchunk * (D + 2);
    for (int i = tid; i < RB * DP; i += NT) {
        const int hd = i / DP, col = i % DP;
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += red[(ww * RB + hd) * DP + col];
        if (hd < nr && col < D) out[hd * head_stride + 2 + col] = s;
    }
    if (tid < nr) {
        float Mh = wm[0][tid];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) Mh = fmaxf(Mh, wm[ww][tid]);
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += wl[ww][tid] * __builtin_amdgcn_exp2f(wm[ww][tid] - Mh);
        out[tid * head_stride] = Mh;
        out[tid * head_stride + 1] = s;
    }
}

struct Call {
    const uint16_t *q, *k, *v;
    Strides3 qs, ks, vs;
    void *state, *o;
    float *lse, *ws;
    int B, H, Hkv, T, D, max_len;
    float c2;
    hipStream_t stream;
};

template <typename T, int NS>
static int launch_attend(const Call& a, const uint16_t* kc, const uint16_t* vc, float* part, int* nchunks, int t0, int ts) {
    auto kern = sm_attend_kernel<T, NS>;
    constexpr int lds = attend_lds<32 * NS>();
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int qpk = a.H / a.Hkv, nhb = (qpk + RB - 1) / RB;
    const int64_t cap = cap_of(a.max_len);
    const dim3 grid((unsigned)(cap / CHUNK), (unsigned)(a.B * a.Hkv), (unsigned)(ts * nhb));
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, a.stream, a.q, a.qs, reinterpret_cast<const int*>(a.state), kc, vc, part, nchunks,
                       a.Hkv, qpk, a.D, a.max_len, cap, a.T, t0, ts, a.c2);
    return (int)hipGetLastError();
}

template <typename T> static int append_attend_t(const Call& a) {
    const int64_t cap = cap_of(a.max_len);
    const int nchunk = (int)(cap / CHUNK), tsmax = a.T < SLICE ? a.T : SLICE;
    int* hdr = reinterpret_cast<int*>(a.state);
    uint16_t* kc = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.state) + HDR_BYTES);
    uint16_t* vc = kc + (int64_t)a.B * a.Hkv * cap * a.D;
    float* part = a.ws;
    int* nchunks = reinterpret_cast<int*>(part + (int64_t)a.B * a.H * tsmax * nchunk * (a.D + 2));
    hipLaunchKernelGGL(sm_append_kernel, dim3((unsigned)a.T, (unsigned)(a.B * a.Hkv), 2), dim3(64), 0, a.stream, a.k, a.v, a.ks, a.vs, hdr,
                       kc, vc, a.Hkv, a.T, a.D, a.max_len, cap);
    const int cthreads = a.D <= 64 ? 64 : (a.D <= 128 ? 128 : 256);
    for (int t0 = 0; t0 < a.T; t0 += SLICE) {
        const int ts = a.T - t0 < SLICE ? a.T - t0 : SLICE;
        int rc;
        if (a.D <= 32) rc = launch_attend<T, 1>(a, kc, vc, part, nchunks, t0, ts);
        else if (a.D <= 64) rc = launch_attend<T, 2>(a, kc, vc, part, nchunks, t0, ts);
        else if (a.D <= 128) rc = launch_attend<T, 4>(a, kc, vc, part, nchunks, t0, ts);
        else rc = launch_attend<T, 8>(a, kc, vc, part, nchunks, t0, ts);
        if (rc != 0) return rc;
        hipLaunchKernelGGL((sm_combine_kernel<T>), dim3((unsigned)(a.B * a.H), (unsigned)ts), dim3(cthreads), 0, a.stream, hdr, part, nchunks,
                           reinterpret_cast<T*>(a.o), a.lse, a.D, a.max_len, a.T, t0, ts, nchunk, (int)(t0 + ts == a.T));
    }
    return (int)hipGetLastError();
}

static bool shape_ok(int B, int H, int Hkv, int T, int D, int max_len) {
    return T > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && D >= 8 && D % 8 == 0 && (int64_t)B * H <= 65535 &&
           fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, FASTMAX_BF16) != 0;
}

}  // namespace smkv
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::smkv;

extern "C" {

size_t fastmax_hip_softmax_kv_workspace(int B, int H, int Hkv, int T, int D, int max_len) {
    if (!shape_ok(B, H, Hkv, T, D, max_len)) return 0;
    return sizeof(float) * (size_t)B * H * (size_t)(T < SLICE ? T : SLICE) * ((size_t)(cap_of(max_len) / CHUNK) * (D + 2) + 2);
}

int fastmax_hip_softmax_kv_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                         const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B, int H,
                                         int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !state || !o || !workspace) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!shape_ok(B, H, Hkv, T, D, max_len) || !std::isfinite(scale)) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(k, k_strides) || !pieces(v, v_strides) || reinterpret_cast<uintptr_t>(state) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(o) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(lse) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_softmax_kv_workspace(B, H, Hkv, T, D, max_len)) return FASTMAX_E_WORKSPACE;
    Call a;
    a.q = reinterpret_cast<const uint16_t*>(q), a.k = reinterpret_cast<const uint16_t*>(k), a.v = reinterpret_cast<const uint16_t*>(v);
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.state = state, a.o = o, a.lse = lse, a.ws = reinterpret_cast<float*>(workspace);
    a.B = B, a.H = H, a.Hkv = Hkv, a.T = T, a.D = D, a.max_len = max_len;
    a.c2 = scale * 1.4426950408889634f;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? append_attend_t<bf16_t>(a) : append_attend_t<f16_t>(a);
}

}  // extern "C"
