// From a hidden state to the next token (include/fastmax_hip_next_token.h): the lm-head over the last position only, an exact
// top-k filter and a seeded sampler whose token stays in device memory.
//
//   last_logits_kernel   256 threads = 4 waves, a wave owns ROWS = 4 rows of W and up to G rows of x (G = 1, 2, 4, 8: the pass's
//                        row count rounded up, the surplus rows re-read the last one and are not stored).  Lane l takes the
//                        16-byte pieces l, l + 64, ... of every row: ROWS loads of W and G loads of x (L1 / L2) feed
//                        ROWS x G x E fused multiply-adds, W straight to registers (it is streamed once, no LDS round trip).
//                        Every (b, v) sum has ONE accumulator per lane, filled in index order from +0, and one xor butterfly
//                        over the lanes: the bits depend on C and the dtype only, not on G, the batch or the load route.
//   select_threshold, sample_kernel   next_token_sample.h (shared with the decode cursor's sampler, decode_cursor.hip); here the
//                        instantiation that takes seed and draw number from the host, and the one with the top-p filter behind
//                        the top-k (include/fastmax_hip_nucleus.h: select_nucleus), with the mask kernel that exposes its kept set.
#include "fastmax_common.h"
#include "next_token_sample.h"
#include "../../include/fastmax_hip_next_token.h"
#include "../../include/fastmax_hip_nucleus.h"

namespace fastmax {

typedef unsigned int nu32x4 __attribute__((ext_vector_type(4)));

// ---- last-row logits ---------------------------------------------------------------------------------------------------------
constexpr int LOGIT_ROWS = 4;            // rows of W per wave
constexpr int LOGIT_WAVES = 4;           // waves per workgroup
constexpr int LOGIT_GROUP = 8;           // rows of x per pass over W

// one piece (16 bytes, E elements) as floats; the element route takes the first n elements of a possibly short piece
template <typename T, bool VEC>
__device__ __forceinline__ void load_piece(const T* p, int n, float (&f)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (VEC) {
        const nu32x4 raw = *reinterpret_cast<const nu32x4*>(p);
        const T* pv = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = to_float(pv[e]);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = e < n ? to_float(p[e]) : 0.f;
    }
}

template <typename T, typename O, int G, bool VEC>
__global__ __launch_bounds__(256) void last_logits_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, int64_t ldw,
                                                          O* __restrict__ out, int64_t ldo, int nb, int V, int C) {
    constexpr int E = 16 / sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t v0 = ((int64_t)blockIdx.x * LOGIT_WAVES + wave) * LOGIT_ROWS;
    if (v0 >= V) return;                                  // the whole wave leaves; the kernel has no barrier
    const T* wr[LOGIT_ROWS];
    const T* xr[G];
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r) wr[r] = w + (v0 + r < V ? v0 + r : (int64_t)V - 1) * ldw;
#pragma unroll
    for (int g = 0; g < G; ++g) xr[g] = x + (int64_t)(g < nb ? g : nb - 1) * ldx;
    float acc[LOGIT_ROWS][G];
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[r][g] = 0.f;
    const int npieces = (C + E - 1) / E;
    constexpr int UNROLL = G <= 2 ? 2 : 1;                // more loads in flight where the registers allow it
#pragma unroll UNROLL
    for (int p = lane; p < npieces; p += 64) {
        const int c = p * E;
        const int n = C - c < E ? C - c : E;
        float wf[LOGIT_ROWS][E];
#pragma unroll
        for (int r = 0; r < LOGIT_ROWS; ++r) load_piece<T, VEC>(wr[r] + c, n, wf[r]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float xf[E];
            load_piece<T, VEC>(xr[g] + c, n, xf);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (VEC || e < n) {
#pragma unroll
                    for (int r = 0; r < LOGIT_ROWS; ++r) acc[r][g] = fmaf(xf[e], wf[r][e], acc[r][g]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float s = wave_sum(acc[r][g]);
            if (lane == 0 && v0 + r < V && g < nb) out[(int64_t)g * ldo + v0 + r] = from_float<O>(s);
        }
}

template <typename T, typename O, int G>
static void launch_logits_route(bool vec, dim3 grid, hipStream_t st, const T* x, int64_t ldx, const T* w, int64_t ldw, O* out,
                                int64_t ldo, int nb, int V, int C) {
    if (vec) hipLaunchKernelGGL((last_logits_kernel<T, O, G, true>), grid, dim3(256), 0, st, x, ldx, w, ldw, out, ldo, nb, V, C);
    else hipLaunchKernelGGL((last_logits_kernel<T, O, G, false>), grid, dim3(256), 0, st, x, ldx, w, ldw, out, ldo, nb, V, C);
}

template <typename T, typename O>
static int launch_logits(const void* xv, int64_t ldx, const void* wv, int64_t ldw, void* ov, int64_t ldo, int B, int V, int C,
                         hipStream_t st) {
    constexpr int E = 16 / sizeof(T);
    const T* x = reinterpret_cast<const T*>(xv);
    const T* w = reinterpret_cast<const T*>(wv);
    O* out = reinterpret_cast<O*>(ov);
    const bool vec = C % E == 0 && ldx % E == 0 && ldw % E == 0 && (reinterpret_cast<uintptr_t>(xv) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(wv) & 15) == 0;
    const int per_block = LOGIT_WAVES * LOGIT_ROWS;
    const dim3 grid((unsigned)(((int64_t)V + per_block - 1) / per_block));
    for (int b0 = 0; b0 < B; b0 += LOGIT_GROUP) {
        const int nb = B - b0 < LOGIT_GROUP ? B - b0 : LOGIT_GROUP;
        const T* xb = x + (int64_t)b0 * ldx;
        O* ob = out + (int64_t)b0 * ldo;
        if (nb == 1) launch_logits_route<T, O, 1>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else if (nb == 2) launch_logits_route<T, O, 2>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else if (nb <= 4) launch_logits_route<T, O, 4>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else launch_logits_route<T, O, 8>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
    }
    return (int)hipGetLastError();
}

// ---- exact top-k: the mask itself ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEL_THREADS) void topk_mask_kernel(const float* __restrict__ logits, int64_t ld, unsigned char* __restrict__ mask,
                                                                int64_t ldm, int V, int top_k) {
    __shared__ SelectShared sh;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    unsigned char* out = mask + (int64_t)blockIdx.x * ldm;
    const Threshold t = select_threshold(row, V, top_k, sh);
    for (int i = threadIdx.x; i < V; i += SEL_THREADS) out[i] = kept(t, order_key(row[i]), i) ? 1 : 0;
}

// ---- top-k, then top-p: the mask itself --------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEL_THREADS) void nucleus_mask_kernel(const float* __restrict__ logits, int64_t ld, unsigned char* __restrict__ mask,
                                                                   int64_t ldm, int V, int top_k, float top_p, float temperature) {
    __shared__ SelectShared sh;
    __shared__ NucleusShared ns;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    unsigned char* out = mask + (int64_t)blockIdx.x * ldm;
    const Threshold t = select_nucleus(row, V, select_threshold(row, V, top_k, sh), top_p, temperature, sh, ns);
    for (int i = threadIdx.x; i < V; i += SEL_THREADS) out[i] = kept(t, order_key(row[i]), i) ? 1 : 0;
}

}  // namespace fastmax

using namespace fastmax;

extern "C" {

int fastmax_hip_last_logits(const void* x, int64_t ldx, const void* w, int64_t ldw, void* logits, int64_t ldo, int B, int V, int C,
                            int dtype, int out_dtype, void* stream) {
    if (!x || !w || !logits) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16 || (out_dtype != FASTMAX_F32 && out_dtype != dtype)) return FASTMAX_E_BAD_DTYPE;
    if (B <= 0 || V <= 0 || C <= 0 || C > MAX_EXTENT || ldx < 0 || ldw < C || ldo < V) return FASTMAX_E_BAD_SHAPE;
    const size_t es = dtype == FASTMAX_F32 ? 4 : 2;
    if (!aligned_to(x, es) || !aligned_to(w, es) || !aligned_to(logits, out_dtype == FASTMAX_F32 ? 4 : 2)) return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FASTMAX_F32) return launch_logits<float, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    if (dtype == FASTMAX_BF16) {
        if (out_dtype == FASTMAX_F32) return launch_logits<bf16_t, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
        return launch_logits<bf16_t, bf16_t>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    }
    if (out_dtype == FASTMAX_F32) return launch_logits<f16_t, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    return launch_logits<f16_t, f16_t>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
}

int fastmax_hip_sample(const float* logits, int64_t ld, int64_t* tokens, int B, int V, int top_k, float temperature, int64_t seed,
                       int64_t draw, void* stream) {
    if (!logits || !tokens) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > MAX_EXTENT || ld < V || top_k < 0 || !(temperature >= 0.f && temperature <= 3.4028234e38f))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(tokens, 8)) return FASTMAX_E_ALIGNMENT;
    const uint64_t s = (uint64_t)seed, d = (uint64_t)draw;
    hipLaunchKernelGGL(sample_kernel<HostDraw>, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld,
                       tokens, V, top_k, temperature, HostDraw{{(unsigned)s, (unsigned)(s >> 32), (unsigned)d, (unsigned)(d >> 32)}});
    return (int)hipGetLastError();
}

int fastmax_hip_topk_mask(const float* logits, int64_t ld, void* mask, int64_t ldm, int B, int V, int top_k, void* stream) {
    if (!logits || !mask) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > MAX_EXTENT || ld < V || ldm < V || top_k < 0) return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4)) return FASTMAX_E_ALIGNMENT;
    hipLaunchKernelGGL(topk_mask_kernel, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld,
                       reinterpret_cast<unsigned char*>(mask), ldm, V, top_k);
    return (int)hipGetLastError();
}

int fastmax_hip_sample_nucleus(const float* logits, int64_t ld, int64_t* tokens, int B, int V, int top_k, float top_p,
                               float temperature, int64_t seed, int64_t draw, void* stream) {
    if (!logits || !tokens) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > NUCLEUS_MAX_V || ld < V || top_k < 0 || !(temperature >= 0.f && temperature <= 3.4028234e38f) ||
        !nucleus_share(top_p))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(tokens, 8)) return FASTMAX_E_ALIGNMENT;
    const uint64_t s = (uint64_t)seed, d = (uint64_t)draw;
    const Nucleus<HostDraw> from{{{(unsigned)s, (unsigned)(s >> 32), (unsigned)d, (unsigned)(d >> 32)}}, top_p};
    hipLaunchKernelGGL(sample_kernel<Nucleus<HostDraw>>, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       logits, ld, tokens, V, top_k, temperature, from);
    return (int)hipGetLastError();
}

int fastmax_hip_nucleus_mask(const float* logits, int64_t ld, void* mask, int64_t ldm, int B, int V, int top_k, float top_p,
                             float temperature, void* stream) {
    if (!logits || !mask) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > NUCLEUS_MAX_V || ld < V || ldm < V || top_k < 0 ||
        !(temperature >= 0.f && temperature <= 3.4028234e38f) || !nucleus_share(top_p))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4)) return FASTMAX_E_ALIGNMENT;
    hipLaunchKernelGGL(nucleus_mask_kernel, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld,
                       reinterpret_cast<unsigned char*>(mask), ldm, V, top_k, top_p, temperature);
    return (int)hipGetLastError();
}

}  // extern "C"
