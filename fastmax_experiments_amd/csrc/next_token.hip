// From the logits to the next token (include/fastmax_hip_next_token.h, include/fastmax_hip_nucleus.h): an exact top-k filter and
// a seeded sampler whose token stays in device memory.  The header's lm-head over the last position, fastmax_hip_last_logits,
// is in last_logits.hip with the other logits entry points.
//
//   select_threshold, sample_kernel   next_token_sample.h (shared with the decode cursor's sampler, decode_cursor.hip); here the
//                        instantiation that takes seed and draw number from the host, and the one with the top-p filter behind
//                        the top-k (include/fastmax_hip_nucleus.h: select_nucleus), with the mask kernel that exposes its kept set.
#include "fastmax_common.h"
#include "next_token_sample.h"
#include "../../include/fastmax_hip_next_token.h"
#include "../../include/fastmax_hip_nucleus.h"

namespace fastmax {

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
