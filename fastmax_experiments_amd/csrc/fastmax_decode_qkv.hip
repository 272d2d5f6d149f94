// The second-order (p = 2) decode step taken straight from the attention block's QKV projection (include/fastmax_hip_generate.h).
//
// One generated token through the attention sub-layer is: QKV projection -> de-interleave + RoPE -> step -> finalize -> output
// projection.  The de-interleave + RoPE launch moves (n_head + 2 groups) head rows that the step kernel only copies into LDS
// anyway, so here the step's loader reads them from the projection's (B, G, qpk + 2, D) block and rotates q and k on the
// way: one launch less per token and layer.  Everything after the loader is p2_decode_step_kernel as it is
// (fastmax_decode_p2_step.h): same grid, same row partition, same fixed-order sums, same finalize.
//
// The loader reproduces fastmax_rope.hip's arithmetic and roundings (x cos + rot(x) sin: two float32 products and their sum
// unfused; with 16-bit tables each product rounded to the tensor dtype first; the result rounded to the tensor dtype, which
// is what the split pass stores and the step reads back), so outputs and state are bit-identical to split + step.
// Every workgroup rotates its own copy of the D-element k and the group's query heads: a few hundred flops beside a pass
// over its share of the state.
#include "../../include/fastmax_hip_generate.h"
#include "fastmax_decode_p2_step.h"

namespace fastmax {
namespace p2dec {

template <typename T>
struct QkvSrc {
    const T* qkv;             // (B, G, qpk + 2, D)
    const float *cos, *sin;   // one row of rope_n each
    int G, total, D, rope_n, tables16;

    __device__ __forceinline__ const T* row(int b, int g, int slot) const {
        return qkv + (((int64_t)b * G + g) * total + slot) * D;
    }
    // element d of a query or key row after RoPE, as the split pass would have stored it
    __device__ __forceinline__ float rotated(const T* r, int d) const {
        const float x = to_float(r[d]);
        if (d >= rope_n) return x;
        const int half = rope_n >> 1;
        // out[d] = x[d] cos[d] - x[d + half] sin[d] (d < half);  out[d] = x[d] cos[d] + x[d - half] sin[d] (d >= half)
        const float y = d < half ? -to_float(r[d + half]) : to_float(r[d - half]);
        const float c = cos[d], s = sin[d];
        float out;
        if (sizeof(T) == 2 && tables16) out = to_float(from_float<T>(x * c)) + to_float(from_float<T>(y * s));
        else out = mul_add_unfused(x, c, y, s);
        return to_float(from_float<T>(out));
    }
    __device__ __forceinline__ float k(int b, int g, int d) const { return rotated(row(b, g, total - 2), d); }
    __device__ __forceinline__ float v(int b, int g, int d) const { return to_float(row(b, g, total - 1)[d]); }
    __device__ __forceinline__ float q(int b, int g, int, int i, int d) const { return rotated(row(b, g, i), d); }
};

template <typename T>
static int launch_step_qkv_t(const void* qkv, const float* cos, const float* sin, float* state, void* o, int B, int G, int qpk,
                             int D, int rope_n, int tables16, int out_dtype, float a, hipStream_t stream) {
    const QkvSrc<T> src{reinterpret_cast<const T*>(qkv), cos, sin, G, qpk + 2, D, rope_n, tables16};
    return launch_step_src<T>(src, state, o, out_dtype, B, G * qpk, G, D, a, stream);
}

}  // namespace p2dec
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::p2dec;

extern "C" {

int fastmax_hip_p2_decode_step_qkv_supported(int G, int qpk, int D, int rope_n, int in_dtype) {
    return in_dtype >= FASTMAX_F32 && in_dtype <= FASTMAX_F16 && G > 0 && qpk > 0 && qpk <= STEP_SLOTS && D > 0 && D <= 128 &&
           rope_n >= 0 && rope_n <= D && (rope_n & 1) == 0;
}

int fastmax_hip_p2_decode_step_qkv(const void* qkv, const float* cos, const float* sin, float* state, void* o, int B, int G,
                                   int qpk, int D, int rope_n, int tables16, int in_dtype, int out_dtype, float a, void* stream) {
    if (!qkv || !cos || !sin || !state || !o) return FASTMAX_E_NULL;
    if (in_dtype < FASTMAX_F32 || in_dtype > FASTMAX_F16 || out_dtype < FASTMAX_F32 || out_dtype > FASTMAX_F16)
        return FASTMAX_E_BAD_DTYPE;
    if (!fastmax_hip_p2_decode_step_qkv_supported(G, qpk, D, rope_n, in_dtype) || B <= 0 || (int64_t)B * G > 65535 ||
        (int64_t)B * G * qpk > (int64_t)0x7fffffff)
        return FASTMAX_E_BAD_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (in_dtype) {
        case FASTMAX_F32: return launch_step_qkv_t<float>(qkv, cos, sin, state, o, B, G, qpk, D, rope_n, tables16, out_dtype, a, st);
        case FASTMAX_BF16: return launch_step_qkv_t<bf16_t>(qkv, cos, sin, state, o, B, G, qpk, D, rope_n, tables16, out_dtype, a, st);
        default: return launch_step_qkv_t<f16_t>(qkv, cos, sin, state, o, B, G, qpk, D, rope_n, tables16, out_dtype, a, st);
    }
}

}  // extern "C"
