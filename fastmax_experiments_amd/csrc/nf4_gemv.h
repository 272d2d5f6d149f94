// What the NF4 kernels share (nf4_lora.hip: the tile kernels and the few-rows kernel of the QLoRA linear; moe_decode.hip: the
// decode-size expert kernels): the codebook, the block scales, the decode of 32 codes, and the few-rows product itself -- the
// K loop of one wave and the fixed-order sum of the four waves' partial tiles.  Private to csrc; each piece is defined here and
// nowhere else, so a row of x gives the same bits through either file.
#pragma once
#include "fastmax_common.h"

namespace fastmax {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// internal linkage: every translation unit that includes this gets its own copy in its own code object
static __constant__ float kNF4[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
                                      -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
                                      0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
                                      0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
                                      0.7229568362236023f, 1.0f};

// Block scales of the NF4 weight: plain (fp32 absmax per 64 weights) or double-quantised ("nf4-dq": the absmax vector is
// itself stored as 8-bit codes of a 256-entry map, one fp32 scale per 256 of them, plus one offset -- QLoRA section 3,
// finetune/lora.py:38 lists the mode).  One scale per 64 weights is decoded where the plain path loads a float.
struct Nf4Scale {
    const float* absmax;      // plain: one per 64 consecutive weights (q == nullptr)
    const uint8_t* q;         // dq: 8-bit code of (absmax - offset) per 64 weights
    const float* absmax2;     // dq: scale per 256 codes
    const float* code2;       // dq: 256-entry map
    float offset;
    __device__ __forceinline__ float operator[](int64_t blk) const {
        return q ? mul_then_add(code2[q[blk]], absmax2[blk >> 8], offset) : absmax[blk];
    }
    // product and sum rounded separately: bit-identical to the host codec (lora.py).  hipcc contracts a * b + c into a
    // fused multiply-add by default, and __fmul_rn / __fadd_rn are plain operators on this target
    static __device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
        const float prod = a * b;
        return prod + c;
    }
};

template <typename T> __device__ __forceinline__ bf16x8 load8_as_bf16(const T* p);
template <> __device__ __forceinline__ bf16x8 load8_as_bf16<__bf16>(const __bf16* p) {
    return *reinterpret_cast<const bf16x8*>(p);
}
template <> __device__ __forceinline__ bf16x8 load8_as_bf16<float>(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = (__bf16)a[i]; o[4 + i] = (__bf16)b[i]; }
    return o;
}

// 16 bytes of packed codes (32 weights, high nibble first) -> 4 x bf16x8, scaled by `amax`
__device__ __forceinline__ void dequant32(const u32x4 pk, float amax, const float* lut, bf16x8 (&out)[4]) {
#pragma unroll
    for (int wd = 0; wd < 4; ++wd) {
        const unsigned int v = pk[wd];
#pragma unroll
        for (int by = 0; by < 4; ++by) {
            const unsigned int byte = (v >> (8 * by)) & 0xffu;
            out[wd][2 * by] = (__bf16)(lut[byte >> 4] * amax);
            out[wd][2 * by + 1] = (__bf16)(lut[byte & 15u] * amax);
        }
    }
}

template <typename T> __device__ __forceinline__ void store4(T* p, const f32x4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void store4<__bf16>(__bf16* p, const f32x4 v) {
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (__bf16)v[i];
    *reinterpret_cast<bf16x4*>(p) = o;
}

// ---- the few-rows product (M <= 16 rows of x, 16 output columns per workgroup, four waves) --------------------------------
// A lane: output column n (the A operand's row lane & 15), the 32 weights at 32 q4 of every 128-wide block of K, and row
// lane & 15 of x (the B operand's column; `mrow` false: zeros).  The C tile a lane ends with: column lane & 15 = the row of x,
// rows 4 q4 + i = the workgroup's output columns 4 q4 + i.  A C column depends on its own row of x only.
//
// The loop and the sum below are TEXT, expanded in the kernel's own body: the few-rows kernel of nf4_lora.hip has to compile to
// the instructions it compiled to before the loop was shared, and a function boundary around it (or around the LDS accesses)
// does not leave the compiler's choices alone.  They use the kernel's names as given: pass plain names, none of those the
// expansion declares itself (nblk, fetch, consume, j, e, pk, amax, pk_b, amax_b, xf, wf, t, i).
//
// acc += x . deq(W)^T over wave w's blocks of K (w, w + 4, ...); with TWO, acc_b += x . deq(W_b)^T from the same pieces of x.
// Two 128-wide blocks per trip: both blocks' codes, scales and x pieces are requested before either is decoded.
#define FASTMAX_GEMV_K_LOOP(T, TWO, wq, absmax, wq_b, absmax_b, xrow, mrow, n, K, w, q4, lut, acc, acc_b)                   \
    {                                                                                                                       \
        const int nblk = K / 128;                                                                                           \
        auto fetch = [&](int j, u32x4& pk, float& amax, u32x4& pk_b, float& amax_b, bf16x8(&xf)[4]) {                       \
            const int64_t e = (int64_t)n * K + 128 * j + 32 * q4; /* first of this lane's 32 weights */                     \
            pk = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wq + (e >> 1)));                                 \
            amax = absmax[e >> 6];                                                                                          \
            if constexpr (TWO) {                                                                                            \
                pk_b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wq_b + (e >> 1)));                         \
                amax_b = absmax_b[e >> 6];                                                                                  \
            }                                                                                                               \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                 \
                if (mrow) xf[t] = load8_as_bf16<T>(xrow + 128 * j + 32 * q4 + 8 * t);                                       \
                else _Pragma("unroll") for (int i = 0; i < 8; ++i) xf[t][i] = (__bf16)0.0f;                                 \
            }                                                                                                               \
        };                                                                                                                  \
        auto consume = [&](const u32x4& pk, float amax, const u32x4& pk_b, float amax_b, const bf16x8(&xf)[4]) {            \
            bf16x8 wf[4];                                                                                                   \
            dequant32(pk, amax, lut, wf);                                                                                   \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], xf[t], acc, 0, 0, 0); \
            if constexpr (TWO) {                                                                                            \
                dequant32(pk_b, amax_b, lut, wf);                                                                           \
                _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                               \
                    acc_b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], xf[t], acc_b, 0, 0, 0);                          \
            }                                                                                                               \
        };                                                                                                                  \
        int j = w;                                                                                                          \
        for (; j + 4 < nblk; j += 8) {                                                                                      \
            u32x4 pk0, pk1, pb0, pb1;                                                                                       \
            float a0, a1, b0, b1;                                                                                           \
            bf16x8 x0[4], x1[4];                                                                                            \
            fetch(j, pk0, a0, pb0, b0, x0);                                                                                 \
            fetch(j + 4, pk1, a1, pb1, b1, x1);                                                                             \
            consume(pk0, a0, pb0, b0, x0);                                                                                  \
            consume(pk1, a1, pb1, b1, x1);                                                                                  \
        }                                                                                                                   \
        if (j < nblk) {                                                                                                     \
            u32x4 pk0, pb0;                                                                                                 \
            float a0, b0;                                                                                                   \
            bf16x8 x0[4];                                                                                                   \
            fetch(j, pk0, a0, pb0, b0, x0);                                                                                 \
            consume(pk0, a0, pb0, b0, x0);                                                                                  \
        }                                                                                                                   \
    }

// a wave's partial tile into its quarter of part (float [4][16 * 16] of LDS): C column (lane & 15) = row of x, rows 4 q4 + i =
// the workgroup's output columns 4 q4 + i; after a barrier the four are added in a fixed order
#define FASTMAX_GEMV_PARK(part, w, q4, r, acc) \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) part[w][(4 * q4 + i) * 16 + r] = acc[i];
#define FASTMAX_GEMV_TOTAL(part, q4, r, tot)                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) tot[i] = (part[0][(4 * q4 + i) * 16 + r] + part[1][(4 * q4 + i) * 16 + r]) + \
                                                           (part[2][(4 * q4 + i) * 16 + r] + part[3][(4 * q4 + i) * 16 + r]);

}  // namespace fastmax
