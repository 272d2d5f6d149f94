// The lm-head over the last position only: the three logits entry points.  fastmax_hip_last_logits
// (include/fastmax_hip_next_token.h) takes a dense weight; include/fastmax_hip_head.h adds a dense weight with a bias
// (fastmax_hip_last_logits_bias: the first is this one with no bias) and a weight stored as NF4 codes (the codebook and the
// block scales of nf4_gemv.h), with or without a bias.
//
//   head_logits_kernel   one plan, with the rows of W behind a policy: 256 threads = 4 waves, a wave owns ROWS = 4 rows of W and
//                        up to G rows of x (G = 1, 2, 4, 8: the pass's row count rounded up, the surplus rows re-read the last
//                        one and are not stored).  A row is cut into pieces of E weights; lane l takes pieces l, l + 64, ...: ROWS
//                        pieces of W and G pieces of x (L1 / L2) feed ROWS x G x E fused multiply-adds, W straight to registers
//                        (it is streamed once, no LDS round trip).  Every (b, v) sum has ONE accumulator per lane, filled in
//                        index order from +0, one xor butterfly over the lanes, then (with a bias) one float32 add of the bias:
//                        the bits depend on C, the dtype and the policy only, not on G, the batch, ldx or the load route of x.
//                        The output type and the presence of a bias are template parameters: without a bias the epilogue is
//                        a butterfly and a store.
//       DenseRows        E = 16 bytes of W, as floats, or on the element route the first n elements of a possibly short piece.
//                        tests/golden/last_logits_*.npz pin its bits.
//       Nf4Rows          float32 and float16.  E = 8: one 32-bit word of codes, high nibble first, each looked up in the LDS copy of
//                        the codebook, times the scale of the piece's 64-block (a piece never straddles one: C % 64 == 0), rounded
//                        to T -- the weight nf4_dequantize returns -- and widened back to float.  x is never rounded: it is
//                        multiplied in float32, which the bf16 matrix instruction could not do.  The codes are streamed once
//                        (non-temporal); x comes from L1 / L2.  About five vector instructions decode a weight: the kernel is
//                        bound by the vector ALU, not by HBM (profiles/r19_nf4_head.md).
//   head_logits_bf16_kernel   bfloat16 on NF4 codes: the few-rows product of nf4_gemv.h on the matrix cores, see there.
#include "nf4_gemv.h"
#include "row_kernels.h"
#include "../../include/fastmax_hip_head.h"
#include "../../include/fastmax_hip_next_token.h"

namespace fastmax {
namespace head {

constexpr int ROWS = 4;             // rows of W per wave
constexpr int WAVES = 4;            // waves per workgroup
constexpr int GROUP = 8;            // rows of x per pass over W
constexpr int MAX_C = 1 << 30;      // DenseRows: piece indices stay in int

// E elements of a row as floats: 16-byte loads, or the first n elements one by one (the rest are zeros)
template <typename T, int E, bool VEC>
__device__ __forceinline__ void load_elems(const T* p, int n, float (&f)[E]) {
    if constexpr (VEC) {
        ld_vec<T, E>(p, f);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = e < n ? to_float(p[e]) : 0.f;
    }
}

template <typename T> struct DenseRows {
    static constexpr int E = 16 / sizeof(T);
    static constexpr bool LUT = false;
    const T* w;
    int64_t ldw;
    struct Row { const T* p; };
    __device__ __forceinline__ Row row(int64_t v, int) const { return Row{w + v * ldw}; }
    template <bool VEC>
    __device__ __forceinline__ void piece(const Row& r, int p, int n, const float*, float (&f)[E]) const {
        load_elems<T, E, VEC>(r.p + p * E, n, f);
    }
};

// code * scale rounded to float32, then to T, as a float: the weight the host codec (lora.py) and nf4_dequantize return.  For
// (_Float16)(a * b) hipcc selects v_fma_mixlo_f16, which rounds the EXACT product once: a few weights in a thousand come out one
// fp16 step away from the twice-rounded value.  The empty statement makes the float32 product a value of its own.
template <typename T> __device__ __forceinline__ float nf4_weight(float code, float amax) {
    float prod = code * amax;
    if constexpr (sizeof(T) == 2) asm("" : "+v"(prod));
    return round_to<T>(prod);
}

template <typename T> struct Nf4Rows {
    static constexpr int E = 8;
    static constexpr bool LUT = true;
    const unsigned int* codes;      // a word = 8 weights
    Nf4Scale scale;
    struct Row { const unsigned int* words; int64_t blk; };
    __device__ __forceinline__ Row row(int64_t v, int C) const { return Row{codes + v * (C >> 3), v * (C >> 6)}; }
    template <bool VEC>
    __device__ __forceinline__ void piece(const Row& r, int p, int, const float* lut, float (&f)[E]) const {
        const unsigned int word = __builtin_nontemporal_load(r.words + p);
        const float amax = scale[r.blk + (p >> 3)];
#pragma unroll
        for (int by = 0; by < 4; ++by) {                 // byte `by` of memory: weights 2 by (high nibble) and 2 by + 1
            const unsigned int byte = (word >> (8 * by)) & 0xffu;
            f[2 * by] = nf4_weight<T>(lut[byte >> 4], amax);
            f[2 * by + 1] = nf4_weight<T>(lut[byte & 15u], amax);
        }
    }
};

template <typename T, typename O, bool BIAS, int G, bool VEC, typename W>
__global__ __launch_bounds__(256) void head_logits_kernel(const T* __restrict__ x, int64_t ldx, const W w, const T* __restrict__ bias,
                                                          O* __restrict__ out, int64_t ldo, int nb, int V, int C) {
    constexpr int E = W::E;
    __shared__ float lut[16];
    if constexpr (W::LUT) {
        if (threadIdx.x < 16) lut[threadIdx.x] = kNF4[threadIdx.x];
        __syncthreads();                                  // the only barrier, ahead of every exit
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t v0 = ((int64_t)blockIdx.x * WAVES + wave) * ROWS;
    if (v0 >= V) return;                                  // the whole wave leaves
    typename W::Row wr[ROWS];
    const T* xr[G];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) wr[r] = w.row(v0 + r < V ? v0 + r : (int64_t)V - 1, C);
#pragma unroll
    for (int g = 0; g < G; ++g) xr[g] = x + (int64_t)(g < nb ? g : nb - 1) * ldx;
    float acc[ROWS][G];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[r][g] = 0.f;
    const int npieces = (C + E - 1) / E;
    // more loads in flight where the registers allow it; a second trip of decoded NF4 pieces would cost a wave per SIMD and more
    constexpr int UNROLL = !W::LUT && G <= 2 ? 2 : 1;
#pragma unroll UNROLL
    for (int p = lane; p < npieces; p += 64) {
        const int c = p * E;
        const int n = C - c < E ? C - c : E;
        float wf[ROWS][E];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) w.template piece<VEC>(wr[r], p, n, lut, wf[r]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float xf[E];
            load_elems<T, E, VEC>(xr[g] + c, n, xf);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (VEC || e < n) {
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) acc[r][g] = fmaf(xf[e], wf[r][e], acc[r][g]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float s = wave_sum(acc[r][g]);
            if (lane == 0 && v0 + r < V && g < nb) {
                if constexpr (BIAS) s += to_float(bias[v0 + r]);
                out[(int64_t)g * ldo + v0 + r] = from_float<O>(s);
            }
        }
}

// ---- bfloat16 on NF4 codes: the few-rows product of nf4_gemv.h ------------------------------------------------------------------
// x and the decoded weights are both bfloat16, so the 16x16x32 bf16 matrix instruction multiplies them exactly and adds in
// float32.  A workgroup owns 16 rows of W (the A operand) and up to 16 rows of x (the B operand), as nf4_gemv_kernel does: lane
// (r = lane & 15, q4 = lane >> 4) decodes the 32 weights at 32 q4 of every 128-wide block of row n0 + r (dequant32) and holds the
// same 32 elements of row r of x; wave w takes blocks w, w + 4, ...; the four partial tiles are added in a fixed order.  Unlike
// that kernel's loop (FASTMAX_GEMV_K_LOOP: K % 128 == 0, N % 16 == 0) this one takes C % 64 == 0 -- the last block may be a half
// block, whose lanes q4 >= 2 feed zeros -- and any V: rows past V - 1 re-read row V - 1 and are not stored.  A C column depends
// on its own row of x only, and rows of x past nb re-read row nb - 1 and are not stored.
constexpr int MFMA_ROWS = 16;       // rows of W per workgroup, and rows of x per pass

template <bool VEC> __device__ __forceinline__ bf16x8 load8_bf16(const __bf16* p) {
    if constexpr (VEC) return *reinterpret_cast<const bf16x8*>(p);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = p[i];
    return o;
}

template <bool VEC>
__global__ __launch_bounds__(256) void head_logits_bf16_kernel(const __bf16* __restrict__ x, int64_t ldx, const uint8_t* __restrict__ codes,
                                                               const Nf4Scale scale, const bf16_t* __restrict__ bias,
                                                               void* __restrict__ out, int out_f32, int64_t ldo, int nb, int V, int C) {
    __shared__ float lut[16];
    __shared__ __attribute__((aligned(16))) float part[4][16 * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int n0 = blockIdx.x * MFMA_ROWS;
    if (tid < 16) lut[tid] = kNF4[tid];
    __syncthreads();
    const int64_t row = (int64_t)min(n0 + r, V - 1) * C;          // first weight of this lane's row of W
    const __bf16* xrow = x + (int64_t)min(r, nb - 1) * ldx;
    f32x4 acc = {0, 0, 0, 0};
    // one 128-wide block: `whole` false is a trailing half block, whose lanes q4 >= 2 have no weights and feed zeros
    auto fetch = [&](int j, bool whole, u32x4& pk, float& amax, bf16x8(&xf)[4]) {
        const int k0 = 128 * j + 32 * q4;
        const bool have = whole || k0 < C;
        const int64_t e = row + (have ? k0 : 0);
        pk = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(codes + (e >> 1)));
        amax = scale[e >> 6];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            xf[t] = load8_bf16<VEC>(xrow + (have ? k0 : 0) + 8 * t);
            if (!have) {
#pragma unroll
                for (int i = 0; i < 8; ++i) xf[t][i] = (__bf16)0.0f;
            }
        }
    };
    auto consume = [&](const u32x4& pk, float amax, const bf16x8(&xf)[4]) {
        bf16x8 wf[4];
        dequant32(pk, amax, lut, wf);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], xf[t], acc, 0, 0, 0);
    };
    // two blocks per trip, as FASTMAX_GEMV_K_LOOP: both blocks' codes, scales and x pieces are requested before either is decoded
    const int nfull = C / 128;
    int j = w;
    for (; j + 4 < nfull; j += 8) {
        u32x4 pk0, pk1;
        float a0, a1;
        bf16x8 x0[4], x1[4];
        fetch(j, true, pk0, a0, x0);
        fetch(j + 4, true, pk1, a1, x1);
        consume(pk0, a0, x0);
        consume(pk1, a1, x1);
    }
    if (j < nfull) {
        u32x4 pk0;
        float a0;
        bf16x8 x0[4];
        fetch(j, true, pk0, a0, x0);
        consume(pk0, a0, x0);
    }
    if ((C & 64) && w == (nfull & 3)) {                          // the wave whose turn the half block is, after its whole ones
        u32x4 pk0;
        float a0;
        bf16x8 x0[4];
        fetch(nfull, false, pk0, a0, x0);
        consume(pk0, a0, x0);
    }
    FASTMAX_GEMV_PARK(part, w, q4, r, acc)
    __syncthreads();
    if (w == 0 && r < nb) {
        f32x4 tot;
        FASTMAX_GEMV_TOTAL(part, q4, r, tot)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 4 * q4 + i;
            if (n < V) {
                float s = tot[i];
                if (bias) s += to_float(bias[n]);
                const int64_t at = (int64_t)r * ldo + n;
                if (out_f32) reinterpret_cast<float*>(out)[at] = s;
                else reinterpret_cast<bf16_t*>(out)[at] = from_float<bf16_t>(s);
            }
        }
    }
}

template <typename T, typename O, bool BIAS, int G, typename W>
static void launch_route(bool vec, dim3 grid, hipStream_t st, const T* x, int64_t ldx, const W& w, const T* bias, O* out, int64_t ldo,
                         int nb, int V, int C) {
    if (vec) hipLaunchKernelGGL((head_logits_kernel<T, O, BIAS, G, true, W>), grid, dim3(256), 0, st, x, ldx, w, bias, out, ldo, nb, V, C);
    else hipLaunchKernelGGL((head_logits_kernel<T, O, BIAS, G, false, W>), grid, dim3(256), 0, st, x, ldx, w, bias, out, ldo, nb, V, C);
}

template <typename T, typename O, bool BIAS, typename W>
static int launch_passes(const T* x, int64_t ldx, const W& w, bool vec, const T* bias, O* out, int64_t ldo, int B, int V, int C,
                         hipStream_t st) {
    const int per_block = WAVES * ROWS;
    const dim3 grid((unsigned)(((int64_t)V + per_block - 1) / per_block));
    for (int b0 = 0; b0 < B; b0 += GROUP) {
        const int nb = B - b0 < GROUP ? B - b0 : GROUP;
        const T* xb = x + (int64_t)b0 * ldx;
        O* ob = out + (int64_t)b0 * ldo;
        if (nb == 1) launch_route<T, O, BIAS, 1, W>(vec, grid, st, xb, ldx, w, bias, ob, ldo, nb, V, C);
        else if (nb == 2) launch_route<T, O, BIAS, 2, W>(vec, grid, st, xb, ldx, w, bias, ob, ldo, nb, V, C);
        else if (nb <= 4) launch_route<T, O, BIAS, 4, W>(vec, grid, st, xb, ldx, w, bias, ob, ldo, nb, V, C);
        else launch_route<T, O, BIAS, 8, W>(vec, grid, st, xb, ldx, w, bias, ob, ldo, nb, V, C);
    }
    return (int)hipGetLastError();
}

// `vec`: x (and the rows of a dense W) move as 16-byte loads.  The output type and the presence of a bias choose the instantiation:
// as run-time arguments they cost the dense kernel 4 to 10 % at 8 rows of x (profiles/r20_one_logits_kernel.md).
template <typename T, typename W>
static int launch_head(const void* xv, int64_t ldx, const W& w, bool vec, const void* bias, void* out, int out_f32, int64_t ldo, int B,
                       int V, int C, hipStream_t st) {
    const T* x = reinterpret_cast<const T*>(xv);
    const T* bs = reinterpret_cast<const T*>(bias);
    if (out_f32) {
        float* o = reinterpret_cast<float*>(out);
        return bs ? launch_passes<T, float, true>(x, ldx, w, vec, bs, o, ldo, B, V, C, st)
                  : launch_passes<T, float, false>(x, ldx, w, vec, bs, o, ldo, B, V, C, st);
    }
    T* o = reinterpret_cast<T*>(out);
    return bs ? launch_passes<T, T, true>(x, ldx, w, vec, bs, o, ldo, B, V, C, st)
              : launch_passes<T, T, false>(x, ldx, w, vec, bs, o, ldo, B, V, C, st);
}

template <typename T>
static int dense_head(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int out_f32, int64_t ldo,
                      int B, int V, int C, hipStream_t st) {
    const DenseRows<T> rows{reinterpret_cast<const T*>(w), ldw};
    const bool vec = C % DenseRows<T>::E == 0 && aligned16(x, ldx, sizeof(T)) && aligned16(w, ldw, sizeof(T));
    return launch_head<T>(x, ldx, rows, vec, bias, out, out_f32, ldo, B, V, C, st);
}

template <typename T>
static int nf4_head(const void* x, int64_t ldx, const uint8_t* codes, const fastmax_nf4_scales& s, const void* bias, void* out,
                    int out_f32, int64_t ldo, int B, int V, int C, hipStream_t st) {
    const Nf4Rows<T> rows{reinterpret_cast<const unsigned int*>(codes), Nf4Scale{s.absmax, s.absmax_q, s.absmax2, s.code2, s.offset}};
    return launch_head<T>(x, ldx, rows, aligned16(x, ldx, sizeof(T)), bias, out, out_f32, ldo, B, V, C, st);
}

static int nf4_head_bf16(const void* x, int64_t ldx, const uint8_t* codes, const fastmax_nf4_scales& s, const void* bias, void* out,
                         int out_f32, int64_t ldo, int B, int V, int C, hipStream_t st) {
    const Nf4Scale scale{s.absmax, s.absmax_q, s.absmax2, s.code2, s.offset};
    const __bf16* xs = reinterpret_cast<const __bf16*>(x);
    const bf16_t* bs = reinterpret_cast<const bf16_t*>(bias);
    const bool vec = aligned16(x, ldx, 2);
    const dim3 grid((unsigned)(((int64_t)V + MFMA_ROWS - 1) / MFMA_ROWS));
    for (int b0 = 0; b0 < B; b0 += MFMA_ROWS) {
        const int nb = B - b0 < MFMA_ROWS ? B - b0 : MFMA_ROWS;
        const __bf16* xb = xs + (int64_t)b0 * ldx;
        void* ob = reinterpret_cast<char*>(out) + (int64_t)b0 * ldo * (out_f32 ? 4 : 2);
        if (vec) hipLaunchKernelGGL(head_logits_bf16_kernel<true>, grid, dim3(256), 0, st, xb, ldx, codes, scale, bs, ob, out_f32, ldo, nb, V, C);
        else hipLaunchKernelGGL(head_logits_bf16_kernel<false>, grid, dim3(256), 0, st, xb, ldx, codes, scale, bs, ob, out_f32, ldo, nb, V, C);
    }
    return (int)hipGetLastError();
}

// what the dense and the NF4 entry points check alike
static int check_common(const void* x, int64_t ldx, const void* bias, const void* logits, int64_t ldo, int B, int V, int C, int dtype,
                        int out_dtype, bool shape_ok) {
    if (dtype < 0 || dtype > FASTMAX_F16 || (out_dtype != FASTMAX_F32 && out_dtype != dtype)) return FASTMAX_E_BAD_DTYPE;
    if (B <= 0 || V <= 0 || C <= 0 || ldx < 0 || ldo < V || !shape_ok) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype);
    if (!elem_aligned(x, es) || !elem_aligned(bias, es) || !elem_aligned(logits, elem_size(out_dtype))) return FASTMAX_E_ALIGNMENT;
    return 0;
}

}  // namespace head
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::head;

extern "C" {

int fastmax_hip_last_logits(const void* x, int64_t ldx, const void* w, int64_t ldw, void* logits, int64_t ldo, int B, int V, int C,
                            int dtype, int out_dtype, void* stream) {
    return fastmax_hip_last_logits_bias(x, ldx, w, ldw, nullptr, logits, ldo, B, V, C, dtype, out_dtype, stream);
}

int fastmax_hip_last_logits_bias(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* logits, int64_t ldo,
                                 int B, int V, int C, int dtype, int out_dtype, void* stream) {
    if (!x || !w || !logits) return FASTMAX_E_NULL;
    const int rc = check_common(x, ldx, bias, logits, ldo, B, V, C, dtype, out_dtype, C <= MAX_C && ldw >= C);
    if (rc) return rc;
    if (!elem_aligned(w, elem_size(dtype))) return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int f32 = out_dtype == FASTMAX_F32;
    if (dtype == FASTMAX_F32) return dense_head<float>(x, ldx, w, ldw, bias, logits, f32, ldo, B, V, C, st);
    if (dtype == FASTMAX_BF16) return dense_head<bf16_t>(x, ldx, w, ldw, bias, logits, f32, ldo, B, V, C, st);
    return dense_head<f16_t>(x, ldx, w, ldw, bias, logits, f32, ldo, B, V, C, st);
}

int fastmax_hip_last_logits_nf4(const void* x, int64_t ldx, const uint8_t* codes, const fastmax_nf4_scales* scales, const void* bias,
                                void* logits, int64_t ldo, int B, int V, int C, int dtype, int out_dtype, void* stream) {
    if (!x || !codes || !scales || !logits) return FASTMAX_E_NULL;
    if (scales->absmax_q ? !scales->absmax2 || !scales->code2 : !scales->absmax) return FASTMAX_E_NULL;
    const int rc = check_common(x, ldx, bias, logits, ldo, B, V, C, dtype, out_dtype,
                                C % 64 == 0 && (int64_t)V * C < ((int64_t)1 << 40));
    if (rc) return rc;
    if (!elem_aligned(codes, 16) || (scales->absmax_q ? !elem_aligned(scales->absmax2, 4) || !elem_aligned(scales->code2, 4)
                                                      : !elem_aligned(scales->absmax, 4)))
        return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int f32 = out_dtype == FASTMAX_F32;
    if (dtype == FASTMAX_F32) return nf4_head<float>(x, ldx, codes, *scales, bias, logits, f32, ldo, B, V, C, st);
    if (dtype == FASTMAX_BF16) return nf4_head_bf16(x, ldx, codes, *scales, bias, logits, f32, ldo, B, V, C, st);
    return nf4_head<f16_t>(x, ldx, codes, *scales, bias, logits, f32, ldo, B, V, C, st);
}

}  // extern "C"
