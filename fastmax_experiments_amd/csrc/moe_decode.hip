// The expert MLPs of the mixture-of-experts layer at decode size (M <= 16 tokens) on device-side row counts.  C ABI and the
// definitions: include/fastmax_hip_moe_decode.h.
//
// moe.hip's route kernel leaves offsets (E + 1) and row_of (S) on the device.  grid = (N / 16, E), block = 256: workgroup
// (c, e) owns 16 output columns of expert e, reads its run offsets[e] .. offsets[e + 1] (at most 16 rows: a token selects an
// expert once), and takes the expert's NF4 operands from a device table -- which weights a workgroup reads is decided by the
// data, so nothing is read back and the layer can be recorded in a graph.  An empty run leaves before any barrier.
//
//   experts_up_kernel    h[s] = round(silu(fc_1(x[row_of[s]]))) * fc_2(x[row_of[s]]): the gather is the x loads, the two
//                        products share them (two accumulators), the activation is gated_act_kernel's (block_neighbours.hip)
//   experts_down_kernel  ys[s] = proj(h[s])
//
// A product is nf4_gemv_kernel's (nf4_lora.hip) through nf4_gemv.h, operation for operation; a C column of the MFMA depends on
// its own row of x only, so a row has the bits the expert's own linear gives it on any run.  Indices read from device memory
// are clamped (the run to 16 rows inside 0 .. S, row_of to 0 .. M - 1): stale offsets give wrong numbers, not a fault.
#include "nf4_gemv.h"
#include "row_kernels.h"
#include "../../include/fastmax_hip_moe_decode.h"

namespace fastmax {
namespace moe_decode {

constexpr int MAX_ROWS = FASTMAX_MOE_DECODE_MAX_ROWS;

struct ExpertsArgs {
    const void* x;                          // up: x (M, C), rows through row_of; down: h (S, I), rows are the slots
    int64_t xs;
    const fastmax_moe_expert_entry* table;
    const int *offsets, *row_of;
    void* y;                                // up: h (S, I); down: ys (S, C)
    int64_t ys;
    int M, S, K;                            // K: the contraction width (up: C, down: I)
};

// the element type of the row kernels for the NF4 kernels' T
template <typename T> struct RowElem { typedef float type; };
template <> struct RowElem<__bf16> { typedef bf16_t type; };

__device__ __forceinline__ Nf4Scale scale_of(const fastmax_nf4_scales& s) {
    return Nf4Scale{s.absmax, s.absmax_q, s.absmax2, s.code2, s.offset};
}

// expert e's run, clamped: first slot and row count (<= 16, inside 0 .. S).  Uniform over the workgroup.
__device__ __forceinline__ int run_of(const int* offsets, int e, int S, int& lo) {
    const int64_t a = offsets[e], b = offsets[e + 1];
    lo = (int)min(max(a, (int64_t)0), (int64_t)S);
    return (int)min(max(b - a, (int64_t)0), (int64_t)min(MAX_ROWS, S - lo));
}

// 4 consecutive values of a row, rounded to U
template <typename U> __device__ __forceinline__ void store4_rounded(U* p, const float (&v)[4]) {
    U o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = from_float<U>(v[i]);
    if constexpr (sizeof(U) == 4) *reinterpret_cast<u32x4*>(p) = *reinterpret_cast<const u32x4*>(o);
    else *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(o);
}

template <typename T>
__global__ __launch_bounds__(256) void experts_up_kernel(ExpertsArgs p) {
    typedef typename RowElem<T>::type U;
    __shared__ float lut[16];
    __shared__ __attribute__((aligned(16))) float part_a[4][16 * 16], part_b[4][16 * 16];
    const int ex = blockIdx.y;
    int lo;
    const int rows = run_of(p.offsets, ex, p.S, lo);
    if (rows <= 0) return;                                       // the whole workgroup, before any barrier
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int K = p.K;
    if (tid < 16) lut[tid] = kNF4[tid];
    __syncthreads();
    const fastmax_moe_expert_entry& en = p.table[ex];
    const uint8_t *wq_a = en.fc_1.wq, *wq_b = en.fc_2.wq;
    const Nf4Scale sc_a = scale_of(en.fc_1.scales), sc_b = scale_of(en.fc_2.scales);
    const int n = n0 + r;
    const bool mrow = r < rows;
    const int t = mrow ? min(max(p.row_of[lo + r], 0), p.M - 1) : 0;
    const T* xrow = reinterpret_cast<const T*>(p.x) + (int64_t)t * p.xs;
    f32x4 acc_a = {0, 0, 0, 0}, acc_b = {0, 0, 0, 0};
    FASTMAX_GEMV_K_LOOP(T, true, wq_a, sc_a, wq_b, sc_b, xrow, mrow, n, K, w, q4, lut, acc_a, acc_b)
    FASTMAX_GEMV_PARK(part_a, w, q4, r, acc_a)
    FASTMAX_GEMV_PARK(part_b, w, q4, r, acc_b)
    __syncthreads();
    if (w == 0) {
        f32x4 ta, tb;
        FASTMAX_GEMV_TOTAL(part_a, q4, r, ta)
        FASTMAX_GEMV_TOTAL(part_b, q4, r, tb)
        if (en.fc_1.bias) ta += *reinterpret_cast<const f32x4*>(en.fc_1.bias + n0 + 4 * q4);
        if (en.fc_2.bias) tb += *reinterpret_cast<const f32x4*>(en.fc_2.bias + n0 + 4 * q4);
        if (mrow) {
            // the linears' stores round a and b to T; then gated_act_kernel: round_to(act(a)) * b, rounded once more on the store
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = (float)(T)ta[i], b = (float)(T)tb[i];
                y[i] = round_to<U>(silu_f(a)) * b;
            }
            store4_rounded<U>(reinterpret_cast<U*>(p.y) + (int64_t)(lo + r) * p.ys + n0 + 4 * q4, y);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void experts_down_kernel(ExpertsArgs p) {
    __shared__ float lut[16];
    __shared__ __attribute__((aligned(16))) float part[4][16 * 16];
    const int ex = blockIdx.y;
    int lo;
    const int rows = run_of(p.offsets, ex, p.S, lo);
    if (rows <= 0) return;                                       // the whole workgroup, before any barrier
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int K = p.K;
    if (tid < 16) lut[tid] = kNF4[tid];
    __syncthreads();
    const fastmax_moe_expert_entry& en = p.table[ex];
    const uint8_t* wq = en.proj.wq;
    const Nf4Scale sc = scale_of(en.proj.scales);
    const int n = n0 + r;
    const bool mrow = r < rows;
    const T* xrow = reinterpret_cast<const T*>(p.x) + (int64_t)(mrow ? lo + r : lo) * p.xs;
    f32x4 acc = {0, 0, 0, 0};
    FASTMAX_GEMV_K_LOOP(T, false, wq, sc, wq, sc, xrow, mrow, n, K, w, q4, lut, acc, acc)
    FASTMAX_GEMV_PARK(part, w, q4, r, acc)
    __syncthreads();
    if (w == 0) {
        f32x4 tot;
        FASTMAX_GEMV_TOTAL(part, q4, r, tot)
        if (en.proj.bias) tot += *reinterpret_cast<const f32x4*>(en.proj.bias + n0 + 4 * q4);
        if (mrow) store4<T>(reinterpret_cast<T*>(p.y) + (int64_t)(lo + r) * p.ys + n0 + 4 * q4, tot);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// in: the rows read (x or h), `in_w` wide; out: the rows written, `out_w` wide
static int experts_check(const void* in, int64_t in_s, int in_w, const void* table, const int* offsets, const int* row_of,
                         bool need_row_of, const void* out, int64_t out_s, int out_w, int M, int E, int k, int C, int I, int dtype) {
    if (!in || !table || !offsets || (need_row_of && !row_of) || !out) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_F32 && dtype != FASTMAX_BF16) return FASTMAX_E_BAD_DTYPE;
    if (M < 1 || M > MAX_ROWS || E < 1 || E > FASTMAX_MOE_MAX_EXPERTS || k < 1 || k > FASTMAX_MOE_MAX_PER_TOKEN || k > E)
        return FASTMAX_E_BAD_SHAPE;
    if (C < 128 || I < 128 || C % 128 || I % 128 || in_s < in_w || out_s < out_w) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype);
    if (!aligned16(in, in_s, es) || !aligned16(out, out_s, es) || !elem_aligned(table, 8) || !elem_aligned(offsets, 4) ||
        (need_row_of && !elem_aligned(row_of, 4)))
        return FASTMAX_E_ALIGNMENT;
    return 0;
}

}  // namespace moe_decode
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::moe_decode;

extern "C" {

size_t fastmax_hip_moe_expert_entry_bytes(void) { return sizeof(fastmax_moe_expert_entry); }

int fastmax_hip_moe_experts_up(const void* x, int64_t x_stride, const fastmax_moe_expert_entry* table, const int* offsets,
                               const int* row_of, void* h, int64_t h_stride, int M, int E, int k, int C, int I, int dtype,
                               void* stream) {
    const int rc = experts_check(x, x_stride, C, table, offsets, row_of, true, h, h_stride, I, M, E, k, C, I, dtype);
    if (rc) return rc;
    ExpertsArgs p{x, x_stride, table, offsets, row_of, h, h_stride, M, M * k, C};
    const dim3 grid((unsigned)(I / 16), (unsigned)E), blk(256);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FASTMAX_BF16) hipLaunchKernelGGL(experts_up_kernel<__bf16>, grid, blk, 0, st, p);
    else hipLaunchKernelGGL(experts_up_kernel<float>, grid, blk, 0, st, p);
    return (int)hipGetLastError();
}

int fastmax_hip_moe_experts_down(const void* h, int64_t h_stride, const fastmax_moe_expert_entry* table, const int* offsets,
                                 void* ys, int64_t ys_stride, int M, int E, int k, int C, int I, int dtype, void* stream) {
    const int rc = experts_check(h, h_stride, I, table, offsets, nullptr, false, ys, ys_stride, C, M, E, k, C, I, dtype);
    if (rc) return rc;
    ExpertsArgs p{h, h_stride, table, offsets, nullptr, ys, ys_stride, M, M * k, I};
    const dim3 grid((unsigned)(C / 16), (unsigned)E), blk(256);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FASTMAX_BF16) hipLaunchKernelGGL(experts_down_kernel<__bf16>, grid, blk, 0, st, p);
    else hipLaunchKernelGGL(experts_down_kernel<float>, grid, blk, 0, st, p);
    return (int)hipGetLastError();
}

}  // extern "C"
