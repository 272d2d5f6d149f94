// The mixture-of-experts MLP around its expert MLPs (lit_gpt/model.py:644-674, LLaMAMoE): top-k routing with the softmax over
// the selected values, the stable dispatch of the (token, expert) pairs to per-expert runs of rows, the gather into those runs,
// the weighted combine, and the backward pass of each.  C ABI and the definitions: include/fastmax_hip_moe.h.
//
// M tokens, E <= 64 experts, k <= 8 per token, S = M k slots.  No atomics anywhere; every sum has a fixed order.
//
// Routing is a counting sort by expert that keeps the tokens in order:
//   route_select_kernel   a THREAD per token, ROUTE_TOK = 256 tokens per workgroup.  k passes of arg-max over the row give the
//                         selection as a 64-bit mask, walked in ascending expert id for the softmax.  Then, expert by expert, a
//                         ballot over the wave: the popcount below the lane is the token's rank among the wave's tokens of that
//                         expert, the whole popcount the wave's count; the four waves' counts meet in LDS.  The workgroup
//                         leaves its histogram and every entry's rank inside the workgroup (parked in slot_of).
//   route_scan_kernel     one wave: thread e walks expert e's column of the histograms in block order and turns it into running
//                         sums; the totals become `offsets`.
//   route_place_kernel    slot = offsets[e] + the histograms' running sum + the rank inside the workgroup.
// Up to ROUTE_TOK tokens there is one histogram, and route_select_kernel<SINGLE> does all three steps itself.
// A slot is therefore a function of the routing alone, whatever ROUTE_TOK is.
//
// The movers work in units of one 16-byte piece (or one element) of one row per thread; combine_backward, which also needs a
// row sum per (token, j), gives a token to a 256-thread workgroup: dy is read once and serves all k of the token's slots.
#include "row_kernels.h"
#include "../../include/fastmax_hip_moe.h"

namespace fastmax {
namespace moe {

constexpr int ROUTE_TOK = 256;                       // tokens per workgroup of the selection (one thread each)
constexpr int MAX_E = FASTMAX_MOE_MAX_EXPERTS;
constexpr int MAX_K = FASTMAX_MOE_MAX_PER_TOKEN;

// torch.topk's order: NaN above every number; equal values do not outrank each other (the lower index, seen first, stays)
__device__ __forceinline__ bool ranks_above(float a, float b) { return a != a ? !(b != b) : a > b; }

struct RouteArgs {
    const void* router;
    int64_t rs;
    int* expert;
    void* prob;
    float* prob32;
    int *offsets, *row_of, *slot_of, *hist;
    int M, E, k;
};

// exclusive scan of tot[0 .. E) into base[0 .. E], by one thread (E <= 64)
__device__ __forceinline__ void scan_totals(const int* tot, int* base, int* offsets, int E) {
    int run = 0;
    for (int e = 0; e < E; ++e) {
        base[e] = run;
        offsets[e] = run;
        run += tot[e];
    }
    base[E] = run;
    offsets[E] = run;
}

template <typename T, bool SINGLE>
__global__ __launch_bounds__(256) void route_select_kernel(RouteArgs p) {
    __shared__ int wcnt[4][MAX_E];                   // per wave and expert: the count, then the count of the waves before it
    __shared__ int tot[MAX_E], base[MAX_E + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * ROUTE_TOK + threadIdx.x;
    const bool live = t < p.M;
    uint64_t sel = 0;
    if (live) {
        const T* r = reinterpret_cast<const T*>(p.router) + t * p.rs;
        for (int j = 0; j < p.k; ++j) {
            int best = -1;
            float bv = 0.f;
            for (int e = 0; e < p.E; ++e) {
                if ((sel >> e) & 1) continue;
                const float v = to_float(r[e]);
                if (best < 0 || ranks_above(v, bv)) {
                    best = e;
                    bv = v;
                }
            }
            sel |= 1ull << best;
        }
        // the selected values in ascending expert id; their softmax in double, rounded once
        int ex[MAX_K];
        double ev[MAX_K];
        float mx = 0.f;
        uint64_t rest = sel;
#pragma unroll
        for (int j = 0; j < MAX_K; ++j) {
            if (j < p.k) {
                ex[j] = __builtin_ctzll(rest);
                rest &= rest - 1;
                const float v = to_float(r[ex[j]]);
                ev[j] = (double)v;
                mx = (j == 0 || ranks_above(v, mx)) ? v : mx;
            }
        }
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < MAX_K; ++j) {
            if (j < p.k) {
                ev[j] = exp(ev[j] - (double)mx);
                sum += ev[j];
            }
        }
#pragma unroll
        for (int j = 0; j < MAX_K; ++j) {
            if (j < p.k) {
                const float pr = (float)(ev[j] / sum);
                p.expert[t * p.k + j] = ex[j];
                p.prob32[t * p.k + j] = pr;
                reinterpret_cast<T*>(p.prob)[t * p.k + j] = from_float<T>(pr);
            }
        }
    }
    // ranks: every thread of the workgroup takes part in every ballot (a thread past M selects nothing)
    int mine_j = 0;
    for (int e = 0; e < p.E; ++e) {
        const bool mine = (sel >> e) & 1;
        const uint64_t votes = __ballot(mine);
        if (mine) p.slot_of[t * p.k + mine_j++] = __popcll(votes & ((1ull << lane) - 1));
        if (lane == 0) wcnt[wave][e] = __popcll(votes);
    }
    __syncthreads();
    if (threadIdx.x < p.E) {
        const int e = threadIdx.x;
        const int c0 = wcnt[0][e], c1 = wcnt[1][e], c2 = wcnt[2][e], c3 = wcnt[3][e];
        wcnt[0][e] = 0;
        wcnt[1][e] = c0;
        wcnt[2][e] = c0 + c1;
        wcnt[3][e] = c0 + c1 + c2;
        if constexpr (SINGLE) tot[e] = c0 + c1 + c2 + c3;
        else p.hist[(int64_t)blockIdx.x * p.E + e] = c0 + c1 + c2 + c3;
    }
    __syncthreads();
    if constexpr (SINGLE) {
        if (threadIdx.x == 0) scan_totals(tot, base, p.offsets, p.E);
        __syncthreads();
    }
    if (!live) return;                               // no barrier below
    uint64_t rest = sel;
    for (int j = 0; j < p.k; ++j) {
        const int e = __builtin_ctzll(rest);
        rest &= rest - 1;
        const int local = p.slot_of[t * p.k + j] + wcnt[wave][e];
        if constexpr (SINGLE) {
            const int slot = base[e] + local;
            p.slot_of[t * p.k + j] = slot;
            p.row_of[slot] = (int)t;
        } else {
            p.slot_of[t * p.k + j] = local;
        }
    }
}

// one wave.  hist[b][e] <- the count of expert e in the blocks before b; offsets <- the exclusive scan of the totals
__global__ __launch_bounds__(64) void route_scan_kernel(RouteArgs p, int nblk) {
    __shared__ int tot[MAX_E], base[MAX_E + 1];
    const int e = threadIdx.x;
    if (e < p.E) {
        int run = 0;
        for (int b = 0; b < nblk; ++b) {
            const int c = p.hist[(int64_t)b * p.E + e];
            p.hist[(int64_t)b * p.E + e] = run;
            run += c;
        }
        tot[e] = run;
    }
    __syncthreads();
    if (e == 0) scan_totals(tot, base, p.offsets, p.E);
}

__global__ __launch_bounds__(256) void route_place_kernel(RouteArgs p) {
    const int64_t t = (int64_t)blockIdx.x * ROUTE_TOK + threadIdx.x;
    if (t >= p.M) return;
    const int* before = p.hist + (int64_t)blockIdx.x * p.E;
    for (int j = 0; j < p.k; ++j) {
        const int e = p.expert[t * p.k + j];
        const int slot = p.offsets[e] + before[e] + p.slot_of[t * p.k + j];
        p.slot_of[t * p.k + j] = slot;
        p.row_of[slot] = (int)t;
    }
}

// d = prob32 (g - sum_j prob32 g) at the selected experts of a row of drouter, zero elsewhere; a thread per token
struct RouteBwdArgs {
    const void* dprob;
    const float* prob32;
    const int* expert;
    void* drouter;
    int64_t ds;
    int M, E, k;
};

template <typename T>
__global__ __launch_bounds__(256) void route_bwd_kernel(RouteBwdArgs p) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.M) return;
    int ex[MAX_K];
    float pr[MAX_K], g[MAX_K];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
        if (j < p.k) {
            ex[j] = p.expert[t * p.k + j];
            pr[j] = p.prob32[t * p.k + j];
            g[j] = to_float(reinterpret_cast<const T*>(p.dprob)[t * p.k + j]);
            dot += pr[j] * g[j];
        }
    }
    T* row = reinterpret_cast<T*>(p.drouter) + t * p.ds;
    for (int e = 0; e < p.E; ++e) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < MAX_K; ++j)
            if (j < p.k && ex[j] == e) d = pr[j] * (g[j] - dot);
        row[e] = from_float<T>(d);
    }
}

// ---- the movers -----------------------------------------------------------------------------------------------------------
// N elements of a row: one 16-byte piece, or one element
template <typename T, bool VEC> struct Unit { static constexpr int N = VEC ? 16 / (int)sizeof(T) : 1; };
template <typename T, bool VEC> __device__ __forceinline__ void ld_unit(const T* p, float (&x)[Unit<T, VEC>::N]) {
    if constexpr (VEC) ld_vec<T, Unit<T, VEC>::N>(p, x);
    else x[0] = to_float(p[0]);
}
template <typename T, bool VEC> __device__ __forceinline__ void st_unit(T* p, const float (&x)[Unit<T, VEC>::N]) {
    if constexpr (VEC) st_vec<T, Unit<T, VEC>::N>(p, x);
    else p[0] = from_float<T>(x[0]);
}

struct MoveArgs {
    const void *src, *prob;
    const int* idx;
    void* dst;
    int64_t ss, ds;
    int rows, k, C;                                  // rows of dst
};

// dst[s] = src[idx[s]], the bits as they are
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gather_kernel(MoveArgs p) {
    constexpr int N = Unit<T, VEC>::N;
    const int upr = p.C / N;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (int64_t)p.rows * upr) return;
    const int64_t s = u / upr;
    const int c = (int)(u - s * upr) * N;
    const T* src = reinterpret_cast<const T*>(p.src) + (int64_t)p.idx[s] * p.ss + c;
    T* dst = reinterpret_cast<T*>(p.dst) + s * p.ds + c;
    if constexpr (VEC) *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
    else *dst = *src;
}

// dst[t] = the token's k slots of src, j ascending:  WEIGHTED  acc = round(acc + round(prob[t][j] src[slot]))   (combine)
//                                                    else      acc += src[slot], rounded once at the end       (gather backward)
template <typename T, bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(256) void slot_sum_kernel(MoveArgs p) {
    constexpr int N = Unit<T, VEC>::N;
    const int upr = p.C / N;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (int64_t)p.rows * upr) return;
    const int64_t t = u / upr;
    const int c = (int)(u - t * upr) * N;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    for (int j = 0; j < p.k; ++j) {
        const int slot = p.idx[t * p.k + j];
        float v[N];
        ld_unit<T, VEC>(reinterpret_cast<const T*>(p.src) + (int64_t)slot * p.ss + c, v);
        if constexpr (WEIGHTED) {
            const float w = to_float(reinterpret_cast<const T*>(p.prob)[t * p.k + j]);
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = round_to<T>(acc[e] + round_to<T>(mul_unfused(w, v[e])));
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] += v[e];
        }
    }
    st_unit<T, VEC>(reinterpret_cast<T*>(p.dst) + t * p.ds + c, acc);
}

struct CombineBwdArgs {
    const void *dy, *ys, *prob;
    const int* slot_of;
    void *dys, *dprob;
    int64_t dy_s, ys_s, dys_s;
    int M, k, C;
};

// a workgroup per token: thread i takes units i, i + 256, ... of the row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void combine_bwd_kernel(CombineBwdArgs p) {
    constexpr int N = Unit<T, VEC>::N;
    __shared__ float red[MAX_K][4];
    const int64_t t = blockIdx.x;
    const int units = p.C / N;
    int slot[MAX_K];
    float w[MAX_K], acc[MAX_K];
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
        acc[j] = 0.f;
        if (j < p.k) {
            slot[j] = p.slot_of[t * p.k + j];
            w[j] = to_float(reinterpret_cast<const T*>(p.prob)[t * p.k + j]);
        }
    }
    const T* dy = reinterpret_cast<const T*>(p.dy) + t * p.dy_s;
    for (int u = threadIdx.x; u < units; u += 256) {
        float g[N];
        ld_unit<T, VEC>(dy + u * N, g);
#pragma unroll
        for (int j = 0; j < MAX_K; ++j) {
            if (j < p.k) {
                float v[N], o[N];
                ld_unit<T, VEC>(reinterpret_cast<const T*>(p.ys) + (int64_t)slot[j] * p.ys_s + u * N, v);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    o[e] = w[j] * g[e];
                    acc[j] += g[e] * v[e];
                }
                st_unit<T, VEC>(reinterpret_cast<T*>(p.dys) + (int64_t)slot[j] * p.dys_s + u * N, o);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
        if (j < p.k) {                               // k is the workgroup's: every thread reaches the barrier inside
            const float s = row_sum<false>(acc[j], red[j]);
            if (threadIdx.x == 0) reinterpret_cast<T*>(p.dprob)[t * p.k + j] = from_float<T>(s);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// reads dtype where it is used
#define MOE_DISPATCH(FN, ...)                                                          \
    do {                                                                               \
        if (dtype == FASTMAX_F32) FN<float>(__VA_ARGS__);                              \
        else if (dtype == FASTMAX_BF16) FN<bf16_t>(__VA_ARGS__);                       \
        else FN<f16_t>(__VA_ARGS__);                                                   \
    } while (0)

static inline int sizes_check(int M, int E, int k, int dtype) {
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (M < 1 || k < 1 || k > MAX_K || E < k || E > MAX_E || (int64_t)M * k > 0x7fffffffLL) return FASTMAX_E_BAD_SHAPE;
    return 0;
}
static inline unsigned token_blocks(int M, int per) { return (unsigned)(((int64_t)M + per - 1) / per); }

// the movers' shared checks over n row operands of C columns; -> the geometry of `rows` rows
static int move_geometry(int n, const void* const* ptrs, const int64_t* strides, int rows, int C, int dtype, bool* vec,
                         unsigned* blocks) {
    if (C < 1) return FASTMAX_E_BAD_SHAPE;
    return elementwise_geometry(n, ptrs, strides, rows, C, dtype, vec, blocks);
}

template <typename T> static void launch_route(const RouteArgs& p, unsigned nblk, hipStream_t st) {
    if (nblk == 1) {
        hipLaunchKernelGGL((route_select_kernel<T, true>), dim3(1), dim3(256), 0, st, p);
        return;
    }
    hipLaunchKernelGGL((route_select_kernel<T, false>), dim3(nblk), dim3(256), 0, st, p);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(64), 0, st, p, (int)nblk);
    hipLaunchKernelGGL(route_place_kernel, dim3(nblk), dim3(256), 0, st, p);
}

template <typename T> static void launch_route_bwd(const RouteBwdArgs& p, hipStream_t st) {
    hipLaunchKernelGGL(route_bwd_kernel<T>, dim3(token_blocks(p.M, 256)), dim3(256), 0, st, p);
}

template <typename T> static void launch_gather(const MoveArgs& p, bool vec, unsigned nb, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((gather_kernel<T, true>), dim3(nb), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gather_kernel<T, false>), dim3(nb), dim3(256), 0, st, p);
}
template <typename T> static void launch_slot_sum(const MoveArgs& p, bool vec, bool weighted, unsigned nb, hipStream_t st) {
    const dim3 grid(nb), blk(256);
    if (vec && weighted) hipLaunchKernelGGL((slot_sum_kernel<T, true, true>), grid, blk, 0, st, p);
    else if (vec) hipLaunchKernelGGL((slot_sum_kernel<T, true, false>), grid, blk, 0, st, p);
    else if (weighted) hipLaunchKernelGGL((slot_sum_kernel<T, false, true>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((slot_sum_kernel<T, false, false>), grid, blk, 0, st, p);
}
template <typename T> static void launch_combine_bwd(const CombineBwdArgs& p, bool vec, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((combine_bwd_kernel<T, true>), dim3((unsigned)p.M), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((combine_bwd_kernel<T, false>), dim3((unsigned)p.M), dim3(256), 0, st, p);
}

// combine and gather backward: dst (M, C) from the k slots of each token of src
static int slot_sum_call(const void* src, int64_t src_stride, const void* prob, const int* slot_of, void* dst, int64_t dst_stride,
                         int M, int k, int C, int dtype, bool weighted, hipStream_t st) {
    if (!src || !slot_of || !dst || (weighted && !prob)) return FASTMAX_E_NULL;
    const int rc = sizes_check(M, k, k, dtype);      // E plays no part here
    if (rc) return rc;
    const int es = elem_size(dtype);
    if (!elem_aligned(slot_of, 4) || (weighted && !elem_aligned(prob, es))) return FASTMAX_E_ALIGNMENT;
    const void* ptrs[2] = {src, dst};
    const int64_t strides[2] = {src_stride, dst_stride};
    bool vec;
    unsigned nb;
    const int gc = move_geometry(2, ptrs, strides, M, C, dtype, &vec, &nb);
    if (gc) return gc;
    MoveArgs p{src, prob, slot_of, dst, src_stride, dst_stride, M, k, C};
    MOE_DISPATCH(launch_slot_sum, p, vec, weighted, nb, st);
    return (int)hipGetLastError();
}

}  // namespace moe
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::moe;

extern "C" {

size_t fastmax_hip_moe_route_workspace(int M, int E) {
    if (M < 1 || E < 1 || E > MAX_E) return 0;
    return (size_t)token_blocks(M, ROUTE_TOK) * (size_t)E * sizeof(int);
}

int fastmax_hip_moe_route(const void* router, int64_t router_stride, int* expert, void* prob, float* prob32, int* offsets,
                          int* row_of, int* slot_of, int M, int E, int k, int dtype, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!router || !expert || !prob || !prob32 || !offsets || !row_of || !slot_of || !workspace) return FASTMAX_E_NULL;
    const int rc = sizes_check(M, E, k, dtype);
    if (rc) return rc;
    if (router_stride < E) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype);
    if (!elem_aligned(router, es) || !elem_aligned(prob, es) || !elem_aligned(expert, 4) || !elem_aligned(prob32, 4) ||
        !elem_aligned(offsets, 4) || !elem_aligned(row_of, 4) || !elem_aligned(slot_of, 4) || !elem_aligned(workspace, 4))
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_moe_route_workspace(M, E)) return FASTMAX_E_WORKSPACE;
    RouteArgs p{router, router_stride, expert, prob, prob32, offsets, row_of, slot_of, reinterpret_cast<int*>(workspace), M, E, k};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MOE_DISPATCH(launch_route, p, token_blocks(M, ROUTE_TOK), st);
    return (int)hipGetLastError();
}

int fastmax_hip_moe_gather(const void* x, int64_t x_stride, const int* row_of, void* xs, int64_t xs_stride, int M, int S, int C,
                           int dtype, void* stream) {
    if (!x || !row_of || !xs) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (M < 1 || S < M || S % M || S / M > MAX_K) return FASTMAX_E_BAD_SHAPE;
    if (!elem_aligned(row_of, 4)) return FASTMAX_E_ALIGNMENT;
    const void* ptrs[2] = {x, xs};
    const int64_t strides[2] = {x_stride, xs_stride};
    bool vec;
    unsigned nb;
    const int gc = move_geometry(2, ptrs, strides, S, C, dtype, &vec, &nb);
    if (gc) return gc;
    MoveArgs p{x, nullptr, row_of, xs, x_stride, xs_stride, S, 0, C};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MOE_DISPATCH(launch_gather, p, vec, nb, st);
    return (int)hipGetLastError();
}

int fastmax_hip_moe_combine(const void* ys, int64_t ys_stride, const void* prob, const int* slot_of, void* y, int64_t y_stride,
                            int M, int k, int C, int dtype, void* stream) {
    return slot_sum_call(ys, ys_stride, prob, slot_of, y, y_stride, M, k, C, dtype, true, reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_moe_combine_backward(const void* dy, int64_t dy_stride, const void* ys, int64_t ys_stride, const void* prob,
                                     const int* slot_of, void* dys, int64_t dys_stride, void* dprob, int M, int k, int C,
                                     int dtype, void* stream) {
    if (!dy || !ys || !prob || !slot_of || !dys || !dprob) return FASTMAX_E_NULL;
    const int rc = sizes_check(M, k, k, dtype);
    if (rc) return rc;
    const int es = elem_size(dtype);
    if (!elem_aligned(slot_of, 4) || !elem_aligned(prob, es) || !elem_aligned(dprob, es)) return FASTMAX_E_ALIGNMENT;
    const void* ptrs[3] = {dy, ys, dys};
    const int64_t strides[3] = {dy_stride, ys_stride, dys_stride};
    bool vec;
    unsigned nb;
    const int gc = move_geometry(3, ptrs, strides, M, C, dtype, &vec, &nb);
    if (gc) return gc;
    CombineBwdArgs p{dy, ys, prob, slot_of, dys, dprob, dy_stride, ys_stride, dys_stride, M, k, C};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MOE_DISPATCH(launch_combine_bwd, p, vec, st);
    return (int)hipGetLastError();
}

int fastmax_hip_moe_gather_backward(const void* dxs, int64_t dxs_stride, const int* slot_of, void* dx, int64_t dx_stride, int M,
                                    int k, int C, int dtype, void* stream) {
    return slot_sum_call(dxs, dxs_stride, nullptr, slot_of, dx, dx_stride, M, k, C, dtype, false,
                         reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_moe_route_backward(const void* dprob, const float* prob32, const int* expert, void* drouter,
                                   int64_t drouter_stride, int M, int E, int k, int dtype, void* stream) {
    if (!dprob || !prob32 || !expert || !drouter) return FASTMAX_E_NULL;
    const int rc = sizes_check(M, E, k, dtype);
    if (rc) return rc;
    if (drouter_stride < E) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype);
    if (!elem_aligned(dprob, es) || !elem_aligned(drouter, es) || !elem_aligned(prob32, 4) || !elem_aligned(expert, 4))
        return FASTMAX_E_ALIGNMENT;
    RouteBwdArgs p{dprob, prob32, expert, drouter, drouter_stride, M, E, k};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MOE_DISPATCH(launch_route_bwd, p, st);
    return (int)hipGetLastError();
}

}  // extern "C"
