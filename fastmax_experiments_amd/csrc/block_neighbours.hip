// The attention sub-layer's neighbours inside a decoder block (lit_gpt/model.py:340-361, rmsnorm.py:20-31, model.py:622-641):
//   RMSNorm with an optional residual add in front, its backward pass (with the add's backward and a two-kernel, fixed-order
//   dweight), and the gated activation act(a) * b of LLaMAMLP / GemmaMLP with its one-pass backward.
// All of it is memory bound: the point is one read of every operand, 16-byte accesses and no launches in between.
//
// RMSNorm launch shapes (E = 16 / sizeof(T) elements per 16-byte piece, pieces = C / E):
//   pieces <= 64        one WAVE per row, four rows per 256-thread workgroup, one piece per lane
//   pieces <= 256 NP    one workgroup per row, NP = 1, 2, 4 or 8 pieces per thread (thread t owns pieces t, t + 256, ...)
//   anything else       (C not whole pieces, misaligned addresses, pieces > 2048): scalar path, one workgroup per row, the row
//                       is read twice
// On the piece paths the row is read once and stays in registers between the statistics and the scaling.
// Backward: a workgroup walks a fixed block of rows (DW_ROWS when dweight is wanted) and keeps its columns' dweight sums in
// registers; they leave as one row of partials per workgroup, and partial_row_sum_kernel (row_kernels.h, with the helpers and
// reductions both files share) adds the partial rows per column in block order.
#include "row_kernels.h"
#include "../../include/fastmax_hip_block.h"

namespace fastmax {

constexpr int DW_ROWS = 16;          // rows per workgroup of the backward pass when dweight is wanted: fixed, so the sums are too
constexpr int MAX_NP = 8;            // pieces per thread on the one-workgroup-per-row path

struct NormFwd {
    const void *x, *r, *w;
    void *s_out, *y;
    float* rstd;
    int64_t xs, rs, ss, ys;
    int M, C;
    float eps;
    int unit_offset;
};

// Y: the output type -- T when the weight has the activation dtype, float when the weight is float32
template <typename T, typename W, int NP, bool WAVE_ROW>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(NormFwd p) {
    using Y = W;                                           // W is T or float; T * float promotes to float
    constexpr int E = 16 / sizeof(T);
    constexpr int TPR = WAVE_ROW ? 64 : 256;
    __shared__ float red_lds[WAVE_ROW ? 1 : 4];            // the wave-per-row shape sums inside the wave: no LDS traffic
    float* const red = red_lds;
    const int tr = WAVE_ROW ? (threadIdx.x & 63) : threadIdx.x;
    const int64_t row = WAVE_ROW ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (WAVE_ROW && row >= p.M) return;                    // whole waves leave; this mode has no workgroup barrier
    const int pieces = p.C / E;
    const T* x = reinterpret_cast<const T*>(p.x) + row * p.xs;
    const T* r = p.r ? reinterpret_cast<const T*>(p.r) + row * p.rs : nullptr;
    float s[NP][E];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int pc = tr + TPR * j;
        if (pc < pieces) {
            ld_vec<T, E>(x + pc * E, s[j]);
            if (r) {
                float rr[E];
                ld_vec<T, E>(r + pc * E, rr);
#pragma unroll
                for (int e = 0; e < E; ++e) s[j][e] = round_to<T>(s[j][e] + rr[e]);
                st_vec<T, E>(reinterpret_cast<T*>(p.s_out) + row * p.ss + pc * E, s[j]);
            }
#pragma unroll
            for (int e = 0; e < E; ++e) acc += s[j][e] * s[j][e];
        }
    }
    const float total = row_sum<WAVE_ROW>(acc, red);
    const float rstd = 1.0f / sqrtf(total / (float)p.C + p.eps);
    if (tr == 0 && p.rstd) p.rstd[row] = rstd;
    const W* w = reinterpret_cast<const W*>(p.w);
    Y* y = reinterpret_cast<Y*>(p.y) + row * p.ys;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int pc = tr + TPR * j;
        if (pc < pieces) {
            float wv[E], out[E];
            ld_vec<W, E>(w + pc * E, wv);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float wf = p.unit_offset ? round_to<W>(1.0f + wv[e]) : wv[e];
                out[e] = round_to<T>(s[j][e] * rstd) * wf;
            }
            st_vec<Y, E>(y + pc * E, out);
        }
    }
}

// any C >= 1, any alignment: one workgroup per row, element accesses, the row read twice
template <typename T, typename W>
__global__ __launch_bounds__(256) void rmsnorm_fwd_scalar_kernel(NormFwd p) {
    using Y = W;
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const T* x = reinterpret_cast<const T*>(p.x) + row * p.xs;
    const T* r = p.r ? reinterpret_cast<const T*>(p.r) + row * p.rs : nullptr;
    T* so = p.r ? reinterpret_cast<T*>(p.s_out) + row * p.ss : nullptr;
    float acc = 0.f;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float s = to_float(x[c]);
        if (r) {
            s = round_to<T>(s + to_float(r[c]));
            so[c] = from_float<T>(s);
        }
        acc += s * s;
    }
    const float total = row_sum<false>(acc, red);
    const float rstd = 1.0f / sqrtf(total / (float)p.C + p.eps);
    if (threadIdx.x == 0 && p.rstd) p.rstd[row] = rstd;
    const W* w = reinterpret_cast<const W*>(p.w);
    Y* y = reinterpret_cast<Y*>(p.y) + row * p.ys;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float s = to_float(x[c]);
        if (r) s = round_to<T>(s + to_float(r[c]));        // recomputed, not read back from s_out
        const float wv = to_float(w[c]);
        const float wf = p.unit_offset ? round_to<W>(1.0f + wv) : wv;
        y[c] = from_float<Y>(round_to<T>(s * rstd) * wf);
    }
}

struct NormBwd {
    const void *dy, *s, *w, *ds_in;
    const float* rstd;
    void* ds;
    float* part;                 // (row blocks, C) partial dweight sums, or null
    int64_t dys, ss, dis, dss;
    int M, C, rows_per_block, unit_offset;
};

template <typename T, typename W, int NP, bool WAVE_ROW, bool DW>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(NormBwd p) {
    using Y = W;
    constexpr int E = 16 / sizeof(T);
    constexpr int TPR = WAVE_ROW ? 64 : 256;
    __shared__ float red[2][4];
    __shared__ float comb[(WAVE_ROW && DW) ? 4 * 64 * E : 1];
    const int wave = threadIdx.x >> 6;
    const int tr = WAVE_ROW ? (threadIdx.x & 63) : threadIdx.x;
    const int pieces = p.C / E;
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int nrows = (int)min((int64_t)p.rows_per_block, (int64_t)p.M - row0);
    const W* w = reinterpret_cast<const W*>(p.w);
    float dw[DW ? NP : 1][E];
    if constexpr (DW) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) dw[j][e] = 0.f;
    }
    // WAVE_ROW: wave w takes rows w, w + 4, ... of the block; else every thread walks all rows (uniform trip count: barriers inside)
    for (int i = WAVE_ROW ? wave : 0; i < nrows; i += WAVE_ROW ? 4 : 1) {
        const int64_t row = row0 + i;
        const float rstd = p.rstd[row];
        const Y* dy = reinterpret_cast<const Y*>(p.dy) + row * p.dys;
        const T* s = reinterpret_cast<const T*>(p.s) + row * p.ss;
        float g[NP][E], n[NP][E];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pc = tr + TPR * j;
            if (pc < pieces) {
                float wv[E];
                ld_vec<Y, E>(dy + pc * E, g[j]);
                ld_vec<T, E>(s + pc * E, n[j]);
                ld_vec<W, E>(w + pc * E, wv);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float wf = p.unit_offset ? round_to<W>(1.0f + wv[e]) : wv[e];
                    n[j][e] *= rstd;
                    if constexpr (DW) dw[j][e] += g[j][e] * round_to<T>(n[j][e]);
                    g[j][e] *= wf;
                    dot += g[j][e] * n[j][e];
                }
            }
        }
        const float mean = row_sum<WAVE_ROW>(dot, red[i & 1]) / (float)p.C;
        T* ds = reinterpret_cast<T*>(p.ds) + row * p.dss;
        const T* di = p.ds_in ? reinterpret_cast<const T*>(p.ds_in) + row * p.dis : nullptr;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pc = tr + TPR * j;
            if (pc < pieces) {
                float out[E];
#pragma unroll
                for (int e = 0; e < E; ++e) out[e] = mul_unfused(rstd, g[j][e] - n[j][e] * mean);
                if (di) {
                    // the incoming gradient is added to the ROUNDED result, as autograd's accumulation of the two would
#pragma unroll
                    for (int e = 0; e < E; ++e) out[e] = round_to<T>(out[e]);
                    float a[E];
                    ld_vec<T, E>(di + pc * E, a);
#pragma unroll
                    for (int e = 0; e < E; ++e) out[e] += a[e];
                }
                st_vec<T, E>(ds + pc * E, out);
            }
        }
    }
    if constexpr (DW) {
        float* part = p.part + (int64_t)blockIdx.x * p.C;
        if constexpr (WAVE_ROW) {
            // the four waves' sums, added in wave order
            if (tr < pieces) {
#pragma unroll
                for (int e = 0; e < E; ++e) comb[wave * 64 * E + tr * E + e] = dw[0][e];
            }
            __syncthreads();
            for (int c = threadIdx.x; c < p.C; c += 256)
                part[c] = ((comb[c] + comb[64 * E + c]) + comb[2 * 64 * E + c]) + comb[3 * 64 * E + c];
        } else {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int pc = tr + TPR * j;
                if (pc < pieces) st_vec<float, E>(part + pc * E, dw[j]);
            }
        }
    }
}

template <typename T, typename W>
__global__ __launch_bounds__(256) void rmsnorm_bwd_scalar_kernel(NormBwd p) {
    using Y = W;
    __shared__ float red[2][4];
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int nrows = (int)min((int64_t)p.rows_per_block, (int64_t)p.M - row0);
    const W* w = reinterpret_cast<const W*>(p.w);
    float* part = p.part ? p.part + (int64_t)blockIdx.x * p.C : nullptr;
    for (int i = 0; i < nrows; ++i) {
        const int64_t row = row0 + i;
        const float rstd = p.rstd[row];
        const Y* dy = reinterpret_cast<const Y*>(p.dy) + row * p.dys;
        const T* s = reinterpret_cast<const T*>(p.s) + row * p.ss;
        float dot = 0.f;
        for (int c = threadIdx.x; c < p.C; c += 256) {
            const float wv = to_float(w[c]);
            const float wf = p.unit_offset ? round_to<W>(1.0f + wv) : wv;
            const float n = to_float(s[c]) * rstd, d = to_float(dy[c]);
            dot += (d * wf) * n;
            // column c of this block's partial row belongs to this thread alone: a plain running sum in row order
            if (part) part[c] = (i == 0 ? 0.f : part[c]) + d * round_to<T>(n);
        }
        const float mean = row_sum<false>(dot, red[i & 1]) / (float)p.C;
        T* ds = reinterpret_cast<T*>(p.ds) + row * p.dss;
        const T* di = p.ds_in ? reinterpret_cast<const T*>(p.ds_in) + row * p.dis : nullptr;
        for (int c = threadIdx.x; c < p.C; c += 256) {
            const float wv = to_float(w[c]);
            const float wf = p.unit_offset ? round_to<W>(1.0f + wv) : wv;
            const float n = to_float(s[c]) * rstd;
            float out = mul_unfused(rstd, to_float(dy[c]) * wf - n * mean);
            if (di) out = round_to<T>(out) + to_float(di[c]);
            ds[c] = from_float<T>(out);
        }
    }
}

// ---- gated activation ---------------------------------------------------------------------------------------------------
template <int ACT> __device__ __forceinline__ float act_f(float a) {
    if constexpr (ACT == FASTMAX_ACT_SILU) return silu_f(a);
    else return gelu_f(a);
}
template <int ACT> __device__ __forceinline__ float act_prime(float a) {
    if constexpr (ACT == FASTMAX_ACT_SILU) {
        const float sg = 1.0f / (1.0f + expf(-a));
        return sg * (1.0f + a * (1.0f - sg));
    } else {
        return gelu_prime(a);
    }
}

struct GatedArgs {
    const void *a, *b, *dy;
    void *y, *da, *db;
    int64_t as, bs, dys, ys, das, dbs;
    int M, I;
};

// VEC: one 16-byte piece of every operand per thread; else one element per thread.  grid.x covers M * units, 64-bit index
template <typename T, int ACT, bool VEC, bool BWD>
__global__ __launch_bounds__(256) void gated_act_kernel(GatedArgs p) {
    constexpr int E = VEC ? 16 / sizeof(T) : 1;
    const int upr = p.I / E;                                           // units per row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)p.M * upr) return;
    const int64_t row = idx / upr;
    const int col = (int)(idx - row * upr) * E;
    const T* pa = reinterpret_cast<const T*>(p.a) + row * p.as + col;
    const T* pb = reinterpret_cast<const T*>(p.b) + row * p.bs + col;
    float a[E], b[E];
    if constexpr (VEC) {
        ld_vec<T, E>(pa, a);
        ld_vec<T, E>(pb, b);
    } else {
        a[0] = to_float(*pa);
        b[0] = to_float(*pb);
    }
    if constexpr (!BWD) {
        float y[E];
#pragma unroll
        for (int e = 0; e < E; ++e) y[e] = round_to<T>(act_f<ACT>(a[e])) * b[e];
        T* py = reinterpret_cast<T*>(p.y) + row * p.ys + col;
        if constexpr (VEC) st_vec<T, E>(py, y);
        else *py = from_float<T>(y[0]);
    } else {
        const T* pdy = reinterpret_cast<const T*>(p.dy) + row * p.dys + col;
        float dy[E], da[E], db[E];
        if constexpr (VEC) ld_vec<T, E>(pdy, dy);
        else dy[0] = to_float(*pdy);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            da[e] = dy[e] * b[e] * act_prime<ACT>(a[e]);
            db[e] = dy[e] * round_to<T>(act_f<ACT>(a[e]));
        }
        T* pda = reinterpret_cast<T*>(p.da) + row * p.das + col;
        T* pdb = reinterpret_cast<T*>(p.db) + row * p.dbs + col;
        if constexpr (VEC) {
            st_vec<T, E>(pda, da);
            st_vec<T, E>(pdb, db);
        } else {
            *pda = from_float<T>(da[0]);
            *pdb = from_float<T>(db[0]);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <typename T, typename W>
static void launch_norm_fwd(const NormFwd& p, int shape, hipStream_t st) {
    const dim3 rows((unsigned)p.M), quads((unsigned)((p.M + 3) / 4)), blk(256);
    switch (shape) {
        case 0: hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, W, 1, true>), quads, blk, 0, st, p); break;
        case 1: hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, W, 1, false>), rows, blk, 0, st, p); break;
        case 2: hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, W, 2, false>), rows, blk, 0, st, p); break;
        case 4: hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, W, 4, false>), rows, blk, 0, st, p); break;
        case 8: hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, W, 8, false>), rows, blk, 0, st, p); break;
        default: hipLaunchKernelGGL((rmsnorm_fwd_scalar_kernel<T, W>), rows, blk, 0, st, p); break;
    }
}

template <typename T, typename W, bool DW>
static void launch_norm_bwd_dw(const NormBwd& p, int shape, unsigned nblk, hipStream_t st) {
    const dim3 grid(nblk), blk(256);
    switch (shape) {
        case 0: hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, W, 1, true, DW>), grid, blk, 0, st, p); break;
        case 1: hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, W, 1, false, DW>), grid, blk, 0, st, p); break;
        case 2: hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, W, 2, false, DW>), grid, blk, 0, st, p); break;
        case 4: hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, W, 4, false, DW>), grid, blk, 0, st, p); break;
        case 8: hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, W, 8, false, DW>), grid, blk, 0, st, p); break;
        default: hipLaunchKernelGGL((rmsnorm_bwd_scalar_kernel<T, W>), grid, blk, 0, st, p); break;
    }
}
template <typename T, typename W>
static void launch_norm_bwd(const NormBwd& p, int shape, unsigned nblk, hipStream_t st) {
    if (p.part) launch_norm_bwd_dw<T, W, true>(p, shape, nblk, st);
    else launch_norm_bwd_dw<T, W, false>(p, shape, nblk, st);
}

template <typename T, int ACT>
static void launch_gated_act(const GatedArgs& p, bool vec, bool bwd, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), blk(256);
    if (vec && bwd) hipLaunchKernelGGL((gated_act_kernel<T, ACT, true, true>), grid, blk, 0, st, p);
    else if (vec) hipLaunchKernelGGL((gated_act_kernel<T, ACT, true, false>), grid, blk, 0, st, p);
    else if (bwd) hipLaunchKernelGGL((gated_act_kernel<T, ACT, false, true>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((gated_act_kernel<T, ACT, false, false>), grid, blk, 0, st, p);
}

static int gated_act(const GatedArgs& p, bool bwd, int act, int dtype, hipStream_t st) {
    if (!p.a || !p.b || (bwd ? (!p.dy || !p.da || !p.db) : !p.y)) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (p.M <= 0 || p.I <= 0 || (act != FASTMAX_ACT_SILU && act != FASTMAX_ACT_GELU)) return FASTMAX_E_BAD_SHAPE;
    const void* ptrs[5] = {p.a, p.b, bwd ? p.dy : p.y, bwd ? p.da : p.y, bwd ? p.db : p.y};
    const int64_t strides[5] = {p.as, p.bs, bwd ? p.dys : p.ys, bwd ? p.das : p.ys, bwd ? p.dbs : p.ys};
    bool vec;
    unsigned nb;
    const int rc = elementwise_geometry(5, ptrs, strides, p.M, p.I, dtype, &vec, &nb);
    if (rc) return rc;
#define GATED_T(T)                                                                   \
    do {                                                                             \
        if (act == FASTMAX_ACT_SILU) launch_gated_act<T, FASTMAX_ACT_SILU>(p, vec, bwd, nb, st); \
        else launch_gated_act<T, FASTMAX_ACT_GELU>(p, vec, bwd, nb, st);             \
    } while (0)
    if (dtype == FASTMAX_F32) GATED_T(float);
    else if (dtype == FASTMAX_BF16) GATED_T(bf16_t);
    else GATED_T(f16_t);
#undef GATED_T
    return (int)hipGetLastError();
}

}  // namespace fastmax

using namespace fastmax;

extern "C" {

int fastmax_hip_rmsnorm_forward(const void* x, int64_t x_stride, const void* r, int64_t r_stride, const void* weight,
                                void* s_out, int64_t s_stride, void* y, int64_t y_stride, float* rstd, int M, int C, float eps,
                                int add_unit_offset, int dtype, int weight_dtype, void* stream) {
    if (!x || !weight || !y || (r && !s_out)) return FASTMAX_E_NULL;
    const int rc = norm_check(M, C, dtype, weight_dtype);
    if (rc) return rc;
    if (x_stride < C || y_stride < C || (r && (r_stride < C || s_stride < C))) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(x, es) || !elem_aligned(weight, ws) || !elem_aligned(y, ws) || !elem_aligned(rstd, 4) ||
        (r && (!elem_aligned(r, es) || !elem_aligned(s_out, es))))
        return FASTMAX_E_ALIGNMENT;
    int shape = norm_shape(C, dtype, MAX_NP);
    if (!aligned16(x, x_stride, es) || !aligned16(y, y_stride, ws) || !aligned16(weight, 0, ws) ||
        (r && (!aligned16(r, r_stride, es) || !aligned16(s_out, s_stride, es))))
        shape = -1;
    NormFwd p{x, r, weight, s_out, y, rstd, x_stride, r_stride, s_stride, y_stride, M, C, eps, add_unit_offset ? 1 : 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_norm_fwd, p, shape, st);
    return (int)hipGetLastError();
}

size_t fastmax_hip_rmsnorm_backward_workspace(int M, int C, int dtype, int want_dweight) {
    if (!want_dweight || M <= 0 || C <= 0 || dtype < 0 || dtype > FASTMAX_F16) return 0;
    return (size_t)((M + DW_ROWS - 1) / DW_ROWS) * (size_t)C * sizeof(float);
}

int fastmax_hip_rmsnorm_backward(const void* dy, int64_t dy_stride, const void* s, int64_t s_stride, const void* weight,
                                 const float* rstd, const void* ds_in, int64_t ds_in_stride, void* ds, int64_t ds_stride,
                                 float* dweight, int M, int C, int add_unit_offset, int dtype, int weight_dtype,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !s || !weight || !rstd || !ds) return FASTMAX_E_NULL;
    const int rc = norm_check(M, C, dtype, weight_dtype);
    if (rc) return rc;
    if (dy_stride < C || s_stride < C || ds_stride < C || (ds_in && ds_in_stride < C)) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(dy, ws) || !elem_aligned(s, es) || !elem_aligned(weight, ws) || !elem_aligned(rstd, 4) ||
        !elem_aligned(ds, es) || !elem_aligned(ds_in, es) || !elem_aligned(dweight, 4))
        return FASTMAX_E_ALIGNMENT;
    const size_t need = fastmax_hip_rmsnorm_backward_workspace(M, C, dtype, dweight != nullptr);
    if (need) {
        if (!workspace) return FASTMAX_E_NULL;
        if (workspace_bytes < need) return FASTMAX_E_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return FASTMAX_E_ALIGNMENT;
    }
    int shape = norm_shape(C, dtype, MAX_NP);
    if (!aligned16(dy, dy_stride, ws) || !aligned16(s, s_stride, es) || !aligned16(weight, 0, ws) ||
        !aligned16(ds, ds_stride, es) || (ds_in && !aligned16(ds_in, ds_in_stride, es)))
        shape = -1;
    // dweight wanted: DW_ROWS rows per workgroup whatever the path, so the partial rows are the query function's; else one
    // row per workgroup (four on the wave-per-row path)
    const int rpb = dweight ? DW_ROWS : (shape == 0 ? 4 : 1);
    const unsigned nblk = (unsigned)(((int64_t)M + rpb - 1) / rpb);
    NormBwd p{dy, s, weight, ds_in, rstd, ds, dweight ? reinterpret_cast<float*>(workspace) : nullptr,
              dy_stride, s_stride, ds_in_stride, ds_stride, M, C, rpb, add_unit_offset ? 1 : 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_norm_bwd, p, shape, nblk, st);
    int err = (int)hipGetLastError();
    if (err || !dweight) return err;
    launch_partial_row_sum<1>(p.part, {{dweight}}, (int)nblk, C, st);
    return (int)hipGetLastError();
}

int fastmax_hip_gated_act_forward(const void* a, int64_t a_stride, const void* b, int64_t b_stride, void* y, int64_t y_stride,
                                  int M, int I, int act, int dtype, void* stream) {
    GatedArgs p{a, b, nullptr, y, nullptr, nullptr, a_stride, b_stride, 0, y_stride, 0, 0, M, I};
    return gated_act(p, false, act, dtype, reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_gated_act_backward(const void* a, int64_t a_stride, const void* b, int64_t b_stride, const void* dy,
                                   int64_t dy_stride, void* da, int64_t da_stride, void* db, int64_t db_stride, int M, int I,
                                   int act, int dtype, void* stream) {
    GatedArgs p{a, b, dy, nullptr, da, db, a_stride, b_stride, dy_stride, 0, da_stride, db_stride, M, I};
    return gated_act(p, true, act, dtype, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
