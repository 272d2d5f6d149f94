// The attention sub-layer's neighbours inside a GPT-NeoX (pythia) decoder block (lit_gpt/model.py:340-361 with
// parallel_residual, torch.nn.LayerNorm, model.py:608-619):
//   LayerNorm as a pair over one row -- norm_1(x) and norm_2(x) normalise the same row with the same eps, so mean and rstd are
//   computed once -- with the three-way residual add  s = mlp + h + x  of the hand-over between two blocks in front of it, its
//   backward pass (ds in one pass, the four parameter gradients as two-kernel fixed-order sums), and the ungated exact GELU of
//   GptNeoxMLP with its one-pass backward.
// All of it is memory bound: one read of every operand, 16-byte accesses, no launches in between.
//
// LayerNorm launch shapes (E = 16 / sizeof(T) elements per 16-byte piece, pieces = C / E):
//   pieces <= 64        one WAVE per row, four rows per 256-thread workgroup, one piece per lane
//   pieces <= 256 NP    one workgroup per row, NP = 1, 2 or 4 pieces per thread (thread t owns pieces t, t + 256, ...)
//   anything else       (C not whole pieces, misaligned addresses, pieces > 1024): scalar path, one workgroup per row, the row
//                       is read three times
// On the piece paths the row is read once and stays in registers: the mean, then the deviations from it, then the scaling.
// Backward: a workgroup walks a fixed block of rows (PG_ROWS when a parameter gradient is wanted) and keeps its columns' sums in
// registers; they leave as NS rows of partials per workgroup (dw1, db1[, dw2, db2]), and partial_row_sum_kernel (row_kernels.h,
// with the helpers and reductions both files share) adds the partial rows per column in block order.
#include "row_kernels.h"
#include "../../include/fastmax_hip_neox.h"

namespace fastmax {
namespace neox {

constexpr int PG_ROWS = 16;          // rows per workgroup of the backward pass when parameter gradients are wanted: fixed, so the sums are too
constexpr int MAX_NP = 4;            // pieces per thread on the one-workgroup-per-row path

// the residual stream: x, round(x + r1), or round(round(r1 + r2) + x) -- the block's mlp + h + x, left to right
template <typename T> __device__ __forceinline__ float stream_sum(float x, float r1, float r2, bool has1, bool has2) {
    if (!has1) return x;
    if (!has2) return round_to<T>(x + r1);
    return round_to<T>(round_to<T>(r1 + r2) + x);
}

struct LnFwd {
    const void *x, *r1, *r2, *w1, *b1, *w2, *b2;
    void *s_out, *y1, *y2;
    float *mean, *rstd;
    int64_t xs, r1s, r2s, ss, y1s, y2s;
    int M, C;
    float eps;
};

template <typename T, typename W, int NP, bool WAVE_ROW>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(LnFwd p) {
    constexpr int E = 16 / sizeof(T);
    constexpr int TPR = WAVE_ROW ? 64 : 256;
    __shared__ float red[2][4];                            // the wave-per-row shape sums inside the wave: no LDS traffic
    const int tr = WAVE_ROW ? (threadIdx.x & 63) : threadIdx.x;
    const int64_t row = WAVE_ROW ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (WAVE_ROW && row >= p.M) return;                    // whole waves leave; this mode has no workgroup barrier
    const int pieces = p.C / E;
    const T* x = reinterpret_cast<const T*>(p.x) + row * p.xs;
    const T* r1 = p.r1 ? reinterpret_cast<const T*>(p.r1) + row * p.r1s : nullptr;
    const T* r2 = p.r2 ? reinterpret_cast<const T*>(p.r2) + row * p.r2s : nullptr;
    float s[NP][E];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int pc = tr + TPR * j;
        if (pc < pieces) {
            ld_vec<T, E>(x + pc * E, s[j]);
            if (r1) {
                float a[E], b[E];
                ld_vec<T, E>(r1 + pc * E, a);
                if (r2) ld_vec<T, E>(r2 + pc * E, b);
#pragma unroll
                for (int e = 0; e < E; ++e) s[j][e] = stream_sum<T>(s[j][e], a[e], r2 ? b[e] : 0.f, true, r2 != nullptr);
                st_vec<T, E>(reinterpret_cast<T*>(p.s_out) + row * p.ss + pc * E, s[j]);
            }
#pragma unroll
            for (int e = 0; e < E; ++e) acc += s[j][e];
        }
    }
    const float mean = row_sum<WAVE_ROW>(acc, red[0]) / (float)p.C;
    acc = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if (tr + TPR * j < pieces) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float d = s[j][e] - mean;
                acc += d * d;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(row_sum<WAVE_ROW>(acc, red[1]) / (float)p.C + p.eps);
    if (tr == 0) {
        if (p.mean) p.mean[row] = mean;
        if (p.rstd) p.rstd[row] = rstd;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const W* w = reinterpret_cast<const W*>(k ? p.w2 : p.w1);
        const W* b = reinterpret_cast<const W*>(k ? p.b2 : p.b1);
        if (!w) break;                                     // a single norm: w2 is null
        T* y = reinterpret_cast<T*>(k ? p.y2 : p.y1) + row * (k ? p.y2s : p.y1s);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pc = tr + TPR * j;
            if (pc < pieces) {
                float wv[E], bv[E], out[E];
                ld_vec<W, E>(w + pc * E, wv);
                if (b) ld_vec<W, E>(b + pc * E, bv);
#pragma unroll
                for (int e = 0; e < E; ++e) out[e] = (s[j][e] - mean) * rstd * wv[e] + (b ? bv[e] : 0.f);
                st_vec<T, E>(y + pc * E, out);
            }
        }
    }
}

// any C >= 1, any alignment: one workgroup per row, element accesses, the row read three times
template <typename T, typename W>
__global__ __launch_bounds__(256) void layernorm_fwd_scalar_kernel(LnFwd p) {
    __shared__ float red[2][4];
    const int64_t row = blockIdx.x;
    const T* x = reinterpret_cast<const T*>(p.x) + row * p.xs;
    const T* r1 = p.r1 ? reinterpret_cast<const T*>(p.r1) + row * p.r1s : nullptr;
    const T* r2 = p.r2 ? reinterpret_cast<const T*>(p.r2) + row * p.r2s : nullptr;
    T* so = p.r1 ? reinterpret_cast<T*>(p.s_out) + row * p.ss : nullptr;
    // recomputed on every pass, not read back from s_out
    auto s_at = [&](int c) {
        return stream_sum<T>(to_float(x[c]), r1 ? to_float(r1[c]) : 0.f, r2 ? to_float(r2[c]) : 0.f, r1 != nullptr, r2 != nullptr);
    };
    float acc = 0.f;
    for (int c = threadIdx.x; c < p.C; c += 256) acc += s_at(c);
    const float mean = row_sum<false>(acc, red[0]) / (float)p.C;
    acc = 0.f;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        const float d = s_at(c) - mean;
        acc += d * d;
    }
    const float rstd = 1.0f / sqrtf(row_sum<false>(acc, red[1]) / (float)p.C + p.eps);
    if (threadIdx.x == 0) {
        if (p.mean) p.mean[row] = mean;
        if (p.rstd) p.rstd[row] = rstd;
    }
    const W* w1 = reinterpret_cast<const W*>(p.w1);
    const W* b1 = reinterpret_cast<const W*>(p.b1);
    const W* w2 = reinterpret_cast<const W*>(p.w2);
    const W* b2 = reinterpret_cast<const W*>(p.b2);
    T* y1 = reinterpret_cast<T*>(p.y1) + row * p.y1s;
    T* y2 = w2 ? reinterpret_cast<T*>(p.y2) + row * p.y2s : nullptr;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        const float s = s_at(c);
        const float n = (s - mean) * rstd;
        y1[c] = from_float<T>(n * to_float(w1[c]) + (b1 ? to_float(b1[c]) : 0.f));
        if (w2) y2[c] = from_float<T>(n * to_float(w2[c]) + (b2 ? to_float(b2[c]) : 0.f));
        if (so) so[c] = from_float<T>(s);                  // after this thread's last read of x[c], r1[c], r2[c]
    }
}

struct LnBwd {
    const void *dy1, *dy2, *s, *w1, *w2, *ds_in;
    const float *mean, *rstd;
    void* ds;
    float* part;                 // (row blocks, ns, C) partial sums dw1, db1[, dw2, db2], or null
    int64_t dy1s, dy2s, ss, dis, dss;
    int M, C, rows_per_block, ns;
};

// NS: rows of partial sums a workgroup leaves -- 0: no parameter gradient is wanted (one norm or two: dy2 decides), 2: one norm
// (dw1, db1), 4: the pair (dw1, db1, dw2, db2)
template <typename T, typename W, int NP, bool WAVE_ROW, int NS>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(LnBwd p) {
    // arithmetic exactly as written: which products the compiler would contract into fused multiply-adds differs between the
    // instantiations, and ds must not depend on whether parameter gradients were asked for
#pragma clang fp contract(off)
    constexpr int E = 16 / sizeof(T);
    constexpr int TPR = WAVE_ROW ? 64 : 256;
    constexpr bool PG = NS > 0;
    __shared__ float red[2][2][4];
    __shared__ float comb[(WAVE_ROW && PG) ? NS * 4 * 64 * E : 1];
    const int wave = threadIdx.x >> 6;
    const int tr = WAVE_ROW ? (threadIdx.x & 63) : threadIdx.x;
    const int pieces = p.C / E;
    const bool pair = NS == 4 || (NS == 0 && p.dy2 != nullptr);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int nrows = (int)min((int64_t)p.rows_per_block, (int64_t)p.M - row0);
    const W* w1 = reinterpret_cast<const W*>(p.w1);
    const W* w2 = reinterpret_cast<const W*>(p.w2);
    float pg[PG ? NS : 1][NP][E];
    if constexpr (PG) {
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int j = 0; j < NP; ++j)
#pragma unroll
                for (int e = 0; e < E; ++e) pg[k][j][e] = 0.f;
    }
    // WAVE_ROW: wave w takes rows w, w + 4, ... of the block; else every thread walks all rows (uniform trip count: barriers inside)
    for (int i = WAVE_ROW ? wave : 0; i < nrows; i += WAVE_ROW ? 4 : 1) {
        const int64_t row = row0 + i;
        const float mean = p.mean[row], rstd = p.rstd[row];
        const T* dy1 = reinterpret_cast<const T*>(p.dy1) + row * p.dy1s;
        const T* dy2 = pair ? reinterpret_cast<const T*>(p.dy2) + row * p.dy2s : nullptr;
        const T* s = reinterpret_cast<const T*>(p.s) + row * p.ss;
        float g[NP][E], n[NP][E];
        float sg = 0.f, sgn = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pc = tr + TPR * j;
            if (pc < pieces) {
                float d[E], wv[E];
                ld_vec<T, E>(s + pc * E, n[j]);
                ld_vec<T, E>(dy1 + pc * E, d);
                ld_vec<W, E>(w1 + pc * E, wv);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    n[j][e] = (n[j][e] - mean) * rstd;
                    g[j][e] = wv[e] * d[e];
                    if constexpr (PG) {
                        pg[0][j][e] += d[e] * n[j][e];
                        pg[1][j][e] += d[e];
                    }
                }
                if (pair) {
                    ld_vec<T, E>(dy2 + pc * E, d);
                    ld_vec<W, E>(w2 + pc * E, wv);
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        g[j][e] += wv[e] * d[e];
                        if constexpr (NS == 4) {
                            pg[2][j][e] += d[e] * n[j][e];
                            pg[3][j][e] += d[e];
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    sg += g[j][e];
                    sgn += g[j][e] * n[j][e];
                }
            }
        }
        row_sum2<WAVE_ROW>(sg, sgn, red[i & 1]);
        const float mg = sg / (float)p.C, mgn = sgn / (float)p.C;
        T* ds = reinterpret_cast<T*>(p.ds) + row * p.dss;
        const T* di = p.ds_in ? reinterpret_cast<const T*>(p.ds_in) + row * p.dis : nullptr;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pc = tr + TPR * j;
            if (pc < pieces) {
                float out[E];
#pragma unroll
                for (int e = 0; e < E; ++e) out[e] = mul_unfused(rstd, (g[j][e] - mg) - n[j][e] * mgn);
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
    if constexpr (PG) {
        float* part = p.part + (int64_t)blockIdx.x * NS * p.C;
        if constexpr (WAVE_ROW) {
            // the four waves' sums, added in wave order
            if (tr < pieces) {
#pragma unroll
                for (int k = 0; k < NS; ++k)
#pragma unroll
                    for (int e = 0; e < E; ++e) comb[(k * 4 + wave) * 64 * E + tr * E + e] = pg[k][0][e];
            }
            __syncthreads();
            for (int k = 0; k < NS; ++k) {
                const float* cb = comb + k * 4 * 64 * E;
                for (int c = threadIdx.x; c < p.C; c += 256)
                    part[(int64_t)k * p.C + c] = ((cb[c] + cb[64 * E + c]) + cb[2 * 64 * E + c]) + cb[3 * 64 * E + c];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const int pc = tr + TPR * j;
                    if (pc < pieces) st_vec<float, E>(part + (int64_t)k * p.C + pc * E, pg[k][j]);
                }
        }
    }
}

template <typename T, typename W>
__global__ __launch_bounds__(256) void layernorm_bwd_scalar_kernel(LnBwd p) {
#pragma clang fp contract(off)
    __shared__ float red[2][2][4];
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int nrows = (int)min((int64_t)p.rows_per_block, (int64_t)p.M - row0);
    const bool pair = p.dy2 != nullptr;
    const W* w1 = reinterpret_cast<const W*>(p.w1);
    const W* w2 = reinterpret_cast<const W*>(p.w2);
    float* part = p.part ? p.part + (int64_t)blockIdx.x * p.ns * p.C : nullptr;
    for (int i = 0; i < nrows; ++i) {
        const int64_t row = row0 + i;
        const float mean = p.mean[row], rstd = p.rstd[row];
        const T* dy1 = reinterpret_cast<const T*>(p.dy1) + row * p.dy1s;
        const T* dy2 = pair ? reinterpret_cast<const T*>(p.dy2) + row * p.dy2s : nullptr;
        const T* s = reinterpret_cast<const T*>(p.s) + row * p.ss;
        float sg = 0.f, sgn = 0.f;
        for (int c = threadIdx.x; c < p.C; c += 256) {
            const float n = (to_float(s[c]) - mean) * rstd, d1 = to_float(dy1[c]);
            float g = to_float(w1[c]) * d1;
            // column c of this block's partial rows belongs to this thread alone: plain running sums in row order
            if (part) {
                part[c] = (i == 0 ? 0.f : part[c]) + d1 * n;
                part[(int64_t)p.C + c] = (i == 0 ? 0.f : part[(int64_t)p.C + c]) + d1;
            }
            if (pair) {
                const float d2 = to_float(dy2[c]);
                g += to_float(w2[c]) * d2;
                if (part && p.ns == 4) {
                    part[2 * (int64_t)p.C + c] = (i == 0 ? 0.f : part[2 * (int64_t)p.C + c]) + d2 * n;
                    part[3 * (int64_t)p.C + c] = (i == 0 ? 0.f : part[3 * (int64_t)p.C + c]) + d2;
                }
            }
            sg += g;
            sgn += g * n;
        }
        row_sum2<false>(sg, sgn, red[i & 1]);
        const float mg = sg / (float)p.C, mgn = sgn / (float)p.C;
        T* ds = reinterpret_cast<T*>(p.ds) + row * p.dss;
        const T* di = p.ds_in ? reinterpret_cast<const T*>(p.ds_in) + row * p.dis : nullptr;
        for (int c = threadIdx.x; c < p.C; c += 256) {
            const float n = (to_float(s[c]) - mean) * rstd;
            float g = to_float(w1[c]) * to_float(dy1[c]);
            if (pair) g += to_float(w2[c]) * to_float(dy2[c]);
            float out = mul_unfused(rstd, (g - mg) - n * mgn);
            if (di) out = round_to<T>(out) + to_float(di[c]);
            ds[c] = from_float<T>(out);
        }
    }
}

// ---- ungated activation -------------------------------------------------------------------------------------------------
struct ActArgs {
    const void *a, *dy;
    void* out;                   // y (forward) or da (backward)
    int64_t as, dys, os;
    int M, I;
};

// VEC: one 16-byte piece of every operand per thread; else one element per thread.  grid.x covers M * units, 64-bit index
template <typename T, bool VEC, bool BWD>
__global__ __launch_bounds__(256) void act_kernel(ActArgs p) {
    constexpr int E = VEC ? 16 / sizeof(T) : 1;
    const int upr = p.I / E;                                           // units per row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)p.M * upr) return;
    const int64_t row = idx / upr;
    const int col = (int)(idx - row * upr) * E;
    const T* pa = reinterpret_cast<const T*>(p.a) + row * p.as + col;
    T* po = reinterpret_cast<T*>(p.out) + row * p.os + col;
    float a[E], out[E];
    if constexpr (VEC) ld_vec<T, E>(pa, a);
    else a[0] = to_float(*pa);
    if constexpr (!BWD) {
#pragma unroll
        for (int e = 0; e < E; ++e) out[e] = gelu_f(a[e]);
    } else {
        const T* pdy = reinterpret_cast<const T*>(p.dy) + row * p.dys + col;
        float dy[E];
        if constexpr (VEC) ld_vec<T, E>(pdy, dy);
        else dy[0] = to_float(*pdy);
#pragma unroll
        for (int e = 0; e < E; ++e) out[e] = dy[e] * gelu_prime(a[e]);
    }
    if constexpr (VEC) st_vec<T, E>(po, out);
    else *po = from_float<T>(out[0]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <typename T, typename W>
static void launch_ln_fwd(const LnFwd& p, int shape, hipStream_t st) {
    const dim3 rows((unsigned)p.M), quads((unsigned)((p.M + 3) / 4)), blk(256);
    switch (shape) {
        case 0: hipLaunchKernelGGL((layernorm_fwd_kernel<T, W, 1, true>), quads, blk, 0, st, p); break;
        case 1: hipLaunchKernelGGL((layernorm_fwd_kernel<T, W, 1, false>), rows, blk, 0, st, p); break;
        case 2: hipLaunchKernelGGL((layernorm_fwd_kernel<T, W, 2, false>), rows, blk, 0, st, p); break;
        case 4: hipLaunchKernelGGL((layernorm_fwd_kernel<T, W, 4, false>), rows, blk, 0, st, p); break;
        default: hipLaunchKernelGGL((layernorm_fwd_scalar_kernel<T, W>), rows, blk, 0, st, p); break;
    }
}

template <typename T, typename W, int NS>
static void launch_ln_bwd_ns(const LnBwd& p, int shape, unsigned nblk, hipStream_t st) {
    const dim3 grid(nblk), blk(256);
    switch (shape) {
        case 0: hipLaunchKernelGGL((layernorm_bwd_kernel<T, W, 1, true, NS>), grid, blk, 0, st, p); break;
        case 1: hipLaunchKernelGGL((layernorm_bwd_kernel<T, W, 1, false, NS>), grid, blk, 0, st, p); break;
        case 2: hipLaunchKernelGGL((layernorm_bwd_kernel<T, W, 2, false, NS>), grid, blk, 0, st, p); break;
        case 4: hipLaunchKernelGGL((layernorm_bwd_kernel<T, W, 4, false, NS>), grid, blk, 0, st, p); break;
        default: hipLaunchKernelGGL((layernorm_bwd_scalar_kernel<T, W>), grid, blk, 0, st, p); break;
    }
}
template <typename T, typename W>
static void launch_ln_bwd(const LnBwd& p, int shape, unsigned nblk, hipStream_t st) {
    if (p.ns == 4) launch_ln_bwd_ns<T, W, 4>(p, shape, nblk, st);
    else if (p.ns == 2) launch_ln_bwd_ns<T, W, 2>(p, shape, nblk, st);
    else launch_ln_bwd_ns<T, W, 0>(p, shape, nblk, st);
}

template <typename T>
static void launch_act(const ActArgs& p, bool vec, bool bwd, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), blk(256);
    if (vec && bwd) hipLaunchKernelGGL((act_kernel<T, true, true>), grid, blk, 0, st, p);
    else if (vec) hipLaunchKernelGGL((act_kernel<T, true, false>), grid, blk, 0, st, p);
    else if (bwd) hipLaunchKernelGGL((act_kernel<T, false, true>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((act_kernel<T, false, false>), grid, blk, 0, st, p);
}

static int act_call(const ActArgs& p, bool bwd, int act, int dtype, hipStream_t st) {
    if (!p.a || !p.out || (bwd && !p.dy)) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (p.M <= 0 || p.I <= 0 || act != FASTMAX_NEOX_ACT_GELU) return FASTMAX_E_BAD_SHAPE;
    const void* ptrs[3] = {p.a, p.out, bwd ? p.dy : p.a};
    const int64_t strides[3] = {p.as, p.os, bwd ? p.dys : p.as};
    bool vec;
    unsigned nb;
    const int rc = elementwise_geometry(3, ptrs, strides, p.M, p.I, dtype, &vec, &nb);
    if (rc) return rc;
    if (dtype == FASTMAX_F32) launch_act<float>(p, vec, bwd, nb, st);
    else if (dtype == FASTMAX_BF16) launch_act<bf16_t>(p, vec, bwd, nb, st);
    else launch_act<f16_t>(p, vec, bwd, nb, st);
    return (int)hipGetLastError();
}

}  // namespace neox
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::neox;

extern "C" {

int fastmax_hip_layernorm_forward(const void* x, int64_t x_stride, const void* r1, int64_t r1_stride, const void* r2,
                                  int64_t r2_stride, const void* w1, const void* b1, const void* w2, const void* b2,
                                  void* s_out, int64_t s_stride, void* y1, int64_t y1_stride, void* y2, int64_t y2_stride,
                                  float* mean, float* rstd, int M, int C, float eps, int dtype, int weight_dtype, void* stream) {
    if (!x || !w1 || !y1 || (r2 && !r1) || (r1 && !s_out) || (w2 && !y2) || (b2 && !w2)) return FASTMAX_E_NULL;
    const int rc = norm_check(M, C, dtype, weight_dtype);
    if (rc) return rc;
    if (x_stride < C || y1_stride < C || (r1 && (r1_stride < C || s_stride < C)) || (r2 && r2_stride < C) || (w2 && y2_stride < C))
        return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(x, es) || !elem_aligned(y1, es) || !elem_aligned(w1, ws) || !elem_aligned(b1, ws) || !elem_aligned(w2, ws) ||
        !elem_aligned(b2, ws) || !elem_aligned(mean, 4) || !elem_aligned(rstd, 4) || !elem_aligned(r1, es) ||
        !elem_aligned(r2, es) || (r1 && !elem_aligned(s_out, es)) || (w2 && !elem_aligned(y2, es)))
        return FASTMAX_E_ALIGNMENT;
    int shape = norm_shape(C, dtype, MAX_NP);
    if (!aligned16(x, x_stride, es) || !aligned16(y1, y1_stride, es) || !aligned16(w1, 0, ws) || !aligned16(b1, 0, ws) ||
        !aligned16(w2, 0, ws) || !aligned16(b2, 0, ws) || (r1 && (!aligned16(r1, r1_stride, es) || !aligned16(s_out, s_stride, es))) ||
        (r2 && !aligned16(r2, r2_stride, es)) || (w2 && !aligned16(y2, y2_stride, es)))
        shape = -1;
    LnFwd p{x, r1, r2, w1, b1, w2, w2 ? b2 : nullptr, r1 ? s_out : nullptr, y1, w2 ? y2 : nullptr, mean, rstd,
            x_stride, r1_stride, r2_stride, s_stride, y1_stride, y2_stride, M, C, eps};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_ln_fwd, p, shape, st);
    return (int)hipGetLastError();
}

size_t fastmax_hip_layernorm_backward_workspace(int M, int C, int dtype, int pair, int want_param_grads) {
    if (!want_param_grads || M <= 0 || C <= 0 || dtype < 0 || dtype > FASTMAX_F16) return 0;
    return (size_t)((M + PG_ROWS - 1) / PG_ROWS) * (size_t)(pair ? 4 : 2) * (size_t)C * sizeof(float);
}

int fastmax_hip_layernorm_backward(const void* dy1, int64_t dy1_stride, const void* dy2, int64_t dy2_stride, const void* s,
                                   int64_t s_stride, const void* w1, const void* w2, const float* mean, const float* rstd,
                                   const void* ds_in, int64_t ds_in_stride, void* ds, int64_t ds_stride, float* dw1, float* db1,
                                   float* dw2, float* db2, int M, int C, int dtype, int weight_dtype, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const bool pair = dy2 != nullptr;
    if (!dy1 || !s || !w1 || !mean || !rstd || !ds || pair != (w2 != nullptr) || (!pair && (dw2 || db2))) return FASTMAX_E_NULL;
    const int rc = norm_check(M, C, dtype, weight_dtype);
    if (rc) return rc;
    if (dy1_stride < C || s_stride < C || ds_stride < C || (pair && dy2_stride < C) || (ds_in && ds_in_stride < C))
        return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(dy1, es) || !elem_aligned(dy2, es) || !elem_aligned(s, es) || !elem_aligned(w1, ws) || !elem_aligned(w2, ws) ||
        !elem_aligned(mean, 4) || !elem_aligned(rstd, 4) || !elem_aligned(ds, es) || !elem_aligned(ds_in, es) ||
        !elem_aligned(dw1, 4) || !elem_aligned(db1, 4) || !elem_aligned(dw2, 4) || !elem_aligned(db2, 4))
        return FASTMAX_E_ALIGNMENT;
    const bool want = dw1 || db1 || dw2 || db2;
    const size_t need = fastmax_hip_layernorm_backward_workspace(M, C, dtype, pair, want);
    if (need) {
        if (!workspace) return FASTMAX_E_NULL;
        if (workspace_bytes < need) return FASTMAX_E_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return FASTMAX_E_ALIGNMENT;
    }
    int shape = norm_shape(C, dtype, MAX_NP);
    if (!aligned16(dy1, dy1_stride, es) || !aligned16(s, s_stride, es) || !aligned16(w1, 0, ws) || !aligned16(ds, ds_stride, es) ||
        (pair && (!aligned16(dy2, dy2_stride, es) || !aligned16(w2, 0, ws))) || (ds_in && !aligned16(ds_in, ds_in_stride, es)))
        shape = -1;
    // parameter gradients wanted: PG_ROWS rows per workgroup whatever the path, so the partial rows are the query function's;
    // else one row per workgroup (four on the wave-per-row path)
    const int rpb = want ? PG_ROWS : (shape == 0 ? 4 : 1);
    const int ns = want ? (pair ? 4 : 2) : 0;
    const unsigned nblk = (unsigned)(((int64_t)M + rpb - 1) / rpb);
    LnBwd p{dy1, dy2, s, w1, w2, ds_in, mean, rstd, ds, want ? reinterpret_cast<float*>(workspace) : nullptr,
            dy1_stride, dy2_stride, s_stride, ds_in_stride, ds_stride, M, C, rpb, ns};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_ln_bwd, p, shape, nblk, st);
    int err = (int)hipGetLastError();
    if (err || !want) return err;
    if (pair) launch_partial_row_sum<4>(p.part, {{dw1, db1, dw2, db2}}, (int)nblk, C, st);
    else launch_partial_row_sum<2>(p.part, {{dw1, db1}}, (int)nblk, C, st);
    return (int)hipGetLastError();
}

int fastmax_hip_act_forward(const void* a, int64_t a_stride, void* y, int64_t y_stride, int M, int I, int act, int dtype,
                            void* stream) {
    ActArgs p{a, nullptr, y, a_stride, 0, y_stride, M, I};
    return act_call(p, false, act, dtype, reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_act_backward(const void* a, int64_t a_stride, const void* dy, int64_t dy_stride, void* da, int64_t da_stride,
                             int M, int I, int act, int dtype, void* stream) {
    ActArgs p{a, dy, da, a_stride, dy_stride, da_stride, M, I};
    return act_call(p, true, act, dtype, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
