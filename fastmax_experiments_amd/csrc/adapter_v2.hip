// Adapter-v2 fine-tuning (lit_gpt/adapter_v2.py:50-62): y = adapter_scale * (linear(x) + adapter_bias) behind every linear of
// the model, as row kernels on the linear's output z.  Rounding points and the order of every sum: include/fastmax_hip_adapter.h.
// Both kernels are bandwidth-bound streams: one read and one write forward; two reads, one write and two rows of partial sums
// per row block backward.
//
// A thread owns one UNIT of columns: a 16-byte piece of z (E = 16 / sizeof(T) columns; the float32 operands beside a 16-bit z
// are then two pieces) on the vector path, one column on the scalar path.  The arithmetic per column and the order of every
// sum are the same on both, so they give the same bits.
//   forward    one unit of one row per thread, the flat index of the gated activation (block_neighbours.hip)
//   backward   a workgroup takes ROWS rows of a slab of 64 units; wave w walks rows w, w + 4, ... of the block in order and keeps
//              its columns' two sums in registers, the four waves' sums are added in wave order through LDS, and the workgroup
//              leaves one partial row per sum; partial_row_sum_kernel (row_kernels.h) adds the partial rows in block order.
//              Without the sums the same kernel only writes dz.
#include "row_kernels.h"
#include "../../include/fastmax_hip_adapter.h"

namespace fastmax {

constexpr int ROWS = FASTMAX_ADAPTER_ROWS_PER_BLOCK;       // fixed, so the sums are too
constexpr int IN_FLIGHT = 4;                               // rows a wave has loads out for (backward)

struct AdapterArgs {
    const void *z, *scale, *bias, *dy;
    void *y, *dz;
    float* part;                 // (row blocks, 2, N) partial sums: dscale's row, then dbias's; or null
    int64_t zs, ys, dys, dzs;
    int M, N, slabs;             // slabs: 64-unit column slabs per row (backward)
};

template <typename U, int E> __device__ __forceinline__ void ld_unit(const U* p, float (&x)[E]) {
    if constexpr (E == 1) x[0] = to_float(*p);
    else ld_vec<U, E>(p, x);
}
template <typename U, int E> __device__ __forceinline__ void st_unit(U* p, const float (&x)[E]) {
    if constexpr (E == 1) *p = from_float<U>(x[0]);
    else st_vec<U, E>(p, x);
}
// A float32 result as a value of its own before it is rounded to 16 bits.  For (_Float16)(a * b) hipcc selects v_fma_mixlo_f16,
// which rounds the EXACT product once; torch rounds the float32 product, then that to fp16, and with float32 parameters the two
// differ by one fp16 step in a few entries per thousand (last_logits.hip meets the same instruction).
__device__ __forceinline__ float own(float x) {
    asm("" : "+v"(x));
    return x;
}
// t of the header: z + bias, rounded to the activation dtype when the parameters have it, the float32 sum when they are float32
template <typename T, typename W> __device__ __forceinline__ float shifted(float z, float bias) {
    if constexpr (sizeof(W) == sizeof(T)) return round_to<T>(own(z + bias));
    else return z + bias;
}

// Y: y's and dy's type -- T when the parameters have the activation dtype, float when they are float32
template <typename T, typename W, bool VEC>
__global__ __launch_bounds__(256) void adapter_fwd_kernel(AdapterArgs p) {
    using Y = W;
    constexpr int E = VEC ? 16 / sizeof(T) : 1;
    const int upr = p.N / E;                                           // units per row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)p.M * upr) return;
    const int64_t row = idx / upr;
    const int col = (int)(idx - row * upr) * E;
    float z[E], sc[E], bi[E], y[E];
    ld_unit<T, E>(reinterpret_cast<const T*>(p.z) + row * p.zs + col, z);
    ld_unit<W, E>(reinterpret_cast<const W*>(p.scale) + col, sc);
    ld_unit<W, E>(reinterpret_cast<const W*>(p.bias) + col, bi);
#pragma unroll
    for (int e = 0; e < E; ++e) y[e] = own(mul_unfused(sc[e], shifted<T, W>(z[e], bi[e])));
    st_unit<Y, E>(reinterpret_cast<Y*>(p.y) + row * p.ys + col, y);
}

template <typename T, typename W, bool VEC, bool DZ, bool SUMS>
__global__ __launch_bounds__(256) void adapter_bwd_kernel(AdapterArgs p) {
    using Y = W;
    constexpr int E = VEC ? 16 / sizeof(T) : 1;
    __shared__ float comb[SUMS ? 2 * 4 * E * 64 : 1];                  // [sum][wave][e][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blk = blockIdx.x / p.slabs;
    const int unit = (int)(blockIdx.x - blk * p.slabs) * 64 + lane;
    const bool live = unit < p.N / E;
    const int col = unit * E;
    const int64_t row0 = blk * ROWS;
    const int nrows = (int)min((int64_t)ROWS, (int64_t)p.M - row0);
    float ds[E], db[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ds[e] = db[e] = 0.f;
    if (live) {
        float sc[E], bi[E];
        ld_unit<W, E>(reinterpret_cast<const W*>(p.scale) + col, sc);
        if constexpr (SUMS) ld_unit<W, E>(reinterpret_cast<const W*>(p.bias) + col, bi);
        // IN_FLIGHT of the wave's rows at a time, their loads issued before any of them is used (unrolled by hand: the partial
        // unroller leaves a loop with an asm statement alone).  The sums still take the rows in order
        for (int i0 = wave; i0 < nrows; i0 += 4 * IN_FLIGHT) {
            float dy[IN_FLIGHT][E], z[SUMS ? IN_FLIGHT : 1][E];
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; ++u) {
                const int64_t row = row0 + i0 + 4 * u;
                if (i0 + 4 * u < nrows) {
                    ld_unit<Y, E>(reinterpret_cast<const Y*>(p.dy) + row * p.dys + col, dy[u]);
                    if constexpr (SUMS) ld_unit<T, E>(reinterpret_cast<const T*>(p.z) + row * p.zs + col, z[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; ++u) {
                const int64_t row = row0 + i0 + 4 * u;
                if (i0 + 4 * u < nrows) {
                    float dz[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) dz[e] = own(mul_unfused(dy[u][e], sc[e]));
                    if constexpr (SUMS) {
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            ds[e] += mul_unfused(dy[u][e], shifted<T, W>(z[u][e], bi[e]));
                            db[e] += dz[e];
                        }
                    }
                    if constexpr (DZ) st_unit<T, E>(reinterpret_cast<T*>(p.dz) + row * p.dzs + col, dz);
                }
            }
        }
    }
    if constexpr (SUMS) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            comb[(wave * E + e) * 64 + lane] = ds[e];
            comb[((4 + wave) * E + e) * 64 + lane] = db[e];
        }
        __syncthreads();
        if (wave == 0 && live) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                float s[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float* q = comb + (k * 4 * E + e) * 64 + lane;
                    s[e] = ((q[0] + q[E * 64]) + q[2 * E * 64]) + q[3 * E * 64];
                }
                st_unit<float, E>(p.part + (blk * 2 + k) * p.N + col, s);
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <typename T, typename W>
static void launch_adapter_fwd(const AdapterArgs& p, bool vec, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), blk(256);
    if (vec) hipLaunchKernelGGL((adapter_fwd_kernel<T, W, true>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((adapter_fwd_kernel<T, W, false>), grid, blk, 0, st, p);
}

template <typename T, typename W, bool VEC>
static void launch_adapter_bwd_vec(const AdapterArgs& p, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), blk(256);
    if (p.dz && p.part) hipLaunchKernelGGL((adapter_bwd_kernel<T, W, VEC, true, true>), grid, blk, 0, st, p);
    else if (p.dz) hipLaunchKernelGGL((adapter_bwd_kernel<T, W, VEC, true, false>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((adapter_bwd_kernel<T, W, VEC, false, true>), grid, blk, 0, st, p);
}
template <typename T, typename W>
static void launch_adapter_bwd(const AdapterArgs& p, bool vec, unsigned blocks, hipStream_t st) {
    if (vec) launch_adapter_bwd_vec<T, W, true>(p, blocks, st);
    else launch_adapter_bwd_vec<T, W, false>(p, blocks, st);
}

// whether every operand allows 16-byte pieces: rows of whole pieces of z (and then of the wider float32 operands), aligned
static bool adapter_vec(const AdapterArgs& p, int dtype, int weight_dtype) {
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (p.N % (16 / es)) return false;
    return aligned16(p.z, p.zs, es) && aligned16(p.scale, 0, ws) && aligned16(p.bias, 0, ws) &&
           (!p.y || aligned16(p.y, p.ys, ws)) && (!p.dy || aligned16(p.dy, p.dys, ws)) && (!p.dz || aligned16(p.dz, p.dzs, es));
}

}  // namespace fastmax

using namespace fastmax;

extern "C" {

int fastmax_hip_adapter_forward(const void* z, int64_t z_stride, const void* scale, const void* bias, void* y, int64_t y_stride,
                                int M, int N, int dtype, int param_dtype, void* stream) {
    if (!z || !scale || !bias || !y) return FASTMAX_E_NULL;
    const int weight_dtype = param_dtype;
    const int rc = norm_check(M, N, dtype, weight_dtype);
    if (rc) return rc;
    if (z_stride < N || y_stride < N) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(z, es) || !elem_aligned(scale, ws) || !elem_aligned(bias, ws) || !elem_aligned(y, ws))
        return FASTMAX_E_ALIGNMENT;
    AdapterArgs p{z, scale, bias, nullptr, y, nullptr, nullptr, z_stride, y_stride, 0, 0, M, N, 0};
    const bool vec = adapter_vec(p, dtype, weight_dtype);
    const int64_t nb = ((int64_t)M * (vec ? N / (16 / es) : N) + 255) / 256;
    if (nb > 0x7fffffff) return FASTMAX_E_BAD_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_adapter_fwd, p, vec, (unsigned)nb, st);
    return (int)hipGetLastError();
}

size_t fastmax_hip_adapter_backward_workspace(int M, int N, int dtype, int want_param_grads) {
    if (!want_param_grads || M <= 0 || N <= 0 || dtype < 0 || dtype > FASTMAX_F16) return 0;
    return (size_t)(((int64_t)M + ROWS - 1) / ROWS) * 2 * (size_t)N * sizeof(float);
}

int fastmax_hip_adapter_backward(const void* dy, int64_t dy_stride, const void* z, int64_t z_stride, const void* scale,
                                 const void* bias, void* dz, int64_t dz_stride, float* dscale, float* dbias, int M, int N,
                                 int dtype, int param_dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !z || !scale || !bias || (dscale == nullptr) != (dbias == nullptr) || (!dz && !dscale)) return FASTMAX_E_NULL;
    const int weight_dtype = param_dtype;
    const int rc = norm_check(M, N, dtype, weight_dtype);
    if (rc) return rc;
    if (dy_stride < N || z_stride < N || (dz && dz_stride < N)) return FASTMAX_E_BAD_SHAPE;
    const int es = elem_size(dtype), ws = elem_size(weight_dtype);
    if (!elem_aligned(dy, ws) || !elem_aligned(z, es) || !elem_aligned(scale, ws) || !elem_aligned(bias, ws) ||
        !elem_aligned(dz, es) || !elem_aligned(dscale, 4) || !elem_aligned(dbias, 4))
        return FASTMAX_E_ALIGNMENT;
    const size_t need = fastmax_hip_adapter_backward_workspace(M, N, dtype, dscale != nullptr);
    if (need) {
        if (!workspace) return FASTMAX_E_NULL;
        if (workspace_bytes < need) return FASTMAX_E_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return FASTMAX_E_ALIGNMENT;
    }
    AdapterArgs p{z, scale, bias, dy, nullptr, dz, dscale ? reinterpret_cast<float*>(workspace) : nullptr,
                  z_stride, 0, dy_stride, dz_stride, M, N, 0};
    const bool vec = adapter_vec(p, dtype, weight_dtype);
    const int units = vec ? N / (16 / es) : N;
    p.slabs = (units + 63) / 64;
    const int nblk = (int)(((int64_t)M + ROWS - 1) / ROWS);
    const int64_t nb = (int64_t)nblk * p.slabs;
    if (nb > 0x7fffffff) return FASTMAX_E_BAD_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NORM_DISPATCH(launch_adapter_bwd, p, vec, (unsigned)nb, st);
    const int err = (int)hipGetLastError();
    if (err || !dscale) return err;
    launch_partial_row_sum<2>(p.part, {{dscale, dbias}}, nblk, N, st);
    return (int)hipGetLastError();
}

}  // extern "C"
