// AdamW over the flat LoRA-gradient bucket (dp.py: FlatGradBucket): the whole accumulation boundary -- the division by the world
// size, the global-norm clip, decoupled weight decay, both moments, bias correction, the update, the parameter written in its
// own dtype and the gradient zeroed -- in at most two launches whose arguments never change (so a step can be recorded in a graph).
//
//   adamw_norm_kernel    sum of (grad_scale g)^2 over the flat buffer as at most NORM_MAX_BLOCKS partial sums.  The flat range is
//                        cut into tiles of NORM_TILE elements by the flat INDEX alone (segments play no part): workgroup b takes
//                        tiles b, b + grid, ... in order, a thread adds its elements in index order, lanes by xor butterfly, the
//                        four waves through LDS in wave order.  One float per workgroup leaves for the workspace.
//   adamw_update_kernel  one workgroup per row of the chunk table (CHUNK elements of ONE segment).  When the norm is wanted every
//                        workgroup adds the partial sums itself, in block order (at most four loads per thread): all workgroups
//                        get the same bits, no kernel in between and no hand-off inside the launch.  Workgroup 0 leaves norm,
//                        coef and the finite flag in the scalar record.  Then the element update, every operation rounded on
//                        its own (no contraction), so the vector route and the element route give the same bits and a result
//                        does not depend on how the flat range is cut into segments.
// The step counter lives in the record.  Every workgroup reads it before it takes a ticket; the workgroup that takes the
// launch's last ticket advances the counter (or the skipped counter), after every other workgroup has read the old value.
// Tickets are 64-bit integer adds that are never reset (launch k ends at k times a launch's count).  They go in two levels,
// because adds to ONE address are served one after the other (measured: 29 ns each, 118 us of a 154 us launch at 4096
// chunks): workgroup b adds to slot b % 64, each slot on a cache line of its own, and the workgroup that completes a slot adds
// to the record's ticket, whose last arrival is the launch's.  No float atomics, plain vector stores only.
#include "fastmax_common.h"
#include "../../include/fastmax_hip_optim.h"

namespace fastmax {

typedef unsigned int au32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int au32x2 __attribute__((ext_vector_type(2)));

constexpr int CHUNK = 1024;              // elements per workgroup of the update pass: 256 threads x one piece of 4
constexpr int NORM_TILE = 4096;          // elements per tile of the norm pass: 256 threads x four pieces of 4
constexpr int NORM_MAX_BLOCKS = 1024;    // at most this many partial sums, whatever n: four per thread of an update workgroup
constexpr size_t RECORD_BYTES = 64;
constexpr int TICKET_SLOTS = 64;         // first-level ticket counters, 64 bytes apart, between the record and the partial sums
constexpr size_t TICKET_BYTES = TICKET_SLOTS * 64;

// include/fastmax_hip_optim.h documents the three records
struct Segment {
    void* param;
    int64_t offset, numel;
    int dtype, pad;
};
struct Chunk {
    int64_t start;                       // flat index of the chunk's first element
    int segment, len;
};
struct Record {
    float norm, coef;
    int finite, pad;
    int64_t step, skipped;
    unsigned long long ticket;
};
static_assert(NORM_MAX_BLOCKS == 4 * 256 && sizeof(Segment) == 32 && sizeof(Chunk) == 16 && sizeof(Record) <= RECORD_BYTES, "record layouts are part of the ABI");

// four consecutive elements <-> float registers: one 16-byte access of a float32 stream, one 8-byte access of a 16-bit stream
template <typename U> __device__ __forceinline__ void ld4(const U* p, float (&x)[4]) {
    if constexpr (sizeof(U) == 4) {
        const au32x4 raw = *reinterpret_cast<const au32x4*>(p);
        const U* pv = reinterpret_cast<const U*>(&raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = to_float(pv[e]);
    } else {
        const au32x2 raw = *reinterpret_cast<const au32x2*>(p);
        const U* pv = reinterpret_cast<const U*>(&raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = to_float(pv[e]);
    }
}
template <typename U> __device__ __forceinline__ void st4(U* p, const float (&x)[4]) {
    if constexpr (sizeof(U) == 4) {
        au32x4 raw;
        U* pv = reinterpret_cast<U*>(&raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = from_float<U>(x[e]);
        *reinterpret_cast<au32x4*>(p) = raw;
    } else {
        au32x2 raw;
        U* pv = reinterpret_cast<U*>(&raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = from_float<U>(x[e]);
        *reinterpret_cast<au32x2*>(p) = raw;
    }
}
template <typename U> __device__ __forceinline__ bool piece_aligned(const U* p) {
    return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(U) - 1)) == 0;
}

// sum over the 256 threads: lanes by xor butterfly, the four waves in wave order; every thread gets the same bits
__device__ __forceinline__ float block_sum(float x, float* red) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// x^2 added to acc with two roundings (hipcc would contract it into a fused multiply-add in one route and not in the other)
__device__ __forceinline__ float add_square(float acc, float x, float scale) {
#pragma clang fp contract(off)
    const float s = x * scale;
    const float q = s * s;
    return acc + q;
}

template <typename G>
__global__ __launch_bounds__(256) void adamw_norm_kernel(const G* g, int64_t n, float scale, float* partials) {
    __shared__ float red[4];
    const int64_t ntiles = (n + NORM_TILE - 1) / NORM_TILE;
    const bool vec = piece_aligned(g);
    float acc = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = tile * NORM_TILE + j * 1024 + (int64_t)threadIdx.x * 4;
            if (vec && i + 4 <= n) {
                float x[4];
                ld4<G>(g + i, x);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = add_square(acc, x[e], scale);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < n) acc = add_square(acc, to_float(g[i + e]), scale);
            }
        }
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

struct UpdateArgs {
    void* g;
    float *m, *v, *master;
    const Segment* segments;
    const Chunk* chunks;
    Record* rec;
    unsigned long long* tickets;
    const float* partials;
    const float* lr_ptr;
    int64_t n_chunks;
    int n_partials;
    float lr, beta1, beta2, omb1, omb2, eps, weight_decay, grad_scale, max_norm;
    int clip, skip_nonfinite, zero_grad;
};

// what every element of a launch shares
struct StepScalars {
    float gscale, coef, decay, step_size, sqrt_bc2;
};

__device__ __forceinline__ double int_power(double b, int64_t e) {
    double r = 1.0;
    while (e > 0) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// torch.optim.AdamW (amsgrad=False, maximize=False), every operation rounded to float32 on its own
__device__ __forceinline__ void adamw_element(float g, float& p, float& m, float& v, const UpdateArgs& a, const StepScalars& s) {
#pragma clang fp contract(off)
    const float gh = (g * s.gscale) * s.coef;
    p = p * s.decay;
    const float m1 = a.beta1 * m;
    const float m2 = a.omb1 * gh;
    m = m1 + m2;
    const float v1 = a.beta2 * v;
    const float v2 = (a.omb2 * gh) * gh;
    v = v1 + v2;
    const float denom = sqrtf(v) / s.sqrt_bc2 + a.eps;
    const float q = m / denom;
    const float u = s.step_size * q;
    p = p - u;
}

template <typename G, typename P, bool VEC>
__device__ __forceinline__ void update_chunk(const UpdateArgs& a, const StepScalars& s, const Chunk& c, const Segment& seg, bool skip) {
    constexpr bool LOWP = sizeof(P) == 2;             // a 16-bit parameter: the float32 master is what the update works on
    G* g = reinterpret_cast<G*>(a.g) + c.start;
    float* m = a.m + c.start;
    float* v = a.v + c.start;
    float* w = LOWP ? a.master + c.start : reinterpret_cast<float*>(seg.param) + (c.start - seg.offset);
    P* p = reinterpret_cast<P*>(seg.param) + (c.start - seg.offset);
    if constexpr (VEC) {
        const int i = threadIdx.x * 4;
        if (i >= c.len) return;
        if (!skip) {
            float gx[4], wx[4], mx[4], vx[4];
            ld4<G>(g + i, gx);
            ld4<float>(w + i, wx);
            ld4<float>(m + i, mx);
            ld4<float>(v + i, vx);
#pragma unroll
            for (int e = 0; e < 4; ++e) adamw_element(gx[e], wx[e], mx[e], vx[e], a, s);
            st4<float>(w + i, wx);
            st4<float>(m + i, mx);
            st4<float>(v + i, vx);
            if constexpr (LOWP) st4<P>(p + i, wx);
        }
        if (a.zero_grad) {
            const float zero[4] = {0.f, 0.f, 0.f, 0.f};
            st4<G>(g + i, zero);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i >= c.len) break;
            if (!skip) {
                float wx = w[i], mx = m[i], vx = v[i];
                adamw_element(to_float(g[i]), wx, mx, vx, a, s);
                w[i] = wx;
                m[i] = mx;
                v[i] = vx;
                if constexpr (LOWP) p[i] = from_float<P>(wx);
            }
            if (a.zero_grad) g[i] = from_float<G>(0.f);
        }
    }
}

template <typename G, typename P>
__device__ __forceinline__ void update_route(const UpdateArgs& a, const StepScalars& s, const Chunk& c, const Segment& seg, bool skip) {
    // the vector route: a whole number of pieces, and every stream's first address on its piece boundary (16 bytes of a float32
    // stream, 8 of a 16-bit one).  The same for all threads of the workgroup.
    const int64_t local = c.start - seg.offset;
    const bool vec = (c.len & 3) == 0 && (c.start & 3) == 0 && piece_aligned(reinterpret_cast<const G*>(a.g) + c.start) &&
                     piece_aligned(reinterpret_cast<const P*>(seg.param) + local);
    if (vec) update_chunk<G, P, true>(a, s, c, seg, skip);
    else update_chunk<G, P, false>(a, s, c, seg, skip);
}

template <typename G>
__global__ __launch_bounds__(256) void adamw_update_kernel(UpdateArgs a) {
    __shared__ float red[4];
    __shared__ StepScalars shared;
    __shared__ int shared_skip;
    __shared__ long long shared_step;
    const bool use_norm = a.clip || a.skip_nonfinite;
    float total = 0.f;
    if (use_norm) {
        // NORM_MAX_BLOCKS = 4 x 256: four independent loads per thread, added in block order (a missing one adds +0)
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = threadIdx.x + 256 * j;
            x[j] = i < a.n_partials ? a.partials[i] : 0.f;
        }
        total = block_sum(((x[0] + x[1]) + x[2]) + x[3], red);
    }
    if (threadIdx.x == 0) {
        float coef = 1.0f;
        int finite = 1;
        if (use_norm) {
            const float norm = sqrtf(total);
            finite = isfinite(norm) ? 1 : 0;
            if (a.clip) {
                const float c = a.max_norm / (norm + 1e-6f);       // torch.nn.utils.clip_grad_norm_
                coef = c > 1.0f ? 1.0f : c;                         // a NaN stays a NaN, as torch.clamp(max=1) leaves it
            }
            if (blockIdx.x == 0) {
                a.rec->norm = norm;
                a.rec->coef = coef;
                a.rec->finite = finite;
            }
        }
        const int64_t t = a.rec->step + 1;
        const double lr = a.lr_ptr ? (double)*a.lr_ptr : (double)a.lr;
        // beta^t from the complements: 1 - beta2 = 0.001 as a float is closer to the caller's double than 0.999 as a float is
        const double bc1 = 1.0 - int_power(1.0 - (double)a.omb1, t);
        const double bc2 = 1.0 - int_power(1.0 - (double)a.omb2, t);
        shared.gscale = a.grad_scale;
        shared.coef = coef;
        shared.decay = (float)(1.0 - lr * (double)a.weight_decay);
        shared.step_size = (float)(lr / bc1);
        shared.sqrt_bc2 = (float)sqrt(bc2);
        shared_skip = (a.skip_nonfinite && !finite) ? 1 : 0;
        shared_step = t;
    }
    __syncthreads();
    const StepScalars s = shared;
    const bool skip = shared_skip != 0;
    const Chunk c = a.chunks[blockIdx.x];
    const Segment seg = a.segments[c.segment];
    if (seg.dtype == FASTMAX_F32) update_route<G, float>(a, s, c, seg, skip);
    else if (seg.dtype == FASTMAX_BF16) update_route<G, bf16_t>(a, s, c, seg, skip);
    else update_route<G, f16_t>(a, s, c, seg, skip);
    if (threadIdx.x == 0) {
        // thread 0's read of the counter is complete (its value went through LDS and the barrier above) before it takes the
        // ticket, and the read is all that has to precede it: no fence, which would write the L2 back once per workgroup
        const unsigned long long n_chunks = (unsigned long long)a.n_chunks;
        const unsigned slot = blockIdx.x % TICKET_SLOTS;
        const unsigned long long members = (n_chunks - slot + TICKET_SLOTS - 1) / TICKET_SLOTS;      // workgroups b with b % 64 == slot
        const unsigned long long slots = n_chunks < TICKET_SLOTS ? n_chunks : (unsigned long long)TICKET_SLOTS;
        const unsigned long long mine = atomicAdd(a.tickets + slot * 8, 1ULL) + 1ULL;
        if (mine % members == 0ULL) {
            const unsigned long long top = atomicAdd(&a.rec->ticket, 1ULL) + 1ULL;
            if (top % slots == 0ULL) {
                if (skip) a.rec->skipped = a.rec->skipped + 1;
                else a.rec->step = shared_step;
            }
        }
    }
}

static inline int norm_blocks(int64_t n) {
    const int64_t tiles = (n + NORM_TILE - 1) / NORM_TILE;
    return (int)(tiles < NORM_MAX_BLOCKS ? tiles : NORM_MAX_BLOCKS);
}
static inline size_t workspace_bytes_for(int64_t n) {
    return RECORD_BYTES + TICKET_BYTES + (((size_t)norm_blocks(n) * sizeof(float) + 15) & ~(size_t)15);
}
static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace fastmax

using namespace fastmax;

extern "C" {

size_t fastmax_hip_adamw_workspace(int64_t n) { return n <= 0 ? 0 : workspace_bytes_for(n); }

int fastmax_hip_adamw_chunk(void) { return CHUNK; }

int fastmax_hip_adamw_norm(const void* g, int g_dtype, int64_t n, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!g || !workspace) return FASTMAX_E_NULL;
    if (g_dtype < 0 || g_dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (n <= 0) return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(g, g_dtype == FASTMAX_F32 ? 4 : 2) || !aligned_to(workspace, 16)) return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < workspace_bytes_for(n)) return FASTMAX_E_WORKSPACE;
    float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + RECORD_BYTES + TICKET_BYTES);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)norm_blocks(n)), blk(256);
    if (g_dtype == FASTMAX_F32) hipLaunchKernelGGL(adamw_norm_kernel<float>, grid, blk, 0, st, reinterpret_cast<const float*>(g), n, grad_scale, partials);
    else if (g_dtype == FASTMAX_BF16) hipLaunchKernelGGL(adamw_norm_kernel<bf16_t>, grid, blk, 0, st, reinterpret_cast<const bf16_t*>(g), n, grad_scale, partials);
    else hipLaunchKernelGGL(adamw_norm_kernel<f16_t>, grid, blk, 0, st, reinterpret_cast<const f16_t*>(g), n, grad_scale, partials);
    return (int)hipGetLastError();
}

int fastmax_hip_adamw_update(void* g, int g_dtype, int64_t n, float* m, float* v, float* master, int64_t n_lowp,
                             const void* segments, int64_t n_segments, const void* chunks, int64_t n_chunks, float lr,
                             const float* lr_ptr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                             float weight_decay, float grad_scale, float max_norm, int clip, int skip_nonfinite, int zero_grad,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!g || !m || !v || !segments || !chunks || !workspace || (n_lowp > 0 && !master)) return FASTMAX_E_NULL;
    if (g_dtype < 0 || g_dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (n <= 0 || n_segments <= 0 || n_segments > n || n_lowp < 0 || n_lowp > n_segments) return FASTMAX_E_BAD_SHAPE;
    // a chunk holds at least one element and at most CHUNK; the grid's x extent ends at 2^31 - 1
    if (n_chunks <= 0 || n_chunks > 0x7fffffffLL || n_chunks > n || n_chunks < (n + CHUNK - 1) / CHUNK) return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(g, g_dtype == FASTMAX_F32 ? 4 : 2) || !aligned_to(m, 16) || !aligned_to(v, 16) || !aligned_to(master, 16) ||
        !aligned_to(workspace, 16) || !aligned_to(segments, 8) || !aligned_to(chunks, 8) || !aligned_to(lr_ptr, 4))
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < workspace_bytes_for(n)) return FASTMAX_E_WORKSPACE;
    UpdateArgs a;
    a.g = g;
    a.m = m;
    a.v = v;
    a.master = master;
    a.segments = reinterpret_cast<const Segment*>(segments);
    a.chunks = reinterpret_cast<const Chunk*>(chunks);
    a.rec = reinterpret_cast<Record*>(workspace);
    a.tickets = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + RECORD_BYTES);
    a.partials = reinterpret_cast<const float*>(reinterpret_cast<char*>(workspace) + RECORD_BYTES + TICKET_BYTES);
    a.lr_ptr = lr_ptr;
    a.n_chunks = n_chunks;
    a.n_partials = norm_blocks(n);
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.omb1 = one_minus_beta1;
    a.omb2 = one_minus_beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.grad_scale = grad_scale;
    a.max_norm = max_norm;
    a.clip = clip ? 1 : 0;
    a.skip_nonfinite = skip_nonfinite ? 1 : 0;
    a.zero_grad = zero_grad ? 1 : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_chunks), blk(256);
    if (g_dtype == FASTMAX_F32) hipLaunchKernelGGL(adamw_update_kernel<float>, grid, blk, 0, st, a);
    else if (g_dtype == FASTMAX_BF16) hipLaunchKernelGGL(adamw_update_kernel<bf16_t>, grid, blk, 0, st, a);
    else hipLaunchKernelGGL(adamw_update_kernel<f16_t>, grid, blk, 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
