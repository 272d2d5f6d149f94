// From a hidden state to the next token (include/fastmax_hip_next_token.h): the lm-head over the last position only, an exact
// top-k filter and a seeded sampler whose token stays in device memory.
//
//   last_logits_kernel   256 threads = 4 waves, a wave owns ROWS = 4 rows of W and up to G rows of x (G = 1, 2, 4, 8: the pass's
//                        row count rounded up, the surplus rows re-read the last one and are not stored).  Lane l takes the
//                        16-byte pieces l, l + 64, ... of every row: ROWS loads of W and G loads of x (L1 / L2) feed
//                        ROWS x G x E fused multiply-adds, W straight to registers (it is streamed once, no LDS round trip).
//                        Every (b, v) sum has ONE accumulator per lane, filled in index order from +0, and one xor butterfly
//                        over the lanes: the bits depend on C and the dtype only, not on G, the batch or the load route.
//   select_threshold     one workgroup (1024 threads) per row: radix select of the k-th largest order-preserving 32-bit key,
//                        8 bits a pass from the top.  A pass counts the keys that share the prefix found so far into 256-bin
//                        histograms in LDS (integer adds, one histogram per wave so that a few hot bins are not shared by 16
//                        waves), then 256 threads scan the bins from the top.  After four passes the key T of the k-th
//                        largest value, the number of entries equal to it that are kept and their total are known; only when
//                        the two differ does an index-ordered count of the ties (ballot + popcount, chunk by chunk) find the
//                        index of the last kept one.  keep(i) = key_i > T or (key_i == T and i <= limit).
//   sample_kernel        the filter, then one pass over the row in quads of four consecutive entries (one Philox call serves
//                        a quad; a quad without a kept entry draws nothing), best (score, index) per thread, per wave by
//                        shuffles, per workgroup through LDS.  The row (128 KB at V = 32000) stays in L2 across the passes.
#include "fastmax_common.h"
#include "../../include/fastmax_hip_next_token.h"

namespace fastmax {

typedef unsigned int nu32x4 __attribute__((ext_vector_type(4)));

// ---- last-row logits ---------------------------------------------------------------------------------------------------------
constexpr int LOGIT_ROWS = 4;            // rows of W per wave
constexpr int LOGIT_WAVES = 4;           // waves per workgroup
constexpr int LOGIT_GROUP = 8;           // rows of x per pass over W

// one piece (16 bytes, E elements) as floats; the element route takes the first n elements of a possibly short piece
template <typename T, bool VEC>
__device__ __forceinline__ void load_piece(const T* p, int n, float (&f)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (VEC) {
        const nu32x4 raw = *reinterpret_cast<const nu32x4*>(p);
        const T* pv = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = to_float(pv[e]);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = e < n ? to_float(p[e]) : 0.f;
    }
}

template <typename T, typename O, int G, bool VEC>
__global__ __launch_bounds__(256) void last_logits_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, int64_t ldw,
                                                          O* __restrict__ out, int64_t ldo, int nb, int V, int C) {
    constexpr int E = 16 / sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t v0 = ((int64_t)blockIdx.x * LOGIT_WAVES + wave) * LOGIT_ROWS;
    if (v0 >= V) return;                                  // the whole wave leaves; the kernel has no barrier
    const T* wr[LOGIT_ROWS];
    const T* xr[G];
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r) wr[r] = w + (v0 + r < V ? v0 + r : (int64_t)V - 1) * ldw;
#pragma unroll
    for (int g = 0; g < G; ++g) xr[g] = x + (int64_t)(g < nb ? g : nb - 1) * ldx;
    float acc[LOGIT_ROWS][G];
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[r][g] = 0.f;
    const int npieces = (C + E - 1) / E;
    constexpr int UNROLL = G <= 2 ? 2 : 1;                // more loads in flight where the registers allow it
#pragma unroll UNROLL
    for (int p = lane; p < npieces; p += 64) {
        const int c = p * E;
        const int n = C - c < E ? C - c : E;
        float wf[LOGIT_ROWS][E];
#pragma unroll
        for (int r = 0; r < LOGIT_ROWS; ++r) load_piece<T, VEC>(wr[r] + c, n, wf[r]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float xf[E];
            load_piece<T, VEC>(xr[g] + c, n, xf);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (VEC || e < n) {
#pragma unroll
                    for (int r = 0; r < LOGIT_ROWS; ++r) acc[r][g] = fmaf(xf[e], wf[r][e], acc[r][g]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < LOGIT_ROWS; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float s = wave_sum(acc[r][g]);
            if (lane == 0 && v0 + r < V && g < nb) out[(int64_t)g * ldo + v0 + r] = from_float<O>(s);
        }
}

template <typename T, typename O, int G>
static void launch_logits_route(bool vec, dim3 grid, hipStream_t st, const T* x, int64_t ldx, const T* w, int64_t ldw, O* out,
                                int64_t ldo, int nb, int V, int C) {
    if (vec) hipLaunchKernelGGL((last_logits_kernel<T, O, G, true>), grid, dim3(256), 0, st, x, ldx, w, ldw, out, ldo, nb, V, C);
    else hipLaunchKernelGGL((last_logits_kernel<T, O, G, false>), grid, dim3(256), 0, st, x, ldx, w, ldw, out, ldo, nb, V, C);
}

template <typename T, typename O>
static int launch_logits(const void* xv, int64_t ldx, const void* wv, int64_t ldw, void* ov, int64_t ldo, int B, int V, int C,
                         hipStream_t st) {
    constexpr int E = 16 / sizeof(T);
    const T* x = reinterpret_cast<const T*>(xv);
    const T* w = reinterpret_cast<const T*>(wv);
    O* out = reinterpret_cast<O*>(ov);
    const bool vec = C % E == 0 && ldx % E == 0 && ldw % E == 0 && (reinterpret_cast<uintptr_t>(xv) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(wv) & 15) == 0;
    const int per_block = LOGIT_WAVES * LOGIT_ROWS;
    const dim3 grid((unsigned)(((int64_t)V + per_block - 1) / per_block));
    for (int b0 = 0; b0 < B; b0 += LOGIT_GROUP) {
        const int nb = B - b0 < LOGIT_GROUP ? B - b0 : LOGIT_GROUP;
        const T* xb = x + (int64_t)b0 * ldx;
        O* ob = out + (int64_t)b0 * ldo;
        if (nb == 1) launch_logits_route<T, O, 1>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else if (nb == 2) launch_logits_route<T, O, 2>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else if (nb <= 4) launch_logits_route<T, O, 4>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
        else launch_logits_route<T, O, 8>(vec, grid, st, xb, ldx, w, ldw, ob, ldo, nb, V, C);
    }
    return (int)hipGetLastError();
}

// ---- exact top-k ----------------------------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int NO_LIMIT = 0x7fffffff;

// larger float <=> larger key; -0.0 and +0.0 share a key; -inf is the smallest key of a number
__device__ __forceinline__ unsigned order_key(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Threshold {
    unsigned key;                        // key of the k-th largest value (0: no filter)
    int limit;                           // entries equal to it are kept up to this index
};
__device__ __forceinline__ bool kept(const Threshold& t, unsigned key, int i) { return key > t.key || (key == t.key && i <= t.limit); }

struct SelectShared {
    int hist[SEL_WAVES][256];
    int wave_total[SEL_WAVES];
    int digit, k, ties, limit;
};

__device__ __forceinline__ int wave_inclusive_scan_int(int x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// every thread of the workgroup calls it with the same arguments and gets the same answer
__device__ Threshold select_threshold(const float* __restrict__ row, int V, int k, SelectShared& sh) {
    if (k <= 0 || k >= V) return Threshold{0u, NO_LIMIT};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u;
    int ties = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned above_mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (int j = tid; j < SEL_WAVES * 256; j += SEL_THREADS) (&sh.hist[0][0])[j] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += SEL_THREADS) {
            const unsigned key = order_key(row[i]);
            if ((key & above_mask) == prefix) atomicAdd(&sh.hist[wave][(key >> shift) & 255u], 1);
        }
        __syncthreads();
        // threads 0..255 (waves 0..3) take the bins from the top: thread t owns digit 255 - t
        int h = 0, incl = 0;
        if (tid < 256) {
#pragma unroll
            for (int wv = 0; wv < SEL_WAVES; ++wv) h += sh.hist[wv][255 - tid];
            incl = wave_inclusive_scan_int(h);
            if (lane == 63) sh.wave_total[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int wv = 0; wv < wave; ++wv) incl += sh.wave_total[wv];
            const int above = incl - h;                  // entries with this prefix and a larger digit
            if (above < k && k <= incl) {
                sh.digit = 255 - tid;
                sh.k = k - above;
                sh.ties = h;
            }
        }
        __syncthreads();
        prefix |= (unsigned)sh.digit << shift;
        k = sh.k;
        ties = sh.ties;
    }
    // k of the `ties` entries whose key is `prefix` are kept: all of them, or the k lowest indices
    if (ties == k) return Threshold{prefix, NO_LIMIT};
    int seen = 0;
    for (int base = 0; base < V; base += SEL_THREADS) {
        const int i = base + tid;
        const bool tie = i < V && order_key(row[i]) == prefix;
        const unsigned long long ballot = __ballot(tie);
        const int rank = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) sh.wave_total[wave] = __popcll(ballot);
        __syncthreads();
        int before = seen, total = 0;
        for (int wv = 0; wv < SEL_WAVES; ++wv) {
            const int c = sh.wave_total[wv];
            if (wv < wave) before += c;
            total += c;
        }
        if (tie && before + rank == k - 1) sh.limit = i;
        seen += total;
        __syncthreads();
        if (seen >= k) break;
    }
    return Threshold{prefix, sh.limit};
}

__global__ __launch_bounds__(SEL_THREADS) void topk_mask_kernel(const float* __restrict__ logits, int64_t ld, unsigned char* __restrict__ mask,
                                                                int64_t ldm, int V, int top_k) {
    __shared__ SelectShared sh;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    unsigned char* out = mask + (int64_t)blockIdx.x * ldm;
    const Threshold t = select_threshold(row, V, top_k, sh);
    for (int i = threadIdx.x; i < V; i += SEL_THREADS) out[i] = kept(t, order_key(row[i]), i) ? 1 : 0;
}

// ---- the seeded draw ------------------------------------------------------------------------------------------------------------
struct Philox4 { unsigned w[4]; };

// Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// -log(-log u), u = ((word >> 9) + 0.5) 2^-23 in (0, 1): exact in float32, never 0 or 1
__device__ __forceinline__ float gumbel(unsigned word) {
    const float u = ((float)(word >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

struct Best {
    float score;
    int index;                           // -1: nothing yet
};
__device__ __forceinline__ bool better(float s, int i, const Best& b) {
    return i >= 0 && (b.index < 0 || s > b.score || (s == b.score && i < b.index));
}

__global__ __launch_bounds__(SEL_THREADS) void sample_kernel(const float* __restrict__ logits, int64_t ld, int64_t* __restrict__ tokens, int V,
                                                             int top_k, float temperature, unsigned seed_lo, unsigned seed_hi,
                                                             unsigned draw_lo, unsigned draw_hi) {
    __shared__ SelectShared sh;
    __shared__ Best wave_best[SEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    const Threshold t = select_threshold(row, V, top_k, sh);
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const bool draw = temperature > 0.f;
    Best best{0.f, -1};
    const int nquads = (V + 3) / 4;
    for (int q = tid; q < nquads; q += SEL_THREADS) {
        const int i0 = 4 * q;
        float v[4];
        if (vec && i0 + 4 <= V) {
            const float4 raw = *reinterpret_cast<const float4*>(row + i0);
            v[0] = raw.x, v[1] = raw.y, v[2] = raw.z, v[3] = raw.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i0 + e < V ? row[i0 + e] : 0.f;
        }
        bool keep[4], any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            keep[e] = i0 + e < V && kept(t, order_key(v[e]), i0 + e);
            any = any || keep[e];
        }
        if (!any) continue;
        Philox4 r{{0u, 0u, 0u, 0u}};
        if (draw) r = philox4x32_10((unsigned)q, blockIdx.x, draw_lo, draw_hi, seed_lo, seed_hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!keep[e]) continue;
            const float s = draw ? v[e] / temperature + gumbel(r.w[e]) : v[e];
            if (best.index < 0 || s > best.score) best = Best{s, i0 + e};          // indices rise: the lowest index stays on ties
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float s = __shfl_xor(best.score, off, 64);
        const int i = __shfl_xor(best.index, off, 64);
        if (better(s, i, best)) best = Best{s, i};
    }
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < SEL_WAVES; ++wv)
            if (better(wave_best[wv].score, wave_best[wv].index, best)) best = wave_best[wv];
        const int token = best.index < 0 || best.index >= V ? 0 : best.index;
        tokens[blockIdx.x] = (int64_t)token;
    }
}

constexpr int MAX_EXTENT = 1 << 30;     // C of the logits, V of the filter and the sampler: piece and quad indices stay in int
static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace fastmax

using namespace fastmax;

extern "C" {

int fastmax_hip_last_logits(const void* x, int64_t ldx, const void* w, int64_t ldw, void* logits, int64_t ldo, int B, int V, int C,
                            int dtype, int out_dtype, void* stream) {
    if (!x || !w || !logits) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16 || (out_dtype != FASTMAX_F32 && out_dtype != dtype)) return FASTMAX_E_BAD_DTYPE;
    if (B <= 0 || V <= 0 || C <= 0 || C > MAX_EXTENT || ldx < 0 || ldw < C || ldo < V) return FASTMAX_E_BAD_SHAPE;
    const size_t es = dtype == FASTMAX_F32 ? 4 : 2;
    if (!aligned_to(x, es) || !aligned_to(w, es) || !aligned_to(logits, out_dtype == FASTMAX_F32 ? 4 : 2)) return FASTMAX_E_ALIGNMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FASTMAX_F32) return launch_logits<float, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    if (dtype == FASTMAX_BF16) {
        if (out_dtype == FASTMAX_F32) return launch_logits<bf16_t, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
        return launch_logits<bf16_t, bf16_t>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    }
    if (out_dtype == FASTMAX_F32) return launch_logits<f16_t, float>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
    return launch_logits<f16_t, f16_t>(x, ldx, w, ldw, logits, ldo, B, V, C, st);
}

int fastmax_hip_sample(const float* logits, int64_t ld, int64_t* tokens, int B, int V, int top_k, float temperature, int64_t seed,
                       int64_t draw, void* stream) {
    if (!logits || !tokens) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > MAX_EXTENT || ld < V || top_k < 0 || !(temperature >= 0.f && temperature <= 3.4028234e38f))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(tokens, 8)) return FASTMAX_E_ALIGNMENT;
    const uint64_t s = (uint64_t)seed, d = (uint64_t)draw;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld, tokens,
                       V, top_k, temperature, (unsigned)s, (unsigned)(s >> 32), (unsigned)d, (unsigned)(d >> 32));
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

}  // extern "C"
