// The exact top-k filter and the seeded draw of the next-token head, as a template over WHERE the random stream's key and
// draw number come from and what happens to the token: host arguments and a plain store (next_token.hip, fastmax_hip_sample)
// or the decode cursor in device memory, which a recorded graph can advance (decode_cursor.hip, fastmax_hip_sample_cursor).
// The filter, the scores, the order of every comparison: one copy, here.
//
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
#pragma once
#include "fastmax_common.h"

namespace fastmax {

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

// the two 64-bit words of the random stream, in 32-bit halves: the Philox key and the draw number
struct DrawStream {
    unsigned seed_lo, seed_hi, draw_lo, draw_hi;
};

// the stream as host arguments; the token goes to tokens[b] and nowhere else
struct HostDraw {
    DrawStream s;
    __device__ __forceinline__ bool open(DrawStream& out) const {
        out = s;
        return true;
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// Draw: open(stream) -> false: the whole launch leaves before it reads a logit (every workgroup gets the same answer);
// close(b, token), called by ONE thread of row b's workgroup after tokens[b] is stored.
template <typename Draw>
__global__ __launch_bounds__(SEL_THREADS) void sample_kernel(const float* __restrict__ logits, int64_t ld, int64_t* __restrict__ tokens, int V,
                                                             int top_k, float temperature, Draw from) {
    __shared__ SelectShared sh;
    __shared__ Best wave_best[SEL_WAVES];
    DrawStream rs;
    if (!from.open(rs)) return;
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
        if (draw) r = philox4x32_10((unsigned)q, blockIdx.x, rs.draw_lo, rs.draw_hi, rs.seed_lo, rs.seed_hi);
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
        from.close(blockIdx.x, token);
    }
}

constexpr int MAX_EXTENT = 1 << 30;     // C of the logits, V of the filter and the sampler: piece and quad indices stay in int
static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace fastmax
