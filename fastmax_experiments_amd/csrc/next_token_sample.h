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
//   select_nucleus       top-p over the candidates the top-k left, again as a Threshold (see the block above it).
//   sample_kernel        the filter(s), then one pass over the row in quads of four consecutive entries (one Philox call serves
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

// ---- top-p (nucleus) -------------------------------------------------------------------------------------------------------------
// The contract is include/fastmax_hip_nucleus.h: of the candidates K the top-k left (all V entries without one), in the order
// "key descending, index ascending", the shortest prefix whose share of the softmax mass at `temperature` reaches top_p.  That is
// again "key above a threshold, or equal to it with index <= limit", so select_nucleus returns a Threshold and kept() and the
// scoring pass are the top-k's.  One workgroup of 1024 per row:
//   1. the largest key of the row (it is a candidate under every top-k): an integer maximum, m = its value;
//   2. a radix select over the candidates' keys, 8 bits a pass from the top, whose bins carry the MASS of their entries;
//   3. 256 threads scan the bins from the top for the digit at which the running mass reaches what is still needed;
//   4. after four passes the crossing key is known; every entry with that key has one weight q, so ceil(needed / q) of them are
//      kept, and only when that is fewer than there are does kth_index_of_key find the index of the last one.
// Mass is exact integer arithmetic, so the kept set is a function of the row's bits, V, top_k, top_p and temperature alone:
//   weight    w_i = expf((logit_i - m) / temperature) in float32, in [0, 1]; the maximum has w = 1
//   format    q_i = floor(w_i 2^40) as an unsigned 64-bit integer (unsigned 24.40 fixed point; w < 2^-40 counts as 0), added with
//             64-bit integer adds (LDS atomics into one histogram per wave, then plain adds): no float sum anywhere
//   target    total = the sum of q over K; needed = ceil(total * top_p) evaluated in float64 (total and top_p convert with at
//             most one rounding, the product rounds once: relative 2^-52), clamped to [1, total].  The nucleus is the shortest
//             prefix of the order whose q sum to >= needed: at least one entry, at most all of K
//   largest V 2^22 = 4194304: total <= V 2^40 <= 2^62 stays inside 64 bits with room for the scan
// top_p >= 1 or temperature == 0 leave the candidates as they are.  A row whose maximum is NaN or an infinity has total == 0 and
// also keeps its candidates (outside the contract; the token stays in [0, V)).
constexpr int NUCLEUS_MAX_V = 1 << 22;

struct NucleusShared {
    unsigned long long mass[SEL_WAVES][256];
    unsigned long long wave_total[SEL_WAVES];
    unsigned long long total, needed, ties;
    int digit;
};

__device__ __forceinline__ float key_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

__device__ __forceinline__ unsigned long long nucleus_mass(float v, float m, float temperature) {
    const float w = expf((v - m) / temperature);
    return w > 0.f ? (unsigned long long)(fminf(w, 1.f) * 0x1p40f) : 0ull;          // a NaN counts as 0
}

// the index of the k-th entry (k >= 1, by index) whose key is `key`; at least k entries have it.  Whole workgroup, same answer.
// select_threshold's tie count as a function: select_threshold keeps its own loop, because calling this one there moves a few
// compares of the two samplers that existed before the nucleus, and their code stays as it was bit for bit.
__device__ __forceinline__ int kth_index_of_key(const float* __restrict__ row, int V, unsigned key, int k, SelectShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int seen = 0;
    for (int base = 0; base < V; base += SEL_THREADS) {
        const int i = base + tid;
        const bool tie = i < V && order_key(row[i]) == key;
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
    return sh.limit;
}

__device__ __forceinline__ unsigned long long wave_inclusive_scan_u64(unsigned long long x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// every thread of the workgroup calls it with the same arguments and gets the same answer; `cand` is select_threshold's
__device__ Threshold select_nucleus(const float* __restrict__ row, int V, Threshold cand, float top_p, float temperature, SelectShared& sh,
                                    NucleusShared& ns) {
    if (!(top_p < 1.f) || !(temperature > 0.f)) return cand;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned top = 0u;
    for (int i = tid; i < V; i += SEL_THREADS) top = max(top, order_key(row[i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, (unsigned)__shfl_xor((int)top, off, 64));
    if (lane == 0) sh.wave_total[wave] = (int)top;
    __syncthreads();
    for (int wv = 0; wv < SEL_WAVES; ++wv) top = max(top, (unsigned)sh.wave_total[wv]);
    const float m = key_value(top);
    unsigned prefix = 0u;
    unsigned long long needed = 0ull, ties = 0ull;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned above_mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (int j = tid; j < SEL_WAVES * 256; j += SEL_THREADS) (&ns.mass[0][0])[j] = 0ull;
        __syncthreads();
        for (int i = tid; i < V; i += SEL_THREADS) {
            const float v = row[i];
            const unsigned key = order_key(v);
            if ((key & above_mask) == prefix && kept(cand, key, i)) {
                const unsigned long long q = nucleus_mass(v, m, temperature);
                if (q) atomicAdd(&ns.mass[wave][(key >> shift) & 255u], q);
            }
        }
        __syncthreads();
        // threads 0..255 take the bins from the top, as in select_threshold
        unsigned long long h = 0ull, incl = 0ull;
        if (tid < 256) {
#pragma unroll
            for (int wv = 0; wv < SEL_WAVES; ++wv) h += ns.mass[wv][255 - tid];
            incl = wave_inclusive_scan_u64(h);
            if (lane == 63) ns.wave_total[wave] = incl;
        }
        __syncthreads();
        if (tid < 256)
            for (int wv = 0; wv < wave; ++wv) incl += ns.wave_total[wv];
        if (pass == 0) {
            if (tid == 255) ns.total = incl;
            __syncthreads();
            const unsigned long long total = ns.total;
            if (total == 0ull) return cand;
            const double want = ceil((double)total * (double)top_p);
            needed = want >= (double)total ? total : (unsigned long long)want;
            if (needed == 0ull) needed = 1ull;
        }
        if (tid < 256) {
            const unsigned long long above = incl - h;   // mass with this prefix and a larger digit
            if (above < needed && needed <= incl) {
                ns.digit = 255 - tid;
                ns.needed = needed - above;
                ns.ties = h;
            }
        }
        __syncthreads();
        prefix |= (unsigned)ns.digit << shift;
        needed = ns.needed;
        ties = ns.ties;
    }
    // the candidates whose key is `prefix` weigh q each and `ties` together; `needed` more mass takes ceil(needed / q) of them
    const unsigned long long q = nucleus_mass(key_value(prefix), m, temperature);
    if (q == 0ull) return cand;
    const unsigned long long take = (needed + q - 1ull) / q;
    if (take >= ties / q) return Threshold{prefix, prefix == cand.key ? cand.limit : NO_LIMIT};
    return Threshold{prefix, kth_index_of_key(row, V, prefix, (int)take, sh)};
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
    static constexpr bool nucleus = false;
    DrawStream s;
    __device__ __forceinline__ bool open(DrawStream& out) const {
        out = s;
        return true;
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// a Draw with the top-p filter behind the top-k: the same stream, the same stores
template <typename Draw>
struct Nucleus : Draw {
    static constexpr bool nucleus = true;
    float top_p;
};

// Draw: open(stream) -> false: the whole launch leaves before it reads a logit (every workgroup gets the same answer);
// close(b, token), called by ONE thread of row b's workgroup after tokens[b] is stored; `nucleus`: select_nucleus(top_p) narrows
// the top-k's threshold before the scoring pass.
template <typename Draw>
__global__ __launch_bounds__(SEL_THREADS) void sample_kernel(const float* __restrict__ logits, int64_t ld, int64_t* __restrict__ tokens, int V,
                                                             int top_k, float temperature, Draw from) {
    __shared__ SelectShared sh;
    __shared__ Best wave_best[SEL_WAVES];
    DrawStream rs;
    if (!from.open(rs)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    Threshold t = select_threshold(row, V, top_k, sh);
    if constexpr (Draw::nucleus) {
        __shared__ NucleusShared ns;
        t = select_nucleus(row, V, t, from.top_p, temperature, sh, ns);
    }
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
static inline bool nucleus_share(float top_p) { return top_p > 0.f && top_p <= 1.f; }          // (0, 1]; false for a NaN

}  // namespace fastmax
