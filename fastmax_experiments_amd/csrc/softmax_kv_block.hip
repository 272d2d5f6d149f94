// Softmax KV cache, many new tokens at once (include/fastmax_hip_softmax_block.h: fastmax_hip_softmax_kv_append_attend_block): the
// contract and the cache of softmax_kv_decode.hip under another work split.  That file gives every new token workgroups of its own,
// which is right for T = 1 and reads the cache T times otherwise; here the new tokens share one pass.
//
// rows     The query rows of a KV group (b, g) are the ts * qpk (token, head) pairs of a slice, token-major: row rho is head
//          rho % qpk of token rho / qpk, with its own bound n = len + t0 + rho / qpk.  A workgroup (4 waves) takes a tile of ROWS of
//          them as ROWS / 16 column tiles of S^T; a token's heads may straddle two tiles, the row index is the unit.  Rows past the
//          group's last have n = -1: no position is live for them.
// keys     grid.x is the span: SPAN consecutive chunks of CHUNK ABSOLUTE positions.  The workgroup walks its span's chunks up to
//          the one that holds nmax, the largest n of its tile, and exits at once if the span starts past nmax.  In every chunk wave
//          w owns positions 32 w .. 32 w + 31, as in the decode kernel, so a wave's keys of a span are a fixed set of positions.
//   Q      the tile's rows once into LDS behind the V image (rows padded to 2 DP + 16 bytes); a column tile's B-operand fragments
//          (lane: row lane & 15, columns 32 s + 8 (lane >> 4)) are read from there per chunk: in registers they cost scratch.
//   K      the wave's two 16-row A operands of the chunk, from the cache into registers; ONE fragment serves every column tile.
//          Rows past nmax and columns past D are zeros and are never loaded.
//   S^T    = K Q^T per column tile; x = s * scale * log2 e, positions past the ROW's n SELECTED to -inf.
//   online per (wave, row): mc = the chunk's maximum, mn = max(m, mc), alpha = exp2(m - mn) -- SELECTED to exactly 1 when mn == m,
//          which covers m = mn = -inf, so no exp2(-inf - (-inf)) exists --, p = exp2(x - mn) (mn = -inf: exp2(-inf - 0) = 0),
//          l = l alpha + sum p, O^T = O^T alpha + V^T P^T.  A chunk with no live position for the row has mc = -inf: mn = m,
//          alpha = 1, p = 0, and l, O^T keep their bits (x * 1 + 0).  A column tile with no live position in the wave's 32 keys is
//          skipped, which is the same no-op.
//   V      one image of the chunk in LDS (rows padded to 2 DP + 64 bytes, pieces past nmax or past D written as zeros), read back
//          transposed by ds_read_b64_tr_b16 ONCE per 16 columns and used by every column tile's O^T += V^T P^T.
//   ahead  the next chunk's K fragments and V pieces are loaded into registers before the current chunk's matrix work; the V
//          pieces go to LDS at the top of the next round.
//   merge  per column tile, the decode kernel's: the four waves' (m, l) meet in LDS, M = their maximum (a row with no live key in
//          the span: M = -inf, taken as 0 in the exponent, and its partial is m = -inf, l = 0, numerator 0), each wave writes
//          O^T exp2(m - M) over the V image, the 256 threads add the four in wave order and write the row's partial of the span.
// combine  sm_combine_kernel (softmax_kv_common.h) with spans for chunks; span 0's workgroups leave each row's number of spans
//          (0: the guard fired) where it expects the number of chunks.
// A row's arithmetic uses its q row, its bound and the positions <= n alone, each position in a fixed (span, wave, chunk, lane)
// place: the bits do not depend on T, the slicing, the tile, B, max_len or the strides.
// LDS: the V image 128 (2 DP + 64), Q ROWS (2 DP + 16) and 512 bytes of wave (m, l): DP = 32: 22,016; 64: 34,304; 128: 58,880; 256 (16
// rows): 82,688.  Registers (VGPRs + AGPRs): 133 + 36 / 197 + 68 / 256 + 206 / 254 + 170; no scratch.
#include "../../include/fastmax_hip_softmax_block.h"
#include "softmax_kv_common.h"

namespace fastmax {
namespace smkv {

constexpr int BLOCK_ROWS = FASTMAX_KV_BLOCK_ROWS, BLOCK_ROWS_D256 = FASTMAX_KV_BLOCK_ROWS_D256, SPAN = FASTMAX_KV_BLOCK_SPAN,
              TOKENS = FASTMAX_KV_BLOCK_TOKENS;
template <int DP> constexpr int q_row() { return 2 * DP + 16; }
template <int DP, int ROWS> constexpr int block_lds() { return attend_lds<DP>() + ROWS * q_row<DP>(); }
static_assert(BLOCK_ROWS % RB == 0 && BLOCK_ROWS_D256 % RB == 0, "a tile is whole 16-row column tiles");

// the wave's K operands (kf) and the thread's V pieces (vp) of the chunk at kbase / vbase; rows 0 .. jn of the chunk are live
template <typename V8, int NS>
__device__ __forceinline__ void load_chunk(V8 (&kf)[2][NS], uint4 (&vp)[CHUNK * (4 * NS) / NT], const uint16_t* kbase, const uint16_t* vbase,
                                           int jn, int D, int tid) {
    constexpr int DP = 32 * NS, PPV = CHUNK * (DP / 8) / NT;
    const int lane = tid & 63, w = tid >> 6, r = lane & 15, gq = lane >> 4;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int col = 32 * s + 8 * gq;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = WPOS * w + 16 * t + r;
            const uint4 x = (j <= jn && col < D) ? *reinterpret_cast<const uint4*>(kbase + (int64_t)j * D + col) : uint4{0, 0, 0, 0};
            kf[t][s] = __builtin_bit_cast(V8, x);
        }
    }
#pragma unroll
    for (int u = 0; u < PPV; ++u) {
        const int i = tid + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        vp[u] = (row <= jn && 8 * pc < D) ? *reinterpret_cast<const uint4*>(vbase + (int64_t)row * D + 8 * pc) : uint4{0, 0, 0, 0};
    }
}

// workspace: part (B * H, ts, nspan, D + 2) floats = (m, l, numerator), then nspans (B * H, ts) ints
// grid: (nspan, B * Hkv, ceil(ts * qpk / ROWS)); block: NT; dynamic LDS: block_lds<32 NS, ROWS>()
template <typename T, int NS, int ROWS>
__global__ __launch_bounds__(NT) void sm_block_attend_kernel(const uint16_t* __restrict__ q, Strides3 qs, const int* __restrict__ hdr,
                                                             const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                             float* __restrict__ part, int* __restrict__ nspans, int Hkv, int qpk, int D,
                                                             int max_len, int64_t cap, int Tn, int t0, int ts, float c2) {
    typedef typename Op<T>::v8 V8;
    constexpr int DP = 32 * NS, DT = DP / 16, PPV = CHUNK * (DP / 8) / NT, CT = ROWS / RB, PPQ = ROWS * (DP / 8) / NT;
    static_assert(PPQ * NT == ROWS * (DP / 8), "the Q pieces divide among the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wm[NW][RB], wl[NW][RB];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, gq = lane >> 4;
    const int sp = blockIdx.x, nspan = gridDim.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv;
    const int nrows = ts * qpk, row0 = blockIdx.z * ROWS;    // the group's rows in this slice; this tile's first
    const int len = hdr[FASTMAX_KV_LEN];
    const bool over = overflows(len, Tn, max_len);
    if (sp == 0 && tid < ROWS && row0 + tid < nrows) {
        const int ti = (row0 + tid) / qpk, hh = (row0 + tid) % qpk;
        nspans[((int64_t)bg * qpk + hh) * ts + ti] = over ? 0 : (len + t0 + ti) / (SPAN * CHUNK) + 1;
    }
    if (over) return;
    const int last = (row0 + ROWS < nrows ? row0 + ROWS : nrows) - 1;
    const int nmax = len + t0 + last / qpk;                  // the largest bound of the tile; < max_len <= cap
    const int64_t c0 = (int64_t)sp * SPAN;
    if (c0 * CHUNK > nmax) return;
    const int c1 = (int)(c0 + SPAN < nmax / CHUNK + 1 ? c0 + SPAN : nmax / CHUNK + 1);
    const uint16_t* kg = kc + (int64_t)bg * cap * D;
    const uint16_t* vg = vc + (int64_t)bg * cap * D;

    // the tile's Q rows into LDS behind the V image (rows padded to 2 DP + 16 bytes; dead rows and columns past D as zeros), and
    // every column tile's bound for this lane's row
    char* qlds = smem + attend_lds<DP>();
#pragma unroll
    for (int u = 0; u < PPQ; ++u) {
        const int i = tid + NT * u, row = i / (DP / 8), pc = i % (DP / 8), rho = row0 + row;
        const bool live = rho < nrows && 8 * pc < D;
        const int ti = live ? rho / qpk : 0, hh = live ? rho % qpk : 0;
        const uint16_t* qrow = q + (int64_t)b * qs.sb + (int64_t)(g * qpk + hh) * qs.sh + (int64_t)(t0 + ti) * qs.sn;
        *reinterpret_cast<uint4*>(qlds + row * q_row<DP>() + 16 * pc) = live ? *reinterpret_cast<const uint4*>(qrow + 8 * pc) : uint4{0, 0, 0, 0};
    }
    int nrow[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int rho = row0 + RB * ct + r;
        nrow[ct] = rho < nrows ? len + t0 + rho / qpk : -1;
    }

    float m[CT], l[CT];
    f32x4 acc[CT][DT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        m[ct] = -INFINITY, l[ct] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[ct][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    V8 kn[2][NS];
    uint4 vn[PPV];
    load_chunk<V8, NS>(kn, vn, kg + c0 * CHUNK * D, vg + c0 * CHUNK * D, nmax - (int)(c0 * CHUNK), D, tid);
    for (int c = (int)c0; c < c1; ++c) {
        const int j0 = c * CHUNK;
        V8 kf[2][NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) kf[0][s] = kn[0][s], kf[1][s] = kn[1][s];
#pragma unroll
        for (int u = 0; u < PPV; ++u) {
            const int i = tid + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
            *reinterpret_cast<uint4*>(smem + row * v_row<DP>() + 16 * pc) = vn[u];
        }
        __syncthreads();                                     // the chunk's V image (and, the first time, Q) is written
        if (c + 1 < c1) load_chunk<V8, NS>(kn, vn, kg + (int64_t)(j0 + CHUNK) * D, vg + (int64_t)(j0 + CHUNK) * D, nmax - j0 - CHUNK, D, tid);

        // S^T and the running (m, l) of every column tile; P and the rescale factor are kept for the products with V
        V8 pf[CT];
        float alpha[CT];
        bool on[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int jn = nrow[ct] - j0;                    // positions 0 .. jn of the chunk are live for this lane's row
            on[ct] = __builtin_amdgcn_ballot_w64(jn >= WPOS * w) != 0;
            if (!on[ct]) continue;                           // no live position among the wave's keys for any row of the tile
            V8 qf[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                qf[s] = __builtin_bit_cast(V8, *reinterpret_cast<const uint4*>(qlds + (RB * ct + r) * q_row<DP>() + 64 * s + 16 * gq));
            float x[8], mc = -INFINITY;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NS; ++s) st = Op<T>::mma(kf[t][s], qf[s], st);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = WPOS * w + 16 * t + 4 * gq + i;
                    x[4 * t + i] = j <= jn ? st[i] * c2 : -INFINITY;
                    mc = fmaxf(mc, x[4 * t + i]);
                }
            }
            mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
            mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
            const float mn = fmaxf(m[ct], mc);
            alpha[ct] = mn == m[ct] ? 1.f : __builtin_amdgcn_exp2f(m[ct] - mn);          // mn > m here: m - mn is -inf or finite
            const float msafe = mn == -INFINITY ? 0.f : mn;
            float lw = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                x[i] = __builtin_amdgcn_exp2f(x[i] - msafe);
                lw += x[i];
            }
            lw += __shfl_xor(lw, 16, 64);
            lw += __shfl_xor(lw, 32, 64);
            l[ct] = l[ct] * alpha[ct] + lw;
            m[ct] = mn;
            pf[ct] = Op<T>::round8(x);
        }

        // O^T = O^T alpha + V^T P^T: tile dt holds columns 16 dt + 4 gq + {0..3} of row r; one V fragment serves every column tile
        {
            const int qq = r >> 2, pp = r & 3;
            const char* va = smem + (WPOS * w + 4 * gq + qq) * v_row<DP>() + 8 * pp;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                union { V8 v; s16x4 h[2]; } u;
                u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt));
                u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt + 16 * v_row<DP>()));
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    if (on[ct]) acc[ct][dt] = Op<T>::mma(u.v, pf[ct], acc[ct][dt] * alpha[ct]);
            }
        }
        __syncthreads();                                     // every wave has read the image: the next chunk's may be written
    }

    // the four waves' partials of each column tile become the workgroup's, as in the decode kernel
    float* red = reinterpret_cast<float*>(smem);             // [wave][row][DP]
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        if (gq == 0) wm[w][r] = m[ct], wl[w][r] = l[ct];
        __syncthreads();
        float M = wm[0][r];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) M = fmaxf(M, wm[ww][r]);
        const float sc = __builtin_amdgcn_exp2f(m[ct] - (M == -INFINITY ? 0.f : M));          // a wave without a live key: 0
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            *reinterpret_cast<f32x4*>(red + ((w * RB + r) * DP + 16 * dt + 4 * gq)) = acc[ct][dt] * sc;
        __syncthreads();
        for (int i = tid; i < RB * DP; i += NT) {
            const int hd = i / DP, col = i % DP, rho = row0 + RB * ct + hd;
            float s = 0.f;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) s += red[(ww * RB + hd) * DP + col];
            if (rho < nrows && col < D) part[((((int64_t)bg * qpk + rho % qpk) * ts + rho / qpk) * nspan + sp) * (D + 2) + 2 + col] = s;
        }
        const int rho = row0 + RB * ct + tid;
        if (tid < RB && rho < nrows) {
            float Mh = wm[0][tid];
#pragma unroll
            for (int ww = 1; ww < NW; ++ww) Mh = fmaxf(Mh, wm[ww][tid]);
            const float Ms = Mh == -INFINITY ? 0.f : Mh;
            float s = 0.f;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) s += wl[ww][tid] * __builtin_amdgcn_exp2f(wm[ww][tid] - Ms);
            float* out = part + ((((int64_t)bg * qpk + rho % qpk) * ts + rho / qpk) * nspan + sp) * (D + 2);
            out[0] = Mh;
            out[1] = s;
        }
        __syncthreads();                                     // wm, wl and red are free for the next column tile
    }
}

struct BlockCall {
    const uint16_t *q, *k, *v;
    Strides3 qs, ks, vs;
    void *state, *o;
    float *lse, *ws;
    int B, H, Hkv, T, D, max_len;
    float c2;
    hipStream_t stream;
};

static int span_count(int max_len) { return (int)((cap_of(max_len) / CHUNK + SPAN - 1) / SPAN); }

template <typename T, int NS, int ROWS>
static int launch_block_attend(const BlockCall& a, const uint16_t* kc, const uint16_t* vc, float* part, int* nspans, int t0, int ts) {
    auto kern = sm_block_attend_kernel<T, NS, ROWS>;
    constexpr int lds = block_lds<32 * NS, ROWS>();
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int qpk = a.H / a.Hkv;
    const dim3 grid((unsigned)span_count(a.max_len), (unsigned)(a.B * a.Hkv), (unsigned)((ts * qpk + ROWS - 1) / ROWS));
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, a.stream, a.q, a.qs, reinterpret_cast<const int*>(a.state), kc, vc, part, nspans,
                       a.Hkv, qpk, a.D, a.max_len, cap_of(a.max_len), a.T, t0, ts, a.c2);
    return (int)hipGetLastError();
}

template <typename T> static int append_attend_block_t(const BlockCall& a) {
    const int64_t cap = cap_of(a.max_len);
    const int nspan = span_count(a.max_len), tsmax = a.T < TOKENS ? a.T : TOKENS;
    int* hdr = reinterpret_cast<int*>(a.state);
    uint16_t* kc = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.state) + HDR_BYTES);
    uint16_t* vc = kc + (int64_t)a.B * a.Hkv * cap * a.D;
    float* part = a.ws;
    int* nspans = reinterpret_cast<int*>(part + (int64_t)a.B * a.H * tsmax * nspan * (a.D + 2));
    hipLaunchKernelGGL(sm_append_kernel, dim3((unsigned)a.T, (unsigned)(a.B * a.Hkv), 2), dim3(64), 0, a.stream, a.k, a.v, a.ks, a.vs, hdr,
                       kc, vc, a.Hkv, a.T, a.D, a.max_len, cap);
    const int cthreads = a.D <= 64 ? 64 : (a.D <= 128 ? 128 : 256);
    for (int t0 = 0; t0 < a.T; t0 += TOKENS) {
        const int ts = a.T - t0 < TOKENS ? a.T - t0 : TOKENS;
        int rc;
        if (a.D <= 32) rc = launch_block_attend<T, 1, BLOCK_ROWS>(a, kc, vc, part, nspans, t0, ts);
        else if (a.D <= 64) rc = launch_block_attend<T, 2, BLOCK_ROWS>(a, kc, vc, part, nspans, t0, ts);
        else if (a.D <= 128) rc = launch_block_attend<T, 4, BLOCK_ROWS>(a, kc, vc, part, nspans, t0, ts);
        else rc = launch_block_attend<T, 8, BLOCK_ROWS_D256>(a, kc, vc, part, nspans, t0, ts);
        if (rc != 0) return rc;
        hipLaunchKernelGGL((sm_combine_kernel<T>), dim3((unsigned)(a.B * a.H), (unsigned)ts), dim3(cthreads), 0, a.stream, hdr, part, nspans,
                           reinterpret_cast<T*>(a.o), a.lse, a.D, a.max_len, a.T, t0, ts, nspan, (int)(t0 + ts == a.T));
    }
    return (int)hipGetLastError();
}

// the decode route's shapes; the tiles of a slice are grid.z, which bounds the query heads per KV head
static bool block_shape_ok(int B, int H, int Hkv, int T, int D, int max_len) {
    return T > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && D >= 8 && D % 8 == 0 && (int64_t)B * H <= 65535 &&
           (int64_t)TOKENS * (H / Hkv) / BLOCK_ROWS_D256 <= 65535 &&
           fastmax_hip_kv_decode_state_bytes(B, Hkv, D, max_len, FASTMAX_BF16) != 0;
}

}  // namespace smkv
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::smkv;

extern "C" {

size_t fastmax_hip_softmax_kv_block_workspace(int B, int H, int Hkv, int T, int D, int max_len) {
    if (!block_shape_ok(B, H, Hkv, T, D, max_len)) return 0;
    return sizeof(float) * (size_t)B * H * (size_t)(T < TOKENS ? T : TOKENS) * ((size_t)span_count(max_len) * (D + 2) + 1);
}

int fastmax_hip_softmax_kv_append_attend_block(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                               const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B,
                                               int H, int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !state || !o || !workspace) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!block_shape_ok(B, H, Hkv, T, D, max_len) || !std::isfinite(scale)) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(k, k_strides) || !pieces(v, v_strides) || reinterpret_cast<uintptr_t>(state) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(o) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(lse) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_softmax_kv_block_workspace(B, H, Hkv, T, D, max_len)) return FASTMAX_E_WORKSPACE;
    BlockCall a;
    a.q = reinterpret_cast<const uint16_t*>(q), a.k = reinterpret_cast<const uint16_t*>(k), a.v = reinterpret_cast<const uint16_t*>(v);
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.state = state, a.o = o, a.lse = lse, a.ws = reinterpret_cast<float*>(workspace);
    a.B = B, a.H = H, a.Hkv = Hkv, a.T = T, a.D = D, a.max_len = max_len;
    a.c2 = scale * 1.4426950408889634f;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? append_attend_block_t<bf16_t>(a) : append_attend_block_t<f16_t>(a);
}

}  // extern "C"
