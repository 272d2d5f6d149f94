// Softmax KV-cache decode on 8-bit rows (include/fastmax_hip_kv_fp8.h): the route of softmax_kv_decode.hip -- the same header words,
// chunks, workgroups, workspace and combine kernel (softmax_kv_common.h) -- on a cache that holds every K and V row as D OCP e4m3
// codes and one float32 scale s = 2^e, the smallest power of two with max |row| <= 448 s.  2 D + 8 bytes per position and KV head
// where the 16-bit cache streams 4 D; the products stay 16-bit matrix-core products, since a code (3 mantissa bits, 2^-9 .. 448) is
// exact in bf16 and in fp16.
//
//     o_i = sum_{j <= n_i} p_j vs_j Vc_j / sum_{j <= n_i} p_j,   p_j = exp(scale ks_j (q_i . Kc_j) - max_j),   n_i = len + i
//
// quantise one wave per (new token, (b, g)): lanes 0 .. 31 take the K row, lanes 32 .. 63 the V row, 16 bytes (8 elements) of the
//          strided input each.  |x| is reduced over the half wave by five butterflies; e comes from the float32 exponent and
//          mantissa of the maximum (v_frexp_*); x 2^-e is exact (v_ldexp_f32) and v_cvt_pk_fp8_f32 rounds it to nearest-even, two
//          codes an instruction; a lane stores its 8 codes as one 8-byte word and lane 0 of each half the scale word.  The same
//          kernel serves append (rows len .. len + T - 1; the header is only read, the guard as in sm_append_kernel) and load
//          (rows 0 .. T - 1 of an empty cache; the header is not read, len = T is written).
// attend   sm_attend_kernel's decomposition, so a row's bits are as independent of B, T, max_len, strides and replay as there:
//          one workgroup (4 waves) per (chunk, (b, g), new token x block of <= 16 query heads), wave w on positions 32 w .. + 31.
//   K     a lane fetches the 8 codes of its A-operand fragment (row lane & 15, columns 32 s + 8 (lane >> 4) ..+7) as ONE 8-byte
//         load straight from the cache and widens them in registers: v_cvt_pk_f32_fp8 (2 codes each, subnormal codes included)
//         and the pack to 16 bits, both exact.  No LDS, half the bytes in flight per lane of the 16-bit route.
//   S^T   = Kc Q^T, float32.  A lane holds keys 4 (lane >> 4) + {0..3} of each 16-key tile for head lane & 15: their K scales are
//         one 16-byte load per tile (the scale arrays are chunk-aligned), and x = s ks_j scale log2 e.  A tile that reaches past n
//         loads its scale words one by one under the same selection as the scores, so a dead word is never read.
//   P     p_j = exp2(x_j - m) enters l as it is; p_j vs_j is what is rounded to the 16-bit B operand of O^T += Vc^T P^T.  vs_j is
//         a power of two, so that rounding has the relative error of rounding p_j alone (down to the dtype's subnormals).
//   V     WIDENED ON THE WAY IN: a thread loads 8 codes (8 bytes), widens them and writes one 16-byte piece of the 16-bit image
//         (rows padded to 2 DP + 64 bytes) that ds_read_b64_tr_b16 hands back transposed, as in the 16-bit route.  The other
//         choice, a byte image read back with ds_read_b64_tr_b8 and widened after the read, would halve the image (128 (DP + 64)
//         bytes) and the ds_write traffic, but not the allocation: the four waves' O^T (4 x 16 heads x DP floats = 256 DP bytes)
//         are merged in the same LDS and already fill what the 16-bit rows take, so occupancy would not move.  It would also put
//         the conversions (4 v_cvt + 4 packs per 8 codes, the same count either way) behind the LDS read on the path to the
//         second product instead of under the global loads' latency, and a lane's 16-byte piece writes keep the conflict-free
//         pattern of the 16-bit route (consecutive lanes, consecutive pieces; the 64-byte pad turns the transposed reads' 4 rows
//         x 32 bytes onto distinct banks) where byte rows of DP + pad bytes would need a new pad per head size.
//         Pieces of positions past n and of columns past D are written as zeros and never loaded.
//   wave / merge / partials   as in softmax_kv_decode.hip.
// combine  sm_combine_kernel; its last launch advances the header.
// LDS of attend: 128 (2 DP + 64) + 512 bytes: DP = 32: 16,896; 64: 25,088; 128: 41,472; 256: 74,240.
// Registers (vector + accumulator file, either dtype): DP = 32: 48 + 6; 64: 62 + 12; 128: 88 + 24; 256: 138 + 48; no spills.  The
// quantise kernel takes 14.
#include "../../include/fastmax_hip_kv_fp8.h"
#include "softmax_kv_common.h"

namespace fastmax {
namespace smkv {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 e4m3 codes (two words, ascending address) -> the 16-bit operand of the same 8 values; every step is exact
template <typename T> __device__ __forceinline__ typename Op<T>::v8 widen8(uint32_t lo, uint32_t hi) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    const float x[8] = {a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    return Op<T>::round8(x);
}

template <typename T> __device__ __forceinline__ void unpack8(uint4 raw, float* x);
template <> __device__ __forceinline__ void unpack8<bf16_t>(uint4 raw, float* x) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) x[2 * i] = __uint_as_float(w[i] << 16), x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
}
template <> __device__ __forceinline__ void unpack8<f16_t>(uint4 raw, float* x) {
    const h8 h = __builtin_bit_cast(h8, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (float)h[i];
}

// e of the row's scale 2^e: the smallest integer with amax <= 448 * 2^e, in -126 .. 127; 0 for an all-zero row
__device__ __forceinline__ int scale_exp(float amax) {
    if (amax == 0.f) return 0;
    const int x = __builtin_amdgcn_frexp_expf(amax);
    const int e = __builtin_amdgcn_frexp_mantf(amax) <= 0.875f ? x - 9 : x - 8;
    return e < -126 ? -126 : (e > 127 ? 127 : e);
}

// grid: (T, B * Hkv); block: 64 = the K row and the V row of one position.  LOAD: rows 0 .. T - 1, the header is not read and
// len = T is written; otherwise rows len .. len + T - 1 unless that passes max_len, and the header is only read.
template <typename T, bool LOAD>
__global__ __launch_bounds__(64) void fp8_quantise_kernel(const uint16_t* k, const uint16_t* v, Strides3 ks, Strides3 vs, int* hdr,
                                                          uint8_t* kc, uint8_t* vc, float* ksc, float* vsc, int Hkv, int Tn, int D,
                                                          int max_len, int64_t cap) {
    int len = 0;
    if (LOAD) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) hdr[FASTMAX_KV_LEN] = Tn;
    } else {
        len = hdr[FASTMAX_KV_LEN];
        if (overflows(len, Tn, max_len)) return;
    }
    const int t = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv, l = threadIdx.x & 31;
    const bool isv = threadIdx.x >= 32, live = 8 * l < D;
    const Strides3 s = isv ? vs : ks;
    const uint16_t* src = (isv ? v : k) + (int64_t)b * s.sb + (int64_t)g * s.sh + (int64_t)t * s.sn;
    const int64_t row = (int64_t)bg * cap + len + t;
    float x[8];
    unpack8<T>(live ? reinterpret_cast<const uint4*>(src)[l] : uint4{0, 0, 0, 0}, x);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));          // over the half wave of this row
    const int e = scale_exp(amax);
    int w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * i], -e), ldexpf(x[4 * i + 1], -e), 0, false);
        w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * i + 2], -e), ldexpf(x[4 * i + 3], -e), w[i], true);
    }
    if (live) reinterpret_cast<uint2*>((isv ? vc : kc) + row * D)[l] = uint2{(uint32_t)w[0], (uint32_t)w[1]};
    if (l == 0) (isv ? vsc : ksc)[row] = ldexpf(1.f, e);
}

// the scale words of keys jb .. jb + 3 of the chunk: one 16-byte load when all four are live, else each under the selection
__device__ __forceinline__ void scales4(const float* __restrict__ sc, int jb, int jn, float* out) {
    if (jb + 3 <= jn) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(sc + jb);
        out[0] = a[0], out[1] = a[1], out[2] = a[2], out[3] = a[3];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = jb + i <= jn ? sc[jb + i] : 0.f;
    }
}

// workspace: part (B * H, ts, nchunk, D + 2) floats = (m, l, numerator), then nchunks (B * H, ts) ints
// grid: (cap / CHUNK, B * Hkv, ts * ceil(qpk / RB)); block: NT; dynamic LDS: attend_lds<32 NS>()
template <typename T, int NS>
__global__ __launch_bounds__(NT) void fp8_attend_kernel(const uint16_t* __restrict__ q, Strides3 qs, const int* __restrict__ hdr,
                                                        const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                        const float* __restrict__ ksc, const float* __restrict__ vsc,
                                                        float* __restrict__ part, int* __restrict__ nchunks, int Hkv, int qpk, int D,
                                                        int max_len, int64_t cap, int Tn, int t0, int ts, float c2) {
    typedef typename Op<T>::v8 V8;
    constexpr int DP = 32 * NS, DT = DP / 16, PPV = CHUNK * (DP / 8) / NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wm[NW][RB], wl[NW][RB];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, gq = lane >> 4;
    const int nhb = (qpk + RB - 1) / RB;
    const int c = blockIdx.x, bg = blockIdx.y, b = bg / Hkv, g = bg % Hkv, ti = blockIdx.z / nhb, h0 = (blockIdx.z % nhb) * RB;
    const int nr = qpk - h0 < RB ? qpk - h0 : RB;            // live query heads of this block
    const int nchunk = gridDim.x;
    const int64_t head0 = (int64_t)bg * qpk + h0;            // b * H + g * qpk + h0
    const int len = hdr[FASTMAX_KV_LEN];
    const bool over = overflows(len, Tn, max_len);
    const int64_t n = (int64_t)len + t0 + ti;                // this token's position
    if (c == 0 && tid < nr) nchunks[(head0 + tid) * ts + ti] = over ? 0 : (int)(n / CHUNK) + 1;
    const int64_t j0 = (int64_t)c * CHUNK;
    if (over || j0 > n) return;
    const uint8_t* kbase = kc + ((int64_t)bg * cap + j0) * D;
    const uint8_t* vbase = vc + ((int64_t)bg * cap + j0) * D;
    const int jn = (int)(n - j0 < CHUNK ? n - j0 : CHUNK - 1);          // positions 0 .. jn of the chunk are live

    // K operands of this wave (8 codes a load, widened in registers) and the Q operands, from global memory
    V8 kf[2][NS], qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int col = 32 * s + 8 * gq;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = WPOS * w + 16 * t + r;
            const uint2 x = (j <= jn && col < D) ? *reinterpret_cast<const uint2*>(kbase + (int64_t)j * D + col) : uint2{0, 0};
            kf[t][s] = widen8<T>(x.x, x.y);
        }
        const uint4 x = (r < nr && col < D) ? *reinterpret_cast<const uint4*>(q + (int64_t)b * qs.sb + (int64_t)(g * qpk + h0 + r) * qs.sh +
                                                                              (int64_t)(t0 + ti) * qs.sn + col)
                                            : uint4{0, 0, 0, 0};
        qf[s] = __builtin_bit_cast(V8, x);
    }
    // the scales of the keys this lane will hold in S^T: 4 (lane >> 4) + {0..3} of each tile
    float ksl[8], vsl[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int jb = WPOS * w + 16 * t + 4 * gq;
        scales4(ksc + (int64_t)bg * cap + j0, jb, jn, ksl + 4 * t);
        scales4(vsc + (int64_t)bg * cap + j0, jb, jn, vsl + 4 * t);
    }
    // the chunk's V rows, widened, into LDS
#pragma unroll
    for (int u = 0; u < PPV; ++u) {
        const int i = tid + NT * u, row = i / (DP / 8), pc = i % (DP / 8);
        const uint2 x = (row <= jn && 8 * pc < D) ? *reinterpret_cast<const uint2*>(vbase + (int64_t)row * D + 8 * pc) : uint2{0, 0};
        *reinterpret_cast<V8*>(smem + row * v_row<DP>() + 16 * pc) = widen8<T>(x.x, x.y);
    }

    // S^T of the wave's 32 positions, each score times its key's scale, masked by selection; the wave's maximum per head
    float x[8], mw = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) st = Op<T>::mma(kf[t][s], qf[s], st);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = WPOS * w + 16 * t + 4 * gq + i;
            x[4 * t + i] = j <= jn ? st[i] * ksl[4 * t + i] * c2 : -INFINITY;
            mw = fmaxf(mw, x[4 * t + i]);
        }
    }
    mw = fmaxf(mw, __shfl_xor(mw, 16, 64));
    mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
    const float msafe = mw == -INFINITY ? 0.f : mw;          // a wave with no live position: every p is exp2(-inf) = 0
    float lw = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = __builtin_amdgcn_exp2f(x[i] - msafe);
        lw += x[i];
        x[i] *= vsl[i];                                      // the V scale rides on p into the second product
    }
    lw += __shfl_xor(lw, 16, 64);
    lw += __shfl_xor(lw, 32, 64);
    const V8 pf = Op<T>::round8(x);
    if (gq == 0) wm[w][r] = mw, wl[w][r] = lw;
    __syncthreads();                                         // the V image and the waves' m, l are written

    // O^T = V^T P^T: tile dt holds columns 16 dt + 4 gq + {0..3} of head r
    f32x4 acc[DT];
    {
        const int qq = r >> 2, pp = r & 3;
        const char* va = smem + (WPOS * w + 4 * gq + qq) * v_row<DP>() + 8 * pp;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            union { V8 v; s16x4 h[2]; } u;
            u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt));
            u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 32 * dt + 16 * v_row<DP>()));
            acc[dt] = Op<T>::mma(u.v, pf, f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    float M = wm[0][r];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) M = fmaxf(M, wm[ww][r]);          // finite: position j0 of wave 0 is live
    const float sc = __builtin_amdgcn_exp2f(mw - M);
    __syncthreads();                                         // every wave has read its V rows: the image becomes the four O^T
    float* red = reinterpret_cast<float*>(smem);             // [wave][head][DP]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<f32x4*>(red + ((w * RB + r) * DP + 16 * dt + 4 * gq)) = acc[dt] * sc;
    __syncthreads();

    float* out = part + (((head0 * ts + ti) * nchunk) + c) * (D + 2);
    const int64_t head_stride = (int64_t)ts * nchunk * (D + 2);
    for (int i = tid; i < RB * DP; i += NT) {
        const int hd = i / DP, col = i % DP;
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += red[(ww * RB + hd) * DP + col];
        if (hd < nr && col < D) out[hd * head_stride + 2 + col] = s;
    }
    if (tid < nr) {
        float Mh = wm[0][tid];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) Mh = fmaxf(Mh, wm[ww][tid]);
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += wl[ww][tid] * __builtin_amdgcn_exp2f(wm[ww][tid] - Mh);
        out[tid * head_stride] = Mh;
        out[tid * head_stride + 1] = s;
    }
}

// the four arrays behind the header
struct Cache {
    uint8_t *kc, *vc;
    float *ksc, *vsc;
    int64_t cap;
    Cache(void* state, int B, int Hkv, int D, int max_len) : cap(cap_of(max_len)) {
        const int64_t rows = (int64_t)B * Hkv * cap;
        kc = reinterpret_cast<uint8_t*>(state) + HDR_BYTES;
        vc = kc + rows * D;
        ksc = reinterpret_cast<float*>(vc + rows * D);
        vsc = ksc + rows;
    }
};

struct Call {
    const uint16_t *q, *k, *v;
    Strides3 qs, ks, vs;
    void *state, *o;
    float *lse, *ws;
    int B, H, Hkv, T, D, max_len;
    float c2;
    hipStream_t stream;
};

template <typename T, bool LOAD> static void launch_quantise(const Call& a, const Cache& c) {
    hipLaunchKernelGGL((fp8_quantise_kernel<T, LOAD>), dim3((unsigned)a.T, (unsigned)(a.B * a.Hkv)), dim3(64), 0, a.stream, a.k, a.v, a.ks,
                       a.vs, reinterpret_cast<int*>(a.state), c.kc, c.vc, c.ksc, c.vsc, a.Hkv, a.T, a.D, a.max_len, c.cap);
}

template <typename T, int NS> static int launch_attend(const Call& a, const Cache& c, float* part, int* nchunks, int t0, int ts) {
    auto kern = fp8_attend_kernel<T, NS>;
    constexpr int lds = attend_lds<32 * NS>();
    static bool configured = false;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured = true;
    }
    const int qpk = a.H / a.Hkv, nhb = (qpk + RB - 1) / RB;
    const dim3 grid((unsigned)(c.cap / CHUNK), (unsigned)(a.B * a.Hkv), (unsigned)(ts * nhb));
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, a.stream, a.q, a.qs, reinterpret_cast<const int*>(a.state), c.kc, c.vc, c.ksc, c.vsc, part,
                       nchunks, a.Hkv, qpk, a.D, a.max_len, c.cap, a.T, t0, ts, a.c2);
    return (int)hipGetLastError();
}

template <typename T> static int append_attend_t(const Call& a) {
    const Cache c(a.state, a.B, a.Hkv, a.D, a.max_len);
    const int nchunk = (int)(c.cap / CHUNK), tsmax = a.T < SLICE ? a.T : SLICE;
    float* part = a.ws;
    int* nchunks = reinterpret_cast<int*>(part + (int64_t)a.B * a.H * tsmax * nchunk * (a.D + 2));
    launch_quantise<T, false>(a, c);
    const int cthreads = a.D <= 64 ? 64 : (a.D <= 128 ? 128 : 256);
    for (int t0 = 0; t0 < a.T; t0 += SLICE) {
        const int ts = a.T - t0 < SLICE ? a.T - t0 : SLICE;
        int rc;
        if (a.D <= 32) rc = launch_attend<T, 1>(a, c, part, nchunks, t0, ts);
        else if (a.D <= 64) rc = launch_attend<T, 2>(a, c, part, nchunks, t0, ts);
        else if (a.D <= 128) rc = launch_attend<T, 4>(a, c, part, nchunks, t0, ts);
        else rc = launch_attend<T, 8>(a, c, part, nchunks, t0, ts);
        if (rc != 0) return rc;
        hipLaunchKernelGGL((sm_combine_kernel<T>), dim3((unsigned)(a.B * a.H), (unsigned)ts), dim3(cthreads), 0, a.stream,
                           reinterpret_cast<int*>(a.state), part, nchunks, reinterpret_cast<T*>(a.o), a.lse, a.D, a.max_len, a.T, t0, ts,
                           nchunk, (int)(t0 + ts == a.T));
    }
    return (int)hipGetLastError();
}

static bool shape_ok(int B, int H, int Hkv, int T, int D, int max_len) {
    return T > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && (int64_t)B * H <= 65535 && fastmax_hip_kv_fp8_state_bytes(B, Hkv, D, max_len) != 0;
}

}  // namespace smkv
}  // namespace fastmax

using namespace fastmax;
using namespace fastmax::smkv;

extern "C" {

size_t fastmax_hip_kv_fp8_state_bytes(int B, int Hkv, int D, int max_len) {
    if (B <= 0 || Hkv <= 0 || D <= 0 || D % 16 != 0 || D > FASTMAX_KV_MAX_D || max_len <= 0 || (int64_t)B * Hkv > 65535) return 0;
    return (size_t)HDR_BYTES + (size_t)B * Hkv * (size_t)cap_of(max_len) * (2 * (size_t)D + 2 * sizeof(float));
}

int fastmax_hip_kv_fp8_load(const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides, void* state, int B, int Hkv,
                            int T, int D, int max_len, int dtype, void* stream) {
    if (!k || !v || !k_strides || !v_strides || !state) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (T <= 0 || fastmax_hip_kv_fp8_state_bytes(B, Hkv, D, max_len) == 0 || T > max_len) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(k, k_strides) || !pieces(v, v_strides) || reinterpret_cast<uintptr_t>(state) % 16 != 0) return FASTMAX_E_ALIGNMENT;
    Call a{};
    a.k = reinterpret_cast<const uint16_t*>(k), a.v = reinterpret_cast<const uint16_t*>(v);
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.state = state, a.B = B, a.Hkv = Hkv, a.T = T, a.D = D, a.max_len = max_len;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    const Cache c(state, B, Hkv, D, max_len);
    if (dtype == FASTMAX_BF16) launch_quantise<bf16_t, true>(a, c);
    else launch_quantise<f16_t, true>(a, c);
    return (int)hipGetLastError();
}

size_t fastmax_hip_kv_fp8_workspace(int B, int H, int Hkv, int T, int D, int max_len) {
    if (!shape_ok(B, H, Hkv, T, D, max_len)) return 0;
    return sizeof(float) * (size_t)B * H * (size_t)(T < SLICE ? T : SLICE) * ((size_t)(cap_of(max_len) / CHUNK) * (D + 2) + 2);
}

int fastmax_hip_softmax_kv_fp8_append_attend(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                                             const void* v, const int64_t* v_strides, void* state, void* o, float* lse, int B, int H,
                                             int Hkv, int T, int D, int max_len, int dtype, float scale, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !q_strides || !k_strides || !v_strides || !state || !o || !workspace) return FASTMAX_E_NULL;
    if (dtype != FASTMAX_BF16 && dtype != FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!shape_ok(B, H, Hkv, T, D, max_len) || !std::isfinite(scale)) return FASTMAX_E_BAD_SHAPE;
    if (!pieces(q, q_strides) || !pieces(k, k_strides) || !pieces(v, v_strides) || reinterpret_cast<uintptr_t>(state) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(o) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(lse) % 4 != 0)
        return FASTMAX_E_ALIGNMENT;
    if (workspace_bytes < fastmax_hip_kv_fp8_workspace(B, H, Hkv, T, D, max_len)) return FASTMAX_E_WORKSPACE;
    Call a;
    a.q = reinterpret_cast<const uint16_t*>(q), a.k = reinterpret_cast<const uint16_t*>(k), a.v = reinterpret_cast<const uint16_t*>(v);
    a.qs = Strides3{q_strides[0], q_strides[1], q_strides[2]};
    a.ks = Strides3{k_strides[0], k_strides[1], k_strides[2]};
    a.vs = Strides3{v_strides[0], v_strides[1], v_strides[2]};
    a.state = state, a.o = o, a.lse = lse, a.ws = reinterpret_cast<float*>(workspace);
    a.B = B, a.H = H, a.Hkv = Hkv, a.T = T, a.D = D, a.max_len = max_len;
    a.c2 = scale * 1.4426950408889634f;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    return dtype == FASTMAX_BF16 ? append_attend_t<bf16_t>(a) : append_attend_t<f16_t>(a);
}

}  // extern "C"
