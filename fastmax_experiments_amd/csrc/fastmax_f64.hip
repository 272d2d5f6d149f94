// float64 fastmax: f(Q K^T) V tiles and their backward on the f64 matrix instruction (v_mfma_f64_16x16x4_f64), gfx950.
//
// Every product, polynomial, sum and division is a double; nothing is held in float.  One wave (64 lanes) owns one 16-row tile
// and walks the other sequence in 16-row tiles; a workgroup is one wave, so there is no LDS and no barrier.  No atomics: every
// sum has a fixed order that depends on the row's own sequence only, so a row's bits do not depend on B, on its batch index or
// on the inputs' strides.  Masked tiles above the diagonal are not visited.
//
// Layouts of the instruction (D = A B + C, 16 x 16 x 4, lane = 0..63, c = lane & 15, r4 = lane >> 4):
//   A: one double per lane, A[row c][k r4];  B: one double per lane, B[k r4][col c];  C / D: four doubles, D[row r4 + 4 i][col c].
// The score tile is computed TRANSPOSED in the forward and in the dQ kernel (keys as rows, the wave's 16 queries as columns):
// its result registers i = 0..3 then hold keys r4 + 4 i of query c, which is the B operand of the next product
// O^T += V^T f(S^T) for the four keys 4 i .. 4 i + 3 after the keys of a tile are taken in the order (r4 + 4 i) -- f(S) never
// goes through memory, and the denominator is the column sum of the same registers.  The dK / dV kernel keeps the score tile
// upright (queries as rows, the wave's 16 keys as columns) for the same reason.  Head sizes are padded to a multiple of 4 (score
// products) or 16 (output columns) with zeros in registers; memory is read and written at d < D only.
//
// Instantiations: DB = 1, 2, 4, 8, 16 blocks of 16 output columns (D <= 16, 32, 64, 128, 256).  The whole range 1..256 runs on
// the matrix instruction -- there is no vector-ALU double instantiation.  At DB = 16 the dK / dV kernel holds K and V of its tile
// (256 VGPRs) and therefore accumulates 8 of the 16 column blocks per wave: two waves per key tile (blockIdx.z) recompute the
// scores and own one half of the columns each.
#include "fastmax_common.h"

namespace fastmax {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

template <int P> __device__ __forceinline__ double fpoly(double s) {
    if constexpr (P == 1) return 1.0 + s;
    else return 1.0 + s + 0.5 * s * s;
}
template <int P> __device__ __forceinline__ double fprime(double s) {
    if constexpr (P == 1) return 1.0;
    else return 1.0 + s;
}

// element (row, d) of one head's (n, D) rows, zero outside
__device__ __forceinline__ double ldz(const double* base, int64_t sn, int row, int n, int d, int D) {
    return (row < n && d < D) ? base[(int64_t)row * sn + d] : 0.0;
}

struct Head {
    const double* p;
    int64_t sb, sh, sn;
    __device__ __forceinline__ const double* at(int b, int h) const { return p + (int64_t)b * sb + (int64_t)h * sh; }
};

// the 16 x 16 tile rows(16 x D) cols(16 x D)^T with `rows` streamed from memory and `cols` held in registers (operand B):
// result register i = row r4 + 4 i of the streamed tile, column c of the held one
template <int DB>
__device__ __forceinline__ d4 tile_product(const double* rows, int64_t sn, int row0, int n, const double (&held)[4 * DB], int D, int c, int r4) {
    d4 s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int blk = 0; blk < DB; ++blk)
        if (16 * blk < D) {          // four steps per (uniform) branch, so that their loads are in flight together
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = ldz(rows, sn, row0 + c, n, 16 * blk + 4 * i + r4, D);
#pragma unroll
            for (int i = 0; i < 4; ++i) s = mfma(x[i], held[4 * blk + i], s);
        }
    return s;
}

// acc^T (D x 16) += rows^T (D x 16 streamed rows) w (16 streamed rows x 16 columns), w in the score tile's register order;
// column blocks db0 .. db0 + NB - 1
template <int NB>
__device__ __forceinline__ void accumulate(d4 (&acc)[NB], const double* rows, int64_t sn, int row0, int n, const double (&w)[4], int D, int db0, int c,
                                           int r4) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
        if (16 * (db0 + j) < D) {
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = ldz(rows, sn, row0 + 4 * i + r4, n, 16 * (db0 + j) + c, D);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j] = mfma(x[i], w[i], acc[j]);
        }
}

// sum over the four lanes that hold the same column c (lanes c, c + 16, c + 32, c + 48): the same bits in all four
__device__ __forceinline__ double column_sum(double x) {
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}

// ---- forward: o (B,H,Nq,D), g (B,H,Nq) ---------------------------------------------------------------------------------------
template <int DB, int P, bool CAUSAL>
__global__ __launch_bounds__(64) void fwd_f64_kernel(Head q, Head k, Head v, double* __restrict__ o, double* __restrict__ g, int H, int Nq, int Nk,
                                                     int D, double a, double gadd) {
    const int lane = threadIdx.x, c = lane & 15, r4 = lane >> 4;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int qt = CAUSAL ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;          // masked: the longest tiles start first
    const double *qb = q.at(b, h), *kb = k.at(b, h), *vb = v.at(b, h);
    const int qrow = qt * 16 + c;

    double qr[4 * DB];
#pragma unroll
    for (int st = 0; st < 4 * DB; ++st) qr[st] = ldz(qb, q.sn, qrow, Nq, 4 * st + r4, D);
    d4 acc[DB];
#pragma unroll
    for (int j = 0; j < DB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    double gs = 0.0;

    const int nkt = CAUSAL ? qt + 1 : (Nk + 15) / 16;
    for (int kt = 0; kt < nkt; ++kt) {
        const d4 s = tile_product<DB>(kb, k.sn, kt * 16, Nk, qr, D, c, r4);
        double w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = kt * 16 + r4 + 4 * i;
            const bool on = key < Nk && (!CAUSAL || key <= qrow);
            w[i] = on ? fpoly<P>(a * s[i]) : 0.0;
            gs += w[i];
        }
        accumulate<DB>(acc, vb, v.sn, kt * 16, Nk, w, D, 0, c, r4);
    }
    const double gt = column_sum(gs) + gadd;
    if (qrow >= Nq) return;
    const int64_t row = (int64_t)bh * Nq + qrow;
    if (g && r4 == 0) g[row] = gt;
#pragma unroll
    for (int j = 0; j < DB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = 16 * j + r4 + 4 * i;
            if (d < D) o[row * D + d] = acc[j][i] / gt;
        }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// rowdot[b,h,i] = sum_d grad_o[i,d] o[i,d], d ascending; one lane per row
__global__ __launch_bounds__(256) void rowdot_f64_kernel(Head go, const double* __restrict__ o, double* __restrict__ rowdot, int H, int Nq, int D) {
    const int i = blockIdx.x * 256 + threadIdx.x, bh = blockIdx.y;
    if (i >= Nq) return;
    const double* gr = go.at(bh / H, bh % H) + (int64_t)i * go.sn;
    const double* orow = o + ((int64_t)bh * Nq + i) * D;
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += gr[d] * orow[d];
    rowdot[(int64_t)bh * Nq + i] = s;
}

// dq per 16-query tile: S^T and dP^T tiles (keys as rows), dS^T is the B operand of dq^T += K^T dS^T
template <int DB, int P, bool CAUSAL>
__global__ __launch_bounds__(64) void bwd_dq_f64_kernel(Head q, Head k, Head v, Head go, const double* __restrict__ g, const double* __restrict__ rowdot,
                                                        double* __restrict__ dq, int H, int Nq, int Nk, int D, double a) {
    const int lane = threadIdx.x, c = lane & 15, r4 = lane >> 4;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int qt = CAUSAL ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;
    const double *qb = q.at(b, h), *kb = k.at(b, h), *vb = v.at(b, h), *gob = go.at(b, h);
    const int qrow = qt * 16 + c;
    const int64_t row = (int64_t)bh * Nq + qrow;

    double qr[4 * DB], gor[4 * DB];
#pragma unroll
    for (int st = 0; st < 4 * DB; ++st) {
        qr[st] = ldz(qb, q.sn, qrow, Nq, 4 * st + r4, D);
        gor[st] = ldz(gob, go.sn, qrow, Nq, 4 * st + r4, D);
    }
    const double gi = qrow < Nq ? g[row] : 1.0, ci = qrow < Nq ? rowdot[row] : 0.0;
    d4 acc[DB];
#pragma unroll
    for (int j = 0; j < DB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};

    const int nkt = CAUSAL ? qt + 1 : (Nk + 15) / 16;
    for (int kt = 0; kt < nkt; ++kt) {
        const d4 s = tile_product<DB>(kb, k.sn, kt * 16, Nk, qr, D, c, r4);
        const d4 dp = tile_product<DB>(vb, v.sn, kt * 16, Nk, gor, D, c, r4);
        double ds[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = kt * 16 + r4 + 4 * i;
            const bool on = key < Nk && (!CAUSAL || key <= qrow);
            ds[i] = on ? fprime<P>(a * s[i]) * ((dp[i] - ci) / gi) : 0.0;
        }
        accumulate<DB>(acc, kb, k.sn, kt * 16, Nk, ds, D, 0, c, r4);
    }
    if (qrow >= Nq) return;
#pragma unroll
    for (int j = 0; j < DB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = 16 * j + r4 + 4 * i;
            if (d < D) dq[row * D + d] = a * acc[j][i];
        }
}

// dk, dv per 16-key tile: S and dP tiles upright (queries as rows), dS and f(S) / g are the B operands of
// dk^T += Q^T dS and dv^T += dO^T (f(S) / g); column blocks blockIdx.z * NB .. + NB - 1
template <int DB, int NB, int P, bool CAUSAL>
__global__ __launch_bounds__(64) void bwd_dkdv_f64_kernel(Head q, Head k, Head v, Head go, const double* __restrict__ g,
                                                          const double* __restrict__ rowdot, double* __restrict__ dk, double* __restrict__ dv, int H,
                                                          int Nq, int Nk, int D, double a) {
    const int lane = threadIdx.x, c = lane & 15, r4 = lane >> 4;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int kt = blockIdx.x, db0 = blockIdx.z * NB;          // masked: key tile 0 has the most query tiles and starts first
    const double *qb = q.at(b, h), *kb = k.at(b, h), *vb = v.at(b, h), *gob = go.at(b, h);
    const int krow = kt * 16 + c;

    double kr[4 * DB], vr[4 * DB];
#pragma unroll
    for (int st = 0; st < 4 * DB; ++st) {
        kr[st] = ldz(kb, k.sn, krow, Nk, 4 * st + r4, D);
        vr[st] = ldz(vb, v.sn, krow, Nk, 4 * st + r4, D);
    }
    d4 acck[NB], accv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acck[j] = accv[j] = d4{0.0, 0.0, 0.0, 0.0};

    const int nqt = (Nq + 15) / 16;
    for (int qt = CAUSAL ? kt : 0; qt < nqt; ++qt) {
        const d4 s = tile_product<DB>(qb, q.sn, qt * 16, Nq, kr, D, c, r4);
        const d4 dp = tile_product<DB>(gob, go.sn, qt * 16, Nq, vr, D, c, r4);
        double ds[4], w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qrow = qt * 16 + r4 + 4 * i;
            const bool on = qrow < Nq && krow < Nk && (!CAUSAL || krow <= qrow);
            const int64_t row = (int64_t)bh * Nq + (qrow < Nq ? qrow : 0);
            const double gi = g[row], ci = rowdot[row];
            const double x = a * s[i];
            w[i] = on ? fpoly<P>(x) / gi : 0.0;
            ds[i] = on ? fprime<P>(x) * ((dp[i] - ci) / gi) : 0.0;
        }
        accumulate<NB>(acck, qb, q.sn, qt * 16, Nq, ds, D, db0, c, r4);
        accumulate<NB>(accv, gob, go.sn, qt * 16, Nq, w, D, db0, c, r4);
    }
    if (krow >= Nk) return;
    const int64_t row = (int64_t)bh * Nk + krow;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = 16 * (db0 + j) + r4 + 4 * i;
            if (d < D) {
                dk[row * D + d] = a * acck[j][i];
                dv[row * D + d] = accv[j][i];
            }
        }
}

Head head(const void* p, const Strides3& s) { return Head{reinterpret_cast<const double*>(p), s.sb, s.sh, s.sn}; }

// 1 / nt of a float64 problem: the struct's two float coefficients carry it as a + b (see include/fastmax_hip.h)
double scale_a(const fastmax_problem& p) { return (double)p.a + (double)p.b; }

int column_blocks(int D) { return D <= 16 ? 1 : D <= 32 ? 2 : D <= 64 ? 4 : D <= 128 ? 8 : 16; }

template <int DB, int P, bool CAUSAL> void fwd_launch(const FwdArgs& a) {
    const fastmax_problem& p = a.prob;
    const dim3 grid((p.Nq + 15) / 16, p.B * p.H);
    fwd_f64_kernel<DB, P, CAUSAL><<<grid, 64, 0, a.stream>>>(head(a.q, a.qs), head(a.k, a.ks), head(a.v, a.vs), reinterpret_cast<double*>(a.o),
                                                            reinterpret_cast<double*>(a.g), p.H, p.Nq, p.Nk, p.D, scale_a(p),
                                                            CAUSAL ? 0.0 : (double)p.g0 - (double)p.Nk);
}
template <int DB> void fwd_pick(const FwdArgs& a) {
    if (a.prob.p == 1) a.prob.causal ? fwd_launch<DB, 1, true>(a) : fwd_launch<DB, 1, false>(a);
    else a.prob.causal ? fwd_launch<DB, 2, true>(a) : fwd_launch<DB, 2, false>(a);
}

template <int DB, int P, bool CAUSAL> void bwd_launch(const BwdArgs& a, double* rowdot) {
    const fastmax_problem& p = a.prob;
    constexpr int NB = DB == 16 ? 8 : DB;
    const Head q = head(a.q, a.qs), k = head(a.k, a.ks), v = head(a.v, a.vs), go = head(a.grad_o, a.gos);
    const double* g = reinterpret_cast<const double*>(a.g);
    bwd_dq_f64_kernel<DB, P, CAUSAL><<<dim3((p.Nq + 15) / 16, p.B * p.H), 64, 0, a.stream>>>(q, k, v, go, g, rowdot, reinterpret_cast<double*>(a.dq), p.H,
                                                                                             p.Nq, p.Nk, p.D, scale_a(p));
    bwd_dkdv_f64_kernel<DB, NB, P, CAUSAL><<<dim3((p.Nk + 15) / 16, p.B * p.H, DB / NB), 64, 0, a.stream>>>(
        q, k, v, go, g, rowdot, reinterpret_cast<double*>(a.dk), reinterpret_cast<double*>(a.dv), p.H, p.Nq, p.Nk, p.D, scale_a(p));
}
template <int DB> void bwd_pick(const BwdArgs& a, double* rowdot) {
    if (a.prob.p == 1) a.prob.causal ? bwd_launch<DB, 1, true>(a, rowdot) : bwd_launch<DB, 1, false>(a, rowdot);
    else a.prob.causal ? bwd_launch<DB, 2, true>(a, rowdot) : bwd_launch<DB, 2, false>(a, rowdot);
}

}  // namespace

int launch_fwd_f64(const FwdArgs& a) {
    switch (column_blocks(a.prob.D)) {
        case 1: fwd_pick<1>(a); break;
        case 2: fwd_pick<2>(a); break;
        case 4: fwd_pick<4>(a); break;
        case 8: fwd_pick<8>(a); break;
        default: fwd_pick<16>(a); break;
    }
    return (int)hipGetLastError();
}

size_t f64_bwd_workspace(const fastmax_problem& p) { return sizeof(double) * (size_t)p.B * p.H * p.Nq; }

int launch_bwd_f64(const BwdArgs& a) {
    const fastmax_problem& p = a.prob;
    if (!a.workspace || a.workspace_bytes < f64_bwd_workspace(p)) return FASTMAX_E_WORKSPACE;
    double* rowdot = reinterpret_cast<double*>(a.workspace);
    rowdot_f64_kernel<<<dim3((p.Nq + 255) / 256, p.B * p.H), 256, 0, a.stream>>>(head(a.grad_o, a.gos), reinterpret_cast<const double*>(a.o), rowdot, p.H,
                                                                               p.Nq, p.D);
    switch (column_blocks(p.D)) {
        case 1: bwd_pick<1>(a, rowdot); break;
        case 2: bwd_pick<2>(a, rowdot); break;
        case 4: bwd_pick<4>(a, rowdot); break;
        case 8: bwd_pick<8>(a, rowdot); break;
        default: bwd_pick<16>(a, rowdot); break;
    }
    return (int)hipGetLastError();
}

}  // namespace fastmax
