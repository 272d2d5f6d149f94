// extern "C" entry points of libfastmax_hip.so (see include/fastmax_hip.h) + path selection.
#include "fastmax_common.h"

#include <climits>
#include <cstdlib>
#include <cstring>

using namespace fastmax;

namespace {
// bf16 problems take the all-MFMA kernel; FASTMAX_BF16_KERNEL=gen (tuning key "bf16_kernel" = 0) keeps the generic one
bool use_bf16_kernel(const fastmax_problem& p) {
    return mfma_bf16_supported(p) && tune_get(TUNE_BF16_KERNEL) != 0;
}
int validate(const fastmax_problem* p) {
    if (!p) return FASTMAX_E_NULL;
    if (p->p != 1 && p->p != 2) return FASTMAX_E_BAD_P;
    if (p->B <= 0 || p->H <= 0 || p->Nq <= 0 || p->Nk <= 0 || p->D <= 0 || p->D > FASTMAX_MAX_D)
        return FASTMAX_E_BAD_SHAPE;
    if (p->causal && p->Nq != p->Nk) return FASTMAX_E_BAD_SHAPE;
    if ((int64_t)p->B * p->H > 65535) return FASTMAX_E_BAD_SHAPE;       // (b,h) rides on gridDim.y in the tile kernels
    if (p->in_dtype < 0 || p->in_dtype > FASTMAX_F64 || p->out_dtype < 0 || p->out_dtype > FASTMAX_F64) return FASTMAX_E_BAD_DTYPE;
    // float64 in, float64 out: the double kernels neither widen nor narrow
    if ((p->in_dtype == FASTMAX_F64) != (p->out_dtype == FASTMAX_F64)) return FASTMAX_E_BAD_DTYPE;
    return FASTMAX_OK;
}
bool is_f64(const fastmax_problem& p) { return p.in_dtype == FASTMAX_F64; }
// the entry points that have no float64 kernels behind them: validate(), then float64 is a bad dtype
int validate_no_f64(const fastmax_problem* p) {
    const int rc = validate(p);
    return rc ? rc : is_f64(*p) ? FASTMAX_E_BAD_DTYPE : FASTMAX_OK;
}
Strides3 st(const int64_t* s) { return Strides3{s[0], s[1], s[2]}; }

int select(const fastmax_problem& p) {
    // float64: one kernel family (fastmax_f64.hip); a forced family does not apply
    if (is_f64(p)) return p.path == FASTMAX_PATH_AUTO ? FASTMAX_PATH_QUADRATIC_MFMA : FASTMAX_E_BAD_SHAPE;
    if (p.path == FASTMAX_PATH_QUADRATIC) return FASTMAX_PATH_QUADRATIC;
    if (p.path == FASTMAX_PATH_QUADRATIC_MFMA) return quad_mfma_supported(p) ? FASTMAX_PATH_QUADRATIC_MFMA : FASTMAX_E_BAD_SHAPE;
    const bool lin = (p.p == 1 && p.causal);
    // unmasked first order at sizes where a pass over K, V + one D x D product per query row beats the O(N_q N_k) tiles
    if (p.p == 1 && !p.causal && (p.path == FASTMAX_PATH_AUTO || p.path == FASTMAX_PATH_MFMA) && unmasked_lin_supported(p)) return FASTMAX_PATH_MFMA;
    // head sizes above 128 (pythia-1b, Gemma, stablelm-3b in lit_gpt/config.py): tile kernels only -- no D x D state is carried
    if (p.D > 128) {
        if (p.path == FASTMAX_PATH_RECURRENT || p.path == FASTMAX_PATH_MFMA) return FASTMAX_E_BAD_SHAPE;
        return quad_mfma_supported(p) ? FASTMAX_PATH_QUADRATIC_MFMA : FASTMAX_PATH_QUADRATIC;
    }
    if (p.path == FASTMAX_PATH_RECURRENT) return lin ? FASTMAX_PATH_RECURRENT : FASTMAX_E_BAD_SHAPE;
    const bool lin_mfma = lin && (mfma_p1_supported(p) || mfma_gen_supported(p, false) || mfma_d128_2p_supported(p));
    if (p.path == FASTMAX_PATH_MFMA) return lin_mfma ? FASTMAX_PATH_MFMA : FASTMAX_E_BAD_SHAPE;
    if (lin && lin_mfma) return FASTMAX_PATH_MFMA;
    // p = 1 masked shapes the linear-time matrix-core kernels do not cover (two-part operands at D > 64: their images and
    // the D x D state do not fit 160 KB of LDS): the matrix-core tiles beat the vector-ALU recurrence up to N ~ 20 k
    // (measured at D = 128: 2.5 vs 8.5 ms at N = 4096, 27 vs 34 ms at N = 16384)
    if (lin) return (quad_mfma_supported(p) && p.Nq <= 20000) ? FASTMAX_PATH_QUADRATIC_MFMA : FASTMAX_PATH_RECURRENT;
    return quad_mfma_supported(p) ? FASTMAX_PATH_QUADRATIC_MFMA : FASTMAX_PATH_QUADRATIC;
}
bool aligned16(const void* ptr, const int64_t* s, int dtype) {
    const int64_t es = dtype == FASTMAX_F64 ? 8 : dtype == FASTMAX_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(ptr) & 15) return false;
    for (int i = 0; i < 3; ++i)
        if ((s[i] * es) & 15) return false;
    return true;
}
// Operand layout of one call: a bit per operand that keeps the 16-byte rule (base address, and for the strided ones every row
// stride); computed once, read by every decision below.  An operand the entry point does not have leaves its bit clear.
enum : unsigned {
    LAY_Q = 1, LAY_K = 2, LAY_V = 4, LAY_GO = 8, LAY_O = 16, LAY_DQ = 32, LAY_DK = 64, LAY_DV = 128,
    LAY_FWD = LAY_Q | LAY_K | LAY_V | LAY_O,                                          // what the matrix-core forwards read and write
    // the callers' rules differ and each is kept as it was: the backward tiles do not ask for o, the linear-time backwards do
    LAY_BWD_TILES = LAY_Q | LAY_K | LAY_V | LAY_GO | LAY_DQ | LAY_DK | LAY_DV,
    LAY_BWD_ALL = LAY_BWD_TILES | LAY_O,
};
bool has(unsigned lay, unsigned need) { return (lay & need) == need; }
unsigned layout(const fastmax_problem& p, const void* q, const int64_t* qs, const void* k, const int64_t* ks, const void* v,
                const int64_t* vs, const void* o, const void* go = nullptr, const int64_t* gos = nullptr, const void* dq = nullptr,
                const void* dk = nullptr, const void* dv = nullptr) {
    auto base = [](const void* ptr) { return ptr && !(reinterpret_cast<uintptr_t>(ptr) & 15); };
    return (aligned16(q, qs, p.in_dtype) ? LAY_Q : 0) | (aligned16(k, ks, p.in_dtype) ? LAY_K : 0) | (aligned16(v, vs, p.in_dtype) ? LAY_V : 0) |
           (go && aligned16(go, gos, p.in_dtype) ? LAY_GO : 0) | (base(o) ? LAY_O : 0) | (base(dq) ? LAY_DQ : 0) | (base(dk) ? LAY_DK : 0) |
           (base(dv) ? LAY_DV : 0);
}

// state tile of the sequence split: the scans carry a 64 x 64 or a 128 x 128 state
int scan_dp(const fastmax_problem& p) { return p.D <= 64 ? 64 : 128; }
// bytes of prefix states a split scan leaves at the start of its workspace (0: this problem is not split)
size_t scan_state_bytes(const fastmax_problem& p) { return split_workspace_bytes(p, scan_dp(p)); }

using FwdKernel = fastmax_fwd_kernel;          // numbered in include/fastmax_hip.h: fastmax_hip_plan reports them
// the scan kernel of a p = 1 masked problem whose q, k may carry the linearmax scales (the headline kernel takes none)
FwdKernel scan_kernel(const fastmax_problem& p) {
    if (mfma_d128_2p_supported(p)) return FASTMAX_FWD_SCAN_D128_2P;
    return use_bf16_kernel(p) ? FASTMAX_FWD_SCAN_BF16 : FASTMAX_FWD_SCAN_GEN;
}
int launch_fwd_scan(const FwdArgs& a, const float* qscale, const float* kscale) {
    switch (scan_kernel(a.prob)) {
        case FASTMAX_FWD_SCAN_D128_2P: return launch_fwd_mfma_d128_2p(a, qscale, kscale);
        case FASTMAX_FWD_SCAN_BF16: return launch_fwd_mfma_bf16(a, qscale, kscale);
        default: return launch_fwd_mfma_gen(a, qscale, kscale);
    }
}

// Everything fastmax_hip_forward decides, as a function of (problem, layout): rc < 0 rejects the call; else the family
// (what fastmax_hip_select_path reports), the kernel, the workspace it needs and how many leading bytes of that workspace
// hold prefix states afterwards.  The size queries have no operands: they plan with LAY_FWD.
struct FwdPlan {
    int rc, path;
    FwdKernel kernel;
    size_t workspace, state_bytes;
};
FwdPlan fwd_plan(const fastmax_problem& p, unsigned lay) {
    FwdPlan f{FASTMAX_OK, select(p), FASTMAX_FWD_QUADRATIC, 0, 0};
    if (f.path < 0) {
        f.rc = f.path;
        return f;
    }
    if (is_f64(p)) {          // no misaligned fallback kernel: the caller copies
        if (!has(lay, LAY_FWD)) f.rc = FASTMAX_E_ALIGNMENT;
        f.kernel = FASTMAX_FWD_F64;
        return f;
    }
    if ((f.path == FASTMAX_PATH_MFMA || f.path == FASTMAX_PATH_QUADRATIC_MFMA) && !has(lay, LAY_FWD)) {
        if (p.path == f.path) {          // the caller forced this family
            f.rc = FASTMAX_E_ALIGNMENT;
            return f;
        }
        f.path = (f.path == FASTMAX_PATH_MFMA && p.causal) ? FASTMAX_PATH_RECURRENT : FASTMAX_PATH_QUADRATIC;
    }
    switch (f.path) {
        case FASTMAX_PATH_MFMA:
            if (!p.causal) {
                f.kernel = FASTMAX_FWD_UNMASKED_LIN;
                f.workspace = unmasked_lin_workspace(p);
            } else {
                f.kernel = mfma_p1_supported(p) ? FASTMAX_FWD_SCAN_V2 : scan_kernel(p);
                f.workspace = f.state_bytes = scan_state_bytes(p);
            }
            break;
        case FASTMAX_PATH_RECURRENT: f.kernel = FASTMAX_FWD_RECURRENT; break;
        case FASTMAX_PATH_QUADRATIC_MFMA: f.kernel = quad32_supported(p) ? FASTMAX_FWD_QUAD32 : FASTMAX_FWD_QUAD_MFMA; break;
        default: break;
    }
    return f;
}

using BwdKernel = fastmax_bwd_kernel;
// what the backward answers before it selects a kernel: float64 has one family and no misaligned fallback
int bwd_check(const fastmax_problem& p, unsigned lay) {
    if (!is_f64(p)) return FASTMAX_OK;
    if (p.path != FASTMAX_PATH_AUTO) return FASTMAX_E_BAD_SHAPE;
    return has(lay, LAY_BWD_ALL) ? FASTMAX_OK : FASTMAX_E_ALIGNMENT;
}
BwdKernel bwd_select(const fastmax_problem& p, unsigned lay) {
    if (is_f64(p)) return FASTMAX_BWD_F64;
    // matrix-core tiles unless the caller forces the vector-ALU family or the layout rules it out
    if (p.path == FASTMAX_PATH_QUADRATIC || !quad_mfma_bwd_supported(p) || !has(lay, LAY_BWD_TILES)) return FASTMAX_BWD_QUADRATIC;
    // the linear-time kernels, unless the caller asks for the tile kernels; they also read o in 16-byte pieces
    if (p.path != FASTMAX_PATH_QUADRATIC_MFMA && has(lay, LAY_O)) {
        // p=1 unmasked at sizes where totals + row-wise D x D products beat the O(N_q N_k) tiles
        if (unmasked_lin_bwd_supported(p)) return FASTMAX_BWD_UNMASKED_LIN;
        // p=1 masked: scans with a carried D x D state
        if (lin_bwd_supported(p) && p.in_dtype == p.out_dtype) return FASTMAX_BWD_LIN;
        // fp32 / fp16 at 64 < D <= 128: the same scans with two-part operands, one per gradient (fastmax_scan_d128_2p.hip)
        if (scan_bwd_supported(p)) return FASTMAX_BWD_SCAN;
    }
    return quad32_bwd_supported(p) ? FASTMAX_BWD_QUAD32 : FASTMAX_BWD_QUAD_MFMA;
}

// null / shape / workspace checks of the normalize family, in the order every entry point applies them
int normalize_check(bool have_ptrs, int B, int H, int rep, int N, int D, const void* workspace, size_t workspace_bytes, size_t need,
                    int dtype = FASTMAX_F32) {
    if (!have_ptrs) return FASTMAX_E_NULL;
    if (B <= 0 || H <= 0 || rep <= 0 || N <= 0 || D <= 0 || D > FASTMAX_MAX_D) return FASTMAX_E_BAD_SHAPE;
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (!workspace || workspace_bytes < need) return FASTMAX_E_WORKSPACE;
    return FASTMAX_OK;
}
}  // namespace

namespace fastmax {
// "mfma_variant": 200 is the headline kernel (fastmax_mfma_v2.hip) and the only number a production build takes.
// -DFASTMAX_ABLATIONS builds also take its ablations 201 and 204..209, which leave out matrix instructions or memory passes
// (timing-only, wrong results)
static bool mfma_variant_ok(int v) {
#ifdef FASTMAX_ABLATIONS
    if (v == 201 || (v >= 204 && v <= 209)) return true;
#endif
    return v == 200;
}
namespace {
struct TuneEntry { const char* name; const char* env; int value; };
TuneEntry g_tune[TUNE_COUNT] = {
    {"mfma_variant", "FASTMAX_MFMA_VARIANT", 200},    // headline forward kernel: 200 = fastmax_mfma_v2.hip, see mfma_variant_ok
    {"bf16_kernel", "FASTMAX_BF16_KERNEL", 1},
    {"gemm_sched", "FASTMAX_GEMM_SCHED", 0},          // QLoRA GEMM: vector instructions per matrix instruction in the decode steps
    {"gemm_group_m", "FASTMAX_GEMM_GROUP_M", 16},     // QLoRA / head GEMM: row blocks per group of the workgroup -> tile map (0: column blocks fastest over the whole matrix)
    {"gemm_xcd", "FASTMAX_GEMM_XCD", 1},              // QLoRA / head GEMM tile map: 1 = every XCD owns a contiguous run of tiles, in 8-row-block groups
};
bool g_tune_loaded = false;
void tune_load() {
    if (g_tune_loaded) return;
    for (int i = 0; i < TUNE_COUNT; ++i) {
        const char* e = getenv(g_tune[i].env);
        if (!e) continue;
        if (i == TUNE_BF16_KERNEL) g_tune[i].value = e[0] == 'g' ? 0 : 1;
        else g_tune[i].value = atoi(e);
        if (i == TUNE_MFMA_VARIANT && !mfma_variant_ok(g_tune[i].value)) g_tune[i].value = 200;   // not in this build
    }
    g_tune_loaded = true;
}
}  // namespace
int tune_get(int key) {
    tune_load();
    return g_tune[key].value;
}
int tune_set(const char* name, int value) {
    tune_load();
    for (int i = 0; i < TUNE_COUNT; ++i)
        if (!strcmp(name, g_tune[i].name)) {
            if (i == TUNE_MFMA_VARIANT && !mfma_variant_ok(value)) return FASTMAX_E_BAD_SHAPE;
            g_tune[i].value = value;
            return FASTMAX_OK;
        }
    return FASTMAX_E_BAD_SHAPE;
}
int tune_get_by_name(const char* name) {
    tune_load();
    for (int i = 0; i < TUNE_COUNT; ++i)
        if (!strcmp(name, g_tune[i].name)) return g_tune[i].value;
    return INT_MIN;
}
}  // namespace fastmax

extern "C" {

int fastmax_hip_abi_version(void) { return FASTMAX_ABI_VERSION; }

int fastmax_hip_tune(const char* name, int value) { return name ? tune_set(name, value) : FASTMAX_E_NULL; }
int fastmax_hip_tune_get(const char* name) { return name ? tune_get_by_name(name) : INT_MIN; }
int fastmax_hip_build_flags(void) {
#ifdef FASTMAX_ABLATIONS
    return 1;
#else
    return 0;
#endif
}

const char* fastmax_hip_error_string(int code) {
    switch (code) {
        case FASTMAX_OK: return "ok";
        case FASTMAX_E_BAD_P: return "p should be 1 or 2";
        case FASTMAX_E_BAD_SHAPE: return "bad shape (sizes must be positive, causal needs Nq == Nk, D <= 256) or path not applicable";
        case FASTMAX_E_BAD_DTYPE: return "bad dtype";
        case FASTMAX_E_WORKSPACE: return "workspace missing or too small";
        case FASTMAX_E_ALIGNMENT: return "pointer / stride alignment";
        case FASTMAX_E_NULL: return "null pointer";
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

int fastmax_hip_select_path(const fastmax_problem* prob) {
    const int rc = validate(prob);
    if (rc) return rc;
    const FwdPlan plan = fwd_plan(*prob, LAY_FWD);
    return plan.rc ? plan.rc : plan.path;
}

size_t fastmax_hip_forward_workspace(const fastmax_problem* prob) {
    if (validate(prob)) return 0;
    return fwd_plan(*prob, LAY_FWD).workspace;
}

int fastmax_hip_forward(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                        const int64_t* k_strides, const void* v, const int64_t* v_strides, void* o, float* g,
                        void* workspace, size_t workspace_bytes, void* stream) {
    int rc = validate(prob);
    if (rc) return rc;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides) return FASTMAX_E_NULL;
    const FwdPlan plan = fwd_plan(*prob, layout(*prob, q, q_strides, k, k_strides, v, v_strides, o));
    if (plan.rc) return plan.rc;
    FwdArgs a{*prob, q, k, v, st(q_strides), st(k_strides), st(v_strides), o, g, workspace, workspace_bytes,
              reinterpret_cast<hipStream_t>(stream)};
    switch (plan.kernel) {
        case FASTMAX_FWD_UNMASKED_LIN: return launch_fwd_unmasked_p1(a);
        case FASTMAX_FWD_SCAN_V2: return launch_fwd_mfma_p1(a);
        case FASTMAX_FWD_SCAN_D128_2P:
        case FASTMAX_FWD_SCAN_BF16:
        case FASTMAX_FWD_SCAN_GEN: return launch_fwd_scan(a, nullptr, nullptr);
        case FASTMAX_FWD_RECURRENT: return launch_fwd_recurrent_p1(a);
        case FASTMAX_FWD_QUAD32: return launch_fwd_quad32(a);
        case FASTMAX_FWD_QUAD_MFMA: return launch_fwd_quad_mfma(a);
        case FASTMAX_FWD_F64: return launch_fwd_f64(a);
        case FASTMAX_FWD_QUADRATIC: break;
    }
    return launch_fwd_quadratic(a);
}

size_t fastmax_hip_backward_workspace(const fastmax_problem* prob) {
    if (validate(prob)) return 0;
    if (is_f64(*prob)) return f64_bwd_workspace(*prob);
    const size_t a = bwd_quadratic_workspace(*prob), b = lin_bwd_workspace(*prob);
    size_t c = scan_bwd_supported(*prob) ? scan_bwd_workspace(*prob) : 0;
    const size_t d = unmasked_lin_bwd_workspace(*prob);
    if (d > c) c = d;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

size_t fastmax_hip_forward_state_bytes(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                                       const int64_t* k_strides, const void* v, const int64_t* v_strides, const void* o) {
    if (validate(prob) || !q || !k || !v || !o || !q_strides || !k_strides || !v_strides) return 0;
    const FwdPlan plan = fwd_plan(*prob, layout(*prob, q, q_strides, k, k_strides, v, v_strides, o));
    return plan.rc ? 0 : plan.state_bytes;
}

int fastmax_hip_backward_with_states(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                         const int64_t* k_strides, const void* v, const int64_t* v_strides, const void* o,
                         const float* g, const void* grad_o, const int64_t* go_strides, void* dq, void* dk, void* dv,
                         void* workspace, size_t workspace_bytes, const void* fwd_states, size_t fwd_state_bytes, void* stream) {
    int rc = validate(prob);
    if (rc) return rc;
    if (!q || !k || !v || !o || !g || !grad_o || !dq || !dk || !dv || !q_strides || !k_strides || !v_strides ||
        !go_strides)
        return FASTMAX_E_NULL;
    BwdArgs a{*prob, q, k, v, o, grad_o, g, st(q_strides), st(k_strides), st(v_strides), st(go_strides), dq, dk, dv,
              workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream)};
    const unsigned lay = layout(*prob, q, q_strides, k, k_strides, v, v_strides, o, grad_o, go_strides, dq, dk, dv);
    rc = bwd_check(*prob, lay);
    if (rc) return rc;
    // the caller's records are taken when they cover what this forward leaves (a rejected or unsplit forward leaves none)
    const FwdPlan fwd = fwd_plan(*prob, lay);
    if (fwd_states && fwd_state_bytes > 0 && fwd_state_bytes >= (fwd.rc ? 0 : fwd.state_bytes) && !(reinterpret_cast<uintptr_t>(fwd_states) & 15))
        a.fwd_states = reinterpret_cast<const float*>(fwd_states);
    switch (bwd_select(*prob, lay)) {
        case FASTMAX_BWD_UNMASKED_LIN: return launch_bwd_unmasked_p1(a);
        case FASTMAX_BWD_LIN: return launch_bwd_lin(a);
        case FASTMAX_BWD_SCAN: return launch_bwd_scan(a);
        case FASTMAX_BWD_QUAD32: return launch_bwd_quad32(a);
        case FASTMAX_BWD_QUAD_MFMA: return launch_bwd_quad_mfma(a);
        case FASTMAX_BWD_F64: return launch_bwd_f64(a);          // ignores the caller's states: this forward leaves none
        case FASTMAX_BWD_QUADRATIC: break;
    }
    return launch_bwd_quadratic(a);
}

int fastmax_hip_backward(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                         const int64_t* k_strides, const void* v, const int64_t* v_strides, const void* o,
                         const float* g, const void* grad_o, const int64_t* go_strides, void* dq, void* dk, void* dv,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return fastmax_hip_backward_with_states(prob, q, q_strides, k, k_strides, v, v_strides, o, g, grad_o, go_strides, dq, dk, dv, workspace,
                                            workspace_bytes, nullptr, 0, stream);
}

// what fastmax_hip_forward and fastmax_hip_backward_with_states would decide for these operands, from the functions they
// call themselves; addresses and strides are only looked at, nothing is read through them and nothing is launched
int fastmax_hip_plan(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides,
                     const void* v, const int64_t* v_strides, const void* o, const void* grad_o, const int64_t* go_strides,
                     const void* dq, const void* dk, const void* dv, fastmax_plan* out) {
    if (!out) return FASTMAX_E_NULL;
    *out = fastmax_plan{FASTMAX_OK, -1, -1, -1, 1, 0};
    const bool with_bwd = grad_o || go_strides || dq || dk || dv;
    out->rc = validate(prob);
    if (!out->rc && (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides ||
                     (with_bwd && (!grad_o || !go_strides || !dq || !dk || !dv))))
        out->rc = FASTMAX_E_NULL;
    if (out->rc) return out->rc;
    const unsigned lay = with_bwd ? layout(*prob, q, q_strides, k, k_strides, v, v_strides, o, grad_o, go_strides, dq, dk, dv)
                                  : layout(*prob, q, q_strides, k, k_strides, v, v_strides, o);
    const FwdPlan fwd = fwd_plan(*prob, lay);
    out->rc = fwd.rc;
    bool split = false;
    if (!fwd.rc) {
        out->path = fwd.path;
        out->fwd_kernel = fwd.kernel;
        out->state_bytes = fwd.state_bytes;
        split = fwd.path == FASTMAX_PATH_MFMA && prob->causal;
    }
    if (with_bwd) {          // the backward does not ask whether the forward was accepted
        if (!out->rc) out->rc = bwd_check(*prob, lay);
        out->bwd_kernel = bwd_select(*prob, lay);
        split = split || out->bwd_kernel == FASTMAX_BWD_LIN;
    }
    if (split) out->nseg = split_plan(*prob).nseg;
    return out->rc;
}

size_t fastmax_hip_normalize_workspace(int B, int H) { return sizeof(unsigned int) * (size_t)B * H; }

int fastmax_hip_normalize(const void* x, const int64_t* x_strides, int dtype, float* y, float* inv_norm, int B, int H,
                          int N, int D, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = normalize_check(x && x_strides && y, B, H, 1, N, D, workspace, workspace_bytes, fastmax_hip_normalize_workspace(B, H));
    if (rc) return rc;
    return launch_normalize(x, st(x_strides), dtype, y, inv_norm, B, H, N, D, workspace,
                            reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_normalize_stats(const void* x, const int64_t* x_strides, int dtype, float* inv_norm, int B, int H, int N,
                                int D, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = normalize_check(x && x_strides && inv_norm, B, H, 1, N, D, workspace, workspace_bytes, fastmax_hip_normalize_workspace(B, H));
    if (rc) return rc;
    return launch_normalize_stats(x, st(x_strides), dtype, inv_norm, B, H, N, D, workspace,
                                  reinterpret_cast<hipStream_t>(stream));
}

size_t fastmax_hip_normalize_stats2_workspace(int B, int H, int N) {
    return sizeof(unsigned long long) * 2 * (size_t)B * H * (size_t)((N + 255) / 256);          // (value, row) keys
}

int fastmax_hip_normalize_stats2(const void* x0, const int64_t* x0_strides, const void* x1, const int64_t* x1_strides, int dtype,
                                 float* inv_norm0, float* inv_norm1, int B, int H, int N, int D, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const bool have = x0 && x1 && x0_strides && x1_strides && inv_norm0 && inv_norm1;
    if (have && (int64_t)B * H > 65535) return FASTMAX_E_BAD_SHAPE;          // (b,h) rides on gridDim.y
    const int rc = normalize_check(have, B, H, 1, N, D, workspace, workspace_bytes, fastmax_hip_normalize_stats2_workspace(B, H, N));
    if (rc) return rc;
    return launch_normalize_stats2(x0, st(x0_strides), x1, st(x1_strides), dtype, inv_norm0, inv_norm1, B, H, N, D, workspace,
                                   reinterpret_cast<hipStream_t>(stream));
}

int fastmax_hip_normalize_cast(const void* x, const int64_t* x_strides, int dtype, void* y, float* inv_norm, int B, int H,
                               int N, int D, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = normalize_check(x && x_strides && y && inv_norm, B, H, 1, N, D, workspace, workspace_bytes, fastmax_hip_normalize_workspace(B, H));
    if (rc) return rc;
    if (dtype < 0 || dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;          // after the workspace check here, before it in _cast_expand
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int npart = (N + 255) / 256;
    if (workspace_bytes >= sizeof(unsigned int) * (size_t)B * H * npart) {
        // two launches: per-block maxima, then the row pass combines them (no zeroing pass, no atomics, no finish pass)
        unsigned int* partials = reinterpret_cast<unsigned int*>(workspace);
        rc = launch_normalize_partial_max(x, st(x_strides), dtype, partials, B, H, N, D, s);
        if (rc) return rc;
        return launch_normalize_cast(x, st(x_strides), dtype, y, nullptr, B, H, N, D, s, partials, npart, inv_norm);
    }
    rc = launch_normalize_stats(x, st(x_strides), dtype, inv_norm, B, H, N, D, workspace, s);
    if (rc) return rc;
    return launch_normalize_cast(x, st(x_strides), dtype, y, inv_norm, B, H, N, D, s);
}

size_t fastmax_hip_normalize_backward_workspace(int B, int H, int N) { return normalize_backward_workspace(B, H, N); }

int fastmax_hip_normalize_backward(const void* x, const int64_t* x_strides, int dtype, const void* grad_y, const float* inv_norm,
                                   void* grad_x, int B, int H, int N, int D, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const int rc = normalize_check(x && x_strides && grad_y && inv_norm && grad_x, B, H, 1, N, D, workspace, workspace_bytes,
                                   normalize_backward_workspace(B, H, N));
    if (rc) return rc;
    return launch_normalize_backward(x, st(x_strides), dtype, grad_y, inv_norm, grad_x, B, H, N, D, workspace,
                                     reinterpret_cast<hipStream_t>(stream));
}

// grouped-query form of the two entry points above: x holds the G key heads, y / grad_y the G * rep query-head copies
// (head g * rep + j) that the attention reads -- the GQA expand of lit_gpt/model.py:404-411 fused into the prologue's store,
// and the sum over a group's heads fused into its backward
int fastmax_hip_normalize_cast_expand(const void* x, const int64_t* x_strides, int dtype, void* y, float* inv_norm, int B, int G,
                                      int rep, int N, int D, void* workspace, size_t workspace_bytes, void* stream) {
    const int npart = (N + 255) / 256;
    int rc = normalize_check(x && x_strides && y && inv_norm, B, G, rep, N, D, workspace, workspace_bytes,
                             sizeof(unsigned int) * (size_t)B * G * npart, dtype);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned int* partials = reinterpret_cast<unsigned int*>(workspace);
    rc = launch_normalize_partial_max(x, st(x_strides), dtype, partials, B, G, N, D, s);
    if (rc) return rc;
    return launch_normalize_cast(x, st(x_strides), dtype, y, nullptr, B, G, N, D, s, partials, npart, inv_norm, rep);
}

int fastmax_hip_normalize_backward_expand(const void* x, const int64_t* x_strides, int dtype, const void* grad_y,
                                          const float* inv_norm, void* grad_x, int B, int G, int rep, int N, int D, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    const int rc = normalize_check(x && x_strides && grad_y && inv_norm && grad_x, B, G, rep, N, D, workspace, workspace_bytes,
                                   normalize_backward_workspace_grouped(B, G, rep, N));
    if (rc) return rc;
    return launch_normalize_backward(x, st(x_strides), dtype, grad_y, inv_norm, grad_x, B, G, N, D, workspace,
                                     reinterpret_cast<hipStream_t>(stream), rep);
}

// what the two fused linearmax forwards ask of a call before they launch a scan that applies q's and k's scales
static int linearmax_fwd_check(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                               const int64_t* k_strides, const void* v, const int64_t* v_strides, const float* q_inv_norm,
                               const float* k_inv_norm, const void* o) {
    const int rc = validate_no_f64(prob);
    if (rc) return rc;
    if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !q_inv_norm || !k_inv_norm) return FASTMAX_E_NULL;
    if (!mfma_gen_supported(*prob, true) && !mfma_d128_2p_supported(*prob)) return FASTMAX_E_BAD_SHAPE;
    return has(layout(*prob, q, q_strides, k, k_strides, v, v_strides, o), LAY_FWD) ? FASTMAX_OK : FASTMAX_E_ALIGNMENT;
}

int fastmax_hip_linearmax_forward(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                                  const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                  const float* q_inv_norm, const float* k_inv_norm, void* o, float* g, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const int rc = linearmax_fwd_check(prob, q, q_strides, k, k_strides, v, v_strides, q_inv_norm, k_inv_norm, o);
    if (rc) return rc;
    FwdArgs a{*prob, q, k, v, st(q_strides), st(k_strides), st(v_strides), o, g, workspace, workspace_bytes,
              reinterpret_cast<hipStream_t>(stream)};
    return launch_fwd_scan(a, q_inv_norm, k_inv_norm);
}

// fastmax_hack.py:36-60 (masked branch) in ONE call: statistics + scan.  With the sequence split the statistics ride on the
// split's state pass (K is read there anyway, the state is linear in K's scale; Q's words come from extra blocks of the same
// launch); otherwise they are the paired statistics pass.  q_inv_norm / k_inv_norm (B*H floats each) are OUTPUTS here.
// workspace = [forward workspace | statistic words]; the first part is the plan's, so a forced prob->path sizes it as it
// sizes fastmax_hip_forward's.
static size_t linearmax_stats_bytes(int B, int H, int N) {
    const size_t per_head = (size_t)((N + 255) / 256) + 32;          // statistics-only blocks of 256 rows + one key per segment
    return sizeof(unsigned long long) * 2 * (size_t)B * H * per_head;
}
static size_t linearmax_fwd_bytes(const fastmax_problem& p) { return (fwd_plan(p, LAY_FWD).workspace + 255) & ~(size_t)255; }

size_t fastmax_hip_linearmax_forward_auto_workspace(const fastmax_problem* prob) {
    if (validate_no_f64(prob)) return 0;
    return linearmax_fwd_bytes(*prob) + linearmax_stats_bytes(prob->B, prob->H, prob->Nq);
}

int fastmax_hip_linearmax_forward_auto(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                                       const int64_t* k_strides, const void* v, const int64_t* v_strides, float* q_inv_norm,
                                       float* k_inv_norm, int* q_nstar, int* k_nstar, void* o, float* g, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const int rc = linearmax_fwd_check(prob, q, q_strides, k, k_strides, v, v_strides, q_inv_norm, k_inv_norm, o);
    if (rc) return rc;
    const size_t fwd_bytes = linearmax_fwd_bytes(*prob);
    if (!workspace || workspace_bytes < fwd_bytes + linearmax_stats_bytes(prob->B, prob->H, prob->Nq)) return FASTMAX_E_WORKSPACE;
    const LinearmaxStats stats{q_inv_norm, k_inv_norm, reinterpret_cast<unsigned int*>(static_cast<char*>(workspace) + fwd_bytes),
                               q_nstar, k_nstar};
    FwdArgs a{*prob, q, k, v, st(q_strides), st(k_strides), st(v_strides), o, g, workspace, fwd_bytes,
              reinterpret_cast<hipStream_t>(stream), &stats};
    return launch_fwd_scan(a, q_inv_norm, k_inv_norm);
}

// Training route of the same branch: the backward of fastmax_hip_linearmax_forward_auto.  q, k are the RAW tensors and
// q_inv_norm / k_inv_norm what the forward left; the linear-time scans apply the prologue while staging (as the forward does), so
// no normalised copy of q or k is ever stored.  dq, dk are the gradients wrt the NORMALISED q, k: the caller finishes with
// fastmax_hip_normalize_backward(q, dq, q_inv_norm) / (k, dk, k_inv_norm) -- unless flags bit 0 is set: then the dK/dV kernel
// applies the prologue's backward to its dK tile itself and dk is the gradient wrt the raw k (one k head per query head only).  fwd_states = the forward's workspace (its prefix
// states), or null.  FASTMAX_E_BAD_SHAPE where the linear-time backward does not cover the problem (fastmax_hip_linearmax_train_supported).
int fastmax_hip_linearmax_train_supported(const fastmax_problem* prob) {
    if (validate_no_f64(prob)) return 0;
    if (!(prob->p == 1 && prob->causal) || prob->in_dtype != prob->out_dtype) return 0;
    return (mfma_gen_supported(*prob, true) && lin_bwd_supported(*prob)) ? 1 : 0;
}

int fastmax_hip_linearmax_backward(const fastmax_problem* prob, const void* q, const int64_t* q_strides, const void* k,
                                   const int64_t* k_strides, const void* v, const int64_t* v_strides, const void* o, const float* g,
                                   const void* grad_o, const int64_t* go_strides, const float* q_inv_norm, const float* k_inv_norm,
                                   const int* q_nstar, const int* k_nstar, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                                   const void* fwd_states, size_t fwd_state_bytes, int flags, void* stream) {
    int rc = validate_no_f64(prob);
    if (rc) return rc;
    if (!q || !k || !v || !o || !g || !grad_o || !dq || !dk || !dv || !q_strides || !k_strides || !v_strides || !go_strides ||
        !q_inv_norm || !k_inv_norm)
        return FASTMAX_E_NULL;
    if (!fastmax_hip_linearmax_train_supported(prob)) return FASTMAX_E_BAD_SHAPE;
    if (!has(layout(*prob, q, q_strides, k, k_strides, v, v_strides, o, grad_o, go_strides, dq, dk, dv), LAY_BWD_ALL)) return FASTMAX_E_ALIGNMENT;
    BwdArgs a{*prob, q, k, v, o, grad_o, g, st(q_strides), st(k_strides), st(v_strides), st(go_strides), dq, dk, dv,
              workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream)};
    a.qscale = q_inv_norm;
    a.kscale = k_inv_norm;
    a.fuse_prologue = ((flags & 1) && k_nstar ? 1 : 0) | ((flags & 2) && q_nstar ? 2 : 0);
    a.k_nstar = k_nstar;
    a.q_nstar = q_nstar;
    // the fused forward ran a scan whatever prob->path says: its states are there iff the sequence was split
    const size_t state_bytes = scan_state_bytes(*prob);
    if (fwd_states && state_bytes > 0 && fwd_state_bytes >= state_bytes && !(reinterpret_cast<uintptr_t>(fwd_states) & 15))
        a.fwd_states = reinterpret_cast<const float*>(fwd_states);
    return launch_bwd_lin(a);
}

}  // extern "C"
