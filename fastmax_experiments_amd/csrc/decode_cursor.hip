// The decode cursor (include/fastmax_hip_cursor.h): position, draw number and output column of a generation loop in device memory,
// so that a decode step takes the same arguments every token and one recorded graph generates a token per replay.
//
//   cursor_feed_kernel   grid B + 1, 256 threads.  Workgroup b < B copies row tok[b] of the embedding table into x[b]; workgroup B
//                        copies row `pos` of cos and of sin into the two one-row buffers and stores next = pos + 1.  Rows move as
//                        16-byte pieces or element by element (the host decides per operand pair, the same rule as last_logits);
//                        a copy has no arithmetic, so the two routes cannot differ.  Every workgroup reads `pos`; only workgroup B
//                        writes `next`, and no workgroup reads it.
//   sample_kernel<CursorDraw>   next_token_sample.h with the stream's key and draw number read from the cursor.  Every workgroup
//                        reads `next`, `draw_base` and `seed`; thread 0 of each stores its token, and pos = next (the same value
//                        from every workgroup).  No workgroup reads `pos`.  sample_kernel<Nucleus<CursorDraw>> is the same with
//                        the top-p filter behind the top-k (include/fastmax_hip_nucleus.h).
// `overflow` is only ever written, with 1.  All stores are plain vector stores.
#include "fastmax_common.h"
#include "next_token_sample.h"
#include "../../include/fastmax_hip_cursor.h"
#include "../../include/fastmax_hip_nucleus.h"

namespace fastmax {

typedef unsigned int cu32x4 __attribute__((ext_vector_type(4)));

constexpr int FEED_THREADS = 256;

// n bytes from src to dst (src == nullptr: zeros), the whole workgroup; `vec`: 16-byte pieces, else elements of `es` (2 or 4) bytes
__device__ __forceinline__ void copy_row(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int64_t nbytes, int es,
                                         bool vec) {
    const int tid = threadIdx.x;
    if (vec) {
        const cu32x4 zero = {0u, 0u, 0u, 0u};
        for (int64_t i = tid; i < nbytes / 16; i += FEED_THREADS)
            reinterpret_cast<cu32x4*>(dst)[i] = src ? reinterpret_cast<const cu32x4*>(src)[i] : zero;
    } else if (es == 4) {
        for (int64_t i = tid; i < nbytes / 4; i += FEED_THREADS)
            reinterpret_cast<uint32_t*>(dst)[i] = src ? reinterpret_cast<const uint32_t*>(src)[i] : 0u;
    } else {
        for (int64_t i = tid; i < nbytes / 2; i += FEED_THREADS)
            reinterpret_cast<uint16_t*>(dst)[i] = src ? reinterpret_cast<const uint16_t*>(src)[i] : (uint16_t)0;
    }
}

struct FeedArgs {
    int64_t* cursor;
    const int64_t* tok;
    const unsigned char* wte;
    int64_t ldw_bytes, n_wte_rows;
    unsigned char* x;
    int64_t ldx_bytes, row_bytes;
    const unsigned char *cos, *sin;
    int64_t ld_rope_bytes, n_rope_rows;
    unsigned char *cos_row, *sin_row;
    int64_t rope_bytes;
    int B, es, rope_es, vec, rope_vec;
};

__global__ __launch_bounds__(FEED_THREADS) void cursor_feed_kernel(FeedArgs a) {
    const int64_t pos = a.cursor[FASTMAX_CURSOR_POS];
    const bool refused = pos < 0 || pos >= a.n_rope_rows;
    const int b = blockIdx.x;
    if (b == a.B) {
        if (!refused) {
            copy_row(a.cos + pos * a.ld_rope_bytes, a.cos_row, a.rope_bytes, a.rope_es, a.rope_vec != 0);
            copy_row(a.sin + pos * a.ld_rope_bytes, a.sin_row, a.rope_bytes, a.rope_es, a.rope_vec != 0);
        }
        if (threadIdx.x == 0) {
            a.cursor[FASTMAX_CURSOR_NEXT] = refused ? (int64_t)-1 : pos + 1;
            if (refused) a.cursor[FASTMAX_CURSOR_OVERFLOW] = 1;
        }
        return;
    }
    if (refused) return;
    const int64_t t = a.tok[b];
    const bool known = t >= 0 && t < a.n_wte_rows;
    copy_row(known ? a.wte + t * a.ldw_bytes : nullptr, a.x + (int64_t)b * a.ldx_bytes, a.row_bytes, a.es, a.vec != 0);
    if (!known && threadIdx.x == 0) a.cursor[FASTMAX_CURSOR_OVERFLOW] = 1;
}

// the stream from the cursor; the token also goes to column `next` of out, the eos flag to done, and the cursor moves on
struct CursorDraw {
    static constexpr bool nucleus = false;
    int64_t* cursor;
    int64_t* out;
    int64_t ldo, L;
    unsigned char* done;
    int64_t eos_id;
    __device__ __forceinline__ bool open(DrawStream& s) const {
        const int64_t next = cursor[FASTMAX_CURSOR_NEXT];
        if (next < 0 || next >= L) {
            if (threadIdx.x == 0) cursor[FASTMAX_CURSOR_OVERFLOW] = 1;
            return false;
        }
        const uint64_t seed = (uint64_t)cursor[FASTMAX_CURSOR_SEED];
        const uint64_t draw = (uint64_t)cursor[FASTMAX_CURSOR_DRAW_BASE] + (uint64_t)next;
        s = DrawStream{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)draw, (unsigned)(draw >> 32)};
        return true;
    }
    __device__ __forceinline__ void close(int b, int token) const {
        const int64_t next = cursor[FASTMAX_CURSOR_NEXT];
        out[(int64_t)b * ldo + next] = (int64_t)token;
        if (eos_id >= 0 && (int64_t)token == eos_id) done[b] = 1;
        cursor[FASTMAX_CURSOR_POS] = next;
    }
};

static inline bool pieces16(int64_t row_bytes, int64_t ld_a_bytes, int64_t ld_b_bytes, const void* a, const void* b, const void* c = nullptr,
                            const void* d = nullptr) {
    return row_bytes % 16 == 0 && ld_a_bytes % 16 == 0 && ld_b_bytes % 16 == 0 && aligned_to(a, 16) && aligned_to(b, 16) &&
           aligned_to(c, 16) && aligned_to(d, 16);
}

}  // namespace fastmax

using namespace fastmax;

extern "C" {

size_t fastmax_hip_cursor_bytes(void) { return FASTMAX_CURSOR_WORDS * sizeof(int64_t); }

int fastmax_hip_cursor_feed(void* cursor, const int64_t* tok, const void* wte, int64_t ldw, int64_t n_wte_rows, void* x, int64_t ldx,
                            int B, int C, int dtype, const void* cos, const void* sin, int64_t ld_rope, int64_t n_rope_rows,
                            void* cos_row, void* sin_row, int n_cols, int rope_dtype, void* stream) {
    if (!cursor || !tok || !wte || !x || !cos || !sin || !cos_row || !sin_row) return FASTMAX_E_NULL;
    if (dtype < 0 || dtype > FASTMAX_F16 || rope_dtype < 0 || rope_dtype > FASTMAX_F16) return FASTMAX_E_BAD_DTYPE;
    if (B <= 0 || C <= 0 || C > MAX_EXTENT || n_cols <= 0 || n_wte_rows <= 0 || n_rope_rows <= 0 || ldw < C || ldx < C || ld_rope < n_cols)
        return FASTMAX_E_BAD_SHAPE;
    const int es = dtype == FASTMAX_F32 ? 4 : 2, res = rope_dtype == FASTMAX_F32 ? 4 : 2;
    if (!aligned_to(cursor, 8) || !aligned_to(tok, 8) || !aligned_to(wte, es) || !aligned_to(x, es) || !aligned_to(cos, res) ||
        !aligned_to(sin, res) || !aligned_to(cos_row, res) || !aligned_to(sin_row, res))
        return FASTMAX_E_ALIGNMENT;
    FeedArgs a;
    a.cursor = reinterpret_cast<int64_t*>(cursor);
    a.tok = tok;
    a.wte = reinterpret_cast<const unsigned char*>(wte);
    a.ldw_bytes = ldw * es;
    a.n_wte_rows = n_wte_rows;
    a.x = reinterpret_cast<unsigned char*>(x);
    a.ldx_bytes = ldx * es;
    a.row_bytes = (int64_t)C * es;
    a.cos = reinterpret_cast<const unsigned char*>(cos);
    a.sin = reinterpret_cast<const unsigned char*>(sin);
    a.ld_rope_bytes = ld_rope * res;
    a.n_rope_rows = n_rope_rows;
    a.cos_row = reinterpret_cast<unsigned char*>(cos_row);
    a.sin_row = reinterpret_cast<unsigned char*>(sin_row);
    a.rope_bytes = (int64_t)n_cols * res;
    a.B = B;
    a.es = es;
    a.rope_es = res;
    a.vec = pieces16(a.row_bytes, a.ldw_bytes, a.ldx_bytes, wte, x);
    a.rope_vec = pieces16(a.rope_bytes, a.ld_rope_bytes, 0, cos, sin, cos_row, sin_row);
    hipLaunchKernelGGL(cursor_feed_kernel, dim3((unsigned)B + 1u), dim3(FEED_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int fastmax_hip_sample_cursor(const float* logits, int64_t ld, void* cursor, int64_t* tok, int64_t* out, int64_t ldo, int64_t L,
                              void* done, int64_t eos_id, int B, int V, int top_k, float temperature, void* stream) {
    if (!logits || !cursor || !tok || !out || (eos_id >= 0 && !done)) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > MAX_EXTENT || L <= 0 || ld < V || ldo < L || top_k < 0 ||
        !(temperature >= 0.f && temperature <= 3.4028234e38f))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(cursor, 8) || !aligned_to(tok, 8) || !aligned_to(out, 8)) return FASTMAX_E_ALIGNMENT;
    const CursorDraw from{reinterpret_cast<int64_t*>(cursor), out, ldo, L, reinterpret_cast<unsigned char*>(done), eos_id};
    hipLaunchKernelGGL(sample_kernel<CursorDraw>, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld,
                       tok, V, top_k, temperature, from);
    return (int)hipGetLastError();
}

int fastmax_hip_sample_cursor_nucleus(const float* logits, int64_t ld, void* cursor, int64_t* tok, int64_t* out, int64_t ldo, int64_t L,
                                      void* done, int64_t eos_id, int B, int V, int top_k, float temperature, float top_p,
                                      void* stream) {
    if (!logits || !cursor || !tok || !out || (eos_id >= 0 && !done)) return FASTMAX_E_NULL;
    if (B <= 0 || V <= 0 || V > NUCLEUS_MAX_V || L <= 0 || ld < V || ldo < L || top_k < 0 ||
        !(temperature >= 0.f && temperature <= 3.4028234e38f) || !nucleus_share(top_p))
        return FASTMAX_E_BAD_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(cursor, 8) || !aligned_to(tok, 8) || !aligned_to(out, 8)) return FASTMAX_E_ALIGNMENT;
    const Nucleus<CursorDraw> from{{reinterpret_cast<int64_t*>(cursor), out, ldo, L, reinterpret_cast<unsigned char*>(done), eos_id}, top_p};
    hipLaunchKernelGGL(sample_kernel<Nucleus<CursorDraw>>, dim3((unsigned)B), dim3(SEL_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       logits, ld, tok, V, top_k, temperature, from);
    return (int)hipGetLastError();
}

}  // extern "C"
