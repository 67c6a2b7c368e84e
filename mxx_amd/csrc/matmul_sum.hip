// matmul_sum.hip — fused multiply-accumulate: gpupoly_matrix_mul_sum, gpupoly_matrix_mul_acc.
//
//   out[:, dst_col .. dst_col + cols) = addend[:, dst_col .. dst_col + cols) +/- sum_{t<n} lhss[t] * rhss[t]
//
// The reference's callers almost never use a product by itself: src/lookup/ggh15/encoding.rs:205-298 builds one output
// chunk from five `add_in_place(&(a * &b))` / `x - (a * &b)` steps and an accumulation loop, src/lookup/ggh15/pubkey_gpu.rs:408
// and :494-505, src/lookup/lwe/encoding_gpu.rs:142-223, src/sampler/trapdoor/gpu.rs:212,286 and
// src/gadgets/fhe/ring_gsw_montgomery_gpu.rs:80 do the same, and the chunks are then glued with concat_columns_owned.
// Through gpu_matrix_mul that is a product launch, an add or sub launch (three more passes over the output), a temporary,
// a neg launch for a negated term and a copy_block per chunk - each of them latency-bound on the small rings.
//
// Term-table product: the shared register-tile loop (matmul_tile.h, which also chooses the tile and the grid) once per
// term.  Where matmul_group_kernel's table runs over operands, this one runs over the INNER dimension.  Up to
// 64 {A_t, B_t, k_t} descriptors ride in the kernel-argument segment; a workgroup takes a TR x TC tile of out's block for
// one limb and a run of slots and walks all terms - the virtual product [A_0 | A_1 | ...] * [B_0; B_1; ...], never
// materialised.  The lazy accumulators AND the pending-product counter carry across term boundaries: one reduction per
// LimbConst::lazy_terms products wherever they fall, one in the epilogue, which also negates, adds the addend block and
// stores at dst_col.  An addend that is `out` is read and written by the same thread.
//
// Above 8 rows the tuned products (gpu_matrix_mul's dispatcher: the streamed 32-row tiles, the LDS tile) go into scratch
// and one combine pass per term folds them into the block (DESIGN.md 5j has the timing behind the rule).
#include "matmul_tile.h"

#include <algorithm>
#include <string>
#include <vector>

struct MulSumItem {
    const void *a;  // lhss[t], words, rows x k
    const void *b;  // rhss[t], words, k x cols
    uint32_t k;     // inner size of this term (may be 0)
    uint32_t pad;
};
constexpr size_t kMulSumMax = 64;
struct MulSumArgs {
    MulSumItem item[kMulSumMax];  // 64 x 24 bytes
};
static_assert(sizeof(MulSumArgs) <= 4096 - 128, "descriptor table must fit the kernel-argument segment");

// out and addend are rows x out_cols; this launch reads addend's and writes out's columns [dst_col, dst_col + cols).  They
// may be the same pointer (no __restrict__): every word is then read and written by the same thread.  blockIdx.y = column
// tile * row_tiles + row tile, as in matmul_group_kernel: the row tiles of one column tile read the same panels of B.
template <typename W, int TR, int TC, int SV, bool NTB>
__global__ void __launch_bounds__(256)
    matmul_sum_kernel(MulSumArgs args, uint32_t terms, W *out, const W *addend, const LimbConst *__restrict__ limbs, uint32_t rows,
                      uint32_t cols, uint32_t out_cols, uint32_t dst_col, uint32_t L, uint32_t N, uint32_t row_tiles, int negate) {
    const uint32_t limb = blockIdx.z;
    const uint32_t ct = blockIdx.y / row_tiles, rt = blockIdx.y - ct * row_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * SV;
    if (i >= N) return;
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    typedef typename TileTypes<W, SV>::VT VT;
    typedef typename TileTypes<W, SV>::wxs wxs;
    typedef typename TileTypes<W, SV>::D D;

    const size_t poly = static_cast<size_t>(L) * N;  // words per polynomial
    const size_t in_poly = static_cast<size_t>(limb) * N + i;
    // rows and columns past the end of the block repeat the last one; their results are never stored
    uint32_t row[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) row[r] = min(r0 + r, rows - 1);
    size_t b_off[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) b_off[c] = static_cast<size_t>(min(c0 + c, cols - 1)) * poly + in_poly;
    const size_t strideBk = static_cast<size_t>(cols) * poly;

    D acc[TR][TC][SV];
    MXX_TILE_CLEAR(acc);
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;  // products since the last reduction: NOT reset at a term boundary
    for (uint32_t t = 0; t < terms; ++t) {
        const MulSumItem it = args.item[t];  // uniform: scalar loads from the kernel-argument segment
        const W *A = static_cast<const W *>(it.a), *B = static_cast<const W *>(it.b);
        const uint32_t inner = it.k;
        size_t a_off[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) a_off[r] = static_cast<size_t>(row[r]) * inner * poly + in_poly;
#define MXX_TILE_A(r, k) (A + a_off[r] + (k) * poly)
#define MXX_TILE_B(c, k) (B + b_off[c] + (k) * strideBk)
#include "matmul_tile_loop.inc"
    }
    // epilogue: reduce, negate, + addend block, store at dst_col
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (r0 + r >= rows) continue;
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            if (c0 + c >= cols) continue;
            const size_t off = (static_cast<size_t>(r0 + r) * out_cols + dst_col + c0 + c) * poly + in_poly;
            W o[SV];
#pragma unroll
            for (int s = 0; s < SV; ++s) {
                o[s] = tile_reduce<W>(acc[r][c][s], q, lc);
                if (negate) o[s] = o[s] ? static_cast<W>(q - o[s]) : static_cast<W>(0);
            }
            if (addend) {
                W ad[SV];
                *reinterpret_cast<VT *>(ad) = *reinterpret_cast<const VT *>(addend + off);
#pragma unroll
                for (int s = 0; s < SV; ++s) o[s] = add_mod<W>(ad[s], o[s], q);
            }
            *reinterpret_cast<VT *>(out + off) = *reinterpret_cast<const VT *>(o);
        }
    }
}

// out's block = src's block +/- prod (rows x cols, dense): the combine pass behind a tuned product above 8 rows.  src is
// null, the addend or out itself (same thread reads and writes a word).  One thread per VN words.
template <typename W, int VN>
__global__ void __launch_bounds__(256)
    mul_sum_combine_kernel(W *out, const W *src, const W *__restrict__ prod, const LimbConst *__restrict__ limbs, size_t vecs, uint32_t cols,
                           uint32_t out_cols, uint32_t dst_col, uint32_t L, uint32_t N, int negate) {
    const size_t v = item_index();
    if (v >= vecs) return;
    typedef typename std::conditional<sizeof(W) * VN == 16, uint4, W>::type VT;
    static_assert(sizeof(VT) == sizeof(W) * VN, "vector width");
    const size_t per_limb = N / VN, per_poly = per_limb * L;
    const size_t p = v / per_poly, rem = v - p * per_poly;
    const uint32_t limb = static_cast<uint32_t>(rem / per_limb);
    const size_t r = p / cols, c = p - r * cols;
    const size_t off = ((r * out_cols + dst_col + c) * per_poly + rem) * VN;
    const W q = static_cast<W>(limbs[limb].q);
    W x[VN], o[VN];
    *reinterpret_cast<VT *>(x) = *reinterpret_cast<const VT *>(prod + v * VN);
    if (src) *reinterpret_cast<VT *>(o) = *reinterpret_cast<const VT *>(src + off);
#pragma unroll
    for (int s = 0; s < VN; ++s) {
        if (negate) x[s] = x[s] ? static_cast<W>(q - x[s]) : static_cast<W>(0);
        o[s] = src ? add_mod<W>(o[s], x[s], q) : x[s];
    }
    *reinterpret_cast<VT *>(out + off) = *reinterpret_cast<const VT *>(o);
}

namespace {

// what one call writes: rows x cols at column dst_col of an out that is out_cols wide
struct SumBlock {
    uint32_t rows, cols, out_cols, dst_col, L;
};

template <typename W, int TR, int TC, int SV>
int launch_sum_cfg(GpuContext *ctx, const MulSumArgs &args, uint32_t terms, size_t b_bytes, void *out, const void *addend,
                   const SumBlock &blk, int negate) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const TileGrid g = tile_grid<TR, TC, SV>(ctx, blk.rows, blk.cols, blk.L, b_bytes);  // its y extent: checked with the refusals
    W *o = static_cast<W *>(out);
    const W *ad = static_cast<const W *>(addend);
    bool streamed = false;  // the 64-bit tiles have no non-temporal instance
    if constexpr (sizeof(W) == 4) {
        if (g.streamed) {
            streamed = true;
            MXX_LAUNCH((matmul_sum_kernel<W, TR, TC, SV, true>), g.grid, dim3(g.threads), 0, ctx->stream, args, terms, o, ad, ctx->d_limbs,
                       blk.rows, blk.cols, blk.out_cols, blk.dst_col, blk.L, N, g.row_tiles, negate);
        }
    }
    if (!streamed)
        MXX_LAUNCH((matmul_sum_kernel<W, TR, TC, SV, false>), g.grid, dim3(g.threads), 0, ctx->stream, args, terms, o, ad, ctx->d_limbs,
                   blk.rows, blk.cols, blk.out_cols, blk.dst_col, blk.L, N, g.row_tiles, negate);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_sum(GpuContext *ctx, const MulSumArgs &args, uint32_t terms, size_t b_bytes, void *out, const void *addend, const SumBlock &blk,
               int negate) {
    return dispatch_stacked_tile(ctx, stacked_tile(ctx, blk.rows, blk.cols, blk.L), [&](auto cfg) {
        typedef decltype(cfg) T;
        return launch_sum_cfg<typename T::W, T::TR, T::TC, T::SV>(ctx, args, terms, b_bytes, out, addend, blk, negate);
    });
}

template <typename W>
int launch_combine(GpuContext *ctx, void *out, const void *src, const void *prod, const SumBlock &blk, int negate) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    constexpr int VN = 16 / sizeof(W);
    const size_t words = static_cast<size_t>(blk.rows) * blk.cols * blk.L * N;
    MXX_TRACE_BYTES(static_cast<double>(words) * sizeof(W) * (src ? 3 : 2));
    if (N >= static_cast<uint32_t>(VN))
        MXX_LAUNCH((mul_sum_combine_kernel<W, VN>), item_grid(words / VN, 256), dim3(256), 0, ctx->stream, static_cast<W *>(out),
                   static_cast<const W *>(src), static_cast<const W *>(prod), ctx->d_limbs, words / VN, blk.cols, blk.out_cols, blk.dst_col, blk.L,
                   N, negate);
    else
        MXX_LAUNCH((mul_sum_combine_kernel<W, 1>), item_grid(words, 256), dim3(256), 0, ctx->stream, static_cast<W *>(out),
                   static_cast<const W *>(src), static_cast<const W *>(prod), ctx->d_limbs, words, blk.cols, blk.out_cols, blk.dst_col, blk.L, N,
                   negate);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mul_sum_impl(const char *who, GpuMatrix *out, size_t dst_col, size_t cols, const GpuMatrix *addend, const GpuMatrix *const *lhss,
                 const GpuMatrix *const *rhss, size_t n, int negate) {
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    // ---- every refusal, for every t, before the first launch ----
    if (!out) return refuse("null output");
    if (n > 0 && (!lhss || !rhss)) return refuse("null array");
    for (size_t t = 0; t < n; ++t)
        if (!lhss[t] || !rhss[t]) return refuse("null matrix (term " + std::to_string(t) + ")");
    GpuContext *ctx = out->ctx;
    const int level = out->level;
    auto same_ring = [&](const GpuMatrix *m, const std::string &at) -> int {
        if (m->ctx != ctx) return refuse("context mismatch" + at);
        if (m->level != level) return refuse("level mismatch" + at);
        return 0;
    };
    if (addend && same_ring(addend, " (addend)")) return 1;
    for (size_t t = 0; t < n; ++t) {
        const std::string at = " (term " + std::to_string(t) + ")";
        if (same_ring(lhss[t], at) || same_ring(rhss[t], at)) return 1;
    }
    if (dst_col > out->cols || cols > out->cols - dst_col) return refuse("column block out of range");
    for (size_t t = 0; t < n; ++t)
        if (lhss[t]->cols != rhss[t]->rows || lhss[t]->rows != out->rows || rhss[t]->cols != cols)
            return refuse("shape mismatch (term " + std::to_string(t) + ")");
    if (addend && (addend->rows != out->rows || addend->cols != out->cols)) return refuse("addend shape mismatch");
    if (addend && addend->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format (addend)");
    for (size_t t = 0; t < n; ++t)
        if (lhss[t]->format != GPU_POLY_FORMAT_EVAL || rhss[t]->format != GPU_POLY_FORMAT_EVAL)
            return refuse("requires Eval format (term " + std::to_string(t) + ")");
    const bool whole = dst_col == 0 && cols == out->cols;
    if (!whole && out->format != GPU_POLY_FORMAT_EVAL) return refuse("a partial column block needs an output already in Eval format");
    // the addend's words are read and written by the same thread only when it is out's very block
    if (addend && partial_overlap(out, addend)) return refuse("the addend overlaps the output without being the same block");
    for (size_t t = 0; t < n; ++t)
        if (storage_overlaps(out, lhss[t]) || storage_overlaps(out, rhss[t]))
            return refuse("the output overlaps an operand (term " + std::to_string(t) + ")");
    const size_t L = matrix_limbs(out);
    bool any_inner = false;
    for (size_t t = 0; t < n; ++t) {
        if (lhss[t]->cols > 0xffffffffull) return refuse("matrix too large");
        any_inner = any_inner || lhss[t]->cols > 0;
    }
    if (out->rows > 0xffffffffull || out->cols > 0xffffffffull) return refuse("matrix too large");
    if (out->rows && cols) {  // the grid's y extent holds row tiles x column tiles
        const TileShape tl = stacked_tile(ctx, out->rows, cols, L);
        if (!tile_grid_fits(out->rows, cols, tl.tr, tl.tc)) return refuse("matrix too large");
    }
    // ---- accepted ----
    out->format = GPU_POLY_FORMAT_EVAL;
    if (out->rows == 0 || cols == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    // PACKED24 operands are unpacked here, all of them before the first launch (words_ptr)
    void *const o = words_ptr(out);
    const void *src = addend ? words_ptr(addend) : nullptr;
    std::vector<const void *> a(n), b(n);
    for (size_t t = 0; t < n; ++t) {
        a[t] = words_ptr(lhss[t]);
        b[t] = words_ptr(rhss[t]);
    }
    if (n == 0 && src == o) return 0;  // accumulate nothing in place
    const SumBlock blk{static_cast<uint32_t>(out->rows), static_cast<uint32_t>(cols), static_cast<uint32_t>(out->cols), static_cast<uint32_t>(dst_col),
                       static_cast<uint32_t>(L)};
    const double block_bytes = static_cast<double>(out->rows) * cols * L * ctx->N * ctx->word_bytes;

    // above 8 rows: the tuned products into scratch, one combine pass per term (MXX_HIP_MUL_SUM_PATH=tile keeps the
    // term-table kernel).  Terms without an inner dimension add nothing.
    if (out->rows > 8 && any_inner && ctx->env.mul_sum_path != 't') {
        GpuMatrix *tmp = nullptr;
        int rc = gpu_matrix_create(ctx, level, out->rows, cols, GPU_POLY_FORMAT_EVAL, &tmp);
        for (size_t t = 0; !rc && t < n; ++t) {
            if (lhss[t]->cols == 0) continue;
            rc = gpu_matrix_mul(tmp, lhss[t], rhss[t]);
            if (!rc) rc = ctx->wide ? launch_combine<uint64_t>(ctx, o, src, words_ptr(tmp), blk, negate)
                                    : launch_combine<uint32_t>(ctx, o, src, words_ptr(tmp), blk, negate);
            src = o;  // later terms accumulate onto what the earlier ones wrote
        }
        gpu_matrix_destroy(tmp);  // stream-ordered: behind the launches that read it
        return rc;
    }
    // up to 64 terms per launch; later launches read out's block as their addend.  n = 0 is one launch without terms: the
    // addend's block, or zeros, lands in out's block
    size_t t0 = 0;
    do {
        MulSumArgs args = {};
        const uint32_t terms = static_cast<uint32_t>(std::min(kMulSumMax, n - t0));
        double bytes = block_bytes * (src ? 2 : 1);
        size_t b_bytes = 0;
        for (uint32_t t = 0; t < terms; ++t) {
            args.item[t].a = a[t0 + t];
            args.item[t].b = b[t0 + t];
            args.item[t].k = static_cast<uint32_t>(lhss[t0 + t]->cols);
            bytes += static_cast<double>(lhss[t0 + t]->bytes) + static_cast<double>(rhss[t0 + t]->bytes);
            b_bytes += rhss[t0 + t]->bytes;
        }
        MXX_TRACE_BYTES(bytes);
        const int rc = launch_sum(ctx, args, terms, b_bytes, o, src, blk, negate);
        if (rc) return rc;
        src = o;
        t0 += terms;
    } while (t0 < n);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_mul_sum(GpuMatrix *out, size_t dst_col, size_t cols, const GpuMatrix *addend, const GpuMatrix *const *lhss,
                                      const GpuMatrix *const *rhss, size_t n, int negate) {
    ABI_GUARD_BEGIN
    return mul_sum_impl("gpupoly_matrix_mul_sum", out, dst_col, cols, addend, lhss, rhss, n, negate);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_mul_acc(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, int negate) {
    ABI_GUARD_BEGIN
    if (!out || !lhs || !rhs) return set_error("gpupoly_matrix_mul_acc: null matrix");
    return mul_sum_impl("gpupoly_matrix_mul_acc", out, 0, out->cols, out, &lhs, &rhs, 1, negate);
    ABI_GUARD_END
}
