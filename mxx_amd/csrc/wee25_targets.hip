// wee25_targets.hip — the preimage targets of T public-parameter indices x P column parts of the Wee25 commitment in one
// call: gpupoly_matrix_wee25_targets.
//
// The public parameters of the commitment ask for one preimage per index and column part (sample_public_params,
// src/commit/wee25.rs:494-758), and every target is (:696-728)
//
//   target(idx, p) = G_s J(idx, p) - W_idx T_bottom[:, p m_b .. (p + 1) m_b),        s x m_b,
//   W_idx = the s x m_b uniform matrix under hash_seed_for_matrix(key, "wee25_w_block_" || idx as 8 LE bytes),
//   J(idx, p) = the rows G^-1(row_i), i < s, of build_j_2m_block (:536-584).
//
// G_s G^-1(X) = X in every limb, so G_s J(idx, p) is the matrix X whose row i is row_i itself, and the index arithmetic of
// build_j_2m_block leaves exactly one row non-zero: with bg = idx / m_g, rho = idx mod m_g, row i* = rho / k carries
// g[kk] g[s'], kk = rho mod k, at the global columns bg k + s', s' < k.  With kk = (tw, e) and s' = (tw', e') that entry is
// the constant 2^((e + e') b) mod q_tw in every slot of limb tw when tw == tw', and zero elsewhere.  So for a group of
// blocks the stacked [W_0; W_1; ...] (the stacked block sample as it lies) against the window of T_bottom is ONE
// register-tiled product whose epilogue negates the reduced sum, adds the constant where it hits and stores the word
// straight into its output: G is never built, nothing is decomposed, and nothing is uploaded, launched or awaited per
// target.  The outputs' pointers, the rows' hits and the L dpt^2 constants go up in one staged copy per group.
#include "matmul_tile.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

struct Wee25Args {
    const void *w;          // stacked [W_0; ...]: rows x m_b
    const void *b;          // T_bottom, m_b x C
    const uint64_t *table;  // device: [Tg][Pg] output pointers, [Tg] {i*, bg k, kk}, [L][dpt][dpt] 2^((e + e') b) mod q_l
    size_t C;               // T_bottom's columns
    size_t gcol0;           // T_bottom's column of this launch's column 0
    uint32_t rows;          // Tg s stacked rows
    uint32_t s, m_b, cw;    // rows per block; inner dimension and width of a part; columns of this launch
    uint32_t Tg, Pg;        // blocks; parts this launch's columns touch, from part gcol0 / m_b
    uint32_t L, N, dpt, k, row_tiles;
};

// out(t, p)[i, cc] = X(t, p)[i, cc] - sum_j W[t s + i, j] T_bottom[j, gcol], gcol = gcol0 + column = p m_b + cc.
// blockIdx as in matmul_group_kernel: y = column tile * row_tiles + row tile, z = limb, x = SV slots per lane.  A column
// tile may cross a part boundary: the part and the local column are taken per tile column.
template <typename W, int TR, int TC, int SV, bool NTB>
__global__ void __launch_bounds__(256) wee25_targets_kernel(Wee25Args a, const LimbConst *__restrict__ limbs) {
    const uint32_t limb = blockIdx.z;
    const uint32_t row_tiles = a.row_tiles;
    const uint32_t ct = blockIdx.y / row_tiles, rt = blockIdx.y - ct * row_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const uint32_t N = a.N;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * SV;
    if (i >= N) return;
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    typedef typename TileTypes<W, SV>::VT VT;
    typedef typename TileTypes<W, SV>::wxs wxs;
    typedef typename TileTypes<W, SV>::D D;

    const size_t poly = static_cast<size_t>(a.L) * N;  // words per polynomial
    const size_t in_poly = static_cast<size_t>(limb) * N + i;
    const uint32_t inner = a.m_b;
    const W *B = static_cast<const W *>(a.b);
    // rows and columns past the end repeat the last one and are never stored
    const W *a_ptr[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r)
        a_ptr[r] = static_cast<const W *>(a.w) + static_cast<size_t>(min(r0 + r, a.rows - 1)) * inner * poly + in_poly;
    size_t b_off[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) b_off[c] = (a.gcol0 + min(c0 + c, a.cw - 1)) * poly + in_poly;
    const size_t strideBk = a.C * poly;

    D acc[TR][TC][SV];
    MXX_TILE_CLEAR(acc);
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
#define MXX_TILE_A(r, k) (a_ptr[r] + (k) * poly)
#define MXX_TILE_B(c, k) (B + b_off[c] + (k) * strideBk)
#include "matmul_tile_loop.inc"
    // epilogue: reduce, negate canonically, + the constant where (row, column, limb) is hit, store into the block's output
    const uint64_t *hits = a.table + static_cast<size_t>(a.Tg) * a.Pg;
    const uint64_t *consts = hits + static_cast<size_t>(a.Tg) * 3 + static_cast<size_t>(limb) * a.dpt * a.dpt;
    const size_t part0 = a.gcol0 / a.m_b;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (r0 + r >= a.rows) continue;
        const uint32_t t = (r0 + r) / a.s, row = (r0 + r) - t * a.s;
        const uint64_t bgk = hits[3 * t + 1];
        const uint32_t kk = static_cast<uint32_t>(hits[3 * t + 2]);
        const uint32_t tw = kk / a.dpt, e = kk - tw * a.dpt;
        const bool row_hit = hits[3 * t] == row && tw == limb;
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            if (c0 + c >= a.cw) continue;
            const size_t gcol = a.gcol0 + c0 + c;
            const size_t part = gcol / a.m_b;
            const uint32_t cc = static_cast<uint32_t>(gcol - part * a.m_b);
            W add = 0;
            const uint64_t sp = gcol - bgk;  // wraps to a huge value left of the hit
            if (row_hit && gcol >= bgk && sp < a.k) {
                const uint32_t tw2 = static_cast<uint32_t>(sp) / a.dpt, e2 = static_cast<uint32_t>(sp) - tw2 * a.dpt;
                if (tw2 == limb) add = static_cast<W>(consts[e * a.dpt + e2]);
            }
            W o[SV];
#pragma unroll
            for (int sl = 0; sl < SV; ++sl) {
                const W red = tile_reduce<W>(acc[r][c][sl], q, lc);
                o[sl] = add_mod<W>(red ? q - red : 0, add, q);
            }
            W *out = reinterpret_cast<W *>(a.table[static_cast<size_t>(t) * a.Pg + (part - part0)]);
            *reinterpret_cast<VT *>(out + (static_cast<size_t>(row) * a.m_b + cc) * poly + in_poly) = *reinterpret_cast<const VT *>(o);
        }
    }
}

template <typename W, int TR, int TC, int SV>
int launch_wee25_cfg(GpuContext *ctx, Wee25Args a, size_t b_bytes) {
    const TileGrid g = tile_grid<TR, TC, SV>(ctx, a.rows, a.cw, a.L, b_bytes);  // its y extent: checked by the caller
    a.row_tiles = g.row_tiles;
    bool streamed = false;  // the 64-bit tiles have no non-temporal instance
    if constexpr (sizeof(W) == 4) {
        if (g.streamed) {
            streamed = true;
            MXX_LAUNCH((wee25_targets_kernel<W, TR, TC, SV, true>), g.grid, dim3(g.threads), 0, ctx->stream, a, ctx->d_limbs);
        }
    }
    if (!streamed) MXX_LAUNCH((wee25_targets_kernel<W, TR, TC, SV, false>), g.grid, dim3(g.threads), 0, ctx->stream, a, ctx->d_limbs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what one accepted call works with
struct Wee25Call : RowCall {
    size_t s, m_b, C, T, P, part_start;
    const GpuMatrix *t_bottom;
};

// Everything both entries refuse, for every output, before anything is launched.  `full`: the sampling entry, whose tags
// are checked; otherwise the product-only entry with the stacked W given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, size_t P, const GpuMatrix *w_stacked, const GpuMatrix *t_bottom,
               size_t part_start, size_t secret_size, uint32_t base_bits, const uint64_t *idx, const GpuHashTags *tags, bool full,
               Wee25Call *call) {
    const Refuse refuse{who};
    if (T > ~size_t(0) / P) return refuse("matrix too large: blocks x parts overflows");
    const size_t count = T * P;
    auto part = [P](size_t j) { return std::to_string(j / P) + ", part " + std::to_string(j % P) + ")"; };
    auto at = [&](size_t j) { return " (block " + part(j); };
    if (!outs || !idx) return refuse("null array");
    if (!t_bottom || (!full && !w_stacked)) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, count, [&](size_t j) { return "null output (block " + part(j); })) return rc;
    if (secret_size == 0) return refuse("secret_size = 0");
    if (int rc = refuse_base_level(refuse, t_bottom, base_bits, full, call)) return rc;
    const size_t s = secret_size, m_b = t_bottom->rows, C = t_bottom->cols;
    if (t_bottom->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
    if (m_b == 0 || C % m_b != 0) return refuse("shape mismatch: T_bottom is m_b x (a multiple of m_b)");
    if (part_start > C / m_b || P > C / m_b - part_start) return refuse("column parts past T_bottom's columns");
    if (s > 0xffffffffull || m_b > 0xffffffffull || T > ~size_t(0) / s) return refuse("matrix too large");
    if (w_stacked)
        if (int rc = refuse_operand(refuse, w_stacked, *call, T * s, m_b, "shape mismatch: the stacked W is (blocks * secret_size) x m_b")) return rc;
    if (int rc = refuse_outputs(refuse, outs, count, *call, at, [&](const GpuMatrix *out) {
            return out->rows != s || out->cols != m_b ? "shape mismatch: an output is secret_size x m_b" : nullptr;
        }))
        return rc;
    call->s = s, call->m_b = m_b, call->C = C, call->T = T, call->P = P, call->part_start = part_start, call->t_bottom = t_bottom;
    // an output is written while every operand is still being read, and by no other tile
    const GpuMatrix *operands[2] = {t_bottom, w_stacked};
    static const char *const names[2] = {"T_bottom", "the stacked W"};
    return refuse_tags_overlap(refuse, full ? tags : nullptr, T, outs, count, operands, names, w_stacked ? 2 : 1);
}

bool grid_fits(const GpuContext *ctx, size_t rows, size_t cols, size_t L) {
    const TileShape t = stacked_tile(ctx, rows, cols, L);
    return tile_grid_fits(rows, cols, t.tr, t.tc);
}

// blocks [t0, t0 + Tg) against the window's columns [col0, col0 + cw) (counted from the window's first column): the table
// in one staged copy, then the one product launch.  `w`: the stacked W of these blocks, (Tg s) x m_b words
int product_group(const Wee25Call &call, GpuMatrix *const *outs, const uint64_t *idx, size_t t0, size_t Tg, size_t col0, size_t cw, const void *w) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, dpt = call.dpt, m_b = call.m_b, m_g = call.s * call.k;
    const size_t gcol0 = call.part_start * m_b + col0;
    const size_t part0 = gcol0 / m_b, Pg = (gcol0 + cw - 1) / m_b - part0 + 1;
    static thread_local std::vector<uint64_t> staging, pw;
    staging.resize(Tg * Pg + Tg * 3 + L * dpt * dpt);
    uint64_t *hits = staging.data() + Tg * Pg, *consts = hits + Tg * 3;
    for (size_t t = 0; t < Tg; ++t) {
        for (size_t p = 0; p < Pg; ++p)
            staging[t * Pg + p] = reinterpret_cast<uint64_t>(words_ptr(outs[(t0 + t) * call.P + (part0 - call.part_start) + p]));
        const uint64_t id = idx[t0 + t], bg = id / m_g, rho = id - bg * m_g;
        hits[3 * t] = rho / call.k;      // i*
        hits[3 * t + 1] = bg * call.k;   // the first global column: at most id
        hits[3 * t + 2] = rho % call.k;  // kk
    }
    pw.resize(2 * dpt);
    for (size_t l = 0; l < L; ++l) {
        base_powers(ctx->moduli[l], call.base_bits, 2 * dpt, pw.data());
        for (size_t e = 0; e < dpt; ++e)
            for (size_t e2 = 0; e2 < dpt; ++e2) consts[(l * dpt + e) * dpt + e2] = pw[e + e2];
    }
    CtxBlock block(ctx);
    if (upload_table(block, "Wee25 target table (host to device)", staging)) return 1;
    Wee25Args a;
    a.w = w;
    a.b = words_ptr(call.t_bottom);
    a.table = static_cast<const uint64_t *>(block.ptr);
    a.C = call.C;
    a.gcol0 = gcol0;
    a.rows = static_cast<uint32_t>(Tg * call.s);
    a.s = static_cast<uint32_t>(call.s);
    a.m_b = static_cast<uint32_t>(m_b);
    a.cw = static_cast<uint32_t>(cw);
    a.Tg = static_cast<uint32_t>(Tg);
    a.Pg = static_cast<uint32_t>(Pg);
    a.L = call.L;
    a.N = static_cast<uint32_t>(ctx->N);
    a.dpt = call.dpt;
    a.k = static_cast<uint32_t>(call.k);
    a.row_tiles = 0;
    const size_t poly_bytes = L * static_cast<size_t>(ctx->N) * ctx->word_bytes;
    const size_t b_bytes = m_b * cw * poly_bytes;
    // the stacked W and the window read once, every target word written once
    MXX_TRACE_BYTES(static_cast<double>(poly_bytes) * (static_cast<double>(a.rows) * m_b + static_cast<double>(m_b) * cw + static_cast<double>(a.rows) * cw));
    static const std::string name = "wee25_targets_kernel (stacked W blocks x T_bottom window x slots per lane; negation, constant and scatter in the epilogue)";
    ctx->last_kernel = name.c_str();
    return dispatch_stacked_tile(ctx, stacked_tile(ctx, a.rows, cw, L), [&](auto cfg) {
        typedef decltype(cfg) T;
        return launch_wee25_cfg<typename T::W, T::TR, T::TC, T::SV>(ctx, a, b_bytes);
    });
}

// the product launches of blocks [t0, t0 + Tg): one where the grid fits, else split by blocks, then by columns
int product_blocks(const Wee25Call &call, GpuMatrix *const *outs, const uint64_t *idx, size_t t0, size_t Tg, const void *w) {
    const size_t cols = call.P * call.m_b;
    const size_t poly_bytes = static_cast<size_t>(call.L) * call.ctx->N * call.ctx->word_bytes;
    size_t step = Tg;
    while (step > 1 && !grid_fits(call.ctx, step * call.s, cols, call.L)) step = (step + 1) / 2;
    size_t cw = cols;
    while (cw > 1 && !grid_fits(call.ctx, step * call.s, cw, call.L)) cw = (cw + 1) / 2;
    for (size_t t = 0; t < Tg; t += step) {
        const size_t n = std::min(step, Tg - t);
        const char *wt = static_cast<const char *>(w) + t * call.s * call.m_b * poly_bytes;
        for (size_t c = 0; c < cols; c += cw)
            if (int rc = product_group(call, outs, idx, t0 + t, n, c, std::min(cw, cols - c), wt)) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_wee25_targets(GpuMatrix *const *outs, size_t nblocks_T, size_t nparts_P, const GpuMatrix *t_bottom,
                                            size_t part_start, size_t secret_size, uint32_t base_bits, const uint64_t *idx,
                                            const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_wee25_targets";
    const size_t T = nblocks_T, P = nparts_P;
    if (T == 0 || P == 0) return 0;
    Wee25Call call;
    if (check_call(who, outs, T, P, nullptr, t_bottom, part_start, secret_size, base_bits, idx, tags, true, &call)) return 1;
    GpuContext *ctx = call.ctx;
    // a group's W scratch is (Tg s) x m_b
    const size_t block_bytes = call.s * call.m_b * static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    if (!grid_fits(ctx, call.s, 1, call.L)) return set_error(std::string(who) + ": matrix too large");
    // ---- accepted ----
    for (size_t j = 0; j < T * P; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    if (ctx_activate(ctx)) return 1;
    words_ptr(t_bottom);  // a PACKED24 operand is unpacked once
    CtxBlock w(ctx);
    if (w.alloc(rows_per_group(T, block_bytes) * block_bytes)) return 1;
    return for_row_groups(T, block_bytes, tags, [&](size_t t0, size_t Tg, const GpuHashTags &part) {
        // row t of the stacked layout = the s m_b polynomials of block t row-major: the (Tg s) x m_b factor as it lies
        GpuMatrix v = scratch_matrix(ctx, call.level, Tg, call.s * call.m_b, w.ptr);
        if (int rc = sample_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, GPUPOLY_BLOCKS_STACKED, nullptr, nullptr)) return rc;
        return product_blocks(call, outs, idx, t0, Tg, w.ptr);
    });
    ABI_GUARD_END
}

// The same with [W_0; W_1; ...] given instead of sampled: the product kernel alone.  A test instrument
// (tests/test_gpu_wee25_targets.py reaches the lazy accumulator's bound with operands no sampler gives).
extern "C" int gpupoly_matrix_wee25_targets_product(GpuMatrix *const *outs, size_t nblocks_T, size_t nparts_P, const GpuMatrix *w_stacked,
                                                    const GpuMatrix *t_bottom, size_t part_start, size_t secret_size, uint32_t base_bits,
                                                    const uint64_t *idx) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_wee25_targets_product";
    const size_t T = nblocks_T, P = nparts_P;
    if (T == 0 || P == 0) return 0;
    Wee25Call call;
    if (check_call(who, outs, T, P, w_stacked, t_bottom, part_start, secret_size, base_bits, idx, nullptr, false, &call)) return 1;
    if (!grid_fits(call.ctx, call.s, 1, call.L)) return set_error(std::string(who) + ": matrix too large");
    for (size_t j = 0; j < T * P; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    if (ctx_activate(call.ctx)) return 1;
    words_ptr(t_bottom);
    return product_blocks(call, outs, idx, 0, T, words_ptr(w_stacked));
    ABI_GUARD_END
}
