// ggh15_lookup.hip — stage 2 of the GGH15 online public lookup for S slots of one gate and one output column chunk in one
// call: gpupoly_matrix_ggh15_lookup.
//
// The evaluator's build_public_lookup_output_chunk (src/lookup/ggh15/encoding.rs:172-300; the device path is
// src/lookup/ggh15/poly_encoding_gpu.rs:338-567,686-1420, one product per task) computes, per slot s and column chunk,
//
//   out_s[:, chunk] = c_b0_s P_id[:, chunk] + c_b0_s (P_gy G^-1(G_d[:, chunk] o y_s)) + c_b0_s (P_v V_s) + c_b0_s (P_vx (V_s o x_s))
//                     - c_b0_s (P_g1 K_s) + sum over inner chunks (c_in_s G^-1(U_g)) V_s,
//
// V_s = G^-1 of columns `chunk` of the d x m_g uniform matrix under hash_seed_for_matrix(key, "ggh15_lut_v_idx_<lut>_<k_s>"),
// K_s the stored chunk of the LUT-row preimage, (k_s, y_s) = plt.get(x_s).  Everything is exact ring arithmetic on canonical
// residues, so the products re-associate without changing a bit.  Stage 1 - the caller's, with the library's product
// entries - is what depends on neither the LUT row nor the chunk: the stacked c_b0 / c_in against P_id, P_gy, P_v, P_vx,
// P_g1 and G^-1(U_g), which gives the six `mid` matrices with slot s in rows [s r, (s + 1) r).  Stage 2, this file:
//
//   out_s[:, chunk] = mid_id_s[:, chunk] + mid_gy_s G^-1(G_d[:, chunk] o y_s) + (mid_v_s + x_s o mid_vx_s + mid_rand_s) V_s - mid_g1_s K_s.
//
// Column c0 + cc of G_d is (j, tw, e) and y_s is a constant, so the second term is sum_{e' < dpt} weight(s, cc, e') *
// mid_gy_s[:, (j, tw, e')] in every limb (lut_targets.hip's rule, here for every row).  Per group of slots: one staged copy
// of the slots' table (output, K_s and x_s pointers, the weights - computed on the host, ggh15_weights.h), the
// decomposed-blocks sample [V_0 | V_1 | ...], one pre-pass kernel that writes the stacked left factor Lhs = [mid_v + x_s o mid_vx + mid_rand | neg(mid_g1)]
// (canonical, neg(0) = 0) so that every product term is additive, and ONE main kernel that forms every output word in one
// lazy accumulator - mid_id's word, the m_g terms against V_s, the w terms against K_s read in place through the table, the
// dpt weighted words of mid_gy - folded every LimbConst::lazy_terms terms wherever they fall, reduced once and stored once
// straight into outs[s].  Nothing is uploaded, launched or awaited per slot.
#include "common.h"
#include "ggh15_weights.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

// the group's device table: [S] output pointers, [S] K_s pointers, [S] x_s pointers, then [S c][L][dpt] weights
struct LookupArgs {
    const void *mid_id, *mid_gy;  // the group's rows of the stage-1 products: (S r) x m_g
    const void *lhs;              // (S r) x (m_g + w)
    const void *v;                // m_g x (S c): slot s at columns [s c, (s + 1) c)
    const uint64_t *table;
    size_t m_g, w, col_start, k, entries;
    uint32_t S, r, c, L, dpt, logN, row_tiles, col_tiles;
};

struct LhsArgs {
    const void *mid_v, *mid_vx, *mid_rand;  // the group's rows: (S r) x m_g
    const void *mid_g1;                     // (S r) x w
    void *lhs;                              // (S r) x (m_g + w)
    const uint64_t *xs;                     // device: [S] x_s pointers
    size_t m_g, w, polys;                   // polys = S r (m_g + w)
    uint32_t r, L, logN;
};

// Lhs[(s r + i), rho] = mid_v + x_s o mid_vx + mid_rand for rho < m_g, q - mid_g1 (0 stays 0) behind it; VN words per thread
template <typename W, int VN>
__global__ void __launch_bounds__(256) ggh15_lookup_lhs_kernel(LhsArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN, vecs = wpp / VN;
    const size_t item = item_index();
    if (item >= a.polys * vecs) return;
    const size_t poly = item / vecs, w0 = (item - poly * vecs) * VN;
    const size_t inner = a.m_g + a.w;
    const size_t row = poly / inner, rho = poly - row * inner;
    const LimbConst lc = limbs[w0 >> a.logN];
    const W q = static_cast<W>(lc.q);
    W o[VN];
    if (rho < a.m_g) {
        const size_t at = (row * a.m_g + rho) * wpp + w0;
        W v[VN], vx[VN], rd[VN], x[VN];
        *reinterpret_cast<V *>(v) = *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_v) + at);
        *reinterpret_cast<V *>(vx) = *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_vx) + at);
        *reinterpret_cast<V *>(rd) = *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_rand) + at);
        *reinterpret_cast<V *>(x) = *reinterpret_cast<const V *>(reinterpret_cast<const W *>(a.xs[row / a.r]) + w0);
#pragma unroll
        for (int i = 0; i < VN; ++i) o[i] = add_mod<W>(add_mod<W>(v[i], mul_mod<W>(x[i], vx[i], q, lc.mu, lc.kbits), q), rd[i], q);
    } else {
        W g[VN];
        *reinterpret_cast<V *>(g) = *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_g1) + (row * a.w + (rho - a.m_g)) * wpp + w0);
#pragma unroll
        for (int i = 0; i < VN; ++i) o[i] = g[i] ? q - g[i] : 0;
    }
    *reinterpret_cast<V *>(static_cast<W *>(a.lhs) + poly * wpp + w0) = *reinterpret_cast<const V *>(o);
}

// A block's tile: rows [r0, r0 + TR) x chunk columns [c0, c0 + TC) of slot s (blockIdx.y/z), blockIdx.x strides the
// polynomial's L N words VN per lane (16 bytes, or one word where a limb vector is narrower; VN divides N: one limb per
// vector).  A lane keeps the TR left words of a term in registers for all TC columns, and every word of V_s and K_s is
// loaded by one tile only (TR = r where r <= 2).  Rows and columns past the end repeat the last one and are never stored.
// The TR x TC x VN sums share one count of pending terms - LazyAcc's rule (row_targets.h) with the count kept once.
template <typename W, int VN, int TR, int TC>
__global__ void __launch_bounds__(256) ggh15_lookup_kernel(LookupArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const uint32_t per_slot = a.row_tiles * a.col_tiles;
    const size_t s = entry / per_slot;
    const uint32_t rest = static_cast<uint32_t>(entry - s * per_slot);
    const uint32_t rt = rest / a.col_tiles, ct = rest - rt * a.col_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN;
    const size_t inner = a.m_g + a.w;
    const W *ksrc = reinterpret_cast<const W *>(a.table[a.S + s]);
    W *out = reinterpret_cast<W *>(a.table[s]);
    const uint64_t *weights = a.table + 3 * static_cast<size_t>(a.S);
    size_t row[TR], cc[TC];
#pragma unroll
    for (int i = 0; i < TR; ++i) row[i] = s * a.r + min(r0 + i, a.r - 1);
#pragma unroll
    for (int j = 0; j < TC; ++j) cc[j] = min(c0 + j, a.c - 1);
    const size_t v_stride = static_cast<size_t>(a.S) * a.c * wpp, k_stride = static_cast<size_t>(a.c) * wpp;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.logN);
        const LimbConst lc = limbs[l];
        const uint32_t lazy = lc.lazy_terms;
        uint32_t pending = 0;
        D acc[TR][TC][VN];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                W first[VN];
                *reinterpret_cast<V *>(first) =
                    *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_id) + (row[i] * a.m_g + a.col_start + cc[j]) * wpp + w0);
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[i][j][x] = first[x];
            }
        auto fold = [&]() {
#pragma unroll
            for (int i = 0; i < TR; ++i)
#pragma unroll
                for (int j = 0; j < TC; ++j)
#pragma unroll
                    for (int x = 0; x < VN; ++x) acc[i][j][x] = lazy_reduce<W>(acc[i][j][x], lc);
            pending = 0;
        };
        // `count` terms Lhs[row, lhs0 + rho] * B[rho, column], B's column j at b[j] + rho * stride
        auto stream = [&](size_t lhs0, size_t count, const W *(&b)[TC], size_t stride) {
            for (size_t rho = 0; rho < count; ++rho) {
                W av[TR][VN], bv[TC][VN];
#pragma unroll
                for (int i = 0; i < TR; ++i)
                    *reinterpret_cast<V *>(av[i]) =
                        *reinterpret_cast<const V *>(static_cast<const W *>(a.lhs) + (row[i] * inner + lhs0 + rho) * wpp + w0);
#pragma unroll
                for (int j = 0; j < TC; ++j) *reinterpret_cast<V *>(bv[j]) = *reinterpret_cast<const V *>(b[j] + rho * stride + w0);
                if (pending >= lazy) fold();
#pragma unroll
                for (int i = 0; i < TR; ++i)
#pragma unroll
                    for (int j = 0; j < TC; ++j)
#pragma unroll
                        for (int x = 0; x < VN; ++x) acc[i][j][x] += static_cast<D>(av[i][x]) * bv[j][x];
                ++pending;
            }
        };
        const W *vb[TC], *kb[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            vb[j] = static_cast<const W *>(a.v) + (s * a.c + cc[j]) * wpp;
            kb[j] = ksrc + cc[j] * wpp;
        }
        stream(0, a.m_g, vb, v_stride);
        stream(a.m_g, a.w, kb, k_stride);
        // the epilogue's terms: dpt weighted words of mid_gy's row, from the block (j, tw, .) of the column
        for (uint32_t ep = 0; ep < a.dpt; ++ep) {
            if (pending >= lazy) fold();
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                const size_t col = a.col_start + cc[j];
                const size_t jb = col / a.k;
                const uint32_t tw = static_cast<uint32_t>(col - jb * a.k) / a.dpt;
                const W wt = static_cast<W>(weights[((s * a.c + cc[j]) * a.L + l) * a.dpt + ep]);
                const size_t gcol = jb * a.k + static_cast<size_t>(tw) * a.dpt + ep;
#pragma unroll
                for (int i = 0; i < TR; ++i) {
                    W gv[VN];
                    *reinterpret_cast<V *>(gv) = *reinterpret_cast<const V *>(static_cast<const W *>(a.mid_gy) + (row[i] * a.m_g + gcol) * wpp + w0);
#pragma unroll
                    for (int x = 0; x < VN; ++x) acc[i][j][x] += static_cast<D>(wt) * gv[x];
                }
            }
            ++pending;
        }
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            if (r0 + i >= a.r) continue;
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                if (c0 + j >= a.c) continue;
                W o[VN];
#pragma unroll
                for (int x = 0; x < VN; ++x) o[x] = lazy_reduce<W>(acc[i][j][x], lc);
                *reinterpret_cast<V *>(out + (static_cast<size_t>(r0 + i) * a.c + (c0 + j)) * wpp + w0) = *reinterpret_cast<const V *>(o);
            }
        }
    }
}

// what one accepted call works with: S slots of r rows; mids (S r) x m_g, mid_gate1 (S r) x w, K_s w x c, outputs r x c
struct LookupCall : RowCall {
    size_t S, r, d, m_g, w, c, col_start;
    const GpuMatrix *mids[6];  // identity, gy, v, vx, rand, gate1
    size_t cap;                // a group's scratch
};

// Everything both entries refuse, for every slot, before anything is launched.  `digits` null: the sampling entry, whose
// tags are checked; otherwise the combine entry with [V_0 | V_1 | ...] given.
int check_call(const char *who, GpuMatrix *const *outs, size_t S, const GpuMatrix *const (&mids)[6], const GpuMatrix *const *luts,
               const GpuMatrix *const *xs, const GpuMatrix *digits, bool full, size_t col_start, uint32_t base_bits, const uint64_t *y_words,
               size_t words_per_y, const GpuHashTags *tags, LookupCall *call) {
    const Refuse refuse{who};
    if (!outs || !luts || !xs || !y_words) return refuse("null array");
    for (const GpuMatrix *m : mids)
        if (!m) return refuse("null operand");
    if (!full && !digits) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, S, [](size_t s) { return "null output" + slot_at(s); })) return rc;
    for (size_t s = 0; s < S; ++s)
        if (!luts[s] || !xs[s]) return refuse("null operand" + slot_at(s));
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (int rc = refuse_base_level(refuse, mids[0], base_bits, full, call)) return rc;
    const size_t rows = mids[0]->rows, m_g = mids[0]->cols, c = outs[0]->cols;
    if (rows % S != 0) return refuse("shape mismatch: the stage-1 products have slots * r rows");
    if (m_g % call->k != 0) return refuse("shape mismatch: the stage-1 products have d * digits per tower * limbs columns");
    const size_t r = rows / S, d = m_g / call->k, w = m_g + 2 * d;
    for (int j = 0; j < 6; ++j)
        if (int rc = refuse_operand(refuse, mids[j], *call, rows, j == 5 ? w : m_g,
                                    "shape mismatch: the stage-1 products are (slots * r) x m_g, mid_gate1 (slots * r) x d * (digits + 2)"))
            return rc;
    if (col_start > m_g || c > m_g - col_start) return refuse("column chunk past the operands' columns");
    if (rows > 0xffffffffull || c > 0xffffffffull || S > 0xffffffffull || c > ~size_t(0) / S) return refuse("matrix too large");
    for (size_t s = 0; s < S; ++s) {
        if (int rc = refuse_foreign(refuse, luts[s], *call, slot_at(s))) return rc;
        if (int rc = refuse_foreign(refuse, xs[s], *call, slot_at(s))) return rc;
        if (luts[s]->rows != w || luts[s]->cols != c) return refuse("shape mismatch: a LUT-row preimage chunk is d * (digits + 2) x chunk columns" + slot_at(s));
        if (xs[s]->rows != 1 || xs[s]->cols != 1) return refuse("shape mismatch: a slot's plaintext is 1 x 1" + slot_at(s));
        if (luts[s]->format != GPU_POLY_FORMAT_EVAL || xs[s]->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + slot_at(s));
    }
    if (digits)
        if (int rc = refuse_operand(refuse, digits, *call, m_g, S * c, "shape mismatch: the digits are m_g x (slots * chunk columns)")) return rc;
    if (int rc = refuse_outputs(refuse, outs, S, *call, slot_at, [&](const GpuMatrix *out) -> const char * {
            if (out->cols != c) return "the outputs differ in width";
            return out->rows != r ? "shape mismatch: an output is r x chunk columns" : nullptr;
        }))
        return rc;
    call->S = S, call->r = r, call->d = d, call->m_g = m_g, call->w = w, call->c = c, call->col_start = col_start;
    for (int j = 0; j < 6; ++j) call->mids[j] = mids[j];
    call->cap = call->ctx->env.ggh15_lookup_budget ? call->ctx->env.ggh15_lookup_budget : kRowGroupBytes;
    // an output is written while every operand is still being read, and by no other slot
    const GpuMatrix *operands[7] = {mids[0], mids[1], mids[2], mids[3], mids[4], mids[5], digits};
    static const char *const names[7] = {"a stage-1 product", "a stage-1 product", "a stage-1 product", "a stage-1 product",
                                         "a stage-1 product", "a stage-1 product", "the digits"};
    if (int rc = refuse_tags_overlap(refuse, full ? tags : nullptr, S, outs, S, operands, names, digits ? 7 : 6)) return rc;
    const std::string overlap = slot_operands_overlap(outs, S, {luts, xs});
    return overlap.empty() ? 0 : refuse(overlap);
}

// the column tile and the row tile of a call, and its blocks' grid for Sg slots; false: too many tiles for one grid
struct LookupTiles {
    int tr, tc;
    uint32_t row_tiles, col_tiles;
};
LookupTiles lookup_tiles(const LookupCall &call) {
    LookupTiles t;
    t.tr = call.r >= 2 ? 2 : 1;
    t.tc = call.c >= 3 ? 4 : call.c == 2 ? 2 : 1;  // (an empty chunk has no tiles: one column per tile, none of them)
    t.row_tiles = static_cast<uint32_t>((call.r + t.tr - 1) / t.tr);
    t.col_tiles = static_cast<uint32_t>((call.c + t.tc - 1) / t.tc);
    return t;
}
bool grid_fits(const LookupCall &call, size_t Sg) {
    const LookupTiles t = lookup_tiles(call);
    return Sg * t.row_tiles * t.col_tiles <= size_t(65535) * 65535;
}

template <typename W, int VN>
int launch_main(GpuContext *ctx, const LookupArgs &a, const LookupTiles &t, dim3 grid, dim3 block) {
#define MXX_LOOKUP_TILE(R, Cc) \
    if (t.tr == R && t.tc == Cc) MXX_LAUNCH((ggh15_lookup_kernel<W, VN, R, Cc>), grid, block, 0, ctx->stream, a, ctx->d_limbs)
    MXX_LOOKUP_TILE(1, 1);
    MXX_LOOKUP_TILE(1, 2);
    MXX_LOOKUP_TILE(1, 4);
    MXX_LOOKUP_TILE(2, 1);
    MXX_LOOKUP_TILE(2, 2);
    MXX_LOOKUP_TILE(2, 4);
#undef MXX_LOOKUP_TILE
    HIP_TRY(hipGetLastError());
    return 0;
}

// slots [s0, s0 + Sg) with their digits at `v` (m_g x (Sg c) words): the table in one staged copy, the pre-pass into
// `lhs` ((Sg r) x (m_g + w) words), the main kernel
int combine_group(const LookupCall &call, GpuMatrix *const *outs, const GpuMatrix *const *luts, const GpuMatrix *const *xs, size_t s0, size_t Sg,
                  const void *v, void *lhs, const uint64_t *y_words, size_t words_per_y) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, dpt = call.dpt, c = call.c;
    static thread_local std::vector<uint64_t> staging;
    staging.resize(3 * Sg + Sg * c * L * dpt);
    uint64_t *weights = staging.data() + 3 * Sg;
    for (size_t s = 0; s < Sg; ++s) {
        staging[s] = reinterpret_cast<uint64_t>(words_ptr(outs[s0 + s]));
        staging[Sg + s] = reinterpret_cast<uint64_t>(words_ptr(luts[s0 + s]));
        staging[2 * Sg + s] = reinterpret_cast<uint64_t>(words_ptr(xs[s0 + s]));
        // weight(s, cc, l, e') for column col_start + cc = (j, tw, e): ggh15_weights.h
        const uint64_t *y = y_words + (s0 + s) * words_per_y;
        for (size_t cc = 0; cc < c; ++cc) {
            const size_t rem = (call.col_start + cc) % call.k, tw = rem / dpt, e = rem - tw * dpt;
            const uint64_t q = ctx->moduli[tw];
            ggh15::gy_weights(words_mod(y, words_per_y, q), q, call.base_bits, call.dpt, static_cast<uint32_t>(e), ctx->moduli.data(), L,
                              weights + (s * c + cc) * L * dpt);
        }
    }
    CtxBlock block(ctx);
    if (upload_table(block, "GGH15 lookup slot table (host to device)", staging)) return 1;
    const uint64_t *d_table = static_cast<const uint64_t *>(block.ptr);
    const size_t wpp = L << ctx->logN, poly_bytes = wpp * ctx->word_bytes;
    const size_t row0 = s0 * call.r;  // the group's first row of the stage-1 products
    auto rows_of = [&](int j) { return static_cast<const char *>(words_ptr(call.mids[j])) + row0 * (j == 5 ? call.w : call.m_g) * poly_bytes; };
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;

    LhsArgs la;
    la.mid_v = rows_of(2), la.mid_vx = rows_of(3), la.mid_rand = rows_of(4), la.mid_g1 = rows_of(5);
    la.lhs = lhs;
    la.xs = d_table + 2 * Sg;
    la.m_g = call.m_g, la.w = call.w, la.polys = Sg * call.r * (call.m_g + call.w);
    la.r = static_cast<uint32_t>(call.r), la.L = call.L, la.logN = ctx->logN;
    const size_t items = la.polys * (wpp / vn);
    // mid_v, mid_vx, mid_rand and mid_gate1 read once, Lhs written once
    MXX_TRACE_BYTES(static_cast<double>(Sg * call.r) * poly_bytes * (4.0 * call.m_g + 2.0 * call.w));
    if (ctx->wide && vn > 1) MXX_LAUNCH((ggh15_lookup_lhs_kernel<uint64_t, 2>), item_grid(items, 256), dim3(256), 0, ctx->stream, la, ctx->d_limbs);
    else if (ctx->wide) MXX_LAUNCH((ggh15_lookup_lhs_kernel<uint64_t, 1>), item_grid(items, 256), dim3(256), 0, ctx->stream, la, ctx->d_limbs);
    else if (vn > 1) MXX_LAUNCH((ggh15_lookup_lhs_kernel<uint32_t, 4>), item_grid(items, 256), dim3(256), 0, ctx->stream, la, ctx->d_limbs);
    else MXX_LAUNCH((ggh15_lookup_lhs_kernel<uint32_t, 1>), item_grid(items, 256), dim3(256), 0, ctx->stream, la, ctx->d_limbs);
    HIP_TRY(hipGetLastError());

    const LookupTiles t = lookup_tiles(call);
    LookupArgs a;
    a.mid_id = rows_of(0), a.mid_gy = rows_of(1);
    a.lhs = lhs, a.v = v, a.table = d_table;
    a.m_g = call.m_g, a.w = call.w, a.col_start = call.col_start, a.k = call.k;
    a.entries = Sg * t.row_tiles * t.col_tiles;
    a.S = static_cast<uint32_t>(Sg), a.r = static_cast<uint32_t>(call.r), a.c = static_cast<uint32_t>(c);
    a.L = call.L, a.dpt = call.dpt, a.logN = ctx->logN, a.row_tiles = t.row_tiles, a.col_tiles = t.col_tiles;
    const size_t vecs = wpp / vn;
    size_t gy, gz;
    (void)fold_yz(a.entries, gy, gz);  // grid_plan.h; the count was held to 65535 x 65535 with the refusals (grid_fits)
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // [V_s; K_s] read once per row tile, Lhs once per column tile, mid_id's chunk and mid_gy's dpt words per output word, the
    // outputs written once
    MXX_TRACE_BYTES(static_cast<double>(Sg) * poly_bytes *
                    (static_cast<double>(t.row_tiles) * (call.m_g + call.w) * c + static_cast<double>(t.col_tiles) * call.r * (call.m_g + call.w) +
                     static_cast<double>(call.r) * c * (2.0 + call.dpt)));
    if (ctx->wide && vn > 1) return launch_main<uint64_t, 2>(ctx, a, t, grid, dim3(threads));
    if (ctx->wide) return launch_main<uint64_t, 1>(ctx, a, t, grid, dim3(threads));
    if (vn > 1) return launch_main<uint32_t, 4>(ctx, a, t, grid, dim3(threads));
    return launch_main<uint32_t, 1>(ctx, a, t, grid, dim3(threads));
}

// after the refusals: the outputs' tags, then (*go) whether anything is left to launch; PACKED24 operands unpacked once
int accept(const LookupCall &call, GpuMatrix *const *outs, const GpuMatrix *const *luts, const GpuMatrix *const *xs, const GpuMatrix *digits, bool *go) {
    for (size_t s = 0; s < call.S; ++s) outs[s]->format = GPU_POLY_FORMAT_EVAL;
    *go = call.r != 0 && call.c != 0;
    if (!*go) return 0;
    if (ctx_activate(call.ctx)) return 1;
    for (const GpuMatrix *m : call.mids) words_ptr(m);
    for (size_t s = 0; s < call.S; ++s) words_ptr(luts[s]), words_ptr(xs[s]), words_ptr(outs[s]);
    if (digits) words_ptr(digits);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_ggh15_lookup(GpuMatrix *const *outs, size_t nslots_S, const GpuMatrix *mid_identity, const GpuMatrix *mid_gy,
                                           const GpuMatrix *mid_v, const GpuMatrix *mid_vx, const GpuMatrix *mid_rand, const GpuMatrix *mid_gate1,
                                           const GpuMatrix *const *lut_preimages, const GpuMatrix *const *xs, size_t col_start, uint32_t base_bits,
                                           const uint64_t *y_words, size_t words_per_y, const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_ggh15_lookup";
    const size_t S = nslots_S;
    if (S == 0) return 0;
    const GpuMatrix *const mids[6] = {mid_identity, mid_gy, mid_v, mid_vx, mid_rand, mid_gate1};
    LookupCall call;
    if (check_call(who, outs, S, mids, lut_preimages, xs, nullptr, true, col_start, base_bits, y_words, words_per_y, tags, &call)) return 1;
    GpuContext *ctx = call.ctx;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // a slot's scratch: its digits m_g x c and its rows of the left factor r x (m_g + w)
    const size_t v_bytes = call.m_g * call.c * poly_bytes, lhs_bytes = call.r * (call.m_g + call.w) * poly_bytes;
    const size_t slot_bytes = std::max<size_t>(v_bytes + lhs_bytes, 1);
    const size_t per_group = rows_per_group(S, slot_bytes, call.cap);
    if (!grid_fits(call, per_group)) return set_error(std::string(who) + ": too many output tiles in one group");
    // ---- accepted ----
    bool go;
    if (accept(call, outs, lut_preimages, xs, nullptr, &go)) return 1;
    if (!go) return 0;
    CtxBlock digits(ctx), lhs(ctx);
    if (digits.alloc(per_group * v_bytes)) return 1;
    if (lhs.alloc(per_group * lhs_bytes)) return 1;
    return for_row_groups(
        S, slot_bytes, tags,
        [&](size_t s0, size_t Sg, const GpuHashTags &part) {
            GpuMatrix v = scratch_matrix(ctx, call.level, call.m_g, Sg * call.c, digits.ptr);
            if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Sg, base_bits, 0, call.d, call.m_g, col_start))
                return rc;
            return combine_group(call, outs, lut_preimages, xs, s0, Sg, digits.ptr, lhs.ptr, y_words, words_per_y);
        },
        call.cap);
    ABI_GUARD_END
}

// The same with the digits [V_0 | V_1 | ...] given instead of sampled: the pre-pass and the main kernel alone, one group.
// A test instrument (tests/test_gpu_ggh15_lookup.py reaches the lazy accumulator's bound with operands no sampler gives).
extern "C" int gpupoly_matrix_ggh15_lookup_combine(GpuMatrix *const *outs, size_t nslots_S, const GpuMatrix *mid_identity, const GpuMatrix *mid_gy,
                                                   const GpuMatrix *mid_v, const GpuMatrix *mid_vx, const GpuMatrix *mid_rand,
                                                   const GpuMatrix *mid_gate1, const GpuMatrix *const *lut_preimages, const GpuMatrix *const *xs,
                                                   size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y,
                                                   const GpuMatrix *digits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_ggh15_lookup_combine";
    const size_t S = nslots_S;
    if (S == 0) return 0;
    const GpuMatrix *const mids[6] = {mid_identity, mid_gy, mid_v, mid_vx, mid_rand, mid_gate1};
    LookupCall call;
    if (check_call(who, outs, S, mids, lut_preimages, xs, digits, false, col_start, base_bits, y_words, words_per_y, nullptr, &call)) return 1;
    if (!grid_fits(call, S)) return set_error(std::string(who) + ": too many output tiles in one group");
    bool go;
    if (accept(call, outs, lut_preimages, xs, digits, &go)) return 1;
    if (!go) return 0;
    CtxBlock lhs(call.ctx);
    const size_t poly_bytes = static_cast<size_t>(call.L) * call.ctx->N * call.ctx->word_bytes;
    if (lhs.alloc(S * call.r * (call.m_g + call.w) * poly_bytes)) return 1;
    return combine_group(call, outs, lut_preimages, xs, 0, S, words_ptr(digits), lhs.ptr, y_words, words_per_y);
    ABI_GUARD_END
}
