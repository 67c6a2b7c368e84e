// lut_targets.hip — the preimage targets of T LUT rows of one column chunk in one call: gpupoly_matrix_lut_targets
// (DESIGN.md section 5r).
//
// The GGH15 LUT preprocessing asks for one preimage per LUT row and column chunk (sample_lut_preimages_gpu,
// src/lookup/ggh15/pubkey_gpu.rs:540-640), and every target comes from build_lut_preimage_target_chunk_gpu (:379-415):
//
//   target_t = W_id[:, chunk] + W_gy G^-1(G_d[:, chunk] o y_t) + W_v V_t + W_vx (V_t o idx_t),
//   V_t = G^-1 of columns `chunk` of the d x m uniform matrix under hash_seed_for_matrix(key, tag_t),
//
// y_t and idx_t constant polynomials.  Column c0 + cc of G_d is (j, tw, e): B^e in tower tw of row j.  Its product with the
// constant y_t has one non-zero residue, (y_t mod q_tw) B^e mod q_tw, whose digits are constants - their own transform - so
//
//   (W_gy G^-1(G_d[:, chunk] o y_t))[i, cc] = sum_{e' < dpt} weight(t, cc, e') * W_gy[i, (j, tw, e')]      in every limb,
//
// weight(t, cc, e') = digit e' of (y_t mod q_tw) B^e mod q_tw, reduced into the limb (section 5l).  A constant idx_t
// commutes with the product: W_v V_t + W_vx (V_t o idx_t) = top_t + idx_t * bottom_t with [top_t; bottom_t] = [W_v; W_vx] V_t.
// Per group of rows: the decomposed-blocks sample gives [V_0 | V_1 | ...] (decompose.hip), one product of the stacked
// [W_v; W_vx] against it gives every top and bottom, one small kernel gives the weights, and one combine kernel writes
// every word of every target straight into the T outputs.  The rows' constants and output pointers go up in one staged
// copy per group; nothing is uploaded, launched or awaited per row.
#include "common.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

// weights[((t c + cc) L + l) dpt + e'] = digit e' of ((y_t mod q_tw) B^e mod q_tw) mod q_l for column col_start + cc =
// (j, tw, e), with decompose_kernel's masks; y: [T][L] residues of the rows' constants.  item = (row, column)
__global__ void lut_weights_kernel(uint64_t *__restrict__ weights, const uint64_t *__restrict__ y, const LimbConst *__restrict__ limbs, size_t T,
                                   uint32_t c, size_t col_start, uint32_t L, uint32_t dpt, uint32_t base_bits) {
    const size_t item = item_index();
    if (item >= T * c) return;
    const size_t t = item / c;
    const size_t col = col_start + (item - t * c);
    const uint32_t rem = static_cast<uint32_t>(col % (static_cast<size_t>(L) * dpt));
    const uint32_t tw = rem / dpt, e = rem - tw * dpt;
    const uint64_t q = limbs[tw].q;
    const uint32_t src_bits = limbs[tw].kbits;
    const uint64_t B = (1ull << base_bits) % q;  // base_bits < 63
    uint64_t v = y[t * L + tw];
    for (uint32_t i = 0; i < e; ++i) v = static_cast<uint64_t>(static_cast<u128_t>(v) * B % q);
    for (uint32_t ep = 0; ep < dpt; ++ep) {
        const uint32_t shift = ep * base_bits;
        uint64_t mask = 0;
        if (shift < src_bits) {
            const uint32_t left = src_bits - shift;
            const uint32_t db = base_bits < left ? base_bits : left;
            mask = (1ull << db) - 1;  // db <= base_bits < 63
        }
        const uint64_t digit = shift >= 64 ? 0 : ((v >> shift) & mask);
        for (uint32_t l = 0; l < L; ++l) {
            const uint64_t ql = limbs[l].q;
            weights[(item * L + l) * dpt + ep] = digit >= ql ? digit % ql : digit;
        }
    }
}

struct CombineArgs {
    const void *w_id, *w_gy;  // d x m
    const void *prod;         // 2d x (T c): rows [0, d) the tops, rows [d, 2d) the bottoms, row t's columns at t c
    const uint64_t *rows;     // device: [T] output pointers, then [T][L] idx_t mod q_l
    const uint64_t *weights;  // device: [T c][L][dpt]
    size_t m, col_start, k, entries;
    uint32_t T, d, c, L, dpt, logN;
};

// out_t[i, cc] = W_id[i, c0 + cc] + sum_e' weight(t, cc, e') W_gy[i, (j, tw, e')] + top_t[i, cc] + idx_t bottom_t[i, cc], word by
// word.  blockIdx.y/z = the output polynomial (t, i, cc), blockIdx.x strides its L N words VN per lane (16 bytes when VN > 1,
// VN divides N: one limb per vector).  The dpt + 1 products (each below q^2) and the two addends go into one lazy
// accumulator - 64 bits for 32-bit words, 128 bits for 64-bit words - reduced once, or every LimbConst::lazy_terms terms
// where the modulus leaves room for fewer.  DPT 0: any digit count, W_gy's words loaded term by term.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256) lut_combine_kernel(CombineArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const size_t per_row = static_cast<size_t>(a.d) * a.c;
    const size_t t = entry / per_row, rest = entry - t * per_row;
    const size_t i = rest / a.c, cc = rest - i * a.c;
    const size_t col = a.col_start + cc;
    const size_t jb = col / a.k;
    const uint32_t dpt = DPT ? DPT : a.dpt;
    const uint32_t tw = static_cast<uint32_t>(col - jb * a.k) / dpt;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN;
    const size_t tc = static_cast<size_t>(a.T) * a.c, pc = t * a.c + cc;
    const W *wid = static_cast<const W *>(a.w_id) + (i * a.m + col) * wpp;
    const W *gy = static_cast<const W *>(a.w_gy) + (i * a.m + jb * a.k + static_cast<size_t>(tw) * dpt) * wpp;
    const W *top = static_cast<const W *>(a.prod) + (i * tc + pc) * wpp;
    const W *bot = static_cast<const W *>(a.prod) + ((a.d + i) * tc + pc) * wpp;
    W *out = reinterpret_cast<W *>(a.rows[t]) + (i * a.c + cc) * wpp;
    const uint64_t *idx = a.rows + a.T + t * a.L;
    const uint64_t *wt = a.weights + pc * a.L * dpt;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.logN);
        const LimbConst lc = limbs[l];
        const uint32_t lazy = lc.lazy_terms;
        const W x = static_cast<W>(idx[l]);
        W av[VN], tv[VN], bv[VN], ov[VN];
        *reinterpret_cast<V *>(av) = *reinterpret_cast<const V *>(wid + w0);
        *reinterpret_cast<V *>(tv) = *reinterpret_cast<const V *>(top + w0);
        *reinterpret_cast<V *>(bv) = *reinterpret_cast<const V *>(bot + w0);
        W gv[DPT ? DPT : 1][VN], wv[DPT ? DPT : 1];
        if constexpr (DPT > 0) {
#pragma unroll
            for (int ep = 0; ep < DPT; ++ep) {
                *reinterpret_cast<V *>(gv[ep]) = *reinterpret_cast<const V *>(gy + ep * wpp + w0);
                wv[ep] = static_cast<W>(wt[l * DPT + ep]);
            }
        }
#pragma unroll
        for (int v = 0; v < VN; ++v) {
            // the accumulator carries a residue (W_id's word, or a folded sum) into every window of `lazy` terms, each at
            // most (q - 1)^2: the bound LimbConst::lazy_terms is computed for
            D acc = av[v];
            uint32_t pending = 0;
            auto fold = [&]() {
                if constexpr (sizeof(W) == 4) acc = reduce_u64_sum(acc, static_cast<uint32_t>(lc.q), lc.mu64);
                else acc = reduce_u128_sum(acc, lc.q, lc.mu, lc.kbits, lc.mu64);
                pending = 0;
            };
            auto add = [&](D term) {
                if (pending >= lazy) fold();
                acc += term;
                ++pending;
            };
            add(static_cast<D>(tv[v]));
            add(static_cast<D>(x) * bv[v]);
            if constexpr (DPT > 0) {
#pragma unroll
                for (int ep = 0; ep < DPT; ++ep) add(static_cast<D>(wv[ep]) * gv[ep][v]);
            } else {
                for (uint32_t ep = 0; ep < dpt; ++ep) add(static_cast<D>(static_cast<W>(wt[l * dpt + ep])) * gy[ep * wpp + w0 + v]);
            }
            fold();
            ov[v] = static_cast<W>(acc);
        }
        *reinterpret_cast<V *>(out + w0) = *reinterpret_cast<const V *>(ov);
    }
}

template <typename W, int VN>
int launch_combine_vn(GpuContext *ctx, const CombineArgs &a) {
    const size_t wpp = static_cast<size_t>(a.L) << a.logN, vecs = wpp / VN;
    const size_t gy = std::min<size_t>(a.entries, 65535), gz = (a.entries + gy - 1) / gy;
    if (gz > 65535) return set_error("gpupoly_matrix_lut_targets: too many target polynomials in one group");
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // the targets written once; W_id's chunk, top and bottom read once, W_gy's dpt words per target word (from cache after the first row)
    MXX_TRACE_BYTES(static_cast<double>(a.entries) * wpp * sizeof(W) * (4.0 + a.dpt));
#define MXX_COMBINE(D) MXX_LAUNCH((lut_combine_kernel<W, VN, D>), grid, dim3(threads), 0, ctx->stream, a, ctx->d_limbs)
    switch (a.dpt) {
        case 1: MXX_COMBINE(1); break;
        case 2: MXX_COMBINE(2); break;
        case 3: MXX_COMBINE(3); break;
        case 4: MXX_COMBINE(4); break;
        default: MXX_COMBINE(0); break;
    }
#undef MXX_COMBINE
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int launch_combine(GpuContext *ctx, const CombineArgs &a) {
    constexpr int VN = 16 / sizeof(W);
    if (ctx->N % VN == 0) return launch_combine_vn<W, VN>(ctx, a);
    return launch_combine_vn<W, 1>(ctx, a);  // a limb vector narrower than 16 bytes
}

// what one accepted call works with
struct LutCall {
    GpuContext *ctx;
    int level;
    uint32_t L, dpt, base_bits;
    size_t d, m, k, c, col_start;
    const GpuMatrix *w_id, *w_gy;
};

// Everything both entries refuse, for every row, before anything is launched.  `prod` null: the full entry, whose w_v, w_vx
// and tags are checked; otherwise the combine-only entry with the product given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, const GpuMatrix *w_id, const GpuMatrix *w_gy, const GpuMatrix *w_v,
               const GpuMatrix *w_vx, const GpuMatrix *prod, size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y,
               const uint64_t *idx, const GpuHashTags *tags, LutCall *call) {
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    if (!outs || !y_words || !idx) return refuse("null array");
    const GpuMatrix *ws[4] = {w_id, w_gy, prod ? w_id : w_v, prod ? w_gy : w_vx};
    for (const GpuMatrix *w : ws)
        if (!w) return refuse("null operand");
    if (!prod && !tags) return refuse("null tags");
    for (size_t t = 0; t < T; ++t)
        if (!outs[t]) return refuse("null output (row " + std::to_string(t) + ")");
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (base_bits == 0 || base_bits >= 63) return refuse("base_bits must be in 1..62");
    GpuContext *ctx = w_id->ctx;
    const int level = w_id->level;
    if (level < 0 || level >= ctx->limb_count) return refuse("level out of range");
    if (ctx->env.rng_compat && !prod) return refuse("unsupported under MXX_HIP_RNG_COMPAT=reference");
    const size_t L = static_cast<size_t>(level) + 1;
    const size_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = dpt * L, d = w_id->rows, m = d * k, c = outs[0]->cols;
    for (const GpuMatrix *w : ws) {
        if (w->ctx != ctx) return refuse("context mismatch");
        if (w->level != level) return refuse("level mismatch");
        if (w->rows != d || w->cols != m) return refuse("shape mismatch: the W operands are d x (d * digits per tower * limbs)");
        if (w->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
    }
    if (prod) {
        if (prod->ctx != ctx) return refuse("context mismatch");
        if (prod->level != level) return refuse("level mismatch");
        if (c && T > ~size_t(0) / c) return refuse("matrix too large");
        if (prod->rows != 2 * d || prod->cols != T * c) return refuse("shape mismatch: the product is 2d x (rows * chunk columns)");
        if (prod->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
    }
    if (col_start > m || c > m - col_start) return refuse("column chunk past the operands' columns");
    if (d > 0xffffffffull || c > 0xffffffffull || T > 0xffffffffull) return refuse("matrix too large");
    for (size_t t = 0; t < T; ++t) {
        const GpuMatrix *out = outs[t];
        const std::string at = " (row " + std::to_string(t) + ")";
        if (out->ctx != ctx) return refuse("context mismatch" + at);
        if (out->level != level) return refuse("level mismatch" + at);
        if (out->cols != c) return refuse("the outputs differ in width" + at);
        if (out->rows != d) return refuse("shape mismatch: an output is d x chunk columns" + at);
    }
    size_t tag_bytes = 0;
    if (!prod && hash_tags_check(who, tags, T, &tag_bytes)) return 1;
    // an output is written while every operand is still being read, and by no other row: no overlap with an operand (the
    // stacked copy of w_v and w_vx is made first, but the rule is the entry's, not the sequence's) or with another output
    const GpuMatrix *operands[5] = {ws[0], ws[1], ws[2], ws[3], prod};
    static const char *const names[5] = {"an operand", "an operand", "an operand", "an operand", "the product"};
    const std::string overlap = row_outputs_overlap(outs, T, operands, names, prod ? 5 : 4);
    if (!overlap.empty()) return refuse(overlap);
    *call = LutCall{ctx, level, static_cast<uint32_t>(L), static_cast<uint32_t>(dpt), base_bits, d, m, k, c, col_start, w_id, w_gy};
    return 0;
}

// rows [0, Tg) of a group: their table (output pointers, idx and y residues) in one staged copy, the weights kernel, the
// combine kernel over `prod` (2d x (Tg c) words)
int combine_group(const LutCall &call, GpuMatrix *const *outs, size_t Tg, const void *prod, const uint64_t *y_words, size_t words_per_y,
                  const uint64_t *idx) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, entries = Tg * call.d * call.c;
    if (entries == 0) return 0;
    const size_t table_words = Tg + 2 * Tg * L, weight_words = Tg * call.c * L * call.dpt;
    CtxBlock block(ctx);
    if (block.alloc(sizeof(uint64_t) * (table_words + weight_words))) return 1;
    static thread_local std::vector<uint64_t> staging;  // the caller's arrays are not read after this call returns
    staging.resize(table_words);
    for (size_t t = 0; t < Tg; ++t) {
        staging[t] = reinterpret_cast<uint64_t>(words_ptr(outs[t]));
        for (size_t l = 0; l < L; ++l) {
            staging[Tg + t * L + l] = idx[t] % ctx->moduli[l];
            staging[Tg + Tg * L + t * L + l] = words_mod(y_words + t * words_per_y, words_per_y, ctx->moduli[l]);
        }
    }
    uint64_t *d_table = static_cast<uint64_t *>(block.ptr), *d_weights = d_table + table_words;
    MXX_TRACED_COPY("LUT row table (host to device)", ctx->stream, sizeof(uint64_t) * table_words,
                    HIP_TRY(hipMemcpyAsync(d_table, staging.data(), sizeof(uint64_t) * table_words, hipMemcpyHostToDevice, ctx->stream)));
    MXX_TRACE_BYTES(sizeof(uint64_t) * (Tg * L + weight_words));
    MXX_LAUNCH(lut_weights_kernel, item_grid(Tg * call.c, 256), dim3(256), 0, ctx->stream, d_weights, d_table + Tg + Tg * L, ctx->d_limbs, Tg,
               static_cast<uint32_t>(call.c), call.col_start, call.L, call.dpt, call.base_bits);
    HIP_TRY(hipGetLastError());
    CombineArgs a;
    a.w_id = words_ptr(call.w_id);
    a.w_gy = words_ptr(call.w_gy);
    a.prod = prod;
    a.rows = d_table;
    a.weights = d_weights;
    a.m = call.m;
    a.col_start = call.col_start;
    a.k = call.k;
    a.entries = entries;
    a.T = static_cast<uint32_t>(Tg);
    a.d = static_cast<uint32_t>(call.d);
    a.c = static_cast<uint32_t>(call.c);
    a.L = call.L;
    a.dpt = call.dpt;
    a.logN = ctx->logN;
    return ctx->wide ? launch_combine<uint64_t>(ctx, a) : launch_combine<uint32_t>(ctx, a);
}

GpuMatrix scratch_matrix(const LutCall &call, size_t rows, size_t cols, void *words) {
    return ::scratch_matrix(call.ctx, call.level, rows, cols, words);
}

}  // namespace

extern "C" int gpupoly_matrix_lut_targets(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *w_identity, const GpuMatrix *w_gy,
                                          const GpuMatrix *w_v, const GpuMatrix *w_vx, size_t col_start, uint32_t base_bits,
                                          const uint64_t *y_words, size_t words_per_y, const uint64_t *idx, const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lut_targets";
    const size_t T = nrows_T;
    if (T == 0) return 0;
    LutCall call;
    if (check_call(who, outs, T, w_identity, w_gy, w_v, w_vx, nullptr, col_start, base_bits, y_words, words_per_y, idx, tags, &call)) return 1;
    // ---- accepted ----
    GpuContext *ctx = call.ctx;
    for (size_t t = 0; t < T; ++t) outs[t]->format = GPU_POLY_FORMAT_EVAL;
    if (call.d == 0 || call.c == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // [W_v; W_vx], 2d x m: rows are contiguous, so the stack is the two operands' words one after the other
    const size_t w_bytes = call.d * call.m * poly_bytes;
    CtxBlock stack(ctx);
    if (stack.alloc(2 * w_bytes)) return 1;
    MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * w_bytes,
                    HIP_TRY(hipMemcpyAsync(stack.ptr, words_ptr(w_v), w_bytes, hipMemcpyDeviceToDevice, ctx->stream)));
    MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * w_bytes,
                    HIP_TRY(hipMemcpyAsync(static_cast<char *>(stack.ptr) + w_bytes, words_ptr(w_vx), w_bytes, hipMemcpyDeviceToDevice, ctx->stream)));
    const GpuMatrix lhs = scratch_matrix(call, 2 * call.d, call.m, stack.ptr);
    // rows per group: the digit scratch m x (Tg c) stays under the cap (one row at least), within the block sampler's 2^20
    const size_t row_bytes = call.m * call.c * poly_bytes;
    const size_t per_group = rows_per_group(T, row_bytes);
    CtxBlock digits(ctx), prod(ctx);
    if (digits.alloc(per_group * row_bytes)) return 1;
    if (prod.alloc(2 * call.d * per_group * call.c * poly_bytes)) return 1;
    std::vector<size_t> offsets;
    for (size_t t0 = 0; t0 < T; t0 += per_group) {
        const size_t Tg = std::min(per_group, T - t0);
        const GpuHashTags part = hash_tags_rows(tags, t0, Tg, offsets);
        GpuMatrix v = scratch_matrix(call, call.m, Tg * call.c, digits.ptr);
        if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, base_bits, 0, call.d, call.m, col_start))
            return rc;
        GpuMatrix p = scratch_matrix(call, 2 * call.d, Tg * call.c, prod.ptr);
        if (int rc = launch_matmul(&p, &lhs, &v)) return rc;
        if (int rc = combine_group(call, outs + t0, Tg, prod.ptr, y_words + t0 * words_per_y, words_per_y, idx + t0)) return rc;
    }
    return 0;
    ABI_GUARD_END
}

// The same with [top; bottom] given instead of sampled and multiplied: the weights and the combine kernel alone, one group.
// A test instrument (tests/test_gpu_lut_targets.py reaches the lazy accumulator's bound with operands no sampler gives).
extern "C" int gpupoly_matrix_lut_targets_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *w_identity, const GpuMatrix *w_gy,
                                                  const GpuMatrix *product, size_t col_start, uint32_t base_bits, const uint64_t *y_words,
                                                  size_t words_per_y, const uint64_t *idx) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lut_targets_combine";
    if (nrows_T == 0) return 0;
    if (!product) return set_error(std::string(who) + ": null operand");
    LutCall call;
    if (check_call(who, outs, nrows_T, w_identity, w_gy, nullptr, nullptr, product, col_start, base_bits, y_words, words_per_y, idx, nullptr, &call))
        return 1;
    for (size_t t = 0; t < nrows_T; ++t) outs[t]->format = GPU_POLY_FORMAT_EVAL;
    if (call.d == 0 || call.c == 0) return 0;
    if (ctx_activate(call.ctx)) return 1;
    return combine_group(call, outs, nrows_T, words_ptr(product), y_words, words_per_y, idx);
    ABI_GUARD_END
}
