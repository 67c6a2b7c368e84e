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
    CombineShape s;
};

// out_t[i, cc] = W_id[i, c0 + cc] + sum_e' weight(t, cc, e') W_gy[i, (j, tw, e')] + top_t[i, cc] + idx_t bottom_t[i, cc], word by
// word, for the block's output polynomial (t, i, cc) (combine_entry), VN words per lane (VN divides N: one limb per vector).
// The dpt + 1 products and the two addends go into one lazy accumulator.  DPT 0: any digit count, W_gy's words loaded term
// by term.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256) lut_combine_kernel(CombineArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.s.entries) return;
    const uint32_t dpt = DPT ? DPT : a.s.dpt;
    const CombineEntry e = combine_entry(a.s, entry, dpt);
    const size_t wpp = e.wpp;
    const W *wid = static_cast<const W *>(a.w_id) + (e.i * a.s.m + e.col) * wpp;
    const W *gy = static_cast<const W *>(a.w_gy) + (e.i * a.s.m + e.jb * a.s.k + static_cast<size_t>(e.tw) * dpt) * wpp;
    const W *top = static_cast<const W *>(a.prod) + (e.i * e.tc + e.pc) * wpp;
    const W *bot = static_cast<const W *>(a.prod) + ((a.s.d + e.i) * e.tc + e.pc) * wpp;
    W *out = reinterpret_cast<W *>(a.rows[e.t]) + (e.i * a.s.c + e.cc) * wpp;
    const uint64_t *idx = a.rows + a.s.T + e.t * a.s.L;
    const uint64_t *wt = a.weights + e.pc * a.s.L * dpt;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.s.logN);
        const LimbConst lc = limbs[l];
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
            LazyAcc<W> sum(av[v], lc.lazy_terms, lc);
            sum.add(static_cast<D>(tv[v]));
            sum.add(static_cast<D>(x) * bv[v]);
            if constexpr (DPT > 0) {
#pragma unroll
                for (int ep = 0; ep < DPT; ++ep) sum.add(static_cast<D>(wv[ep]) * gv[ep][v]);
            } else {
                for (uint32_t ep = 0; ep < dpt; ++ep) sum.add(static_cast<D>(static_cast<W>(wt[l * dpt + ep])) * gy[ep * wpp + w0 + v]);
            }
            ov[v] = sum.result();
        }
        *reinterpret_cast<V *>(out + w0) = *reinterpret_cast<const V *>(ov);
    }
}

// what one accepted call works with
struct LutCall : ChunkCall {
    const GpuMatrix *w_id, *w_gy;
};

// Everything both entries refuse, for every row, before anything is launched.  `prod` null: the full entry, whose w_v, w_vx
// and tags are checked; otherwise the combine-only entry with the product given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, const GpuMatrix *w_id, const GpuMatrix *w_gy, const GpuMatrix *w_v,
               const GpuMatrix *w_vx, const GpuMatrix *prod, size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y,
               const uint64_t *idx, const GpuHashTags *tags, LutCall *call) {
    const Refuse refuse{who};
    if (!outs || !y_words || !idx) return refuse("null array");
    const GpuMatrix *ws[4] = {w_id, w_gy, prod ? w_id : w_v, prod ? w_gy : w_vx};
    for (const GpuMatrix *w : ws)
        if (!w) return refuse("null operand");
    if (!prod && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, T, null_row)) return rc;
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (int rc = refuse_base_level(refuse, w_id, base_bits, !prod, call)) return rc;
    const size_t d = w_id->rows, m = d * call->k, c = outs[0]->cols;
    for (const GpuMatrix *w : ws)
        if (int rc = refuse_operand(refuse, w, *call, d, m, "shape mismatch: the W operands are d x (d * digits per tower * limbs)")) return rc;
    if (prod) {
        if (int rc = refuse_foreign(refuse, prod, *call)) return rc;
        if (c && T > ~size_t(0) / c) return refuse("matrix too large");
        if (int rc = refuse_form(refuse, prod, 2 * d, T * c, "shape mismatch: the product is 2d x (rows * chunk columns)")) return rc;
    }
    call->d = d, call->m = m, call->c = c, call->col_start = col_start, call->w_id = w_id, call->w_gy = w_gy;
    if (int rc = refuse_chunk_outputs(refuse, outs, T, *call)) return rc;
    // an output is written while every operand is still being read, and by no other row: no overlap with an operand (the
    // stacked copy of w_v and w_vx is made first, but the rule is the entry's, not the sequence's) or with another output
    const GpuMatrix *operands[5] = {ws[0], ws[1], ws[2], ws[3], prod};
    static const char *const names[5] = {"an operand", "an operand", "an operand", "an operand", "the product"};
    return refuse_tags_overlap(refuse, prod ? nullptr : tags, T, outs, T, operands, names, prod ? 5 : 4);
}

// rows [0, Tg) of a group: their table (output pointers, idx and y residues) in one staged copy, the weights kernel, the
// combine kernel over `prod` (2d x (Tg c) words)
int combine_group(const LutCall &call, GpuMatrix *const *outs, size_t Tg, const void *prod, const uint64_t *y_words, size_t words_per_y,
                  const uint64_t *idx) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, weight_words = Tg * call.c * L * call.dpt;
    static thread_local std::vector<uint64_t> staging;
    staging.resize(Tg + 2 * Tg * L);
    for (size_t t = 0; t < Tg; ++t) {
        staging[t] = reinterpret_cast<uint64_t>(words_ptr(outs[t]));
        for (size_t l = 0; l < L; ++l) {
            staging[Tg + t * L + l] = idx[t] % ctx->moduli[l];
            staging[Tg + Tg * L + t * L + l] = words_mod(y_words + t * words_per_y, words_per_y, ctx->moduli[l]);
        }
    }
    CtxBlock block(ctx);
    if (upload_table(block, "LUT row table (host to device)", staging, weight_words)) return 1;
    uint64_t *d_table = static_cast<uint64_t *>(block.ptr), *d_weights = d_table + staging.size();
    MXX_TRACE_BYTES(sizeof(uint64_t) * (Tg * L + weight_words));
    MXX_LAUNCH(lut_weights_kernel, item_grid(Tg * call.c, 256), dim3(256), 0, ctx->stream, d_weights, d_table + Tg + Tg * L, ctx->d_limbs, Tg,
               static_cast<uint32_t>(call.c), call.col_start, call.L, call.dpt, call.base_bits);
    HIP_TRY(hipGetLastError());
    const CombineArgs a{words_ptr(call.w_id), words_ptr(call.w_gy), prod, d_table, d_weights, combine_shape(call, Tg)};
    // the targets written once; W_id's chunk, top and bottom read once, W_gy's dpt words per target word (from cache after the first row)
    const double bytes = static_cast<double>(a.s.entries) * (L << ctx->logN) * ctx->word_bytes * (4.0 + call.dpt);
    return launch_combine(call.who, ctx, bytes, a.s.entries, call.L, ctx->logN, call.dpt, [&](auto cfg, dim3 grid, dim3 block_dim) {
        MXX_LAUNCH_COMBINE(lut_combine_kernel, cfg, grid, block_dim, 0, ctx->stream, a, ctx->d_limbs);
    });
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
    const GpuMatrix lhs = scratch_matrix(ctx, call.level, 2 * call.d, call.m, stack.ptr);
    // a group's digit scratch is m x (Tg c)
    const size_t row_bytes = call.m * call.c * poly_bytes;
    const size_t per_group = rows_per_group(T, row_bytes);
    CtxBlock digits(ctx), prod(ctx);
    if (digits.alloc(per_group * row_bytes)) return 1;
    if (prod.alloc(2 * call.d * per_group * call.c * poly_bytes)) return 1;
    return for_row_groups(T, row_bytes, tags, [&](size_t t0, size_t Tg, const GpuHashTags &part) {
        GpuMatrix v = scratch_matrix(ctx, call.level, call.m, Tg * call.c, digits.ptr);
        if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, base_bits, 0, call.d, call.m, col_start))
            return rc;
        GpuMatrix p = scratch_matrix(ctx, call.level, 2 * call.d, Tg * call.c, prod.ptr);
        if (int rc = launch_matmul(&p, &lhs, &v)) return rc;
        return combine_group(call, outs + t0, Tg, prod.ptr, y_words + t0 * words_per_y, words_per_y, idx + t0);
    });
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
