// lwe_targets.hip — the preimage targets of T LUT rows of one column chunk of the LWE public lookup in one call:
// gpupoly_matrix_lwe_targets.
//
// The LWE lookup preprocessing asks for one preimage per LUT row and column chunk (sample_aux_matrices_gpu,
// src/lookup/lwe/pubkey_gpu.rs:397-520), and every target comes from build_adjusted_target_chunk (:193-222):
//
//   target_t = A_lt[:, chunk] - G_d[:, chunk] o y_t - (A_z - G_d o x_t) D_t,
//   D_t = G^-1 of columns `chunk` of the d x m uniform matrix U_t under hash_seed_for_matrix(key, tag_t),
//
// x_t and y_t constant polynomials.  G_d G^-1(U) = U in every limb - the digits of a canonical residue, weighted by B^e mod
// q, sum to that residue - so (G_d o x_t) D_t = x_t U_t[:, chunk], and limb l of its entry (i, cc) is
//
//   sum_{e < dpt} (x_t B^e mod q_l) * D_t[(i, l, e), cc]      taken in limb l,
//
// by linearity for the transformed digits as well: it is read off the digit scratch that the product needs anyway.  Column
// c0 + cc of G_d is (j, tw, e), so G_d[:, chunk] o y_t is (y_t mod q_tw) B^e mod q_tw in every slot of limb tw of row j and
// zero elsewhere.  Per group of rows: the decomposed-blocks sample gives [D_0 | D_1 | ...] (decompose.hip), one product of
// A_z - as it is - against it gives every A_z D_t, and one combine kernel writes every word of every target straight into
// the T outputs.  The rows' constants and output pointers go up in one staged copy per group; nothing of size d x m is
// built per row, G is never filled, and nothing is uploaded, launched or awaited per row.
#include "common.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

struct LweCombineArgs {
    const void *a_lt;      // d x m
    const void *digits;    // m x (T c): row (i, l, e) = i k + l dpt + e, row t's columns at t c
    const void *prod;      // d x (T c) = A_z digits
    const uint64_t *rows;  // device: [T] output pointers, [T][L][dpt] x_t B^e mod q_l, [T][c] (y_t mod q_tw) B^e mod q_tw
    CombineShape s;
};

// out_t[i, cc] = A_lt[i, c0 + cc] - prod_t[i, cc] - [i == j, l == tw] gy(t, cc) + sum_e xw(t, l, e) D_t[(i, l, e), cc] in limb l,
// word by word, column c0 + cc = (j, tw, e'), for the block's output polynomial (t, i, cc) (combine_entry), VN words per lane
// (VN divides N: one limb per vector).  The negated words go in as q - word (q - word <= q counts as one term), so the dpt
// products and the up to two such addends join A_lt's word in one lazy accumulator.  Only limb l of the digit rows
// (i, l, .) is read.  DPT 0: any digit count, the digits loaded term by term.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256) lwe_combine_kernel(LweCombineArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.s.entries) return;
    const uint32_t dpt = DPT ? DPT : a.s.dpt;
    const CombineEntry e = combine_entry(a.s, entry, dpt);
    const size_t wpp = e.wpp;
    const size_t digit_row = e.tc * wpp;  // words from one digit row to the next
    const W *alt = static_cast<const W *>(a.a_lt) + (e.i * a.s.m + e.col) * wpp;
    const W *prod = static_cast<const W *>(a.prod) + (e.i * e.tc + e.pc) * wpp;
    const W *dig = static_cast<const W *>(a.digits) + (e.i * a.s.k * e.tc + e.pc) * wpp;
    W *out = reinterpret_cast<W *>(a.rows[e.t]) + (e.i * a.s.c + e.cc) * wpp;
    const uint64_t *xw = a.rows + a.s.T + e.t * a.s.L * dpt;
    const W gy = static_cast<W>(a.rows[a.s.T + static_cast<size_t>(a.s.T) * a.s.L * dpt + e.pc]);
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.s.logN);
        const LimbConst lc = limbs[l];
        const W q = static_cast<W>(lc.q);
        const bool hit = e.i == e.jb && l == e.tw;
        const W *dl = dig + static_cast<size_t>(l) * dpt * digit_row + w0;
        W av[VN], pv[VN], ov[VN];
        *reinterpret_cast<V *>(av) = *reinterpret_cast<const V *>(alt + w0);
        *reinterpret_cast<V *>(pv) = *reinterpret_cast<const V *>(prod + w0);
        W dv[DPT ? DPT : 1][VN], wv[DPT ? DPT : 1];
        if constexpr (DPT > 0) {
#pragma unroll
            for (int ed = 0; ed < DPT; ++ed) {
                *reinterpret_cast<V *>(dv[ed]) = *reinterpret_cast<const V *>(dl + ed * digit_row);
                wv[ed] = static_cast<W>(xw[l * DPT + ed]);
            }
        }
#pragma unroll
        for (int v = 0; v < VN; ++v) {
            LazyAcc<W> sum(av[v], lc.lazy_terms, lc);
            sum.add(static_cast<D>(static_cast<W>(q - pv[v])));
            if (hit) sum.add(static_cast<D>(static_cast<W>(q - gy)));
            if constexpr (DPT > 0) {
#pragma unroll
                for (int ed = 0; ed < DPT; ++ed) sum.add(static_cast<D>(wv[ed]) * dv[ed][v]);
            } else {
                for (uint32_t ed = 0; ed < dpt; ++ed) sum.add(static_cast<D>(static_cast<W>(xw[l * dpt + ed])) * dl[ed * digit_row + v]);
            }
            ov[v] = sum.result();
        }
        *reinterpret_cast<V *>(out + w0) = *reinterpret_cast<const V *>(ov);
    }
}

// what one accepted call works with
struct LweCall : ChunkCall {
    const GpuMatrix *a_lt;
};

// Everything both entries refuse, for every row, before anything is launched.  `full`: the sampling entry, whose a_z and
// tags are checked; otherwise the combine-only entry with the digits and the product given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, const GpuMatrix *a_z, const GpuMatrix *a_lt, const GpuMatrix *digits,
               const GpuMatrix *prod, size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *x,
               const GpuHashTags *tags, bool full, LweCall *call) {
    const Refuse refuse{who};
    if (!outs || !y_words || !x) return refuse("null array");
    if (!a_lt || (full ? !a_z : (!digits || !prod))) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, T, null_row)) return rc;
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (int rc = refuse_base_level(refuse, a_lt, base_bits, full, call)) return rc;
    const size_t d = a_lt->rows, m = d * call->k, c = outs[0]->cols;
    if (c && T > ~size_t(0) / c) return refuse("matrix too large");
    if (int rc = full ? refuse_operand(refuse, a_z, *call, d, m, "shape mismatch: A_z is d x (d * digits per tower * limbs)")
                      : refuse_operand(refuse, digits, *call, m, T * c, "shape mismatch: the digits are m x (rows * chunk columns)"))
        return rc;
    if (int rc = refuse_operand(refuse, a_lt, *call, d, m, "shape mismatch: A_lt is d x (d * digits per tower * limbs)")) return rc;
    if (int rc = full ? 0 : refuse_operand(refuse, prod, *call, d, T * c, "shape mismatch: the product is d x (rows * chunk columns)")) return rc;
    call->d = d, call->m = m, call->c = c, call->col_start = col_start, call->a_lt = a_lt;
    if (int rc = refuse_chunk_outputs(refuse, outs, T, *call)) return rc;
    // an output is written while every operand is still being read, and by no other row
    const GpuMatrix *operands[3] = {full ? a_z : digits, a_lt, prod};
    static const char *const names[3] = {"an operand", "an operand", "the product"};
    return refuse_tags_overlap(refuse, full ? tags : nullptr, T, outs, T, operands, names, full ? 2 : 3);
}

// rows [0, Tg) of a group: their table (output pointers, x_t B^e mod q_l, (y_t mod q_tw) B^e mod q_tw per chunk column) in
// one staged copy, then the combine kernel over `digits` (m x (Tg c) words) and `prod` (d x (Tg c) words)
int combine_group(const LweCall &call, GpuMatrix *const *outs, size_t Tg, const void *digits, const void *prod, const uint64_t *y_words,
                  size_t words_per_y, const uint64_t *x) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, dpt = call.dpt, c = call.c;
    static thread_local std::vector<uint64_t> staging, bpow, ypow;
    staging.resize(Tg + Tg * L * dpt + Tg * c);
    bpow.resize(L * dpt);  // B^e mod q_l, once for the group's rows
    ypow.resize(L * dpt);
    for (size_t l = 0; l < L; ++l) base_powers(ctx->moduli[l], call.base_bits, dpt, bpow.data() + l * dpt);
    uint64_t *xw = staging.data() + Tg, *gy = xw + Tg * L * dpt;
    for (size_t t = 0; t < Tg; ++t) {
        staging[t] = reinterpret_cast<uint64_t>(words_ptr(outs[t]));
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = ctx->moduli[l];
            const u128_t xv = x[t] % q, yv = words_mod(y_words + t * words_per_y, words_per_y, q);
            for (size_t e = l * dpt; e < (l + 1) * dpt; ++e) {
                xw[t * L * dpt + e] = static_cast<uint64_t>(xv * bpow[e] % q);
                ypow[e] = static_cast<uint64_t>(yv * bpow[e] % q);
            }
        }
        for (size_t cc = 0; cc < c; ++cc) gy[t * c + cc] = ypow[(call.col_start + cc) % call.k];  // column (j, tw, e): index tw dpt + e
    }
    CtxBlock block(ctx);
    if (upload_table(block, "LWE row table (host to device)", staging)) return 1;
    const LweCombineArgs a{words_ptr(call.a_lt), digits, prod, static_cast<const uint64_t *>(block.ptr), combine_shape(call, Tg)};
    // the targets written once; A_lt's chunk and the product read once, limb l of dpt digit rows per target word
    const double bytes = static_cast<double>(a.s.entries) * (L << ctx->logN) * ctx->word_bytes * (3.0 + call.dpt);
    return launch_combine(call.who, ctx, bytes, a.s.entries, call.L, ctx->logN, call.dpt, [&](auto cfg, dim3 grid, dim3 block_dim) {
        MXX_LAUNCH_COMBINE(lwe_combine_kernel, cfg, grid, block_dim, 0, ctx->stream, a, ctx->d_limbs);
    });
}

}  // namespace

extern "C" int gpupoly_matrix_lwe_targets(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *a_z, const GpuMatrix *a_lt, size_t col_start,
                                          uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *x,
                                          const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lwe_targets";
    const size_t T = nrows_T;
    if (T == 0) return 0;
    LweCall call;
    if (check_call(who, outs, T, a_z, a_lt, nullptr, nullptr, col_start, base_bits, y_words, words_per_y, x, tags, true, &call)) return 1;
    // ---- accepted ----
    GpuContext *ctx = call.ctx;
    for (size_t t = 0; t < T; ++t) outs[t]->format = GPU_POLY_FORMAT_EVAL;
    if (call.d == 0 || call.c == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    words_ptr(a_z);  // a PACKED24 operand is unpacked once; the product reads it as it is
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // a group's digit scratch is m x (Tg c)
    const size_t row_bytes = call.m * call.c * poly_bytes;
    const size_t per_group = rows_per_group(T, row_bytes);
    CtxBlock digits(ctx), prod(ctx);
    if (digits.alloc(per_group * row_bytes)) return 1;
    if (prod.alloc(call.d * per_group * call.c * poly_bytes)) return 1;
    return for_row_groups(T, row_bytes, tags, [&](size_t t0, size_t Tg, const GpuHashTags &part) {
        GpuMatrix v = scratch_matrix(ctx, call.level, call.m, Tg * call.c, digits.ptr);
        if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, base_bits, 0, call.d, call.m, col_start))
            return rc;
        GpuMatrix p = scratch_matrix(ctx, call.level, call.d, Tg * call.c, prod.ptr);
        if (int rc = launch_matmul(&p, a_z, &v)) return rc;
        return combine_group(call, outs + t0, Tg, digits.ptr, prod.ptr, y_words + t0 * words_per_y, words_per_y, x + t0);
    });
    ABI_GUARD_END
}

// The same with the digits and A_z * digits given instead of sampled and multiplied: the combine kernel alone, one group.
// A test instrument (tests/test_gpu_lwe_targets.py reaches the lazy accumulator's bound with operands no sampler gives).
extern "C" int gpupoly_matrix_lwe_targets_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *a_lt, const GpuMatrix *digits,
                                                  const GpuMatrix *product, size_t col_start, uint32_t base_bits, const uint64_t *y_words,
                                                  size_t words_per_y, const uint64_t *x) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lwe_targets_combine";
    if (nrows_T == 0) return 0;
    LweCall call;
    if (check_call(who, outs, nrows_T, nullptr, a_lt, digits, product, col_start, base_bits, y_words, words_per_y, x, nullptr, false, &call)) return 1;
    for (size_t t = 0; t < nrows_T; ++t) outs[t]->format = GPU_POLY_FORMAT_EVAL;
    if (call.d == 0 || call.c == 0) return 0;
    if (ctx_activate(call.ctx)) return 1;
    return combine_group(call, outs, nrows_T, words_ptr(digits), words_ptr(product), y_words, words_per_y, x);
    ABI_GUARD_END
}
