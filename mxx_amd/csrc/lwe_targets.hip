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
    size_t m, col_start, k, entries;
    uint32_t T, d, c, L, dpt, logN;
};

// out_t[i, cc] = A_lt[i, c0 + cc] - prod_t[i, cc] - [i == j, l == tw] gy(t, cc) + sum_e xw(t, l, e) D_t[(i, l, e), cc] in limb l,
// word by word, column c0 + cc = (j, tw, e').  blockIdx.y/z = the output polynomial (t, i, cc), blockIdx.x strides its L N
// words VN per lane (16 bytes when VN > 1, VN divides N: one limb per vector).  The negated words go in as q - word, so
// the dpt products (each below q^2) and the up to two such addends join A_lt's word in one lazy accumulator - 64 bits for
// 32-bit words, 128 bits for 64-bit words - reduced once, or every LimbConst::lazy_terms terms where the modulus leaves
// room for fewer.  Only limb l of the digit rows (i, l, .) is read.  DPT 0: any digit count, the digits loaded term by term.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256) lwe_combine_kernel(LweCombineArgs a, const LimbConst *__restrict__ limbs) {
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
    const size_t digit_row = tc * wpp;  // words from one digit row to the next
    const W *alt = static_cast<const W *>(a.a_lt) + (i * a.m + col) * wpp;
    const W *prod = static_cast<const W *>(a.prod) + (i * tc + pc) * wpp;
    const W *dig = static_cast<const W *>(a.digits) + (i * a.k * tc + pc) * wpp;
    W *out = reinterpret_cast<W *>(a.rows[t]) + (i * a.c + cc) * wpp;
    const uint64_t *xw = a.rows + a.T + t * a.L * dpt;
    const W gy = static_cast<W>(a.rows[a.T + static_cast<size_t>(a.T) * a.L * dpt + pc]);
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.logN);
        const LimbConst lc = limbs[l];
        const uint32_t lazy = lc.lazy_terms;
        const W q = static_cast<W>(lc.q);
        const bool hit = i == jb && l == tw;
        const W *dl = dig + static_cast<size_t>(l) * dpt * digit_row + w0;
        W av[VN], pv[VN], ov[VN];
        *reinterpret_cast<V *>(av) = *reinterpret_cast<const V *>(alt + w0);
        *reinterpret_cast<V *>(pv) = *reinterpret_cast<const V *>(prod + w0);
        W dv[DPT ? DPT : 1][VN], wv[DPT ? DPT : 1];
        if constexpr (DPT > 0) {
#pragma unroll
            for (int e = 0; e < DPT; ++e) {
                *reinterpret_cast<V *>(dv[e]) = *reinterpret_cast<const V *>(dl + e * digit_row);
                wv[e] = static_cast<W>(xw[l * DPT + e]);
            }
        }
#pragma unroll
        for (int v = 0; v < VN; ++v) {
            // the accumulator carries a residue (A_lt's word, or a folded sum) into every window of `lazy` terms, each at
            // most (q - 1)^2 (q - word <= q is one): the bound LimbConst::lazy_terms is computed for
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
            add(static_cast<D>(static_cast<W>(q - pv[v])));
            if (hit) add(static_cast<D>(static_cast<W>(q - gy)));
            if constexpr (DPT > 0) {
#pragma unroll
                for (int e = 0; e < DPT; ++e) add(static_cast<D>(wv[e]) * dv[e][v]);
            } else {
                for (uint32_t e = 0; e < dpt; ++e) add(static_cast<D>(static_cast<W>(xw[l * dpt + e])) * dl[e * digit_row + v]);
            }
            fold();
            ov[v] = static_cast<W>(acc);
        }
        *reinterpret_cast<V *>(out + w0) = *reinterpret_cast<const V *>(ov);
    }
}

template <typename W, int VN>
int launch_combine_vn(const char *who, GpuContext *ctx, const LweCombineArgs &a) {
    const size_t wpp = static_cast<size_t>(a.L) << a.logN, vecs = wpp / VN;
    const size_t gy = std::min<size_t>(a.entries, 65535), gz = (a.entries + gy - 1) / gy;
    if (gz > 65535) return set_error(std::string(who) + ": too many target polynomials in one group");
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // the targets written once; A_lt's chunk and the product read once, limb l of dpt digit rows per target word
    MXX_TRACE_BYTES(static_cast<double>(a.entries) * wpp * sizeof(W) * (3.0 + a.dpt));
#define MXX_COMBINE(D) MXX_LAUNCH((lwe_combine_kernel<W, VN, D>), grid, dim3(threads), 0, ctx->stream, a, ctx->d_limbs)
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
int launch_combine(const char *who, GpuContext *ctx, const LweCombineArgs &a) {
    constexpr int VN = 16 / sizeof(W);
    if (ctx->N % VN == 0) return launch_combine_vn<W, VN>(who, ctx, a);
    return launch_combine_vn<W, 1>(who, ctx, a);  // a limb vector narrower than 16 bytes
}

// what one accepted call works with
struct LweCall {
    const char *who;
    GpuContext *ctx;
    int level;
    uint32_t L, dpt, base_bits;
    size_t d, m, k, c, col_start;
    const GpuMatrix *a_lt;
};

// Everything both entries refuse, for every row, before anything is launched.  `digits` null: the full entry, whose a_z
// and tags are checked; otherwise the combine-only entry with the digits and the product given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, const GpuMatrix *a_z, const GpuMatrix *a_lt, const GpuMatrix *digits,
               const GpuMatrix *prod, size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *x,
               const GpuHashTags *tags, bool full, LweCall *call) {
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    if (!outs || !y_words || !x) return refuse("null array");
    if (!a_lt || (full ? !a_z : (!digits || !prod))) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    for (size_t t = 0; t < T; ++t)
        if (!outs[t]) return refuse("null output (row " + std::to_string(t) + ")");
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (base_bits == 0 || base_bits >= 63) return refuse("base_bits must be in 1..62");
    GpuContext *ctx = a_lt->ctx;
    const int level = a_lt->level;
    if (level < 0 || level >= ctx->limb_count) return refuse("level out of range");
    if (ctx->env.rng_compat && full) return refuse("unsupported under MXX_HIP_RNG_COMPAT=reference");
    const size_t L = static_cast<size_t>(level) + 1;
    const size_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = dpt * L, d = a_lt->rows, m = d * k, c = outs[0]->cols;
    if (c && T > ~size_t(0) / c) return refuse("matrix too large");
    // operand, rows, cols, what its shape is
    struct Operand {
        const GpuMatrix *mat;
        size_t rows, cols;
        const char *shape;
    };
    const Operand given[3] = {{full ? a_z : digits, full ? d : m, full ? m : T * c, full ? "A_z is d x (d * digits per tower * limbs)" : "the digits are m x (rows * chunk columns)"},
                              {a_lt, d, m, "A_lt is d x (d * digits per tower * limbs)"},
                              {full ? nullptr : prod, d, T * c, "the product is d x (rows * chunk columns)"}};
    for (const Operand &o : given) {
        if (!o.mat) continue;
        if (o.mat->ctx != ctx) return refuse("context mismatch");
        if (o.mat->level != level) return refuse("level mismatch");
        if (o.mat->rows != o.rows || o.mat->cols != o.cols) return refuse(std::string("shape mismatch: ") + o.shape);
        if (o.mat->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
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
    if (full && hash_tags_check(who, tags, T, &tag_bytes)) return 1;
    // an output is written while every operand is still being read, and by no other row
    const GpuMatrix *operands[3] = {given[0].mat, a_lt, prod};
    static const char *const names[3] = {"an operand", "an operand", "the product"};
    const std::string overlap = row_outputs_overlap(outs, T, operands, names, full ? 2 : 3);
    if (!overlap.empty()) return refuse(overlap);
    *call = LweCall{who, ctx, level, static_cast<uint32_t>(L), static_cast<uint32_t>(dpt), base_bits, d, m, k, c, col_start, a_lt};
    return 0;
}

// rows [0, Tg) of a group: their table (output pointers, x_t B^e mod q_l, (y_t mod q_tw) B^e mod q_tw per chunk column) in
// one staged copy, then the combine kernel over `digits` (m x (Tg c) words) and `prod` (d x (Tg c) words)
int combine_group(const LweCall &call, GpuMatrix *const *outs, size_t Tg, const void *digits, const void *prod, const uint64_t *y_words,
                  size_t words_per_y, const uint64_t *x) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, dpt = call.dpt, c = call.c, entries = Tg * call.d * c;
    if (entries == 0) return 0;
    const size_t table_words = Tg + Tg * L * dpt + Tg * c;
    CtxBlock block(ctx);
    if (block.alloc(sizeof(uint64_t) * table_words)) return 1;
    static thread_local std::vector<uint64_t> staging, ypow;  // the caller's arrays are not read after this call returns
    staging.resize(table_words);
    ypow.resize(L * dpt);
    uint64_t *xw = staging.data() + Tg, *gy = xw + Tg * L * dpt;
    for (size_t t = 0; t < Tg; ++t) {
        staging[t] = reinterpret_cast<uint64_t>(words_ptr(outs[t]));
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = ctx->moduli[l];
            const uint64_t B = (1ull << call.base_bits) % q;  // base_bits < 63
            uint64_t xv = x[t] % q, yv = words_mod(y_words + t * words_per_y, words_per_y, q);
            for (size_t e = 0; e < dpt; ++e) {
                xw[(t * L + l) * dpt + e] = xv;
                ypow[l * dpt + e] = yv;
                xv = static_cast<uint64_t>(static_cast<unsigned __int128>(xv) * B % q);
                yv = static_cast<uint64_t>(static_cast<unsigned __int128>(yv) * B % q);
            }
        }
        for (size_t cc = 0; cc < c; ++cc) gy[t * c + cc] = ypow[(call.col_start + cc) % call.k];  // column (j, tw, e): index tw dpt + e
    }
    uint64_t *d_table = static_cast<uint64_t *>(block.ptr);
    MXX_TRACED_COPY("LWE row table (host to device)", ctx->stream, sizeof(uint64_t) * table_words,
                    HIP_TRY(hipMemcpyAsync(d_table, staging.data(), sizeof(uint64_t) * table_words, hipMemcpyHostToDevice, ctx->stream)));
    LweCombineArgs a;
    a.a_lt = words_ptr(call.a_lt);
    a.digits = digits;
    a.prod = prod;
    a.rows = d_table;
    a.m = call.m;
    a.col_start = call.col_start;
    a.k = call.k;
    a.entries = entries;
    a.T = static_cast<uint32_t>(Tg);
    a.d = static_cast<uint32_t>(call.d);
    a.c = static_cast<uint32_t>(c);
    a.L = call.L;
    a.dpt = call.dpt;
    a.logN = ctx->logN;
    return ctx->wide ? launch_combine<uint64_t>(call.who, ctx, a) : launch_combine<uint32_t>(call.who, ctx, a);
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
    // rows per group: the digit scratch m x (Tg c) stays under the cap (one row at least), within the block sampler's 2^20
    const size_t row_bytes = call.m * call.c * poly_bytes;
    const size_t per_group = rows_per_group(T, row_bytes);
    CtxBlock digits(ctx), prod(ctx);
    if (digits.alloc(per_group * row_bytes)) return 1;
    if (prod.alloc(call.d * per_group * call.c * poly_bytes)) return 1;
    std::vector<size_t> offsets;
    for (size_t t0 = 0; t0 < T; t0 += per_group) {
        const size_t Tg = std::min(per_group, T - t0);
        const GpuHashTags part = hash_tags_rows(tags, t0, Tg, offsets);
        GpuMatrix v = scratch_matrix(ctx, call.level, call.m, Tg * call.c, digits.ptr);
        if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, base_bits, 0, call.d, call.m, col_start))
            return rc;
        GpuMatrix p = scratch_matrix(ctx, call.level, call.d, Tg * call.c, prod.ptr);
        if (int rc = launch_matmul(&p, a_z, &v)) return rc;
        if (int rc = combine_group(call, outs + t0, Tg, digits.ptr, prod.ptr, y_words + t0 * words_per_y, words_per_y, x + t0)) return rc;
    }
    return 0;
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
