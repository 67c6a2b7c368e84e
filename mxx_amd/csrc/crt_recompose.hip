// crt_recompose.hip — rounded CRT recomposition of decoded level vectors in one call (extension).
//
// gpupoly_matrix_crt_recompose_rounded replaces crt_recompose_rows (src/noise_refresh/naive_vec.rs:2086-2118) and the
// four-term combination in front of it (:1654-1690).  For every output row (slot) and CRT limb i the reference decodes
// one level vector with t = q_i (decode_centered_masked_matrix, src/decoder/masked_high_bit.rs:21-29), multiplies by
// the constant polynomial e_i = reconst_coeffs[i] (src/poly/mod.rs:45-60) and accumulates.  e_i is 1 mod q_i and 0 mod
// every other limb, so limb j of sum_i v_i e_i is v_j: each output limb comes from exactly one level,
//   out[slot][col][limb i][k] = floor((q_i c + floor(Q/2)) / Q) mod q_i,  c = coefficient k of entry col of level (slot, i).
//
// Per chunk of whole slots:
//   stage   level (slot, i) = sum_t signs[t] * term_t into call-owned scratch, 16 bytes per lane, up to 64 term pointers
//           by value per launch (a plain copy for one term).  EVAL terms are summed as they lie.
//   intt    one inverse transform of the scratch (EVAL terms only): one per level, not one per term.
//   round   the exact scale-and-round of scale_round.hip with t = q_i per thread and h = floor(Q/2): Garner on the level's
//           residues and on (q_i r_k + h_k) mod q_k, both digit sets mod m = 2^64 - 59, v = (q_i c + h - y) Q^-1 mod m,
//           v = q_i -> 0; only limb i of `out` is stored.  q_i mod q_k is one reduce_word, no L x L table.
// Then one forward transform of `out`.
#include "common.h"
#include "crt.h"
#include "modarith.h"
#include "scale_exact.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace {

constexpr size_t kStagePtrs = 64;  // term pointers per stage launch
constexpr size_t kMaxTerms = 8;    // terms per level

struct StageArgs {
    const void *term[kStagePtrs];  // [level of the group][t]
};

struct RoundConsts {
    int limbs;
    uint64_t h_m;     // floor(Q/2) mod m
    uint64_t qinv_m;  // Q^-1 mod m
    uint64_t q[GPUPOLY_MAX_LIMBS];
    uint64_t hq[GPUPOLY_MAX_LIMBS];  // floor(Q/2) mod q_k
    uint64_t pm[GPUPOLY_MAX_LIMBS];  // q_0 .. q_{k-1} mod m
};

template <typename W, int SV>
struct StageVec {
    typedef typename std::conditional<sizeof(W) * SV == 16, uint4, W>::type type;
};

// scratch[level][w] = sum_t +-term[level * T + t][w]; grid y = level of the group, x (item-numbered within y) = SV words.
// SV > 1 only when N % SV == 0: the words of a vector then share one limb.  neg_mask bit t: term t is subtracted.
template <typename W, int SV>
__global__ void __launch_bounds__(256) crt_stage_kernel(W *__restrict__ scratch, StageArgs args, uint32_t T, uint32_t neg_mask,
                                                        size_t level_words, const LimbConst *__restrict__ limbs, uint32_t L,
                                                        uint32_t logN) {
    typedef typename StageVec<W, SV>::type VT;
    const size_t v = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t w0 = v * SV;
    if (w0 >= level_words) return;
    const uint32_t lvl = blockIdx.y;
    const W q = static_cast<W>(limbs[(w0 >> logN) % L].q);
    W acc[SV];
#pragma unroll
    for (int s = 0; s < SV; ++s) acc[s] = 0;
    for (uint32_t t = 0; t < T; ++t) {
        W a[SV];
        *reinterpret_cast<VT *>(a) = *reinterpret_cast<const VT *>(static_cast<const W *>(args.term[lvl * T + t]) + w0);
        const bool neg = (neg_mask >> t) & 1u;
#pragma unroll
        for (int s = 0; s < SV; ++s) acc[s] = neg ? sub_mod<W>(acc[s], a[s], q) : add_mod<W>(acc[s], a[s], q);
    }
    *reinterpret_cast<VT *>(scratch + static_cast<size_t>(lvl) * level_words + w0) = *reinterpret_cast<const VT *>(acc);
}

// One thread per output word: dst is the chunk's rows of `out`, [slot][col][limb i][N]; src the chunk's levels in COEFF form,
// [slot][i][col][limb k][N].  The thread decodes coefficient `coef` of entry `col` of level (slot, i) for t = q_i.
template <typename W, int ML>
__global__ void __launch_bounds__(256) crt_round_kernel(const W *__restrict__ src, W *__restrict__ dst, size_t out_words, uint32_t cols,
                                                        uint32_t N, RoundConsts rc_, const uint64_t *__restrict__ garner,
                                                        size_t garner_stride, const LimbConst *__restrict__ limbs) {
    const size_t idx = item_index();
    if (idx >= out_words) return;
    const int L = rc_.limbs;
    const uint32_t coef = static_cast<uint32_t>(idx % N);
    const size_t rest = idx / N;
    const uint32_t i = static_cast<uint32_t>(rest % L);
    const size_t entry = rest / L;  // slot * cols + col
    const size_t slot = entry / cols, col = entry % cols;
    const size_t poly = (slot * L + i) * cols + col;  // the level's entry in src
    const uint64_t t = limbs[i].q;
    uint64_t rc[ML], rx[ML];
    load_residues<W, ML>(src, poly, coef, N, L, rc);
    auto residue_of_x = [&](int k) {  // (q_i r_k + h_k) mod q_k; q_i mod q_k is 0 at k = i
        const W qk = static_cast<W>(rc_.q[k]);
        const W tq = static_cast<W>(reduce_word(t, rc_.q[k], limbs[k].mu64));
        const W p = mul_mod<W>(tq, static_cast<W>(rc[k]), qk, limbs[k].mu, limbs[k].kbits);
        rx[k] = static_cast<uint64_t>(add_mod<W>(p, static_cast<W>(rc_.hq[k]), qk));
    };
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) residue_of_x(k);
    } else {
        for (int k = 0; k < L; ++k) residue_of_x(k);
    }
    crt_garner_digits<W, ML>(rc, rc, L, rc_.q, garner, garner_stride, limbs);
    crt_garner_digits<W, ML>(rx, rx, L, rc_.q, garner, garner_stride, limbs);
    uint64_t cm = 0, ym = 0;  // c mod m, y mod m
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) {
                cm = aux_add(cm, aux_mul(rc[k], rc_.pm[k]));
                ym = aux_add(ym, aux_mul(rx[k], rc_.pm[k]));
            }
    } else {
        for (int k = 0; k < L; ++k) {
            cm = aux_add(cm, aux_mul(rc[k], rc_.pm[k]));
            ym = aux_add(ym, aux_mul(rx[k], rc_.pm[k]));
        }
    }
    const uint64_t v = aux_mul(aux_sub(aux_add(aux_mul(t, cm), rc_.h_m), ym), rc_.qinv_m);  // in [0, q_i]
    dst[idx] = static_cast<W>(v >= t ? v - t : v);                                           // below q_i: its own residue
}

template <typename W>
int stage_group(GpuContext *ctx, W *scratch, const StageArgs &args, uint32_t levels, uint32_t T, uint32_t neg_mask, size_t level_words) {
    constexpr int VN = 16 / sizeof(W);
    const uint32_t N = static_cast<uint32_t>(ctx->N), L = static_cast<uint32_t>(ctx->limb_count);
    // every term of the group read once, the scratch written once
    MXX_TRACE_BYTES(static_cast<double>(levels) * static_cast<double>(level_words) * sizeof(W) * (T + 1));
    if (N % VN == 0) {
        const dim3 grid(static_cast<unsigned>((level_words / VN + 255) / 256), levels);
        MXX_LAUNCH((crt_stage_kernel<W, VN>), grid, dim3(256), 0, ctx->stream, scratch, args, T, neg_mask, level_words, ctx->d_limbs, L,
                   ctx->logN);
    } else {
        const dim3 grid(static_cast<unsigned>((level_words + 255) / 256), levels);
        MXX_LAUNCH((crt_stage_kernel<W, 1>), grid, dim3(256), 0, ctx->stream, scratch, args, T, neg_mask, level_words, ctx->d_limbs, L,
                   ctx->logN);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int round_chunk(GpuContext *ctx, const W *src, W *dst, size_t out_words, uint32_t cols, const RoundConsts &rc) {
    const int L = ctx->limb_count;
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const dim3 grid = item_grid(out_words, 256);
    const size_t gstride = static_cast<size_t>(L);
    // L residues read per output word, one word written
    MXX_TRACE_BYTES(static_cast<double>(out_words) * sizeof(W) * (L + 1));
    if (L <= 8) MXX_LAUNCH((crt_round_kernel<W, 8>), grid, dim3(256), 0, ctx->stream, src, dst, out_words, cols, N, rc, ctx->d_garner, gstride, ctx->d_limbs);
    else if (L <= 16) MXX_LAUNCH((crt_round_kernel<W, 16>), grid, dim3(256), 0, ctx->stream, src, dst, out_words, cols, N, rc, ctx->d_garner, gstride, ctx->d_limbs);
    else MXX_LAUNCH((crt_round_kernel<W, 64>), grid, dim3(256), 0, ctx->stream, src, dst, out_words, cols, N, rc, ctx->d_garner, gstride, ctx->d_limbs);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int recompose(GpuContext *ctx, GpuMatrix *out, const std::vector<const void *> &ptrs, size_t T, uint32_t neg_mask, size_t num_slots,
              bool eval, const RoundConsts &rc) {
    const size_t L = static_cast<size_t>(ctx->limb_count), N = static_cast<size_t>(ctx->N), cols = out->cols;
    const size_t level_words = cols * L * N, slot_words = L * level_words;  // scratch of one level, of one slot
    const size_t slot_bytes = slot_words * sizeof(W);
    const size_t chunk_slots = std::min(num_slots, std::max<size_t>(1, ctx->env.crt_recompose_chunk_bytes / slot_bytes));
    CtxBlock scratch(ctx);
    if (scratch.alloc(chunk_slots * slot_bytes)) return 1;
    W *const sc = static_cast<W *>(scratch.ptr);
    W *const o = static_cast<W *>(words_ptr(out));
    const size_t group_levels = kStagePtrs / T;
    for (size_t s0 = 0; s0 < num_slots; s0 += chunk_slots) {
        const size_t slots = std::min(chunk_slots, num_slots - s0), levels = slots * L;
        for (size_t l0 = 0; l0 < levels; l0 += group_levels) {
            const size_t g = std::min(group_levels, levels - l0);
            StageArgs args;
            for (size_t j = 0; j < kStagePtrs; ++j) args.term[j] = ptrs[(s0 * L + l0) * T + std::min(j, g * T - 1)];
            const int rcode = stage_group<W>(ctx, sc + l0 * level_words, args, static_cast<uint32_t>(g), static_cast<uint32_t>(T), neg_mask,
                                             level_words);
            if (rcode) return rcode;
        }
        if (eval) {
            const int rcode = launch_ntt(ctx, sc, levels * cols * L, static_cast<int>(L), true);
            if (rcode) return rcode;
        }
        // the chunk's rows of `out` have as many words as one slot of scratch per slot / L
        const int rcode = round_chunk<W>(ctx, sc, o + s0 * level_words, slots * level_words, static_cast<uint32_t>(cols), rc);
        if (rcode) return rcode;
    }
    return launch_ntt(ctx, o, num_slots * cols * L, static_cast<int>(L), false);
}

}  // namespace

extern "C" int gpupoly_matrix_crt_recompose_rounded(GpuMatrix *out, const GpuMatrix *const *terms, const int *signs,
                                                    size_t terms_per_level, size_t num_slots) {
    ABI_GUARD_BEGIN
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_crt_recompose_rounded: " + what); };
    // ---- every refusal, for every term, before the first launch and before `out` or its tag is touched ----
    if (!out || !terms || !signs) return refuse("null argument");
    if (num_slots == 0) return refuse("num_slots must be at least 1");
    const size_t T = terms_per_level;
    if (T == 0 || T > kMaxTerms) return refuse("terms_per_level must be in 1..8");
    uint32_t neg_mask = 0;
    for (size_t t = 0; t < T; ++t) {
        if (signs[t] != 1 && signs[t] != -1) return refuse("signs must be +1 or -1 (term " + std::to_string(t) + ")");
        if (signs[t] < 0) neg_mask |= 1u << t;
    }
    GpuContext *ctx = out->ctx;
    const size_t L = static_cast<size_t>(ctx->limb_count);
    if (num_slots > (~static_cast<size_t>(0)) / (L * T)) return refuse("num_slots too large");
    const size_t count = num_slots * L * T;
    for (size_t j = 0; j < count; ++j)
        if (!terms[j]) return refuse("null matrix (terms[" + std::to_string(j) + "])");
    if (out->level != static_cast<int>(L) - 1) return refuse("level mismatch (out must be at full level)");
    if (out->rows != num_slots) return refuse("shape mismatch (out must have num_slots rows)");
    const int format = terms[0]->format;
    if (format != GPU_POLY_FORMAT_COEFF && format != GPU_POLY_FORMAT_EVAL) return refuse("unknown format");
    for (size_t j = 0; j < count; ++j) {
        const GpuMatrix *m = terms[j];
        const std::string at = " (terms[" + std::to_string(j) + "])";
        if (m->ctx != ctx) return refuse("context mismatch" + at);
        if (m->level != out->level) return refuse("unsupported term below full level: use the host path" + at);
        if (m->rows != 1 || m->cols != out->cols) return refuse("shape mismatch: every term is 1 x out's columns" + at);
        if (m->format != format) return refuse("terms must share one format" + at);
        if (storage_overlaps(out, m)) return refuse("the output overlaps a term" + at);
    }
    if (out->cols == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    // blockIdx.x of the stage kernel numbers the words of one level: below 2^32 threads along x
    if (out->cols * L * static_cast<size_t>(ctx->N) > 0xffffffffull) return refuse("level vector too large");
    if (ctx_activate(ctx)) return 1;

    RoundConsts rc;
    rc.limbs = static_cast<int>(L);
    const std::vector<uint64_t> Q = h_product_words(ctx->moduli, rc.limbs);
    const std::vector<uint64_t> half = h_half_words(Q);
    rc.h_m = h_words_mod(half, kAuxM);
    rc.qinv_m = h_powmod64(h_words_mod(Q, kAuxM), kAuxM - 2, kAuxM);
    uint64_t pm = 1;
    for (size_t k = 0; k < GPUPOLY_MAX_LIMBS; ++k) {
        const bool on = k < L;
        const uint64_t q = on ? ctx->moduli[k] : 1;
        rc.q[k] = on ? q : 0;
        rc.hq[k] = on ? h_words_mod(half, q) : 0;
        rc.pm[k] = on ? pm : 0;
        if (on) pm = h_mulmod64(pm, q, kAuxM);
    }
    // PACKED24 terms are unpacked here, all of them before the first launch of the recomposition
    std::vector<const void *> ptrs(count);
    for (size_t j = 0; j < count; ++j) ptrs[j] = words_ptr(terms[j]);
    const bool eval = format == GPU_POLY_FORMAT_EVAL;
    const int rcode = ctx->wide ? recompose<uint64_t>(ctx, out, ptrs, T, neg_mask, num_slots, eval, rc)
                                : recompose<uint32_t>(ctx, out, ptrs, T, neg_mask, num_slots, eval, rc);
    if (rcode) return rcode;
    out->format = GPU_POLY_FORMAT_EVAL;
    return 0;
    ABI_GUARD_END
}
