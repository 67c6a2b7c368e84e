// scale_round.hip — exact scale-and-round of every coefficient, and the coefficients as multi-word integers.
//
// gpupoly_matrix_scale_round: coefficient c in [0, Q) -> floor((t c + h) / Q) mod t, Q the context's full modulus,
// h = floor(Q/2) or 0.  Replaces the host loops of modulus_switch (src/matrix/gpu_dcrt_poly.rs:1352-1372 with
// src/element/finite_ring.rs:22-26; h = 0) and of decode_centered_masked_matrix (src/decoder/masked_high_bit.rs:21-29,
// 39-70; h = floor(Q/2)), which rebuild N big integers per entry on the host.
//
// Exact method, one thread per coefficient, no multi-word arithmetic:
//   1. Garner on the residues r_k of c gives c's mixed-radix digits; Garner on (t r_k + h_k) mod q_k gives the digits of
//      y = (t c + h) mod Q.
//   2. With P_k = q_0 .. q_{k-1} mod m for the prime m = 2^64 - 59 (coprime to every q_k < 2^62), both digit sets give
//      c mod m and y mod m in O(L).
//   3. v = floor((t c + h) / Q) = (t c + h - y) / Q, and 0 <= v <= t < m, so v = (t c + h - y) Q^-1 mod m exactly.
//   4. v mod t (v - t when v = t) is written as its residue mod every limb.
// Two O(L^2) Garner passes and O(L) further work per coefficient; any t < m.
//
// gpupoly_matrix_store_coeff_words: the same Garner digits, Horner-evaluated to 64-bit words (coeffs(),
// src/poly/dcrt/gpu.rs:959-994).
#include "common.h"
#include "crt.h"
#include "modarith.h"
#include "scale_exact.h"

namespace {

struct ScaleConsts {
    int limbs;
    uint64_t t;       // 1 <= t < m
    uint64_t h_m;     // h mod m
    uint64_t qinv_m;  // Q^-1 mod m
    uint64_t q[GPUPOLY_MAX_LIMBS];
    uint64_t tq[GPUPOLY_MAX_LIMBS];  // t mod q_k
    uint64_t hq[GPUPOLY_MAX_LIMBS];  // h mod q_k
    uint64_t pm[GPUPOLY_MAX_LIMBS];  // q_0 .. q_{k-1} mod m
};

struct WordConsts {
    int limbs;
    int words;  // 64-bit words of Q_level
    uint64_t q[GPUPOLY_MAX_LIMBS];
};

// src and dst may be the same matrix: a thread reads all residues of its coefficient before it writes any
template <typename W, int ML>
__global__ void __launch_bounds__(256) scale_round_kernel(const W *src, W *dst, size_t polys, uint32_t N, ScaleConsts sc,
                                                          const uint64_t *__restrict__ garner, size_t garner_stride,
                                                          const LimbConst *__restrict__ limbs) {
    const size_t idx = item_index();
    if (idx >= polys * N) return;
    const size_t poly = idx / N;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const int L = sc.limbs;
    uint64_t rc[ML], rx[ML];
    load_residues<W, ML>(src, poly, i, N, L, rc);
    auto residue_of_x = [&](int k) {  // (t r_k + h_k) mod q_k
        const W qk = static_cast<W>(sc.q[k]);
        const W p = mul_mod<W>(static_cast<W>(sc.tq[k]), static_cast<W>(rc[k]), qk, limbs[k].mu, limbs[k].kbits);
        rx[k] = static_cast<uint64_t>(add_mod<W>(p, static_cast<W>(sc.hq[k]), qk));
    };
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) residue_of_x(k);
    } else {
        for (int k = 0; k < L; ++k) residue_of_x(k);
    }
    crt_garner_digits<W, ML>(rc, rc, L, sc.q, garner, garner_stride, limbs);
    crt_garner_digits<W, ML>(rx, rx, L, sc.q, garner, garner_stride, limbs);
    uint64_t cm = 0, ym = 0;  // c mod m, y mod m
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) {
                cm = aux_add(cm, aux_mul(rc[k], sc.pm[k]));
                ym = aux_add(ym, aux_mul(rx[k], sc.pm[k]));
            }
    } else {
        for (int k = 0; k < L; ++k) {
            cm = aux_add(cm, aux_mul(rc[k], sc.pm[k]));
            ym = aux_add(ym, aux_mul(rx[k], sc.pm[k]));
        }
    }
    const uint64_t v = aux_mul(aux_sub(aux_add(aux_mul(sc.t, cm), sc.h_m), ym), sc.qinv_m);  // in [0, t]
    const uint64_t r = v >= sc.t ? v - sc.t : v;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) dst[(poly * L + k) * N + i] = static_cast<W>(reduce_word(r, sc.q[k], limbs[k].mu64));
    } else {
        for (int k = 0; k < L; ++k) dst[(poly * L + k) * N + i] = static_cast<W>(reduce_word(r, sc.q[k], limbs[k].mu64));
    }
}

// out[idx * wpc + w]: word w of coefficient idx = poly * N + i, zero above the words of Q_level
template <typename W, int ML>
__global__ void __launch_bounds__(256) coeff_words_kernel(const W *__restrict__ src, size_t polys, uint32_t N, WordConsts wc,
                                                          const uint64_t *__restrict__ garner, size_t garner_stride,
                                                          const LimbConst *__restrict__ limbs, uint64_t *__restrict__ out,
                                                          uint32_t wpc) {
    const size_t idx = item_index();
    if (idx >= polys * N) return;
    const int L = wc.limbs;
    uint64_t v[ML], x[ML];
    load_residues<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, L, v);
    crt_garner_digits<W, ML>(v, v, L, wc.q, garner, garner_stride, limbs);
    crt_horner_words<ML>(v, L, wc.q, wc.words, x);
    uint64_t *o = out + idx * wpc;
    for (int w = 0; w < wc.words; ++w) o[w] = x[w];
    for (uint32_t w = static_cast<uint32_t>(wc.words); w < wpc; ++w) o[w] = 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// the multi-word helpers that build the constants: scale_exact.h
#define BY_LIMBS(KERNEL, WT, L, ...)                                                                       \
    do {                                                                                                   \
        if ((L) <= 8) MXX_LAUNCH((KERNEL<WT, 8>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__);           \
        else if ((L) <= 16) MXX_LAUNCH((KERNEL<WT, 16>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__);    \
        else MXX_LAUNCH((KERNEL<WT, 64>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__);                   \
    } while (0)

}  // namespace

extern "C" int gpupoly_matrix_scale_round(GpuMatrix *out, const GpuMatrix *in, uint64_t t, int round_half) {
    ABI_GUARD_BEGIN
    // every refusal comes before the first launch and before `out` or its tag is touched
    if (!out || !in) return set_error("gpupoly_matrix_scale_round: null matrix");
    if (t == 0) return set_error("gpupoly_matrix_scale_round: t must be at least 1");
    if (out->ctx != in->ctx) return set_error("gpupoly_matrix_scale_round: context mismatch");
    if (out->rows != in->rows || out->cols != in->cols) return set_error("gpupoly_matrix_scale_round: shape mismatch");
    GpuContext *ctx = in->ctx;
    const int L = ctx->limb_count;
    if (out->level != L - 1) return set_error("gpupoly_matrix_scale_round: level mismatch (out must be at full level)");
    if (t >= kAuxM) return set_error("gpupoly_matrix_scale_round: unsupported t (t >= 2^64 - 59): use the host path");
    if (in->level != L - 1) return set_error("gpupoly_matrix_scale_round: unsupported input below full level: use the host path");
    if (partial_overlap(out, in))
        return set_error("gpupoly_matrix_scale_round: the output overlaps the input without being the same block");
    const size_t polys = matrix_polys(in);
    if (polys == 0) {
        out->format = GPU_POLY_FORMAT_COEFF;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;

    ScaleConsts sc;
    sc.limbs = L;
    sc.t = t;
    const std::vector<uint64_t> Q = h_product_words(ctx->moduli, L);
    const std::vector<uint64_t> half = round_half ? h_half_words(Q) : std::vector<uint64_t>(Q.size(), 0);  // h
    sc.h_m = h_words_mod(half, kAuxM);
    sc.qinv_m = h_powmod64(h_words_mod(Q, kAuxM), kAuxM - 2, kAuxM);
    uint64_t pm = 1;
    for (int k = 0; k < static_cast<int>(GPUPOLY_MAX_LIMBS); ++k) {
        const bool on = k < L;
        const uint64_t q = on ? ctx->moduli[k] : 1;
        sc.q[k] = on ? q : 0;
        sc.tq[k] = on ? t % q : 0;
        sc.hq[k] = on ? h_words_mod(half, q) : 0;
        sc.pm[k] = on ? pm : 0;
        if (on) pm = h_mulmod64(pm, q, kAuxM);
    }

    const size_t words = matrix_words(in);
    const size_t word_bytes = static_cast<size_t>(ctx->word_bytes);
    const void *src = words_ptr(in);
    if (in->format == GPU_POLY_FORMAT_EVAL) {
        // inverse transform in `out` (a copy of `in` first when they differ): `in` is left as it was
        if (!same_block(out, in))
            MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * in->bytes,
                            HIP_TRY(hipMemcpyAsync(words_ptr(out), words_ptr(in), in->bytes, hipMemcpyDeviceToDevice, ctx->stream)));
        const int rc = launch_ntt(ctx, words_ptr(out), polys * static_cast<size_t>(L), L, true);
        if (rc) return rc;
        out->format = GPU_POLY_FORMAT_COEFF;
        src = words_ptr(out);
    }
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const dim3 grid = item_grid(polys * N, 256);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    MXX_TRACE_BYTES(2.0 * static_cast<double>(words * word_bytes));
    if (ctx->wide)
        BY_LIMBS(scale_round_kernel, uint64_t, L, static_cast<const uint64_t *>(src), static_cast<uint64_t *>(words_ptr(out)), polys, N,
                 sc, ctx->d_garner, gstride, ctx->d_limbs);
    else
        BY_LIMBS(scale_round_kernel, uint32_t, L, static_cast<const uint32_t *>(src), static_cast<uint32_t *>(words_ptr(out)), polys, N,
                 sc, ctx->d_garner, gstride, ctx->d_limbs);
    HIP_TRY(hipGetLastError());
    out->format = GPU_POLY_FORMAT_COEFF;
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_store_coeff_words(const GpuMatrix *mat, uint64_t *out, size_t words_per_coeff) {
    ABI_GUARD_BEGIN
    if (!mat || !out) return set_error("gpupoly_matrix_store_coeff_words: null argument");
    GpuContext *ctx = mat->ctx;
    const int L = mat->level + 1;
    const std::vector<uint64_t> Q = h_product_words(ctx->moduli, L);
    if (words_per_coeff < Q.size())
        return set_error("gpupoly_matrix_store_coeff_words: words_per_coeff is below the " + std::to_string(Q.size()) +
                         " words the level's modulus needs");
    if (words_per_coeff > 0xffffffffull) return set_error("gpupoly_matrix_store_coeff_words: words_per_coeff too large");
    const size_t polys = matrix_polys(mat);
    if (polys == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    WordConsts wc;
    wc.limbs = L;
    wc.words = static_cast<int>(Q.size());
    for (int k = 0; k < static_cast<int>(GPUPOLY_MAX_LIMBS); ++k) wc.q[k] = k < L ? ctx->moduli[k] : 0;

    const void *src = words_ptr(mat);
    CtxBlock scratch(ctx);
    if (mat->format == GPU_POLY_FORMAT_EVAL) {  // scratch inverse transform: `mat` is left as it was
        if (scratch.alloc(mat->bytes)) return 1;
        MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * mat->bytes,
                        HIP_TRY(hipMemcpyAsync(scratch.ptr, words_ptr(mat), mat->bytes, hipMemcpyDeviceToDevice, ctx->stream)));
        const int rc = launch_ntt(ctx, scratch.ptr, polys * static_cast<size_t>(L), L, true);
        if (rc) return rc;
        src = scratch.ptr;
    }
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const size_t coeffs = polys * N;
    const size_t out_bytes = coeffs * words_per_coeff * sizeof(uint64_t);
    CtxBlock dev_out(ctx);
    if (dev_out.alloc(out_bytes)) return 1;
    const dim3 grid = item_grid(coeffs, 256);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    const uint32_t wpc = static_cast<uint32_t>(words_per_coeff);
    MXX_TRACE_BYTES(static_cast<double>(matrix_words(mat) * ctx->word_bytes + out_bytes));
    if (ctx->wide)
        BY_LIMBS(coeff_words_kernel, uint64_t, L, static_cast<const uint64_t *>(src), polys, N, wc, ctx->d_garner, gstride,
                 ctx->d_limbs, static_cast<uint64_t *>(dev_out.ptr), wpc);
    else
        BY_LIMBS(coeff_words_kernel, uint32_t, L, static_cast<const uint32_t *>(src), polys, N, wc, ctx->d_garner, gstride,
                 ctx->d_limbs, static_cast<uint64_t *>(dev_out.ptr), wpc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dev_out.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
    ABI_GUARD_END
}
