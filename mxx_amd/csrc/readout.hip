// readout.hip — bits and machine integers of every coefficient, without the big integers in between.
//
// gpupoly_matrix_extract_bits: one bit per coefficient, set iff the coefficient c in [0, Q) lies in an interval
// [lo, hi) (wrapping round Q when lo > hi), Q = q_0 .. q_level the matrix's own modulus.  Replaces the host loops of
// extract_bits_with_threshold (src/poly/dcrt/gpu.rs:1070-1081) and of the boolean centred decode
// (decode_centered_masked_boolean_coeff, src/decoder/masked_high_bit.rs:31-35), which rebuild every coefficient as a
// big integer for two comparisons.
// gpupoly_matrix_store_coeff_ints: the coefficients (or their centred representatives) truncated to 32 / 64 bits, with
// the number and the first position of those that do not fit.  Replaces to_bool_vec (gpu.rs:1083-1097), coeffs_digits
// (src/poly/mod.rs:130-139) and const_coeff_u64 (gpu.rs:1103-1120).
//
// Exact method, one thread per coefficient, no floating point and no multi-word arithmetic:
//   1. Garner on the residues gives the mixed-radix digits v_k of c = v_0 + v_1 q_0 + v_2 q_0 q_1 + .. (v_k < q_k).
//   2. c < B for a bound B in [0, Q) is the lexicographic comparison of (v_{L-1}, .., v_0) with B's digits, the top digit
//      first: the representation is unique and the weight of digit k exceeds everything the digits below it can add
//      up to.  The host computes every bound's digits once per call (readout_bounds.h); B = Q is a flag.
//   3. c mod 2^64 = sum_k v_k (q_0 .. q_{k-1} mod 2^64) in wrapping 64-bit arithmetic; the centred representative of a
//      c above floor(Q/2) is that minus Q mod 2^64.
// The bits of a wave come from one __ballot and leave as whole words (whole bytes where N < 8).
#include "common.h"
#include "crt.h"
#include "modarith.h"
#include "readout_bounds.h"

#include <algorithm>
#include <cstring>

namespace {

static_assert(readout::kMaxLimbs == static_cast<int>(GPUPOLY_MAX_LIMBS), "readout_bounds.h covers the library's limb bound");

constexpr uint32_t kReadoutThreads = 256;

struct ReadoutConsts {
    int limbs;
    int is_q[3];       // bound j is Q itself: every coefficient lies below it
    int wrap;          // extract_bits: lo > hi, the interval is [lo, Q) u [0, hi)
    int centred;       // store_coeff_ints: the element is the centred representative
    int elem_bytes;    // store_coeff_ints: 4 or 8
    uint64_t q_low;    // Q mod 2^64
    uint64_t q[GPUPOLY_MAX_LIMBS];
    uint64_t pw[GPUPOLY_MAX_LIMBS];    // q_0 .. q_{k-1} mod 2^64
    // digits of the bounds.  extract_bits: lo, hi.  store_coeff_ints: min(2^b, Q) (plain) or min(2^(b-1), Q) (centred),
    // max(Q - 2^(b-1), 0), floor(Q/2) + 1
    uint64_t b[3][GPUPOLY_MAX_LIMBS];
};

template <typename W, int ML>
__device__ __forceinline__ void readout_digits(const W *src, size_t poly, uint32_t i, uint32_t N, const ReadoutConsts &rc,
                                               const uint64_t *__restrict__ garner, size_t garner_stride,
                                               const LimbConst *__restrict__ limbs, uint64_t *v) {
    const int L = rc.limbs;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) v[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    } else {
        for (int k = 0; k < L; ++k) v[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    }
    crt_garner_digits<W, ML>(v, v, L, rc.q, garner, garner_stride, limbs);
}

// c < bound j, c given by its digits: the highest digit where they differ decides
template <int ML>
__device__ __forceinline__ bool digits_below(const uint64_t *v, const ReadoutConsts &rc, int j) {
    bool lt = false;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < rc.limbs && v[k] != rc.b[j][k]) lt = v[k] < rc.b[j][k];
    } else {
        for (int k = 0; k < rc.limbs; ++k)
            if (v[k] != rc.b[j][k]) lt = v[k] < rc.b[j][k];
    }
    return lt || rc.is_q[j] != 0;
}

// c mod 2^64
template <int ML>
__device__ __forceinline__ uint64_t digits_low_word(const uint64_t *v, const ReadoutConsts &rc) {
    uint64_t s = 0;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < rc.limbs) s += v[k] * rc.pw[k];
    } else {
        for (int k = 0; k < rc.limbs; ++k) s += v[k] * rc.pw[k];
    }
    return s;
}

}  // namespace

// Bit idx = poly * N + i of the stream is the membership of coefficient i of entry `poly`.  N >= 8: the stream itself is
// the output (N / 8 bytes per entry), written as the waves' 64-bit ballot words: words[idx / 64], `words` holding
// ceil(total / 64) words.  N < 8: entry `poly` owns byte `poly`, bits [0, N) of it, the rest zero.
template <typename W, int ML>
__global__ void __launch_bounds__(kReadoutThreads) extract_bits_kernel(const W *__restrict__ src, size_t polys, uint32_t N,
                                                                       ReadoutConsts rc, const uint64_t *__restrict__ garner,
                                                                       size_t garner_stride, const LimbConst *__restrict__ limbs,
                                                                       uint64_t *__restrict__ words) {
    const size_t idx = item_index(), total = polys * N;
    const bool live = idx < total;  // no early return: the whole wave takes part in the ballot
    bool bit = false;
    if (live) {
        uint64_t v[ML];
        readout_digits<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, rc, garner, garner_stride, limbs, v);
        const bool ge_lo = !digits_below<ML>(v, rc, 0), lt_hi = digits_below<ML>(v, rc, 1);
        bit = rc.wrap ? (ge_lo || lt_hi) : (ge_lo && lt_hi);
    }
    const uint64_t ballot = __ballot(bit);  // bit l: lane l, whose idx is the wave's first idx + l (256 = 4 waves per block)
    const uint32_t lane = threadIdx.x & 63u;
    if (N >= 8) {
        if (lane == 0 && live) words[idx >> 6] = ballot;
    } else if (live && idx % N == 0) {  // N divides 64: the entry's bits are lanes [lane, lane + N)
        reinterpret_cast<uint8_t *>(words)[idx / N] = static_cast<uint8_t>((ballot >> lane) & ((1u << N) - 1u));
    }
}

// out element idx = poly * cpp + i: coefficient i < cpp of entry `poly`.  stats[0] += misfits, stats[1] = min(their idx).
template <typename W, int ML>
__global__ void __launch_bounds__(kReadoutThreads) coeff_ints_kernel(const W *__restrict__ src, size_t polys, uint32_t N,
                                                                     uint32_t cpp, ReadoutConsts rc,
                                                                     const uint64_t *__restrict__ garner, size_t garner_stride,
                                                                     const LimbConst *__restrict__ limbs, void *__restrict__ out,
                                                                     unsigned long long *__restrict__ stats) {
    const size_t idx = item_index(), total = polys * cpp;
    const bool live = idx < total;
    bool misfit = false;
    if (live) {
        uint64_t v[ML];
        readout_digits<W, ML>(src, idx / cpp, static_cast<uint32_t>(idx % cpp), N, rc, garner, garner_stride, limbs, v);
        uint64_t x = digits_low_word<ML>(v, rc);
        if (rc.centred) {
            // x in [-2^(b-1), 2^(b-1) - 1]  <=>  c < 2^(b-1) or c >= Q - 2^(b-1)
            misfit = !(digits_below<ML>(v, rc, 0) || !digits_below<ML>(v, rc, 1));
            if (!digits_below<ML>(v, rc, 2)) x -= rc.q_low;  // c > floor(Q/2): x = c - Q
        } else {
            misfit = !digits_below<ML>(v, rc, 0);
        }
        if (rc.elem_bytes == 4) static_cast<uint32_t *>(out)[idx] = static_cast<uint32_t>(x);
        else static_cast<uint64_t *>(out)[idx] = x;
    }
    const uint64_t ballot = __ballot(misfit);
    if (ballot != 0 && (threadIdx.x & 63u) == 0) {  // lane 0 is live whenever any lane of its wave is
        atomicAdd(&stats[0], static_cast<unsigned long long>(__popcll(ballot)));
        atomicMin(&stats[1], static_cast<unsigned long long>(idx + static_cast<size_t>(__ffsll(static_cast<long long>(ballot)) - 1)));
    }
}

namespace {

#define READOUT_BY_LIMBS(KERNEL, WT, L, ...)                                                                          \
    do {                                                                                                              \
        if ((L) <= 8) MXX_LAUNCH((KERNEL<WT, 8>), grid, dim3(kReadoutThreads), 0, ctx->stream, __VA_ARGS__);          \
        else if ((L) <= 16) MXX_LAUNCH((KERNEL<WT, 16>), grid, dim3(kReadoutThreads), 0, ctx->stream, __VA_ARGS__);   \
        else MXX_LAUNCH((KERNEL<WT, 64>), grid, dim3(kReadoutThreads), 0, ctx->stream, __VA_ARGS__);                  \
    } while (0)

void set_bound(ReadoutConsts &rc, int j, const readout::BoundDigits &b) {
    rc.is_q[j] = b.is_q;
    for (size_t k = 0; k < GPUPOLY_MAX_LIMBS; ++k) rc.b[j][k] = b.d[k];
}

void init_consts(ReadoutConsts &rc, const GpuContext *ctx, int L) {
    std::memset(&rc, 0, sizeof(rc));
    rc.limbs = L;
    for (int k = 0; k < L; ++k) rc.q[k] = ctx->moduli[k];
    readout::wrapping_prefix_products(rc.q, L, rc.pw, &rc.q_low);
}

}  // namespace

extern "C" int gpupoly_matrix_extract_bits(const GpuMatrix *mat, const uint64_t *lo, const uint64_t *hi, size_t words_per_bound,
                                           uint8_t *out, size_t bytes_per_poly) {
    ABI_GUARD_BEGIN
    // every refusal comes before the first launch and before `out` is touched
    if (!mat || !lo || !hi || !out) return set_error("gpupoly_matrix_extract_bits: null argument");
    if (words_per_bound == 0) return set_error("gpupoly_matrix_extract_bits: words_per_bound must be at least 1");
    GpuContext *ctx = mat->ctx;
    const int L = mat->level + 1;
    ReadoutConsts rc;
    init_consts(rc, ctx, L);
    readout::BoundDigits blo, bhi;
    if (readout::bound_digits(lo, words_per_bound, rc.q, L, &blo))
        return set_error("gpupoly_matrix_extract_bits: lo lies above the level's modulus");
    if (readout::bound_digits(hi, words_per_bound, rc.q, L, &bhi))
        return set_error("gpupoly_matrix_extract_bits: hi lies above the level's modulus");
    const size_t N = static_cast<size_t>(ctx->N);
    const size_t min_bytes = (N + 7) / 8;
    if (bytes_per_poly < min_bytes)
        return set_error("gpupoly_matrix_extract_bits: bytes_per_poly is below the " + std::to_string(min_bytes) +
                         " bytes the ring dimension needs");
    const size_t polys = matrix_polys(mat);
    if (polys == 0) return 0;
    set_bound(rc, 0, blo);
    set_bound(rc, 1, bhi);
    rc.wrap = readout::compare_words(lo, words_per_bound, hi, words_per_bound) > 0;
    if (ctx_activate(ctx)) return 1;

    CtxBlock scratch(ctx), dev_out(ctx);
    const void *src = nullptr;
    if (const int st = coeff_domain_source(mat, scratch, &src)) return st;
    const size_t total = polys * N;
    // N >= 8: ceil(total / 64) ballot words, of which polys * N / 8 bytes are the output; N < 8: one byte per entry
    const size_t dense_bytes = polys * min_bytes;
    const size_t dev_bytes = (std::max(dense_bytes, (total + 7) / 8) + 7) / 8 * 8;
    if (dev_out.alloc(dev_bytes)) return 1;
    const dim3 grid = item_grid(total, kReadoutThreads);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    uint64_t *const d_words = static_cast<uint64_t *>(dev_out.ptr);
    const uint32_t n32 = static_cast<uint32_t>(N);
    MXX_TRACE_BYTES(static_cast<double>(matrix_words(mat) * ctx->word_bytes + dense_bytes));
    if (ctx->wide)
        READOUT_BY_LIMBS(extract_bits_kernel, uint64_t, L, static_cast<const uint64_t *>(src), polys, n32, rc, ctx->d_garner, gstride,
                         ctx->d_limbs, d_words);
    else
        READOUT_BY_LIMBS(extract_bits_kernel, uint32_t, L, static_cast<const uint32_t *>(src), polys, n32, rc, ctx->d_garner, gstride,
                         ctx->d_limbs, d_words);
    HIP_TRY(hipGetLastError());
    if (bytes_per_poly == min_bytes) {
        HIP_TRY(hipMemcpyAsync(out, dev_out.ptr, dense_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    } else {  // padded slots: the dense bytes through a host buffer, the padding written as zero
        std::vector<uint8_t> dense(dense_bytes);
        HIP_TRY(hipMemcpyAsync(dense.data(), dev_out.ptr, dense_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t p = 0; p < polys; ++p) {
            std::memcpy(out + p * bytes_per_poly, dense.data() + p * min_bytes, min_bytes);
            std::memset(out + p * bytes_per_poly + min_bytes, 0, bytes_per_poly - min_bytes);
        }
    }
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_store_coeff_ints(const GpuMatrix *mat, void *out, int elem_bytes, int centred, size_t coeffs_per_poly,
                                               uint64_t *out_misfit_count, uint64_t *out_first_misfit) {
    ABI_GUARD_BEGIN
    // every refusal comes before the first launch and before `out` or a counter is touched
    if (!mat || !out || !out_misfit_count || !out_first_misfit) return set_error("gpupoly_matrix_store_coeff_ints: null argument");
    if (elem_bytes != 4 && elem_bytes != 8) return set_error("gpupoly_matrix_store_coeff_ints: elem_bytes must be 4 or 8");
    GpuContext *ctx = mat->ctx;
    const size_t N = static_cast<size_t>(ctx->N);
    if (coeffs_per_poly > N) return set_error("gpupoly_matrix_store_coeff_ints: coeffs_per_poly exceeds the ring dimension");
    const size_t polys = matrix_polys(mat);
    *out_misfit_count = 0;
    *out_first_misfit = UINT64_MAX;
    if (polys == 0 || coeffs_per_poly == 0) return 0;
    const int L = mat->level + 1;
    ReadoutConsts rc;
    init_consts(rc, ctx, L);
    rc.centred = centred != 0;
    rc.elem_bytes = elem_bytes;
    const unsigned bits = 8u * static_cast<unsigned>(elem_bytes);
    if (rc.centred) {
        set_bound(rc, 0, readout::power_of_two_bound(bits - 1, rc.q, L));
        set_bound(rc, 1, readout::q_minus_power_of_two_bound(bits - 1, rc.q, L));
        set_bound(rc, 2, readout::half_plus_one_bound(rc.q, L));
    } else {
        set_bound(rc, 0, readout::power_of_two_bound(bits, rc.q, L));
    }
    if (ctx_activate(ctx)) return 1;

    CtxBlock scratch(ctx), dev_out(ctx), dev_stats(ctx);
    const void *src = nullptr;
    if (const int st = coeff_domain_source(mat, scratch, &src)) return st;
    const size_t total = polys * coeffs_per_poly;
    const size_t out_bytes = total * static_cast<size_t>(elem_bytes);
    if (dev_out.alloc(out_bytes)) return 1;
    if (dev_stats.alloc(2 * sizeof(uint64_t))) return 1;
    uint64_t stats[2] = {0, UINT64_MAX};
    HIP_TRY(hipMemcpyAsync(dev_stats.ptr, stats, sizeof(stats), hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid = item_grid(total, kReadoutThreads);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    unsigned long long *const d_stats = static_cast<unsigned long long *>(dev_stats.ptr);
    const uint32_t n32 = static_cast<uint32_t>(N), cpp = static_cast<uint32_t>(coeffs_per_poly);
    MXX_TRACE_BYTES(static_cast<double>(polys * static_cast<size_t>(L) * coeffs_per_poly * ctx->word_bytes + out_bytes));
    if (ctx->wide)
        READOUT_BY_LIMBS(coeff_ints_kernel, uint64_t, L, static_cast<const uint64_t *>(src), polys, n32, cpp, rc, ctx->d_garner,
                         gstride, ctx->d_limbs, dev_out.ptr, d_stats);
    else
        READOUT_BY_LIMBS(coeff_ints_kernel, uint32_t, L, static_cast<const uint32_t *>(src), polys, n32, cpp, rc, ctx->d_garner,
                         gstride, ctx->d_limbs, dev_out.ptr, d_stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dev_out.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(stats, dev_stats.ptr, sizeof(stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out_misfit_count = stats[0];
    *out_first_misfit = stats[1];
    return 0;
    ABI_GUARD_END
}
