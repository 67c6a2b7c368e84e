// monomial.hip — products by monomials x^s and sums of such products, on the data as it lies (extension).
//
//   gpupoly_matrix_fill_monomial   every entry of out = x^shift, written directly in COEFF or EVAL form
//   gpupoly_matrix_mul_monomial    out = in * x^shift
//   gpupoly_matrix_monomial_sum    out = addend +- sum_j mats[j] * x^shifts[j]
//
// Replaces the per-term host loop of the reference's slot-packing steps - collapse_slot_matrices
// (src/noise_refresh/naive_vec.rs:1983-1998), the slot-transfer reduce step (src/slot_transfer/bgg_poly_encoding.rs:362-380),
// the target of slot_reduce (src/slot_transfer/bgg_pubkey_gpu.rs:448-464) and rotate_gate / monomial_scalar
// (src/circuit/poly_circuit/construction.rs:352-357) -, which builds a one-hot vector on the host, uploads and transforms
// it (const_rotate_poly, src/poly/mod.rs:151-156, even goes through a host CRT), then gpu_matrix_mul_scalar and
// gpu_matrix_add: three launches, one upload and five passes over a matrix per term.
//
// Shifts are taken mod 2N (x^N = -1).
//   EVAL   slot k of limb l holds a(psi_l^(2 bitrev(k) + 1)), so the product by x^s is the point-wise product by psi_l^e,
//          e = s (2 bitrev(k) + 1) mod 2N.  The forward twiddle table holds it: d_tw_fwd[l][bitrev(e mod N)] = psi_l^(e mod N),
//          negated when e >= N.  A gather into N words per limb (L2-resident), paid once per (slot, term) for a tile of
//          polynomials.  Raw products are accumulated lazily (64-bit sums for 32-bit words, 128-bit for 64-bit words) and
//          folded after LimbConst::lazy_terms of them.
//   COEFF  a signed rotation: coefficient i receives +a[m] when m = (i - s) mod 2N < N, else -a[m - N].  No products.
// Up to kMonoMax terms per launch, operand pointers and reduced shifts by value in the kernel arguments; later groups of a
// call read `out` as their addend.  Every output word is produced by the one thread that reads the addend word at the same
// place: out == addend accumulates in place.
#include "common.h"
#include "modarith.h"
#include "monomial_factor.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace {

constexpr size_t kMonoMax = 64;

struct MonoArgs {
    const void *mat[kMonoMax];
    uint32_t shift[kMonoMax];  // reduced mod 2N
};

// bitrev_n and monomial_factor - psi^(s * odd) of one limb through the forward twiddle table - stand in monomial_factor.h

template <typename W, int SV>
struct VecOf {
    typedef typename std::conditional<sizeof(W) * SV == 16, uint4, W>::type type;
};

template <typename W>
__device__ __forceinline__ W fold_sum(typename Wide<W>::type acc, const LimbConst &lc) {
    if constexpr (sizeof(W) == 4) return reduce_u64_sum(acc, static_cast<uint32_t>(lc.q), lc.mu64);
    else return reduce_u128_sum(acc, lc.q, lc.mu, lc.kbits, lc.mu64);
}

// addend +- sum, the store's last step
template <typename W>
__device__ __forceinline__ W combine(bool has_add, W add, W sum, bool negate, W q) {
    if (has_add) return negate ? sub_mod<W>(add, sum, q) : add_mod<W>(add, sum, q);
    return negate ? (sum ? static_cast<W>(q - sum) : static_cast<W>(0)) : sum;
}

// EVAL: grid x = polynomial tile * slot_blocks + slot block, z = limb; a thread owns SV consecutive slots of PT polynomials of one limb.
// KU terms' operands are loaded before any is multiplied (small rings are a serial chain of load latencies otherwise).
template <typename W, int SV, int PT, int KU>
__global__ void __launch_bounds__(256)
    monomial_sum_eval_kernel(W *__restrict__ out, const W *addend, MonoArgs args, uint32_t terms, const W *__restrict__ tw,
                             const LimbConst *__restrict__ limbs, uint32_t polys, uint32_t L, uint32_t N, uint32_t logN,
                             uint32_t slot_blocks, int negate) {
    typedef typename Wide<W>::type D;
    typedef typename VecOf<W, SV>::type VT;
    const uint32_t tile_id = blockIdx.x / slot_blocks, sb = blockIdx.x - tile_id * slot_blocks;
    const uint32_t k0 = (sb * blockDim.x + threadIdx.x) * SV;
    if (k0 >= N) return;
    const uint32_t limb = blockIdx.z, p0 = tile_id * PT;
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    const W *twl = tw + static_cast<size_t>(limb) * N;
    const size_t polyw = static_cast<size_t>(L) * N;
    size_t off[PT];  // a tile row past the last polynomial re-reads the last one and is never stored
#pragma unroll
    for (int p = 0; p < PT; ++p) off[p] = static_cast<size_t>(min(p0 + p, polys - 1)) * polyw + static_cast<size_t>(limb) * N + k0;
    uint32_t odd[SV];
#pragma unroll
    for (int s = 0; s < SV; ++s) odd[s] = 2u * bitrev_n(k0 + s, logN) + 1u;

    W add[PT][SV];
    if (addend) {
#pragma unroll
        for (int p = 0; p < PT; ++p) *reinterpret_cast<VT *>(add[p]) = *reinterpret_cast<const VT *>(addend + off[p]);
    }
    D acc[PT][SV];
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int s = 0; s < SV; ++s) acc[p][s] = 0;
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
    for (uint32_t j0 = 0; j0 < terms; j0 += KU) {
        W a[KU][PT][SV], f[KU][SV];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t j = min(j0 + u, terms - 1);  // the tail re-reads the last term and is not accumulated
            const W *m = static_cast<const W *>(args.mat[j]);
            const uint32_t sh = args.shift[j];
#pragma unroll
            for (int p = 0; p < PT; ++p) *reinterpret_cast<VT *>(a[u][p]) = *reinterpret_cast<const VT *>(m + off[p]);
#pragma unroll
            for (int s = 0; s < SV; ++s) f[u][s] = monomial_factor<W>(twl, sh, odd[s], N, logN, q);
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            if (KU > 1 && j0 + u >= terms) break;
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int s = 0; s < SV; ++s) acc[p][s] += static_cast<D>(a[u][p][s]) * f[u][s];
            if (++pending == lazy) {
                pending = 0;
#pragma unroll
                for (int p = 0; p < PT; ++p)
#pragma unroll
                    for (int s = 0; s < SV; ++s) acc[p][s] = fold_sum<W>(acc[p][s], lc);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if (p0 + p >= polys) continue;
        W o[SV];
#pragma unroll
        for (int s = 0; s < SV; ++s) o[s] = combine<W>(addend != nullptr, add[p][s], fold_sum<W>(acc[p][s], lc), negate != 0, q);
        *reinterpret_cast<VT *>(out + off[p]) = *reinterpret_cast<const VT *>(o);
    }
}

// COEFF: one thread per SV consecutive coefficients of one (polynomial, limb).  SV > 1 only when every shift of the launch
// is a multiple of SV: the rotated read is then an aligned 16-byte load whose elements share one sign (N % SV == 0).
// Otherwise SV = 1: lanes read consecutive words from an arbitrary start, coalesced whatever the shift.
template <typename W, int SV, int KU>
__global__ void __launch_bounds__(256)
    monomial_sum_coeff_kernel(W *__restrict__ out, const W *addend, MonoArgs args, uint32_t terms,
                              const LimbConst *__restrict__ limbs, size_t total_vecs, uint32_t L, uint32_t N, uint32_t logN,
                              int negate) {
    typedef typename VecOf<W, SV>::type VT;
    const size_t v = item_index();
    if (v >= total_vecs) return;
    const size_t w0 = v * SV;
    const uint32_t i0 = static_cast<uint32_t>(w0 & (N - 1u));
    const size_t base = w0 - i0;  // first word of this (polynomial, limb)
    const W q = static_cast<W>(limbs[(w0 >> logN) % L].q);
    W add[SV];
    if (addend) *reinterpret_cast<VT *>(add) = *reinterpret_cast<const VT *>(addend + w0);
    W acc[SV];
#pragma unroll
    for (int s = 0; s < SV; ++s) acc[s] = 0;
    for (uint32_t j0 = 0; j0 < terms; j0 += KU) {
        W a[KU][SV];
        bool neg[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t j = min(j0 + u, terms - 1);
            const uint32_t m = (i0 - args.shift[j]) & (2u * N - 1u);
            neg[u] = (m & N) != 0;
            *reinterpret_cast<VT *>(a[u]) = *reinterpret_cast<const VT *>(static_cast<const W *>(args.mat[j]) + base + (m & (N - 1u)));
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            if (KU > 1 && j0 + u >= terms) break;
#pragma unroll
            for (int s = 0; s < SV; ++s) acc[s] = neg[u] ? sub_mod<W>(acc[s], a[u][s], q) : add_mod<W>(acc[s], a[u][s], q);
        }
    }
    W o[SV];
#pragma unroll
    for (int s = 0; s < SV; ++s) o[s] = combine<W>(addend != nullptr, add[s], acc[s], negate != 0, q);
    *reinterpret_cast<VT *>(out + w0) = *reinterpret_cast<const VT *>(o);
}

// every polynomial of out = x^s: COEFF a one-hot vector of +1 or -1 (q - 1), EVAL the factor vector
template <typename W>
__global__ void __launch_bounds__(256)
    fill_monomial_kernel(W *__restrict__ out, size_t words, uint32_t s, int eval, const W *__restrict__ tw,
                         const LimbConst *__restrict__ limbs, uint32_t L, uint32_t N, uint32_t logN) {
    const size_t w = item_index();
    if (w >= words) return;
    const uint32_t k = static_cast<uint32_t>(w & (N - 1u)), limb = static_cast<uint32_t>((w >> logN) % L);
    const W q = static_cast<W>(limbs[limb].q);
    if (eval) {
        out[w] = monomial_factor<W>(tw + static_cast<size_t>(limb) * N, s, 2u * bitrev_n(k, logN) + 1u, N, logN, q);
    } else {
        const W one = (s & N) ? static_cast<W>(q - 1) : static_cast<W>(1);
        out[w] = k == (s & (N - 1u)) ? one : static_cast<W>(0);
    }
}

template <typename W>
int launch_group(GpuMatrix *out, W *o, const W *addend, const MonoArgs &args, uint32_t terms, int format, int negate) {
    GpuContext *ctx = out->ctx;
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(out)), N = static_cast<uint32_t>(ctx->N), logN = ctx->logN;
    const size_t polys = matrix_polys(out), words = matrix_words(out);
    constexpr int VN = 16 / sizeof(W);
    // each operand read once, the addend read once, the output written once
    MXX_TRACE_BYTES(static_cast<double>(words) * sizeof(W) * (terms + 1 + (addend ? 1 : 0)));
    if (format == GPU_POLY_FORMAT_EVAL) {
        const W *tw = static_cast<const W *>(ctx->d_tw_fwd);
        const bool vec = N >= static_cast<uint32_t>(VN);
        const uint32_t lanes = vec ? N / VN : N;
        // a tile of 4 polynomials shares one factor look-up; taken once the tiled grid still fills the chip (two waves on
        // every SIMD), else one polynomial per thread
        // (64-bit words without a 16-byte vector would be N = 1: never tiled)
        const bool tile = polys >= 4 && (vec || sizeof(W) == 4) && static_cast<uint64_t>(lanes) * L * ((polys + 3) / 4) >= 1024ull * 2 * 64;
        const uint32_t threads = std::min<uint32_t>(256, std::max<uint32_t>(64, lanes));
        const size_t tiles = tile ? (polys + 3) / 4 : polys;
        const uint32_t slot_blocks = (lanes + threads - 1) / threads;
        const dim3 grid(static_cast<unsigned>(slot_blocks * tiles), 1, L);  // below 2^31: checked with the refusals
#define MONO_EVAL(SV, PT, KU)                                                                                            \
    MXX_LAUNCH((monomial_sum_eval_kernel<W, SV, PT, KU>), grid, dim3(threads), 0, ctx->stream, o, addend, args, terms, tw, \
               ctx->d_limbs, static_cast<uint32_t>(polys), L, N, logN, slot_blocks, negate)
        if (vec) {
            if (tile) MONO_EVAL(VN, 4, 1);
            else MONO_EVAL(VN, 1, 4);
        } else {
            if constexpr (sizeof(W) == 4) {
                if (tile) MONO_EVAL(1, 4, 1);
                else MONO_EVAL(1, 1, 4);
            } else {
                MONO_EVAL(1, 1, 4);
            }
        }
#undef MONO_EVAL
    } else {
        bool vec = N >= static_cast<uint32_t>(VN);
        for (uint32_t j = 0; j < terms && vec; ++j) vec = args.shift[j] % VN == 0;
        const size_t vecs = vec ? words / VN : words;
        if (vec)
            MXX_LAUNCH((monomial_sum_coeff_kernel<W, VN, 2>), item_grid(vecs, 256), dim3(256), 0, ctx->stream, o, addend, args,
                       terms, ctx->d_limbs, vecs, L, N, logN, negate);
        else
            MXX_LAUNCH((monomial_sum_coeff_kernel<W, 1, 4>), item_grid(vecs, 256), dim3(256), 0, ctx->stream, o, addend, args,
                       terms, ctx->d_limbs, vecs, L, N, logN, negate);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int monomial_sum_impl(const char *who, GpuMatrix *out, const GpuMatrix *addend, const GpuMatrix *const *mats,
                      const uint64_t *shifts, size_t n, int negate) {
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    // ---- every refusal, for every j, before the first launch ----
    if (!out) return refuse("null output");
    if (n > 0 && (!mats || !shifts)) return refuse("null array");
    GpuContext *ctx = out->ctx;
    for (size_t j = 0; j < n; ++j)
        if (!mats[j]) return refuse("null matrix (term " + std::to_string(j) + ")");
    const GpuMatrix *first = addend ? addend : (n ? mats[0] : nullptr);  // the operand whose format all share
    auto check = [&](const GpuMatrix *m, const std::string &at) -> int {
        if (m->ctx != ctx) return refuse("context mismatch" + at);
        if (m->level != out->level) return refuse("level mismatch" + at);
        if (m->rows != out->rows || m->cols != out->cols) return refuse("shape mismatch" + at);
        if (m->format != first->format) return refuse("operands must share a format" + at);
        return 0;
    };
    if (addend) {
        if (check(addend, " (addend)")) return 1;
        // in place means the same words: a shifted overlap (a row view of out's parent) would be read after it is written
        if (addend != out && storage_overlaps(out, addend) && (addend->storage != out->storage || addend->bytes != out->bytes))
            return refuse("the addend overlaps the output without being the same block");
    }
    for (size_t j = 0; j < n; ++j) {
        const std::string at = " (term " + std::to_string(j) + ")";
        if (check(mats[j], at)) return 1;
        if (storage_overlaps(out, mats[j])) return refuse("the output overlaps an operand" + at);
    }
    if (first && first->format != GPU_POLY_FORMAT_COEFF && first->format != GPU_POLY_FORMAT_EVAL) return refuse("unknown format");
    // the EVAL grid numbers (slot block, polynomial tile) pairs along x
    if (matrix_polys(out) * ((static_cast<size_t>(ctx->N) + 63) / 64) > 0x7fffffffull) return refuse("matrix too large");

    if (first) out->format = first->format;  // n = 0 without an addend leaves the tag as it was
    if (matrix_polys(out) == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    if (n == 0) {
        if (!addend) {
            HIP_TRY(hipMemsetAsync(words_ptr(out), 0, out->bytes, ctx->stream));
        } else if (words_ptr(addend) != words_ptr(out)) {
            MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * out->bytes,
                            HIP_TRY(hipMemcpyAsync(words_ptr(out), words_ptr(addend), out->bytes, hipMemcpyDeviceToDevice, ctx->stream)));
        }
        return 0;
    }
    // PACKED24 operands are unpacked here, all of them before the first launch of the sum
    void *const o = words_ptr(out);
    const void *add = addend ? words_ptr(addend) : nullptr;
    std::vector<const void *> ptrs(n);
    for (size_t j = 0; j < n; ++j) ptrs[j] = words_ptr(mats[j]);
    const uint64_t mask = 2ull * static_cast<uint64_t>(ctx->N) - 1ull;
    for (size_t j0 = 0; j0 < n; j0 += kMonoMax) {
        MonoArgs args;
        const uint32_t terms = static_cast<uint32_t>(std::min(kMonoMax, n - j0));
        for (uint32_t t = 0; t < kMonoMax; ++t) {
            args.mat[t] = ptrs[j0 + std::min(t, terms - 1)];
            args.shift[t] = static_cast<uint32_t>(shifts[j0 + std::min(t, terms - 1)] & mask);
        }
        const int rc = ctx->wide ? launch_group<uint64_t>(out, static_cast<uint64_t *>(o), static_cast<const uint64_t *>(add), args,
                                                          terms, first->format, negate)
                                 : launch_group<uint32_t>(out, static_cast<uint32_t *>(o), static_cast<const uint32_t *>(add), args,
                                                          terms, first->format, negate);
        if (rc) return rc;
        add = o;  // later groups accumulate onto what the earlier ones wrote
    }
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_monomial_sum(GpuMatrix *out, const GpuMatrix *addend, const GpuMatrix *const *mats,
                                           const uint64_t *shifts, size_t n, int negate) {
    ABI_GUARD_BEGIN
    return monomial_sum_impl("gpupoly_matrix_monomial_sum", out, addend, mats, shifts, n, negate);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_mul_monomial(GpuMatrix *out, const GpuMatrix *in, uint64_t shift) {
    ABI_GUARD_BEGIN
    if (!out || !in) return set_error("gpupoly_matrix_mul_monomial: null matrix");
    return monomial_sum_impl("gpupoly_matrix_mul_monomial", out, nullptr, &in, &shift, 1, 0);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_fill_monomial(GpuMatrix *out, uint64_t shift, int format) {
    ABI_GUARD_BEGIN
    if (!out) return set_error("gpupoly_matrix_fill_monomial: null matrix");
    if (format != GPU_POLY_FORMAT_COEFF && format != GPU_POLY_FORMAT_EVAL)
        return set_error("gpupoly_matrix_fill_monomial: format must be GPU_POLY_FORMAT_COEFF or GPU_POLY_FORMAT_EVAL");
    GpuContext *ctx = out->ctx;
    out->format = format;
    const size_t words = matrix_words(out);
    if (words == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(out)), N = static_cast<uint32_t>(ctx->N);
    const uint32_t s = static_cast<uint32_t>(shift & (2ull * N - 1ull));
    MXX_TRACE_BYTES(static_cast<double>(out->bytes));
    if (ctx->wide)
        MXX_LAUNCH(fill_monomial_kernel<uint64_t>, item_grid(words, 256), dim3(256), 0, ctx->stream, static_cast<uint64_t *>(words_ptr(out)),
                   words, s, format == GPU_POLY_FORMAT_EVAL ? 1 : 0, static_cast<const uint64_t *>(ctx->d_tw_fwd), ctx->d_limbs, L, N, ctx->logN);
    else
        MXX_LAUNCH(fill_monomial_kernel<uint32_t>, item_grid(words, 256), dim3(256), 0, ctx->stream, static_cast<uint32_t *>(words_ptr(out)),
                   words, s, format == GPU_POLY_FORMAT_EVAL ? 1 : 0, static_cast<const uint32_t *>(ctx->d_tw_fwd), ctx->d_limbs, L, N, ctx->logN);
    HIP_TRY(hipGetLastError());
    return 0;
    ABI_GUARD_END
}
