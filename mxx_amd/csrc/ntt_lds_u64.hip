// ntt_lds_u64.hip — the transforms' entry points for 64-bit residue words: the integer launchers of ntt_rings.h and, for
// moduli below 2^51, the double-precision transforms (ntt_f64.h) over the same ring table.
#include "ntt_rings.h"
#include "ntt_f64.h"

using W = uint64_t;

// ---- moduli below 2^51: the double-precision transforms ------------------------------------------------------------------
static bool f64_transforms(const GpuContext *ctx) { return ctx->f64_ok && !ctx->env.ntt64_int && ctx->env.ntt_path <= 1; }

// f(std::integral_constant<int, ELIM>{}).  ELIM: the largest bound (units of q / 4) a value may reach: |x| < 2^53 means
// < 4 q at 51 bits, < 16 q below 2^49, and below 2^40 no stage of a pass ever needs a fold
template <typename F>
static int by_elim(const GpuContext *ctx, F &&f) {
    return ctx->crt_bits <= 40   ? f(std::integral_constant<int, 4095>{})
           : ctx->crt_bits <= 49 ? f(std::integral_constant<int, 63>{})
                                 : f(std::integral_constant<int, 15>{});
}

static const TwF *twf_fwd(const GpuContext *ctx) { return static_cast<const TwF *>(ctx->d_twf_fwd); }
static const TwF *twf_inv(const GpuContext *ctx) { return static_cast<const TwF *>(ctx->d_twf_inv); }
static const F64Limb *flimbs(const GpuContext *ctx) { return static_cast<const F64Limb *>(ctx->d_flimbs); }

template <typename R, int ELIM>
static int launch_f64(GpuContext *ctx, uint64_t *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = R::template lds<double>();
    const bool nt = (vectors << R::LOGN) * sizeof(uint64_t) >= (size_t(1) << 30);  // as launch_lazy: batches no cache holds
    if (int rc = lds_opt_in<nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false>, nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, true>,
                            nttf::inv_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false>,
                            nttf::inv_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, true>>(ctx, lds))
        return rc;
    const dim3 grid(static_cast<unsigned>(vectors));
    return bool_dispatch(inverse, nt, [&](auto INV, auto NT) {
        if constexpr (!INV())
            MXX_LAUNCH((nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, NT()>), grid, R::block(), lds, ctx->stream, data, twf_fwd(ctx),
                       flimbs(ctx), L);
        else
            MXX_LAUNCH((nttf::inv_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, NT()>), grid, R::block(), lds, ctx->stream, data, twf_inv(ctx),
                       flimbs(ctx), L);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// 2^(LOGN + PRE) points: head / tail kernel on the strided sets + the LDS kernels on the 2^PRE sub-vectors (folded doubles
// travel between the two launches in the vector's own 8-byte slots)
template <typename R, int ELIM>
static int launch_f64_split(GpuContext *ctx, uint64_t *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = R::template lds<double>();
    if (!R::fits(vectors)) return -1;
    if (int rc = lds_opt_in<nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>,
                            nttf::inv_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>>(ctx, lds))
        return rc;
    const uint32_t logN = R::RING;
    const dim3 sub_grid = R::sub_grid(vectors), set_grid(static_cast<unsigned>(vectors * R::set_blocks)), set_block(256);
    if (!inverse) {
        MXX_LAUNCH((nttf::head_kernel<R::PRE, ELIM, false, false, false>), set_grid, set_block, 0, ctx->stream, data, data, twf_fwd(ctx),
                   flimbs(ctx), ctx->d_limbs, L, logN, 0u, 0u, 0u, 0u, 0u);
        MXX_LAUNCH((nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>), sub_grid, R::block(), lds, ctx->stream, data,
                   twf_fwd(ctx), flimbs(ctx), L);
    } else {
        MXX_LAUNCH((nttf::inv_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>), sub_grid, R::block(), lds, ctx->stream, data,
                   twf_inv(ctx), flimbs(ctx), L);
        MXX_LAUNCH((nttf::tail_kernel<R::PRE, ELIM>), set_grid, set_block, 0, ctx->stream, data, twf_inv(ctx), flimbs(ctx), L, logN);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// rings below 2^10 points with moduli below 2^51: the double-precision form of the generic one-stage-per-barrier kernel
static int launch_f64_small(GpuContext *ctx, uint64_t *data, size_t vectors, uint32_t L, bool inverse) {
    const uint32_t logN = ctx->logN;
    const size_t N = size_t(1) << logN;
    unsigned threads = static_cast<unsigned>(N / 2);
    if (threads < 64) threads = 64;
    if (threads > 512) threads = 512;
    const dim3 grid(static_cast<unsigned>(vectors)), block(threads);
    const size_t lds = N * sizeof(double);
    if (!inverse) MXX_LAUNCH((nttf::small_kernel<false>), grid, block, lds, ctx->stream, data, twf_fwd(ctx), flimbs(ctx), L, logN);
    else MXX_LAUNCH((nttf::small_kernel<true>), grid, block, lds, ctx->stream, data, twf_inv(ctx), flimbs(ctx), L, logN);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ntt_lds_u64(GpuContext *ctx, uint64_t *data, size_t vectors, uint32_t L, bool inverse) {
    if (f64_transforms(ctx) && vectors <= 0x7fffffffull) {
        // the small-ring kernel first: the launch-bound M4 chain runs here
        if (ctx->logN >= 1 && ctx->logN < 10) return launch_f64_small(ctx, data, vectors, L, inverse);
        const int rc = by_elim(ctx, [&](auto elim) {
            constexpr int ELIM = decltype(elim)::value;
            return visit_ring<W>(ctx->logN, [&](auto ring) {
                using R = decltype(ring);
                if constexpr (R::PRE > 0) return launch_f64_split<R, ELIM>(ctx, data, vectors, L, inverse);
                else return launch_f64<R, ELIM>(ctx, data, vectors, L, inverse);
            });
        });
        if (rc >= 0) return rc;
    }
    return launch_ntt_lds<W>(ctx, data, vectors, L, inverse);
}

// ---- decompose + forward transform in one pass (DigitLaunch, ntt_rings.h) -------------------------------------------------
template <typename R, int ELIM>
static int launch_f64_digits(GpuContext *ctx, const DigitLaunch<W> &d) {
    const size_t lds = R::template lds<double>();
    if (int rc = lds_opt_in<nttf::fwd_digits_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, false>,
                            nttf::fwd_digits_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, true>,
                            nttf::fwd_digits_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, true, false>,
                            nttf::fwd_digits_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, true, true>>(ctx, lds))
        return rc;
    return bool_dispatch(d.reduce, d.nts, [&](auto RED, auto NTS) {
        MXX_LAUNCH((nttf::fwd_digits_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, RED(), NTS()>), d.grid(), R::block(), lds, ctx->stream, d.out,
                   d.coeff, twf_fwd(ctx), flimbs(ctx), ctx->d_limbs, d.L, d.src_cols, d.dpt, d.base_bits, d.k, d.td0);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// the split sizes: head kernel with the digits in its load, then the sub-vectors
template <typename R, int ELIM>
static int launch_f64_split_digits(GpuContext *ctx, const DigitLaunch<W> &d) {
    const size_t lds = R::template lds<double>();
    if (!R::fits(d.vectors) || static_cast<uint64_t>(R::set_blocks) * d.L * d.src_cols > 0x7fffffffull) return -1;
    if (int rc = lds_opt_in<nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>>(ctx, lds)) return rc;
    const uint32_t logN = R::RING;
    return bool_dispatch(d.reduce, d.nts, [&](auto RED, auto NTS) {
        MXX_LAUNCH((nttf::head_kernel<R::PRE, ELIM, true, RED(), NTS()>), d.grid(R::set_blocks), dim3(256), 0, ctx->stream, d.out, d.coeff,
                   twf_fwd(ctx), flimbs(ctx), ctx->d_limbs, d.L, logN, d.src_cols, d.dpt, d.base_bits, d.k, d.td0);
        MXX_LAUNCH((nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, false, R::PRE>), R::sub_grid(d.vectors), R::block(), lds, ctx->stream,
                   d.out, twf_fwd(ctx), flimbs(ctx), d.L);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// -1: not available (see launch_ntt_digits_u32)
int launch_ntt_digits_u64(GpuContext *ctx, uint64_t *out, const uint64_t *coeff, size_t out_vectors, uint32_t L,
                          uint32_t src_cols, uint32_t towers, uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0) {
    DigitLaunch<W> d{out, coeff, L, src_cols, towers, dpt, base_bits, 0, td0};
    if (!ctx->lazy_ok || !d.plan(ctx, out_vectors, k)) return -1;
    if (f64_transforms(ctx)) {
        const int rc = by_elim(ctx, [&](auto elim) {
            constexpr int ELIM = decltype(elim)::value;
            return visit_ring<W>(ctx->logN, [&](auto ring) {
                using R = decltype(ring);
                if constexpr (R::PRE > 0) return launch_f64_split_digits<R, ELIM>(ctx, d);
                else return launch_f64_digits<R, ELIM>(ctx, d);
            });
        });
        if (rc >= 0) return rc;
    }
    return launch_ntt_digits<W>(ctx, d);
}
