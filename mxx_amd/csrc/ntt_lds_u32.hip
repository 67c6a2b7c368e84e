// ntt_lds_u32.hip — the transforms' entry points for 32-bit residue words (ring shapes and shared launchers: ntt_rings.h).
#include "ntt_rings.h"

using W = uint32_t;

int launch_ntt_lds_u32(GpuContext *ctx, uint32_t *data, size_t vectors, uint32_t L, bool inverse) {
    return launch_ntt_lds<W>(ctx, data, vectors, L, inverse);
}

// Instantiated, never launched.  launch_ntt14 has always sent the signed grouped inverse off before it looked at the batch
// size, so this non-temporal instance was never selected.  Whether it should be is a measurement at 1 GiB for a change of
// its own; until then the library keeps the instance, and the selection it had.
template __global__ void ntt14::inv_kernel<W, true, false, 31, 8, true>(W *, const TwPair<W> *, const LimbConst *, uint32_t, const W *,
                                                                        const W *);

// ---- out <- INTT(in o w) in one pass over the data (gpupoly_matrix_mul_scalar_intt) -------------------------------------
// w is used as it stands (EVAL residues): the kernels' product is a Montgomery one and ctx->d_limbs_r carries the
// compensating 2^32 in the N^-1 constants of whichever kernel runs the last stage.  32-bit words only.
template <typename R, bool TIGHT>
static int launch_lazy_mulw(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes) return -1;
    if (int rc = lds_opt_in<ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, false, true>>(ctx, lds)) return rc;
    MXX_LAUNCH((ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, false, true>), dim3(static_cast<unsigned>(vectors)), R::block(),
               lds, ctx->stream, out, tw_inv<W>(ctx), ctx->d_limbs_r, L, in, w);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename R, bool TIGHT>
static int launch_split_mulw(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes || !R::fits(vectors)) return -1;
    if (int rc = lds_opt_in<ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT, false, true>>(ctx, lds)) return rc;
    const uint32_t logN = R::RING;
    // sub-vectors with the product in their load (their own constants are the plain ones: N^-1 is the tail's business)
    MXX_LAUNCH((ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT, false, true>), R::sub_grid(vectors), R::block(), lds,
               ctx->stream, out, tw_inv<W>(ctx), ctx->d_limbs, L, in, w);
    MXX_LAUNCH((ntt_inv_tail_kernel<W, R::PRE, TIGHT>), dim3(static_cast<unsigned>(vectors * R::set_blocks)), dim3(256), 0, ctx->stream, out,
               tw_inv<W>(ctx), ctx->d_limbs_r, L, logN);
    HIP_TRY(hipGetLastError());
    return 0;
}

// -1 when no fused kernel covers this context (the caller then runs the point-wise product and the transform separately)
int launch_mul_intt_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, const uint32_t *w, size_t vectors, uint32_t L) {
    if (!(ctx->lazy_ok || ctx->tight_ok) || !ctx->d_limbs_r || ctx->env.ntt_path > 1 || vectors > 0x7fffffffull) return -1;
    MXX_TRACE_BYTES(2.0 * vectors * ctx->N * sizeof(W));  // the resident ring element's L vectors are not counted
    dim3 grid;
    if (ntt14_grouped(ctx, vectors, L, false, true, grid)) {  // lazy moduli only: tight 2^14 takes the whole-vector form below
        // the grouped 2^14 kernel (ntt14.h): next group's operands requested a group ahead
        const dim3 block(ntt14::T);
        const size_t lds = ntt14::lds_bytes(sizeof(W));
        if (ntt14_signed(ctx))
            MXX_LAUNCH((ntt14::inv_kernel<W, true, true>), grid, block, lds, ctx->stream, out,
                       static_cast<const TwPair<W> *>(ctx->d_tw2s_inv), ctx->d_limbs_r, L, in, w);
        else
            MXX_LAUNCH((ntt14::inv_kernel<W, false, true>), grid, block, lds, ctx->stream, out, tw_inv<W>(ctx), ctx->d_limbs_r, L, in, w);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    return by_width_class<W>(ctx, [&](auto tight) {
        constexpr bool TIGHT = decltype(tight)::value;
        return visit_ring<W>(ctx->logN, [&](auto ring) {
            using R = decltype(ring);
            if constexpr (R::PRE > 0) return launch_split_mulw<R, TIGHT>(ctx, out, in, w, vectors, L);
            else return launch_lazy_mulw<R, TIGHT>(ctx, out, in, w, vectors, L);
        });
    });
}

// out = INTT(in), `in` left untouched (ntt14.h, inv_kernel reading from `in`): the decompose paths need the coefficients
// of an EVAL source that must stay EVAL - a device copy followed by the in-place transform moves the matrix three
// times, this moves it twice.  -1: the grouped 2^14 kernel does not run for this context / path override, the caller
// then copies and transforms in place.
int launch_intt_oop_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, size_t vectors, uint32_t L) {
    dim3 grid;
    if (vectors == 0 || !ntt14_grouped(ctx, vectors, L, true, true, grid)) return -1;
    MXX_TRACE_BYTES(2.0 * vectors * ntt14::N * sizeof(W));
    return launch_ntt_lds<W>(ctx, out, vectors, L, true, in);
}

// out = NTT(in) as PACKED24 rows in one pass (ntt14.h, fwd_pack24_kernel; layout.hip); -1: no fused kernel for this
// context / path override, the caller then transforms in place and packs
int launch_ntt_fwd_pack24_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, size_t vectors, uint32_t L) {
    dim3 grid;
    if (vectors == 0 || !ntt14_grouped(ctx, vectors, L, false, false, grid)) return -1;
    const bool nt = (vectors << 14) * sizeof(W) >= (size_t(1) << 30);  // as launch_ntt14
    MXX_TRACE_BYTES(1.75 * vectors * ntt14::N * sizeof(W));  // words read, 3 bytes per residue written
    return bool_dispatch(nt, [&](auto NT) {
        MXX_LAUNCH((ntt14::fwd_pack24_kernel<NT()>), grid, dim3(ntt14::T), ntt14::lds_bytes(sizeof(W)), ctx->stream, out, in, tw_fwd<W>(ctx),
                   ctx->d_limbs, L);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// out = NTT(src) + add in one pass (ntt14.h, fwd_add_kernel); -1: no fused kernel for this context / path override,
// the caller then copies, transforms in place and adds
int launch_ntt_add_u32(GpuContext *ctx, uint32_t *out, const uint32_t *src, const uint32_t *add, size_t vectors, uint32_t L) {
    dim3 grid;
    if (!ntt14_grouped(ctx, vectors, L, true, true, grid)) return -1;
    MXX_TRACE_BYTES(3.0 * vectors * ntt14::N * sizeof(W));  // coefficients + addend read, the sum's transform written
    return bool_dispatch(!ctx->lazy_ok, [&](auto TIGHT) {
        MXX_LAUNCH((ntt14::fwd_add_kernel<W, TIGHT()>), grid, dim3(ntt14::T), ntt14::lds_bytes(sizeof(W)), ctx->stream, out, src, add,
                   tw_fwd<W>(ctx), ctx->d_limbs, L);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// decompose + forward NTT in one pass (DigitLaunch, ntt_rings.h); -1: not available for this context / path override,
// the caller then runs the digit kernel and the transform separately.  2^14 points: ntt14.h, fwd_digits_kernel
int launch_ntt_digits_u32(GpuContext *ctx, uint32_t *out, const uint32_t *coeff, size_t out_vectors, uint32_t L,
                          uint32_t src_cols, uint32_t towers, uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0) {
    DigitLaunch<W> d{out, coeff, L, src_cols, towers, dpt, base_bits, 0, td0};
    // the grouped kernels' switches (MXX_HIP_NTT14=whole among them) rule the fused form at every ring size
    if (!ntt14_switches(ctx, true, true) || !d.plan(ctx, out_vectors, k)) return -1;
    // SURVEY 8d decompose: (r c + r k c) n L w - the source read once, the digit matrix written once
    MXX_TRACE_BYTES((static_cast<double>(d.src_rows) * src_cols * L + static_cast<double>(out_vectors)) * ctx->N * sizeof(W));
    if (ctx->logN != 14) return launch_ntt_digits<W>(ctx, d);
    const dim3 grid(8u * L * ((src_cols + 7u) / 8u), d.k, static_cast<unsigned>(d.src_rows));
    return bool_dispatch(d.reduce, !ctx->lazy_ok, d.nts, [&](auto RED, auto TIGHT, auto NTS) {
        MXX_LAUNCH((ntt14::fwd_digits_kernel<W, RED(), TIGHT(), NTS()>), grid, dim3(ntt14::T), ntt14::lds_bytes(sizeof(W)), ctx->stream, out,
                   coeff, tw_fwd<W>(ctx), ctx->d_limbs, L, src_cols, towers, dpt, base_bits, d.k, td0);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
