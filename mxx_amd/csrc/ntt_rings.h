// ntt_rings.h — host side of the transform kernels (ntt_lds.h, ntt14.h): the table of ring shapes and the launchers of
// the integer kernels, templates on the word type W.  ntt_lds_u32.hip / ntt_lds_u64.hip instantiate them behind the entry
// points of common.h; the double-precision launchers (ntt_lds_u64.hip) walk the same table.
#pragma once
#include "ntt14.h"

#include <algorithm>
#include <type_traits>

static constexpr size_t kLdsLimitBytes = 160 * 1024;

// ---- the ring table -----------------------------------------------------------------------------------------------------
// How a ring of 2^RING points is launched: the LDS kernel holds 2^LOGN points, 2^LOGR per thread, under a bound of WPE
// waves per SIMD (it sits in __launch_bounds__: register allocation follows it).  PRE = 0: the whole vector.  PRE > 0: a
// head / tail kernel runs the PRE outer stages and the LDS kernel the 2^PRE sub-vectors of 2^LOGN points.
template <int LOGN_, int LOGR_, int WPE_, int PRE_ = 0>
struct RingShape {
    static constexpr int LOGN = LOGN_, LOGR = LOGR_, WPE = WPE_, PRE = PRE_, RING = LOGN_ + PRE_;
    template <typename T>  // T: what a point takes in LDS (the word, or a double)
    static size_t lds() { return lds_padded_words(size_t(1) << LOGN) * sizeof(T); }
    static dim3 block() { return dim3(1u << (LOGN - LOGR)); }
    // split forms: one LDS workgroup per sub-vector; the head / tail kernels take 256 strided sets per workgroup
    static bool fits(size_t vectors) { return vectors <= (0x7fffffffull >> PRE); }
    static dim3 sub_grid(size_t vectors) { return dim3(static_cast<unsigned>(vectors << PRE)); }
    static constexpr uint32_t set_blocks = (1u << LOGN) / 256u;  // per vector
};

// The one place that knows a ring's launch shape: f(RingShape<...>{}) for 2^logN points in words of type W (the
// double-precision kernels of 64-bit contexts take the 64-bit column); -1: no tuned transform for this ring.
// Two entries differ by word size, both for LDS capacity (160 KB per workgroup): a padded 2^14-point
// vector is 76 KB in 32-bit words - two workgroups of 8 waves per CU, WPE 4 - and 152 KB in 64-bit words - one, WPE 2;
// a padded 2^15-point vector is 152 KB in 32-bit words and fits whole, in 64-bit words it is 303 KB and must be split.
// The cases stand split forms first, then whole vectors: kernels are instantiated in this order, LLVM inlines in it, and
// the operand order of two additions in nine TIGHT inverse kernels follows (profiles/ntt_dispatch_refactor.txt) - reorder
// only with a byte comparison of the code objects at hand.
template <typename W, typename F>
static int visit_ring(uint32_t logN, F &&f) {
    constexpr bool w32 = sizeof(W) == 4;
    switch (logN) {
        case 16: return f(RingShape<12, 4, 1, 4>{});
        case 17: return f(RingShape<12, 4, 1, 5>{});
        case 10: return f(RingShape<10, 4, 1>{});
        case 11: return f(RingShape<11, 4, 1>{});
        case 12: return f(RingShape<12, 4, 1>{});
        case 13: return f(RingShape<13, 5, 1>{});
        case 14: return f(RingShape<14, 5, w32 ? 4 : 2>{});  // 32-bit words: the grouped kernels of ntt14.h run instead by default
        case 15: return f(std::conditional_t<w32, RingShape<15, 5, 4>, RingShape<11, 4, 1, 4>>{});
        default: return -1;
    }
}

// ---- shared helpers -----------------------------------------------------------------------------------------------------
// f(std::bool_constant<a>{}, ...): runtime bools become template arguments
template <typename F>
static int bool_dispatch(bool a, F &&f) {
    return a ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
static int bool_dispatch(bool a, bool b, F &&f) {
    return bool_dispatch(a, [&](auto A) { return bool_dispatch(b, [&](auto B) { return f(A, B); }); });
}
template <typename F>
static int bool_dispatch(bool a, bool b, bool c, F &&f) {
    return bool_dispatch(a, b, [&](auto A, auto B) { return bool_dispatch(c, [&](auto C) { return f(A, B, C); }); });
}

// f(std::bool_constant<TIGHT>{}): the lazy kernels where every modulus leaves seven spare bits (ctx->lazy_ok), their TIGHT
// forms for 26..28-bit moduli in 32-bit words (ctx->tight_ok, ntt_lds.h); -1: neither
template <typename W, typename F>
static int by_width_class(const GpuContext *ctx, F &&f) {
    if constexpr (sizeof(W) == 4) {
        if (!ctx->lazy_ok) return ctx->tight_ok ? f(std::true_type{}) : -1;
    }
    return ctx->lazy_ok ? f(std::false_type{}) : -1;
}

template <typename W>
static const TwPair<W> *tw_fwd(const GpuContext *ctx) { return static_cast<const TwPair<W> *>(ctx->d_tw2_fwd); }
template <typename W>
static const TwPair<W> *tw_inv(const GpuContext *ctx) { return static_cast<const TwPair<W> *>(ctx->d_tw2_inv); }

// ---- plain transforms ---------------------------------------------------------------------------------------------------
// TIGHT: 26..28-bit moduli in 32-bit words (ntt_lds.h); NT: non-temporal data accesses (eligible kernel, batch >= 1 GiB)
template <typename W, typename R, bool TIGHT, bool NT>
static int launch_lazy_nt(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes) return -1;
    if (int rc = lds_opt_in<ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, NT>,
                            ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, NT>>(ctx, lds))
        return rc;
    const dim3 grid(static_cast<unsigned>(vectors));
    if (!inverse)
        MXX_LAUNCH((ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, NT>), grid, R::block(), lds, ctx->stream, data,
                   tw_fwd<W>(ctx), ctx->d_limbs, L);
    else
        MXX_LAUNCH((ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, 0, TIGHT, NT>), grid, R::block(), lds, ctx->stream, data,
                   tw_inv<W>(ctx), ctx->d_limbs, L);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W, typename R, bool TIGHT>
static int launch_lazy(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    if constexpr (ntt_nt_data<W, R::LOGN, 0>()) {
        if ((vectors << R::LOGN) * sizeof(W) >= (size_t(1) << 30)) return launch_lazy_nt<W, R, TIGHT, true>(ctx, data, vectors, L, inverse);
    }
    return launch_lazy_nt<W, R, TIGHT, false>(ctx, data, vectors, L, inverse);
}

// 2^(LOGN + PRE) points: head / tail kernel for the PRE outer stages + the LDS kernel on the 2^PRE sub-vectors
template <typename W, typename R, bool TIGHT>
static int launch_split(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes || !R::fits(vectors)) return -1;
    if (int rc = lds_opt_in<ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>,
                            ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>>(ctx, lds))
        return rc;
    const uint32_t logN = R::RING;
    const dim3 sub_grid = R::sub_grid(vectors), set_grid(static_cast<unsigned>(vectors * R::set_blocks)), set_block(256);
    if (!inverse) {
        MXX_LAUNCH((ntt_fwd_head_kernel<W, R::PRE>), set_grid, set_block, 0, ctx->stream, data, tw_fwd<W>(ctx), ctx->d_limbs, L, logN);
        MXX_LAUNCH((ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>), sub_grid, R::block(), lds, ctx->stream, data,
                   tw_fwd<W>(ctx), ctx->d_limbs, L);
    } else {
        MXX_LAUNCH((ntt_inv_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>), sub_grid, R::block(), lds, ctx->stream, data,
                   tw_inv<W>(ctx), ctx->d_limbs, L);
        MXX_LAUNCH((ntt_inv_tail_kernel<W, R::PRE, TIGHT>), set_grid, set_block, 0, ctx->stream, data, tw_inv<W>(ctx), ctx->d_limbs, L, logN);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- 2^14 points in 32-bit words: the grouped kernels of ntt14.h (4 workgroups per CU) ----------------------------------
// MXX_HIP_NTT14=whole selects the whole-vector-in-LDS kernels instead (kept for A/B runs and as a second implementation
// the tests compare); MXX_HIP_NTT14=unsigned keeps the grouped inverse kernel on the unsigned butterflies
static bool ntt14_signed(const GpuContext *ctx) { return ctx->signed_ok && ctx->d_tw2s_inv && ctx->env.ntt14 != 2; }

// the grid of the grouped 2^14 kernels, (limb, poly) with the poly index split exactly over y and z: ntt14_grid (grid_plan.h)

// Do the context and the switches admit a fused form of the grouped kernels?  tight_too: the form has a TIGHT instance;
// phase_too: it takes the phase switch (MXX_HIP_NTT_PHASE)
static bool ntt14_switches(const GpuContext *ctx, bool tight_too, bool phase_too) {
    const EnvSwitches &env = ctx->env;
    return (ctx->lazy_ok || (tight_too && ctx->tight_ok)) && env.ntt14 != 1 && env.ntt_path <= 1 && (phase_too || !env.ntt_phase);
}

// Does a grouped 2^14 kernel serve this batch?  Then `grid` is its grid.
static bool ntt14_grouped(const GpuContext *ctx, size_t vectors, uint32_t L, bool tight_too, bool phase_too, dim3 &grid) {
    return ctx->logN == 14 && ntt14_switches(ctx, tight_too, phase_too) && vectors <= 0x7fffffffull && ntt14_grid(vectors, L, grid);
}

// `in`: inverse only, read the vectors from there instead of `data` (out of place; launch_intt_oop_u32 checks that this kernel runs)
template <typename R, bool TIGHT>
static int launch_ntt14(GpuContext *ctx, uint32_t *data, size_t vectors, uint32_t L, bool inverse, const uint32_t *in = nullptr) {
    using W = uint32_t;
    dim3 grid;
    if (ctx->env.ntt14 == 1 || !ntt14_grid(vectors, L, grid)) return launch_lazy<W, R, TIGHT>(ctx, data, vectors, L, inverse);
    const dim3 block(ntt14::T);
    const size_t lds = ntt14::lds_bytes(sizeof(W));
    if (!inverse) {
        // batches no cache level can hold (>= 1 GiB): non-temporal data accesses, as the whole-vector LDS kernels do - the
        // stream then leaves the twiddle tables (and whatever the next kernel wants) in L2 / the Infinity Cache: forward
        // 31.8 -> 30.2 ns per vector on 4096 polys x 4 limbs (same-box A/B, profiles/r03_notes.md)
        const bool nt = (vectors << 14) * sizeof(W) >= (size_t(1) << 30);
        return bool_dispatch(nt, [&](auto NT) {
            MXX_LAUNCH((ntt14::fwd_kernel<W, TIGHT, NT()>), grid, block, lds, ctx->stream, data, tw_fwd<W>(ctx), ctx->d_limbs, L,
                       static_cast<uint32_t>(ctx->env.ntt_phase));
            HIP_TRY(hipGetLastError());
            return 0;
        });
    }
    // the inverse runs the same instance at every batch size (the unsigned one has no non-temporal form; the signed one's
    // is instantiated in ntt_lds_u32.hip and has never been selected)
    if constexpr (!TIGHT) {  // the signed butterflies have no TIGHT form
        if (ntt14_signed(ctx)) {
            MXX_LAUNCH((ntt14::inv_kernel<W, true>), grid, block, lds, ctx->stream, data, static_cast<const TwPair<W> *>(ctx->d_tw2s_inv),
                       ctx->d_limbs, L, in, nullptr);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    MXX_LAUNCH((ntt14::inv_kernel<W, false, false, TIGHT ? kTightCap : 31>), grid, block, lds, ctx->stream, data, tw_inv<W>(ctx),
               ctx->d_limbs, L, in, nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// every ring with a tuned transform; the caller has checked ctx->lazy_ok || ctx->tight_ok.  `in`: see launch_ntt14 (the
// caller has checked ntt14_grouped)
template <typename W>
static int launch_ntt_lds(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse, const W *in = nullptr) {
    return by_width_class<W>(ctx, [&](auto tight) {
        constexpr bool TIGHT = decltype(tight)::value;
        return visit_ring<W>(ctx->logN, [&](auto ring) {
            using R = decltype(ring);
            if constexpr (R::PRE > 0) return launch_split<W, R, TIGHT>(ctx, data, vectors, L, inverse);
            else if constexpr (sizeof(W) == 4 && R::RING == 14) return launch_ntt14<R, TIGHT>(ctx, data, vectors, L, inverse, in);
            else return launch_lazy<W, R, TIGHT>(ctx, data, vectors, L, inverse);
        });
    });
}

// ---- decompose + forward transform in one pass --------------------------------------------------------------------------
// One digit-fused launch: digit rows [td0, td0 + k) of each of src_rows source rows, k consecutive output rows per source
// row - the whole decomposition is td0 = 0 and k = its digit count, a row window is a few such launches (decompose.hip,
// decompose_window).  plan() holds the preconditions every form shares, and what they all derive.
template <typename W>
struct DigitLaunch {
    W *out;
    const W *coeff;
    uint32_t L, src_cols, towers, dpt, base_bits, k, td0;
    size_t src_rows, vectors;  // vectors = src_rows k src_cols L: what the launch writes
    bool reduce;               // can a digit reach an output modulus?  (digits are below 2^min(base_bits, bits of the widest limb))
    // outputs that fit the Infinity Cache stay cacheable for their consumer ((1 x 64) G^-1(4 x 4): 180 -> 168 us); from 0.5 GB
    // the non-temporal hint wins (8 x 8: 442 -> 390 us)
    bool nts;

    // false: no fused launch for these arguments (the caller then runs the digit kernel and the transform separately)
    bool plan(const GpuContext *ctx, size_t out_vectors, size_t k_rows) {
        if (ctx->env.ntt_path > 1 || !ctx->env.decompose_fused || out_vectors > 0x7fffffffull || k_rows >> 32) return false;
        if (k_rows == 0 || src_cols == 0 || out_vectors % (k_rows * src_cols * L) != 0) return false;
        src_rows = out_vectors / (k_rows * src_cols * L);
        if (src_rows > 65535 || k_rows > 65535 || static_cast<uint64_t>(src_cols) * L > 0x7fffffffull) return false;  // grid limits
        k = static_cast<uint32_t>(k_rows);
        vectors = out_vectors;
        const uint32_t digit_bits = std::min<uint32_t>(base_bits, ctx->crt_bits);
        uint64_t min_q = ~0ull;
        for (uint32_t l = 0; l < L; ++l) min_q = std::min<uint64_t>(min_q, ctx->moduli[l]);
        reduce = digit_bits >= 63 || ((1ull << digit_bits) - 1) >= min_q;
        nts = out_vectors * ctx->N * sizeof(W) >= (size_t(1) << 29);
        return true;
    }
    // (blocks per (limb, column)) x digit row x source row
    dim3 grid(uint32_t blocks = 1) const { return dim3(blocks * L * src_cols, k, static_cast<unsigned>(src_rows)); }
};

// the whole vector in LDS (ntt_fwd_lazy_digits_kernel)
template <typename W, typename R, bool TIGHT>
static int launch_lazy_digits(GpuContext *ctx, const DigitLaunch<W> &d) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes) return -1;
    if (int rc = lds_opt_in<ntt_fwd_lazy_digits_kernel<W, R::LOGN, R::LOGR, R::WPE, TIGHT, false, false>,
                            ntt_fwd_lazy_digits_kernel<W, R::LOGN, R::LOGR, R::WPE, TIGHT, false, true>,
                            ntt_fwd_lazy_digits_kernel<W, R::LOGN, R::LOGR, R::WPE, TIGHT, true, false>,
                            ntt_fwd_lazy_digits_kernel<W, R::LOGN, R::LOGR, R::WPE, TIGHT, true, true>>(ctx, lds))
        return rc;
    return bool_dispatch(d.reduce, d.nts, [&](auto RED, auto NTS) {
        MXX_LAUNCH((ntt_fwd_lazy_digits_kernel<W, R::LOGN, R::LOGR, R::WPE, TIGHT, RED(), NTS()>), d.grid(), R::block(), lds, ctx->stream,
                   d.out, d.coeff, tw_fwd<W>(ctx), ctx->d_limbs, d.L, d.src_cols, d.dpt, d.base_bits, d.k, d.td0);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// the split sizes: head kernel with the digits in its load, then the sub-vectors
template <typename W, typename R, bool TIGHT>
static int launch_split_digits(GpuContext *ctx, const DigitLaunch<W> &d) {
    const size_t lds = R::template lds<W>();
    if (lds > kLdsLimitBytes || !R::fits(d.vectors) || static_cast<uint64_t>(R::set_blocks) * d.L * d.src_cols > 0x7fffffffull) return -1;
    if (int rc = lds_opt_in<ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>>(ctx, lds)) return rc;
    const uint32_t logN = R::RING;
    return bool_dispatch(d.reduce, d.nts, [&](auto RED, auto NTS) {
        MXX_LAUNCH((ntt_fwd_head_digits_kernel<W, R::PRE, RED(), NTS()>), d.grid(R::set_blocks), dim3(256), 0, ctx->stream, d.out, d.coeff,
                   tw_fwd<W>(ctx), ctx->d_limbs, d.L, logN, d.src_cols, d.dpt, d.base_bits, d.k, d.td0);
        MXX_LAUNCH((ntt_fwd_lazy_kernel<W, R::LOGN, R::LOGR, R::WPE, R::PRE, TIGHT>), R::sub_grid(d.vectors), R::block(), lds, ctx->stream,
                   d.out, tw_fwd<W>(ctx), ctx->d_limbs, d.L);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// every ring with a tuned transform except 2^14 in 32-bit words, where the grouped kernel is the only digit-fused form
// (launch_ntt_digits_u32); -1: none for this ring
template <typename W>
static int launch_ntt_digits(GpuContext *ctx, const DigitLaunch<W> &d) {
    return by_width_class<W>(ctx, [&](auto tight) {
        constexpr bool TIGHT = decltype(tight)::value;
        return visit_ring<W>(ctx->logN, [&](auto ring) {
            using R = decltype(ring);
            if constexpr (R::PRE > 0) return launch_split_digits<W, R, TIGHT>(ctx, d);
            else if constexpr (sizeof(W) == 4 && R::RING == 14) return -1;
            else return launch_lazy_digits<W, R, TIGHT>(ctx, d);
        });
    });
}
