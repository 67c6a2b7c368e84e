// included by ntt_lds_u32.hip / ntt_lds_u64.hip after `typedef ... W;`
static constexpr size_t kLdsLimitBytes = 160 * 1024;

// TIGHT: 26..28-bit moduli in 32-bit words (ntt_lds.h); NT: non-temporal data accesses (eligible kernel, batch >= 1 GiB)
template <int LOGN, int LOGR, int WPE, bool TIGHT, bool NT>
static int launch_lazy_nt(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = lds_padded_words(size_t(1) << LOGN) * sizeof(W);
    if (lds > kLdsLimitBytes) return -1;
    const void *fwd = reinterpret_cast<const void *>(ntt_fwd_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, NT>);
    const void *inv = reinterpret_cast<const void *>(ntt_inv_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, NT>);
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        HIP_TRY(hipFuncSetAttribute(fwd, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        HIP_TRY(hipFuncSetAttribute(inv, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    const dim3 grid(static_cast<unsigned>(vectors)), block(1u << (LOGN - LOGR));
    if (!inverse)
        MXX_LAUNCH((ntt_fwd_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, NT>), grid, block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L);
    else
        MXX_LAUNCH((ntt_inv_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, NT>), grid, block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs, L);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int LOGN, int LOGR, int WPE, bool TIGHT = false>
static int launch_lazy(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    if constexpr (ntt_nt_data<W, LOGN, 0>()) {
        if ((vectors << LOGN) * sizeof(W) >= (size_t(1) << 30))
            return launch_lazy_nt<LOGN, LOGR, WPE, TIGHT, true>(ctx, data, vectors, L, inverse);
    }
    return launch_lazy_nt<LOGN, LOGR, WPE, TIGHT, false>(ctx, data, vectors, L, inverse);
}

// 2^14 points: the grouped kernels of ntt14.h (4 workgroups per CU); MXX_HIP_NTT14=whole
// selects the whole-vector-in-LDS kernels instead (kept for A/B runs and as a second
// implementation the tests compare)
// MXX_HIP_NTT14=unsigned keeps the grouped inverse kernel on the unsigned butterflies
static bool ntt14_signed(const GpuContext *ctx) {
    return sizeof(W) == 4 && ctx->signed_ok && ctx->d_tw2s_inv && ctx->env.ntt14 != 2;
}

// grid of the grouped 2^14 kernels: (limb, poly) with the poly index split over y and z (each <= 65535)
static bool ntt14_grid(size_t vectors, uint32_t L, dim3 &grid) {
    if (L == 0 || vectors % L != 0) return false;
    const size_t polys = vectors / L;
    size_t z = (polys + 65534) / 65535;
    if (z == 0) z = 1;
    if (z > 65535 || polys % z != 0) {  // keep the grid exact (no out-of-range blocks): find a divisor split
        z = 0;
        for (size_t cand = (polys + 65534) / 65535; cand <= 65535 && cand <= polys; ++cand)
            if (polys % cand == 0 && polys / cand <= 65535) { z = cand; break; }
        if (z == 0) return false;
    }
    grid = dim3(L, static_cast<unsigned>(polys / z), static_cast<unsigned>(z));
    return true;
}

template <bool TIGHT>
static int launch_ntt14(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse, const W *in = nullptr) {
    // `in`: inverse only, read the vectors from there instead of `data` (out of place; launch_intt_oop_u32 checks that this kernel runs)
    const bool whole = ctx->env.ntt14 == 1;
    if (whole || sizeof(W) != 4) return launch_lazy<14, 5, sizeof(W) == 4 ? 4 : 2, TIGHT>(ctx, data, vectors, L, inverse);
    const size_t lds = ntt14::lds_bytes(sizeof(W));
    dim3 grid, block(ntt14::T);
    if (!ntt14_grid(vectors, L, grid)) return launch_lazy<14, 5, sizeof(W) == 4 ? 4 : 2, TIGHT>(ctx, data, vectors, L, inverse);
    if constexpr (sizeof(W) == 4 && !TIGHT) {
        if (inverse && ntt14_signed(ctx)) {
            MXX_LAUNCH((ntt14::inv_kernel<W, true>), grid, block, lds, ctx->stream, data,
                               static_cast<const TwPair<W> *>(ctx->d_tw2s_inv), ctx->d_limbs, L, in, nullptr);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    // batches no cache level can hold (>= 1 GiB): non-temporal data accesses, as the whole-vector LDS kernels do - the
    // stream then leaves the twiddle tables (and whatever the next kernel wants) in L2 / the Infinity Cache: forward
    // 31.8 -> 30.2 ns per vector on 4096 polys x 4 limbs (same-box A/B, profiles/r03_notes.md)
    const bool nt = (vectors << 14) * sizeof(W) >= (size_t(1) << 30);
    if constexpr (sizeof(W) == 4 && !TIGHT) {
        if (inverse && nt && ntt14_signed(ctx)) {
            MXX_LAUNCH((ntt14::inv_kernel<W, true, false, 31, 8, true>), grid, block, lds, ctx->stream, data,
                               static_cast<const TwPair<W> *>(ctx->d_tw2s_inv), ctx->d_limbs, L, in, nullptr);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    if (!inverse && nt)
        MXX_LAUNCH((ntt14::fwd_kernel<W, TIGHT, true>), grid, block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L, static_cast<uint32_t>(ctx->env.ntt_phase));
    else if (!inverse)
        MXX_LAUNCH((ntt14::fwd_kernel<W, TIGHT>), grid, block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L, static_cast<uint32_t>(ctx->env.ntt_phase));
    else
        MXX_LAUNCH((ntt14::inv_kernel<W, false, false, TIGHT ? kTightCap : 31>), grid, block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs, L, in, nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// 2^(SUBLOG + PRE) points: head / tail kernel for the PRE outer stages + the LDS kernel on the 2^PRE sub-vectors
template <int SUBLOG, int LOGR, int WPE, int PRE, bool TIGHT = false>
static int launch_split(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    const size_t lds = lds_padded_words(size_t(1) << SUBLOG) * sizeof(W);
    if (lds > kLdsLimitBytes || vectors > (0x7fffffffull >> PRE)) return -1;
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ntt_fwd_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ntt_inv_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    const uint32_t logN = SUBLOG + PRE;
    const dim3 sub_grid(static_cast<unsigned>(vectors << PRE)), sub_block(1u << (SUBLOG - LOGR));
    const dim3 set_grid(static_cast<unsigned>(vectors * (((1u << logN) >> PRE) / 256u))), set_block(256);
    if (!inverse) {
        MXX_LAUNCH((ntt_fwd_head_kernel<W, PRE>), set_grid, set_block, 0, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L, logN);
        MXX_LAUNCH((ntt_fwd_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>), sub_grid, sub_block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L);
    } else {
        MXX_LAUNCH((ntt_inv_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>), sub_grid, sub_block, lds, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs, L);
        MXX_LAUNCH((ntt_inv_tail_kernel<W, PRE, TIGHT>), set_grid, set_block, 0, ctx->stream, data,
                           static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs, L, logN);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// decompose + forward transform at the split sizes: head kernel with the digits in its load, then the sub-vectors
template <int SUBLOG, int LOGR, int WPE, int PRE, bool TIGHT>
static int launch_split_digits(GpuContext *ctx, W *out, const W *coeff, uint32_t L, uint32_t src_cols, size_t src_rows,
                               uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0, bool reduce) {
    const size_t lds = lds_padded_words(size_t(1) << SUBLOG) * sizeof(W);
    const size_t vectors = src_rows * k * src_cols * L;
    if (lds > kLdsLimitBytes || vectors > (0x7fffffffull >> PRE)) return -1;
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ntt_fwd_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    const uint32_t logN = SUBLOG + PRE;
    const uint64_t gx = static_cast<uint64_t>(((1u << logN) >> PRE) / 256u) * L * src_cols;
    if (gx > 0x7fffffffull || k > 65535 || src_rows > 65535) return -1;
    const dim3 set_grid(static_cast<unsigned>(gx), static_cast<unsigned>(k), static_cast<unsigned>(src_rows));
    const dim3 sub_grid(static_cast<unsigned>(vectors << PRE)), sub_block(1u << (SUBLOG - LOGR));
    const bool nts = (vectors << logN) * sizeof(W) >= (size_t(1) << 29);  // outputs that fit the Infinity Cache stay cacheable for the sub-vector kernel
#define MXX_HEAD(RED, NTSF)                                                                                                   \
    MXX_LAUNCH((ntt_fwd_head_digits_kernel<W, PRE, RED, NTSF>), set_grid, dim3(256), 0, ctx->stream, out, coeff,         \
                       static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L, logN, src_cols, dpt, base_bits,          \
                       static_cast<uint32_t>(k), td0)
    if (reduce) {
        if (nts) MXX_HEAD(true, true);
        else MXX_HEAD(true, false);
    } else {
        if (nts) MXX_HEAD(false, true);
        else MXX_HEAD(false, false);
    }
#undef MXX_HEAD
    MXX_LAUNCH((ntt_fwd_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT>), sub_grid, sub_block, lds, ctx->stream, out,
                       static_cast<const TwPair<W> *>(ctx->d_tw2_fwd), ctx->d_limbs, L);
    HIP_TRY(hipGetLastError());
    return 0;
}

// decompose + forward transform with the whole vector in LDS (ntt_fwd_lazy_digits_kernel)
template <int LOGN, int LOGR, int WPE, bool TIGHT>
static int launch_lazy_digits(GpuContext *ctx, W *out, const W *coeff, uint32_t L, uint32_t src_cols, size_t src_rows,
                              uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0, bool reduce) {
    const size_t lds = lds_padded_words(size_t(1) << LOGN) * sizeof(W);
    if (lds > kLdsLimitBytes) return -1;
    const size_t vectors = src_rows * k * src_cols * L;
    const bool nts = (vectors << LOGN) * sizeof(W) >= (size_t(1) << 29);  // outputs that fit the Infinity Cache stay cacheable for their consumer
    const void *fs[4] = {reinterpret_cast<const void *>(ntt_fwd_lazy_digits_kernel<W, LOGN, LOGR, WPE, TIGHT, false, false>),
                         reinterpret_cast<const void *>(ntt_fwd_lazy_digits_kernel<W, LOGN, LOGR, WPE, TIGHT, false, true>),
                         reinterpret_cast<const void *>(ntt_fwd_lazy_digits_kernel<W, LOGN, LOGR, WPE, TIGHT, true, false>),
                         reinterpret_cast<const void *>(ntt_fwd_lazy_digits_kernel<W, LOGN, LOGR, WPE, TIGHT, true, true>)};
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        for (const void *f : fs) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    const uint64_t gx = static_cast<uint64_t>(L) * src_cols;
    if (gx > 0x7fffffffull || k > 65535 || src_rows > 65535) return -1;
    const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(k), static_cast<unsigned>(src_rows)), block(1u << (LOGN - LOGR));
    const TwPair<W> *tw = static_cast<const TwPair<W> *>(ctx->d_tw2_fwd);
#define MXX_LZD(RED, NTSF)                                                                                                      \
    MXX_LAUNCH((ntt_fwd_lazy_digits_kernel<W, LOGN, LOGR, WPE, TIGHT, RED, NTSF>), grid, block, lds, ctx->stream, out,     \
                       coeff, tw, ctx->d_limbs, L, src_cols, dpt, base_bits, static_cast<uint32_t>(k), td0)
    if (reduce) {
        if (nts) MXX_LZD(true, true);
        else MXX_LZD(true, false);
    } else {
        if (nts) MXX_LZD(false, true);
        else MXX_LZD(false, false);
    }
#undef MXX_LZD
    HIP_TRY(hipGetLastError());
    return 0;
}

// every ring with a tuned transform except the 32-bit 2^14 grouped kernel (ntt_lds_u32.hip); -1: none for this ring
template <bool TIGHT>
static int dispatch_ntt_digits_impl(GpuContext *ctx, W *out, const W *coeff, uint32_t L, uint32_t src_cols, size_t src_rows,
                                    uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0, bool reduce) {
#define MXX_ARGS ctx, out, coeff, L, src_cols, src_rows, dpt, base_bits, k, td0, reduce
    if constexpr (sizeof(W) == 8) {
        switch (ctx->logN) {
            case 14: return launch_lazy_digits<14, 5, 2, false>(MXX_ARGS);
            case 15: return launch_split_digits<11, 4, 1, 4, false>(MXX_ARGS);
            case 16: return launch_split_digits<12, 4, 1, 4, false>(MXX_ARGS);
            case 17: return launch_split_digits<12, 4, 1, 5, false>(MXX_ARGS);
            default: break;
        }
    } else {
        switch (ctx->logN) {
            case 15: return launch_lazy_digits<15, 5, 4, TIGHT>(MXX_ARGS);
            case 16: return launch_split_digits<12, 4, 1, 4, TIGHT>(MXX_ARGS);
            case 17: return launch_split_digits<12, 4, 1, 5, TIGHT>(MXX_ARGS);
            default: break;
        }
    }
    switch (ctx->logN) {
        case 10: return launch_lazy_digits<10, 4, 1, TIGHT>(MXX_ARGS);
        case 11: return launch_lazy_digits<11, 4, 1, TIGHT>(MXX_ARGS);
        case 12: return launch_lazy_digits<12, 4, 1, TIGHT>(MXX_ARGS);
        case 13: return launch_lazy_digits<13, 5, 1, TIGHT>(MXX_ARGS);
        default: return -1;
    }
#undef MXX_ARGS
}

static int dispatch_ntt_digits(GpuContext *ctx, W *out, const W *coeff, uint32_t L, uint32_t src_cols, size_t src_rows,
                               uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0, bool reduce) {
    if constexpr (sizeof(W) == 4) {
        if (!ctx->lazy_ok)
            return ctx->tight_ok ? dispatch_ntt_digits_impl<true>(ctx, out, coeff, L, src_cols, src_rows, dpt, base_bits, k, td0, reduce) : -1;
    } else {
        if (!ctx->lazy_ok) return -1;
    }
    return dispatch_ntt_digits_impl<false>(ctx, out, coeff, L, src_cols, src_rows, dpt, base_bits, k, td0, reduce);
}

template <bool TIGHT>
static int dispatch_ntt_lds_impl(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    if constexpr (sizeof(W) == 8) {  // 64-bit words: the whole vector fits LDS up to 2^14 points
        switch (ctx->logN) {
            case 15: return launch_split<11, 4, 1, 4>(ctx, data, vectors, L, inverse);
            case 16: return launch_split<12, 4, 1, 4>(ctx, data, vectors, L, inverse);
            case 17: return launch_split<12, 4, 1, 5>(ctx, data, vectors, L, inverse);
            default: break;
        }
    } else {
        switch (ctx->logN) {
            case 16: return launch_split<12, 4, 1, 4, TIGHT>(ctx, data, vectors, L, inverse);
            case 17: return launch_split<12, 4, 1, 5, TIGHT>(ctx, data, vectors, L, inverse);
            default: break;
        }
    }
    switch (ctx->logN) {
        case 10: return launch_lazy<10, 4, 1, TIGHT>(ctx, data, vectors, L, inverse);
        case 11: return launch_lazy<11, 4, 1, TIGHT>(ctx, data, vectors, L, inverse);
        case 12: return launch_lazy<12, 4, 1, TIGHT>(ctx, data, vectors, L, inverse);
        case 13: return launch_lazy<13, 5, 1, TIGHT>(ctx, data, vectors, L, inverse);
        case 14: return launch_ntt14<TIGHT>(ctx, data, vectors, L, inverse);
        case 15: return launch_lazy<15, 5, 4, TIGHT>(ctx, data, vectors, L, inverse);
        default: return -1;
    }
}

// the caller has checked ctx->lazy_ok || ctx->tight_ok
static int dispatch_ntt_lds(GpuContext *ctx, W *data, size_t vectors, uint32_t L, bool inverse) {
    if constexpr (sizeof(W) == 4) {
        if (!ctx->lazy_ok) return ctx->tight_ok ? dispatch_ntt_lds_impl<true>(ctx, data, vectors, L, inverse) : -1;
    } else {
        if (!ctx->lazy_ok) return -1;
    }
    return dispatch_ntt_lds_impl<false>(ctx, data, vectors, L, inverse);
}

// ---- out <- INTT(in o w) in one pass over the data (gpupoly_matrix_mul_scalar_intt) -------------------------------------
// w is used as it stands (EVAL residues): the kernels' product is a Montgomery one and ctx->d_limbs_r carries the
// compensating 2^32 in the N^-1 constants of whichever kernel runs the last stage.  32-bit words only.
template <int LOGN, int LOGR, int WPE, bool TIGHT>
static int launch_lazy_mulw(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    const size_t lds = lds_padded_words(size_t(1) << LOGN) * sizeof(W);
    if (lds > kLdsLimitBytes) return -1;
    const void *fn = reinterpret_cast<const void *>(ntt_inv_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, false, true>);
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    MXX_LAUNCH((ntt_inv_lazy_kernel<W, LOGN, LOGR, WPE, 0, TIGHT, false, true>), dim3(static_cast<unsigned>(vectors)),
                       dim3(1u << (LOGN - LOGR)), lds, ctx->stream, out, static_cast<const TwPair<W> *>(ctx->d_tw2_inv),
                       ctx->d_limbs_r, L, in, w);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int SUBLOG, int LOGR, int WPE, int PRE, bool TIGHT>
static int launch_split_mulw(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    const size_t lds = lds_padded_words(size_t(1) << SUBLOG) * sizeof(W);
    if (lds > kLdsLimitBytes || vectors > (0x7fffffffull >> PRE)) return -1;
    const void *fn = reinterpret_cast<const void *>(ntt_inv_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT, false, true>);
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds > 64 * 1024 && !(configured.load() & bit)) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        configured.fetch_or(bit);
    }
    const uint32_t logN = SUBLOG + PRE;
    const dim3 sub_grid(static_cast<unsigned>(vectors << PRE)), sub_block(1u << (SUBLOG - LOGR));
    const dim3 set_grid(static_cast<unsigned>(vectors * (((1u << logN) >> PRE) / 256u))), set_block(256);
    // sub-vectors with the product in their load (their own constants are the plain ones: N^-1 is the tail's business)
    MXX_LAUNCH((ntt_inv_lazy_kernel<W, SUBLOG, LOGR, WPE, PRE, TIGHT, false, true>), sub_grid, sub_block, lds, ctx->stream,
                       out, static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs, L, in, w);
    MXX_LAUNCH((ntt_inv_tail_kernel<W, PRE, TIGHT>), set_grid, set_block, 0, ctx->stream, out,
                       static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs_r, L, logN);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <bool TIGHT>
static int dispatch_mul_intt(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    if constexpr (sizeof(W) != 4) {
        return -1;
    } else {
        switch (ctx->logN) {
            case 10: return launch_lazy_mulw<10, 4, 1, TIGHT>(ctx, out, in, w, vectors, L);
            case 11: return launch_lazy_mulw<11, 4, 1, TIGHT>(ctx, out, in, w, vectors, L);
            case 12: return launch_lazy_mulw<12, 4, 1, TIGHT>(ctx, out, in, w, vectors, L);
            case 13: return launch_lazy_mulw<13, 5, 1, TIGHT>(ctx, out, in, w, vectors, L);
            case 14: return launch_lazy_mulw<14, 5, 4, TIGHT>(ctx, out, in, w, vectors, L);
            case 15: return launch_lazy_mulw<15, 5, 4, TIGHT>(ctx, out, in, w, vectors, L);
            case 16: return launch_split_mulw<12, 4, 1, 4, TIGHT>(ctx, out, in, w, vectors, L);
            case 17: return launch_split_mulw<12, 4, 1, 5, TIGHT>(ctx, out, in, w, vectors, L);
            default: return -1;
        }
    }
}

// -1 when no fused kernel covers this context (the caller then runs the point-wise product and the transform separately)
static int launch_mul_intt(GpuContext *ctx, W *out, const W *in, const W *w, size_t vectors, uint32_t L) {
    if constexpr (sizeof(W) != 4) {
        return -1;
    } else {
        if (!(ctx->lazy_ok || ctx->tight_ok) || !ctx->d_limbs_r || ctx->env.ntt_path > 1 || vectors > 0x7fffffffull) return -1;
        dim3 grid, block(ntt14::T);
        MXX_TRACE_BYTES(2.0 * vectors * ctx->N * sizeof(W));  // the resident ring element's L vectors are not counted
        if (ctx->logN == 14 && ctx->lazy_ok && ctx->env.ntt14 != 1 && ntt14_grid(vectors, L, grid)) {
            // the grouped 2^14 kernel (ntt14.h): next group's operands requested a group ahead
            const size_t lds = ntt14::lds_bytes(sizeof(W));
            if (ntt14_signed(ctx))
                MXX_LAUNCH((ntt14::inv_kernel<W, true, true>), grid, block, lds, ctx->stream, out,
                                   static_cast<const TwPair<W> *>(ctx->d_tw2s_inv), ctx->d_limbs_r, L, in, w);
            else
                MXX_LAUNCH((ntt14::inv_kernel<W, false, true>), grid, block, lds, ctx->stream, out,
                                   static_cast<const TwPair<W> *>(ctx->d_tw2_inv), ctx->d_limbs_r, L, in, w);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        return ctx->lazy_ok ? dispatch_mul_intt<false>(ctx, out, in, w, vectors, L) : dispatch_mul_intt<true>(ctx, out, in, w, vectors, L);
    }
}
