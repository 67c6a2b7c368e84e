// norm.hip — exact centred infinity norm of every entry of a matrix.
//
// gpupoly_matrix_centered_max_abs: entry (row, col) -> max_i |x_i|, x_i the representative of coefficient i in
// (-Q/2, Q/2], Q = q_0 .. q_level the matrix's own level (= min(v, Q - v) for v in [0, Q): Q is odd).  Replaces the host
// loops that rebuild every coefficient as a big integer and take that maximum: the preimage predicate
// (src/sampler/trapdoor/gpu.rs:690-752, the p-hat form :756-812) and matrix_centered_max_abs
// (tests/test_gpu_diamond_injector_q_bits_vs_max_error_plot_generates_svg.rs:145-163).
//
// Exact method, no rounding anywhere:
//   1. norm_partial_kernel: a workgroup takes one chunk (kNormChunk coefficients at most) of one entry.  Every thread keeps
//      the running maximum of its coefficients' |x| as little-endian words: reconstruct_small's two O(L) fast paths first,
//      reconstruct_centered's Garner path for a coefficient they do not cover (centred.h).  The workgroup's maximum is taken
//      word by word from the top: the max of word w over the lanes still in the running, after which only the lanes that
//      hold it stay in - by shuffles within a wave, then once more over the waves' results in LDS.  Ties in the top words are
//      thus settled by the lower ones.  The chunk's words go to partial[entry][chunk].
//   2. norm_final_kernel: one thread per entry picks the largest of its chunks' values (whole-word comparisons, top word
//      first) and writes it with words_per_value words, zero above the words of Q.
#include "centred.h"

#include <algorithm>

namespace {

constexpr uint32_t kNormThreads = 256;
constexpr uint32_t kNormWaves = kNormThreads / 64;
constexpr uint32_t kNormChunk = 2048;  // coefficients of one entry per workgroup task: 8 per thread

// a > b as WC-word little-endian integers: the highest word where they differ decides
template <int ML>
__device__ __forceinline__ bool words_greater(const uint64_t *a, const uint64_t *b, int WC) {
    bool gt = false;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int w = 0; w < ML; ++w)
            if (w < WC && a[w] != b[w]) gt = a[w] > b[w];
    } else {
        for (int w = 0; w < WC; ++w)
            if (a[w] != b[w]) gt = a[w] > b[w];
    }
    return gt;
}

template <int ML>
__device__ __forceinline__ void words_take_max(uint64_t *best, const uint64_t *x, int WC) {
    if (!words_greater<ML>(x, best, WC)) return;
    if constexpr (ML <= 16) {
#pragma unroll
        for (int w = 0; w < ML; ++w)
            if (w < WC) best[w] = x[w];
    } else {
        for (int w = 0; w < WC; ++w) best[w] = x[w];
    }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// v <- the largest of the 64 lanes' WC-word values, in every lane.  From the top word down: m = the max of word w over the
// lanes still in, and a lane stays in only if its word w is m.  Lanes that dropped out offer 0, which never exceeds the
// word of a lane still in, and the lane that holds the maximum is never dropped - so the words m are its words.
template <int ML>
__device__ __forceinline__ void wave_max_words(uint64_t *v, int WC) {
    bool in = true;
    auto step = [&](int w) {
        const uint64_t m = wave_max_u64(in ? v[w] : 0);
        in = in && v[w] == m;
        v[w] = m;
    };
    if constexpr (ML <= 16) {
#pragma unroll
        for (int w = ML - 1; w >= 0; --w)
            if (w < WC) step(w);
    } else {
        for (int w = WC - 1; w >= 0; --w) step(w);
    }
}

}  // namespace

// partial[(poly * chunks + c) * WC + w]: word w of max |x| over coefficients [c chunk, (c + 1) chunk) of entry `poly`
template <typename W, int ML>
__global__ void __launch_bounds__(kNormThreads) norm_partial_kernel(const W *__restrict__ src, size_t polys, uint32_t N,
                                                                    uint32_t chunk, uint32_t chunks, SerdeConsts sc,
                                                                    const uint64_t *__restrict__ garner, size_t garner_stride,
                                                                    const LimbConst *__restrict__ limbs,
                                                                    uint64_t *__restrict__ partial) {
    __shared__ uint64_t wave_best[kNormWaves][ML];
    const int WC = sc.words;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t tasks = polys * chunks;
    for (size_t task = blockIdx.x; task < tasks; task += gridDim.x) {  // uniform over the workgroup
        const size_t poly = task / chunks;
        const uint32_t first = static_cast<uint32_t>(task % chunks) * chunk, end = min(first + chunk, N);
        uint64_t best[ML];
        if constexpr (ML <= 16) {
#pragma unroll
            for (int w = 0; w < ML; ++w) best[w] = 0;
            uint64_t small[ML];  // the largest fast-path value: at most two words
#pragma unroll
            for (int w = 0; w < ML; ++w) small[w] = 0;
            for (uint32_t i = first + threadIdx.x; i < end; i += kNormThreads) {
                uint64_t lo, hi;
                bool neg;
                if (reconstruct_small<W, ML>(src, poly, i, N, sc, garner, garner_stride, limbs, lo, hi, neg)) {
                    if (hi > small[1] || (hi == small[1] && lo > small[0])) {
                        small[0] = lo;
                        small[1] = hi;
                    }
                } else {  // beyond the fast paths: this coefficient alone goes through Garner
                    uint64_t x[ML];
                    reconstruct_centered<W, ML>(src, poly, i, N, sc, garner, garner_stride, limbs, x, neg);
                    words_take_max<ML>(best, x, WC);
                }
            }
            words_take_max<ML>(best, small, WC);  // small[1] is 0 when WC == 1 (|x| < Q / 2 < 2^63)
        } else {
            for (int w = 0; w < WC; ++w) best[w] = 0;
            for (uint32_t i = first + threadIdx.x; i < end; i += kNormThreads) {
                uint64_t x[ML];
                bool neg;
                reconstruct_centered<W, ML>(src, poly, i, N, sc, garner, garner_stride, limbs, x, neg);
                words_take_max<ML>(best, x, WC);
            }
        }
        wave_max_words<ML>(best, WC);
        if (lane == 0)
            for (int w = 0; w < WC; ++w) wave_best[wave][w] = best[w];
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < WC; ++w) best[w] = lane < kNormWaves ? wave_best[lane][w] : 0;
            wave_max_words<ML>(best, WC);
            if (lane == 0)
                for (int w = 0; w < WC; ++w) partial[task * WC + w] = best[w];
        }
        __syncthreads();  // wave_best is rewritten by the next task
    }
}

// out[poly * wpv + w]: the largest of the entry's chunk values, zero above its WC words
__global__ void __launch_bounds__(256) norm_final_kernel(const uint64_t *__restrict__ partial, size_t polys, uint32_t chunks,
                                                         int WC, uint64_t *__restrict__ out, uint32_t wpv) {
    const size_t poly = item_index();
    if (poly >= polys) return;
    const uint64_t *p = partial + poly * chunks * WC;
    uint32_t top = 0;  // chunk holding the largest value so far
    for (uint32_t c = 1; c < chunks; ++c) {
        const uint64_t *a = p + static_cast<size_t>(c) * WC, *b = p + static_cast<size_t>(top) * WC;
        for (int w = WC - 1; w >= 0; --w)
            if (a[w] != b[w]) {
                if (a[w] > b[w]) top = c;
                break;
            }
    }
    const uint64_t *m = p + static_cast<size_t>(top) * WC;
    uint64_t *o = out + poly * wpv;
    for (int w = 0; w < WC; ++w) o[w] = m[w];
    for (uint32_t w = static_cast<uint32_t>(WC); w < wpv; ++w) o[w] = 0;
}

extern "C" int gpupoly_matrix_centered_max_abs(const GpuMatrix *mat, uint64_t *out, size_t words_per_value) {
    ABI_GUARD_BEGIN
    // every refusal comes before the first launch and before `out` is touched
    if (!mat || !out) return set_error("gpupoly_matrix_centered_max_abs: null argument");
    GpuContext *ctx = mat->ctx;
    SerdeConsts sc;
    if (build_consts(mat, sc)) return 1;
    if (words_per_value < static_cast<size_t>(sc.words))
        return set_error("gpupoly_matrix_centered_max_abs: words_per_value is below the " + std::to_string(sc.words) +
                         " words the level's modulus needs");
    if (words_per_value > 0xffffffffull) return set_error("gpupoly_matrix_centered_max_abs: words_per_value too large");
    const size_t polys = matrix_polys(mat);
    if (polys == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const int L = sc.limbs;

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
    const uint32_t chunk = std::min(N, kNormChunk), chunks = N / chunk;  // N is a power of two
    const size_t tasks = polys * chunks;
    const size_t WC = static_cast<size_t>(sc.words);
    CtxBlock partial(ctx), dev_out(ctx);
    if (partial.alloc(tasks * WC * sizeof(uint64_t))) return 1;
    const size_t out_bytes = polys * words_per_value * sizeof(uint64_t);
    if (dev_out.alloc(out_bytes)) return 1;
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(tasks, size_t(1) << 20)));
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    uint64_t *const d_partial = static_cast<uint64_t *>(partial.ptr);
    MXX_TRACE_BYTES(static_cast<double>(matrix_words(mat) * ctx->word_bytes + tasks * WC * sizeof(uint64_t)));
#define NORM_PARTIAL(WT, ML)                                                                                             \
    MXX_LAUNCH((norm_partial_kernel<WT, ML>), grid, dim3(kNormThreads), 0, ctx->stream, static_cast<const WT *>(src), polys, \
               N, chunk, chunks, sc, ctx->d_garner, gstride, ctx->d_limbs, d_partial)
#define NORM_BY_LIMBS(WT)                        \
    do {                                         \
        if (L <= 8) NORM_PARTIAL(WT, 8);         \
        else if (L <= 16) NORM_PARTIAL(WT, 16);  \
        else NORM_PARTIAL(WT, 64);               \
    } while (0)
    if (ctx->wide) NORM_BY_LIMBS(uint64_t);
    else NORM_BY_LIMBS(uint32_t);
#undef NORM_BY_LIMBS
#undef NORM_PARTIAL
    HIP_TRY(hipGetLastError());
    MXX_TRACE_BYTES(static_cast<double>(tasks * WC * sizeof(uint64_t) + out_bytes));
    MXX_LAUNCH(norm_final_kernel, item_grid(polys, 256), dim3(256), 0, ctx->stream, d_partial, polys, chunks,
               static_cast<int>(WC), static_cast<uint64_t *>(dev_out.ptr), static_cast<uint32_t>(words_per_value));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dev_out.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
    ABI_GUARD_END
}
