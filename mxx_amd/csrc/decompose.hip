// decompose.hip — gadget matrices and base-2^b digit decomposition.
// Replaces cuda/src/matrix/MatrixDecompose.cu behind
// cuda/include/matrix/MatrixDecompose.cuh:26-37.
//
// Indexing (MatrixDecompose.cu:77-113, CPU twin
// src/matrix/dcrt_poly.rs:134-198,453-493): dpt = ceil(crt_bits/base_bits),
// k = dpt*(level+1); digit d of the limb-t residue of coefficient i of M[r,c]
// goes to row r*k + t*dpt + d, column c, coefficient i, replicated into every
// limb; the last digit of a tower keeps bits(q_t) - (dpt-1)*base_bits bits.
//
// One launch reads every source residue once and writes all its digits for all
// output limbs (the reference launches per source limb with a z-slice per digit
// after a full memset).  A constant polynomial is its own NTT, so the gadget
// matrices are written directly in EVAL form with no transform.
#include "common.h"
#include "modarith.h"

#include <algorithm>

static inline uint32_t host_bits(uint64_t v) { return v ? 64 - (uint32_t)__builtin_clzll(v) : 0; }

template <typename W>
__global__ void decompose_kernel(W *__restrict__ out, const W *__restrict__ src, const LimbConst *__restrict__ limbs,
                                 size_t src_polys, uint32_t src_cols, uint32_t L, uint32_t N, uint32_t towers,
                                 uint32_t dpt, uint32_t base_bits, size_t k) {
    // item = (src poly, tower, coefficient)
    const size_t idx = item_index();
    const size_t total = src_polys * towers * N;
    if (idx >= total) return;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const size_t pt = idx / N;
    const uint32_t t = static_cast<uint32_t>(pt % towers);
    const size_t p = pt / towers;
    const size_t r = p / src_cols, c = p - r * src_cols;
    const uint64_t residue = static_cast<uint64_t>(src[(p * L + t) * N + i]);
    const uint32_t src_bits = limbs[t].kbits;
    for (uint32_t d = 0; d < dpt; ++d) {
        const uint32_t shift = d * base_bits;
        uint64_t mask = 0;
        if (shift < src_bits) {
            const uint32_t rem = src_bits - shift;
            const uint32_t db = base_bits < rem ? base_bits : rem;
            mask = db >= 64 ? ~0ull : ((1ull << db) - 1);
        }
        const uint64_t digit = shift >= 64 ? 0 : ((residue >> shift) & mask);
        const size_t orow = r * k + static_cast<size_t>(t) * dpt + d;
        const size_t opoly = orow * src_cols + c;
        for (uint32_t l = 0; l < L; ++l) {
            const uint64_t ql = limbs[l].q;
            out[(opoly * L + l) * N + i] = static_cast<W>(digit >= ql ? digit % ql : digit);
        }
    }
}

// The same digits for a launch that writes only digit rows [td0, td0 + ky) of each source row, ky consecutive output
// rows per source row (a piece of a row window, decompose_window): item = (source row, local digit row, column,
// coefficient), so the work is that of the rows written
template <typename W>
__global__ void decompose_rows_kernel(W *__restrict__ out, const W *__restrict__ src, const LimbConst *__restrict__ limbs,
                                      size_t src_rows, uint32_t src_cols, uint32_t L, uint32_t N, uint32_t dpt,
                                      uint32_t base_bits, uint32_t ky, uint32_t td0) {
    const size_t idx = item_index();
    const size_t total = src_rows * ky * src_cols * N;
    if (idx >= total) return;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const size_t opoly = idx / N;  // (r * ky + y) * src_cols + c
    const size_t orow = opoly / src_cols, c = opoly - orow * src_cols;
    const size_t r = orow / ky;
    const uint32_t td = static_cast<uint32_t>(orow - r * ky) + td0;
    const uint32_t t = td / dpt, d = td - t * dpt;
    const uint64_t residue = static_cast<uint64_t>(src[((r * src_cols + c) * L + t) * N + i]);
    const uint32_t src_bits = limbs[t].kbits, shift = d * base_bits;
    uint64_t mask = 0;
    if (shift < src_bits) {
        const uint32_t rem = src_bits - shift;
        const uint32_t db = base_bits < rem ? base_bits : rem;
        mask = db >= 64 ? ~0ull : ((1ull << db) - 1);
    }
    const uint64_t digit = shift >= 64 ? 0 : ((residue >> shift) & mask);
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t ql = limbs[l].q;
        out[(opoly * L + l) * N + i] = static_cast<W>(digit >= ql ? digit % ql : digit);
    }
}

// G = I_size (x) g written in EVAL form (all slots of a constant poly are equal)
template <typename W>
__global__ void fill_gadget_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs, size_t rows, size_t cols,
                                   uint32_t L, uint32_t N, uint32_t dpt, size_t k, uint32_t base_bits, int small) {
    const size_t idx = item_index();
    const size_t total = rows * cols * L * N;
    if (idx >= total) return;
    const size_t pl = idx / N;
    const uint32_t l = static_cast<uint32_t>(pl % L);
    const size_t p = pl / L;
    const size_t r = p / cols, c = p - r * cols;
    W value = 0;
    const size_t start = r * k;
    if (c >= start && c < start + k) {
        const size_t local = c - start;
        const uint32_t tower = static_cast<uint32_t>(local / dpt), digit = static_cast<uint32_t>(local % dpt);
        if (small || tower == l) {
            const LimbConst lc = limbs[l];
            const uint64_t q = lc.q;
            // base^digit mod q by repeated multiplication (digit < dpt <= 64)
            const uint64_t base = (base_bits >= 64 ? 0 : (1ull << base_bits)) % q;
            uint64_t v = 1 % q;
            for (uint32_t e = 0; e < digit; ++e) v = static_cast<uint64_t>((static_cast<u128_t>(v) * base) % q);
            value = static_cast<W>(v);
        }
    }
    out[idx] = value;
}

// out[local_row, src_row] = scalar_by_digit[0, digit]; everything else was zeroed
template <typename W>
__global__ void identity_chunk_kernel(W *__restrict__ out, const W *__restrict__ src, size_t size, size_t chunk_idx,
                                      size_t chunk_count, size_t words_per_poly) {
    const size_t local_row = blockIdx.y;
    const size_t global_row = chunk_idx * size + local_row;
    const size_t src_row = global_row / chunk_count;
    const size_t digit = global_row - src_row * chunk_count;
    if (src_row >= size) return;
    const W *s = src + digit * words_per_poly;
    W *d = out + (local_row * size + src_row) * words_per_poly;
    for (size_t w = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < words_per_poly;
         w += static_cast<size_t>(gridDim.x) * blockDim.x)
        d[w] = s[w];
}

static int fill_gadget_impl(GpuMatrix *out, uint32_t base_bits, bool small) {
    if (!out) return set_error("gpu_matrix_fill_gadget: null matrix");
    if (base_bits == 0 || base_bits >= 63) return set_error("gpu_matrix_fill_gadget: invalid base_bits");
    GpuContext *ctx = out->ctx;
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t L = matrix_limbs(out);
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (out->cols != out->rows * k) return set_error("gpu_matrix_fill_gadget: output must be size x size*log_base_q");
    out->format = GPU_POLY_FORMAT_EVAL;
    const size_t total = matrix_words(out);
    if (total == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const dim3 blocks = item_grid(total, 256);
    if (ctx->wide)
        MXX_LAUNCH(fill_gadget_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream,
                           static_cast<uint64_t *>(words_ptr(out)), ctx->d_limbs, out->rows, out->cols, (uint32_t)L,
                           (uint32_t)ctx->N, dpt, k, base_bits, small ? 1 : 0);
    else
        MXX_LAUNCH(fill_gadget_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream,
                           static_cast<uint32_t *>(words_ptr(out)), ctx->d_limbs, out->rows, out->cols, (uint32_t)L,
                           (uint32_t)ctx->N, dpt, k, base_bits, small ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Digit rows [td0, td0 + ky) of each of `nsrc` source rows at `coeff` (coefficient words, rows x src_cols x L), written
// as nsrc * ky consecutive rows at `out`.  EVAL: the digits are generated inside the forward transform's load where such a
// kernel exists (no COEFF digit matrix is written), else the plain kernel followed by the transform.
static int decompose_segment(GpuContext *ctx, void *out, const void *coeff, size_t nsrc, size_t cols, size_t L, size_t k,
                             uint32_t towers, uint32_t dpt, uint32_t base_bits, size_t ky, uint32_t td0, bool eval) {
    const size_t out_vectors = nsrc * ky * cols * L;
    if (eval) {
        const int frc = ctx->wide ? launch_ntt_digits_u64(ctx, static_cast<uint64_t *>(out), static_cast<const uint64_t *>(coeff), out_vectors,
                                                          static_cast<uint32_t>(L), (uint32_t)cols, towers, dpt, base_bits, ky, td0)
                                  : launch_ntt_digits_u32(ctx, static_cast<uint32_t *>(out), static_cast<const uint32_t *>(coeff), out_vectors,
                                                          static_cast<uint32_t>(L), (uint32_t)cols, towers, dpt, base_bits, ky, td0);
        if (frc >= 0) return frc;
    }
    if (td0 == 0 && ky == k) {  // every digit row: each source residue is read once for all its digits
        const size_t polys = nsrc * cols;
        const dim3 blocks = item_grid(polys * towers * static_cast<size_t>(ctx->N), 256);
        if (ctx->wide)
            MXX_LAUNCH(decompose_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(out),
                       static_cast<const uint64_t *>(coeff), ctx->d_limbs, polys, (uint32_t)cols, (uint32_t)L, (uint32_t)ctx->N, towers,
                       dpt, base_bits, k);
        else
            MXX_LAUNCH(decompose_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(out),
                       static_cast<const uint32_t *>(coeff), ctx->d_limbs, polys, (uint32_t)cols, (uint32_t)L, (uint32_t)ctx->N, towers,
                       dpt, base_bits, k);
    } else {
        const dim3 blocks = item_grid(nsrc * ky * cols * static_cast<size_t>(ctx->N), 256);
        if (ctx->wide)
            MXX_LAUNCH(decompose_rows_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(out),
                       static_cast<const uint64_t *>(coeff), ctx->d_limbs, nsrc, (uint32_t)cols, (uint32_t)L, (uint32_t)ctx->N, dpt,
                       base_bits, (uint32_t)ky, td0);
        else
            MXX_LAUNCH(decompose_rows_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(out),
                       static_cast<const uint32_t *>(coeff), ctx->d_limbs, nsrc, (uint32_t)cols, (uint32_t)L, (uint32_t)ctx->N, dpt,
                       base_bits, (uint32_t)ky, td0);
    }
    HIP_TRY(hipGetLastError());
    // output honours the format it was created with (MatrixDecompose.cu:910-914,1318-1328)
    return eval ? launch_ntt(ctx, out, out_vectors, static_cast<int>(L), false) : 0;
}

// Rows [row_start, row_start + R) of G^-1 of the source rows at `coeff` (row 0 there = source row row_start / k), cut at
// source-row boundaries: the rest of the first source row, the source rows the window holds whole, the start of the
// last one - at most three launches, each with exactly one workgroup set per window row and none of the kernels
// dividing by k.  The whole matrix (row_start = 0, R = r k) is the middle piece alone: the one launch it always was.
static int decompose_window(GpuContext *ctx, void *out, const void *coeff, size_t cols, size_t L, size_t k, uint32_t towers,
                            uint32_t dpt, uint32_t base_bits, size_t row_start, size_t R, bool eval) {
    const size_t row_bytes = cols * L * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    char *o = static_cast<char *>(out);
    const char *c = static_cast<const char *>(coeff);
    const size_t first = row_start % k;
    size_t done = 0;
    if (first || R < k) {
        const size_t ky = std::min(R, k - first);
        if (int rc = decompose_segment(ctx, o, c, 1, cols, L, k, towers, dpt, base_bits, ky, static_cast<uint32_t>(first), eval)) return rc;
        done = ky;
        c += row_bytes;
    }
    if (const size_t whole = (R - done) / k) {
        if (int rc = decompose_segment(ctx, o + done * row_bytes, c, whole, cols, L, k, towers, dpt, base_bits, k, 0, eval)) return rc;
        done += whole * k;
        c += whole * row_bytes;
    }
    if (done < R) return decompose_segment(ctx, o + done * row_bytes, c, 1, cols, L, k, towers, dpt, base_bits, R - done, 0, eval);
    return 0;
}

// out (R x cols, checked by the caller together with everything else that can refuse) <- rows [row_start, row_start + R)
// of G^-1(src).  Digits are taken from coefficient-domain residues: of an EVAL source, the rows the window touches are
// inverse-transformed into scratch.
static int decompose_core(const GpuMatrix *src, uint32_t base_bits, bool small, size_t row_start, GpuMatrix *out) {
    GpuContext *ctx = src->ctx;
    const int requested = out->format;
    const size_t L = matrix_limbs(src), R = out->rows, cols = src->cols;
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (R == 0 || cols == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const size_t r0 = row_start / k, nsrc = (row_start + R - 1) / k - r0 + 1;
    const size_t row_bytes = cols * L * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    const void *coeff = static_cast<const char *>(words_ptr(src)) + r0 * row_bytes;
    CtxBlock tmp_block(ctx);  // back to the cache at scope exit (stream-ordered behind its readers), error paths included
    if (src->format == GPU_POLY_FORMAT_EVAL) {
        const size_t bytes = nsrc * row_bytes;
        if (tmp_block.alloc(bytes)) return 1;
        int rc = ctx->wide ? -1 : launch_intt_oop_u32(ctx, static_cast<uint32_t *>(tmp_block.ptr), static_cast<const uint32_t *>(coeff),
                                                      nsrc * cols * L, static_cast<uint32_t>(L));
        if (rc < 0) {  // no out-of-place transform for this context: copy, then in place
            MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * bytes,
                            HIP_TRY(hipMemcpyAsync(tmp_block.ptr, coeff, bytes, hipMemcpyDeviceToDevice, ctx->stream)));
            rc = launch_ntt(ctx, tmp_block.ptr, nsrc * cols * L, static_cast<int>(L), true);
        }
        if (rc) return rc;
        coeff = tmp_block.ptr;
    }
    const uint32_t towers = small ? 1u : static_cast<uint32_t>(L);
    const bool eval = requested == GPU_POLY_FORMAT_EVAL;
    const int rc = decompose_window(ctx, words_ptr(out), coeff, cols, L, k, towers, dpt, base_bits, row_start - r0 * k, R, eval);
    if (rc == 0) out->format = eval ? GPU_POLY_FORMAT_EVAL : GPU_POLY_FORMAT_COEFF;
    return rc;
}

static int decompose_impl(const GpuMatrix *src, uint32_t base_bits, GpuMatrix *out, bool small) {
    if (!src || !out) return set_error("gpu_matrix_decompose_base: null matrix");
    if (base_bits == 0) return set_error("base_bits must be non-zero in gpu_matrix_decompose_base");
    if (src->ctx != out->ctx || src->level != out->level)
        return set_error("context mismatch in gpu_matrix_decompose_base");
    if (storage_overlaps(src, out)) return set_error("gpu_matrix_decompose_base: output must not alias the source");
    const size_t L = matrix_limbs(src);
    const uint32_t dpt = (src->ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (out->rows != src->rows * k || out->cols != src->cols)
        return set_error("output size mismatch in gpu_matrix_decompose_base");
    return decompose_core(src, base_bits, small, 0, out);
}

extern "C" int gpu_matrix_fill_gadget(GpuMatrix *out, uint32_t base_bits) {
    ABI_GUARD_BEGIN
    return fill_gadget_impl(out, base_bits, false);
    ABI_GUARD_END
}

extern "C" int gpu_matrix_fill_small_gadget(GpuMatrix *out, uint32_t base_bits) {
    ABI_GUARD_BEGIN
    return fill_gadget_impl(out, base_bits, true);
    ABI_GUARD_END
}

extern "C" int gpu_matrix_decompose_base(const GpuMatrix *src, uint32_t base_bits, GpuMatrix *out) {
    ABI_GUARD_BEGIN
    return decompose_impl(src, base_bits, out, false);
    ABI_GUARD_END
}

extern "C" int gpu_matrix_decompose_base_small(const GpuMatrix *src, uint32_t base_bits, GpuMatrix *out) {
    ABI_GUARD_BEGIN
    return decompose_impl(src, base_bits, out, true);
    ABI_GUARD_END
}

extern "C" int gpu_matrix_fill_small_decomposed_identity_chunk(GpuMatrix *out, const GpuMatrix *scalar_by_digit,
                                                               size_t chunk_idx) {
    ABI_GUARD_BEGIN
    if (!out || !scalar_by_digit) return set_error("invalid gpu_matrix_fill_small_decomposed_identity_chunk arguments");
    if (out->ctx != scalar_by_digit->ctx || out->level != scalar_by_digit->level)
        return set_error("context mismatch in gpu_matrix_fill_small_decomposed_identity_chunk");
    if (out->rows != out->cols)
        return set_error("output must be square in gpu_matrix_fill_small_decomposed_identity_chunk");
    if (scalar_by_digit->rows != 1 || scalar_by_digit->cols == 0)
        return set_error("scalar_by_digit must be 1 x chunk_count in gpu_matrix_fill_small_decomposed_identity_chunk");
    if (out->format != scalar_by_digit->format)
        return set_error("format mismatch in gpu_matrix_fill_small_decomposed_identity_chunk");
    const size_t size = out->rows, chunk_count = scalar_by_digit->cols;
    if (chunk_idx >= chunk_count)
        return set_error("chunk_idx out of range in gpu_matrix_fill_small_decomposed_identity_chunk");
    if (storage_overlaps(out, scalar_by_digit))
        return set_error("gpu_matrix_fill_small_decomposed_identity_chunk: output must not alias scalar_by_digit");
    if (size == 0) return 0;
    if (size > 65535) return set_error("gpu_matrix_fill_small_decomposed_identity_chunk: size too large");
    GpuContext *ctx = out->ctx;
    if (ctx_activate(ctx)) return 1;
    HIP_TRY(hipMemsetAsync(words_ptr(out), 0, out->bytes, ctx->stream));
    const size_t wpp = matrix_limbs(out) * static_cast<size_t>(ctx->N);
    const unsigned gx = static_cast<unsigned>(std::min<size_t>((wpp + 255) / 256, 64));
    dim3 grid(gx, static_cast<unsigned>(size));
    if (ctx->wide)
        MXX_LAUNCH(identity_chunk_kernel<uint64_t>, grid, dim3(256), 0, ctx->stream,
                           static_cast<uint64_t *>(words_ptr(out)), static_cast<const uint64_t *>(words_ptr(scalar_by_digit)),
                           size, chunk_idx, chunk_count, wpp);
    else
        MXX_LAUNCH(identity_chunk_kernel<uint32_t>, grid, dim3(256), 0, ctx->stream,
                           static_cast<uint32_t *>(words_ptr(out)), static_cast<const uint32_t *>(words_ptr(scalar_by_digit)),
                           size, chunk_idx, chunk_count, wpp);
    HIP_TRY(hipGetLastError());
    return 0;
    ABI_GUARD_END
}

// Extension: G^-1 of a freshly sampled matrix in one call.  The reference samples (coefficients -> NTT), then
// decomposes (INTT of a copy -> digits -> NTT): src/sampler/gpu.rs:91-115 (`sample_hash_decomposed`,
// `sample_hash_small_decomposed`).  Here the samples stay coefficients and go straight into the digit transform:
// the source's NTT, its copy and its INTT are never run.  `out` is (rows * k) x cols, created EVAL or COEFF like
// the output of gpu_matrix_decompose_base; the samples are those of gpu_matrix_sample_distribution(rows x cols).
extern "C" int gpupoly_matrix_sample_decomposed(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed,
                                                uint32_t base_bits, int small) {
    ABI_GUARD_BEGIN
    if (!out) return set_error("gpupoly_matrix_sample_decomposed: null matrix");
    if (base_bits == 0) return set_error("base_bits must be non-zero in gpupoly_matrix_sample_decomposed");
    GpuContext *ctx = out->ctx;
    const size_t L = matrix_limbs(out);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (out->rows % k) return set_error("gpupoly_matrix_sample_decomposed: output rows must be a multiple of the digit count");
    GpuMatrix src;
    src.ctx = ctx;
    src.level = out->level;
    src.rows = out->rows / k;
    src.cols = out->cols;
    src.bytes = src.rows * src.cols * L * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    if (matrix_polys(&src) == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    CtxBlock block(ctx);
    if (block.alloc(src.bytes)) return 1;
    src.storage = block.ptr;
    src.borrowed = true;  // the block is this scope's: never swapped for packed storage
    int rc = sample_impl(&src, dist_type, sigma, seed, src.cols, 0, true);
    if (rc == 0) rc = decompose_impl(&src, base_bits, out, small != 0);
    return rc;
    ABI_GUARD_END
}

// ---- row windows of a decomposition ----------------------------------------------------------------------------------
// Every production caller of the decomposed hash samples asks for a window: a column chunk of the conceptual d x m_g
// matrix (src/lookup/ggh15/pubkey_gpu.rs:398-407,495-504, poly_encoding_gpu.rs:453-462,520-543), of which
// poly_encoding_gpu.rs:515,566 keep only rows [inner_start, inner_start + inner_len).  The digit transforms are the cost
// of a decomposition, so both entries run them for the window's rows only, and touch (inverse-transform / sample) only
// the source rows - for uniform samples, only the towers - those rows are digits of.
static size_t window_digit_count(const GpuMatrix *out, uint32_t base_bits, int small) {
    const uint32_t dpt = (out->ctx->crt_bits + base_bits - 1) / base_bits;
    return small ? dpt : static_cast<size_t>(dpt) * matrix_limbs(out);
}

extern "C" int gpupoly_matrix_decompose_rows(const GpuMatrix *src, uint32_t base_bits, int small, size_t row_start,
                                             GpuMatrix *out) {
    ABI_GUARD_BEGIN
    if (!src || !out) return set_error("gpupoly_matrix_decompose_rows: null matrix");
    if (base_bits == 0 || base_bits >= 63) return set_error("gpupoly_matrix_decompose_rows: base_bits must be in 1..62");
    if (src->ctx != out->ctx) return set_error("gpupoly_matrix_decompose_rows: context mismatch");
    if (src->level != out->level) return set_error("gpupoly_matrix_decompose_rows: level mismatch");
    if (src->cols != out->cols) return set_error("gpupoly_matrix_decompose_rows: column count mismatch");
    const size_t k = window_digit_count(out, base_bits, small);
    const size_t total = src->rows * k;
    if (row_start > total || out->rows > total - row_start)
        return set_error("gpupoly_matrix_decompose_rows: row window past the decomposition's rows");
    if (storage_overlaps(src, out)) return set_error("gpupoly_matrix_decompose_rows: output must not overlap the source");
    return decompose_core(src, base_bits, small != 0, row_start, out);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_sample_decomposed_window(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed,
                                                       uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                                       size_t col_offset, size_t row_start) {
    ABI_GUARD_BEGIN
    if (!out) return set_error("gpupoly_matrix_sample_decomposed_window: null matrix");
    if (base_bits == 0 || base_bits >= 63) return set_error("gpupoly_matrix_sample_decomposed_window: base_bits must be in 1..62");
    if (dist_type < GPU_MATRIX_DIST_UNIFORM || dist_type > GPU_MATRIX_DIST_TERNARY)
        return set_error("gpupoly_matrix_sample_decomposed_window: invalid dist_type");
    if (dist_type == GPU_MATRIX_DIST_GAUSS && !(sigma > 0.0))
        return set_error("gpupoly_matrix_sample_decomposed_window: sigma must be positive for Gaussian sampling");
    if (col_offset > full_ncol || out->cols > full_ncol - col_offset)
        return set_error("gpupoly_matrix_sample_decomposed_window: column window past full_ncol");
    GpuContext *ctx = out->ctx;
    const size_t L = matrix_limbs(out);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = window_digit_count(out, base_bits, small);
    if (src_rows > ~size_t(0) / k || row_start > src_rows * k || out->rows > src_rows * k - row_start)
        return set_error("gpupoly_matrix_sample_decomposed_window: row window past the decomposition's rows");
    // the stream ids of the whole conceptual matrix (sample_impl's rule)
    if (full_ncol && src_rows > ((size_t(1) << 48) - 2) / full_ncol)
        return set_error("gpupoly_matrix_sample_decomposed_window: matrix too large for the RNG's 48-bit stream ids");
    const size_t R = out->rows;
    if (R == 0 || out->cols == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    const size_t r0 = row_start / k, r1 = (row_start + R - 1) / k;
    if (dist_type == GPU_MATRIX_DIST_GAUSS && ((r1 - r0 + 1) * out->cols) >> 32)
        return set_error("gpupoly_matrix_sample_decomposed_window: too many polynomials");
    GpuMatrix src;
    src.ctx = ctx;
    src.level = out->level;
    src.rows = r1 - r0 + 1;
    src.cols = out->cols;
    src.bytes = src.rows * src.cols * L * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    if (ctx_activate(ctx)) return 1;
    CtxBlock block(ctx);
    if (block.alloc(src.bytes)) return 1;
    src.storage = block.ptr;
    src.borrowed = true;  // the block is this scope's: never swapped for packed storage
    // the towers whose digits the window holds: a contiguous run when it lies inside one source row
    uint32_t t0 = 0, tn = small ? 1u : static_cast<uint32_t>(L);
    if (r0 == r1) {
        t0 = static_cast<uint32_t>((row_start - r0 * k) / dpt);
        tn = static_cast<uint32_t>((row_start + R - 1 - r0 * k) / dpt) - t0 + 1;
    }
    int rc = sample_impl(&src, dist_type, sigma, seed, full_ncol, col_offset, true, r0, t0, tn);
    if (rc == 0) rc = decompose_core(&src, base_bits, small != 0, row_start - r0 * k, out);
    return rc;
    ABI_GUARD_END
}

// ---- decomposed blocks: G^-1 of many independently seeded samples in one call -------------------
// out = [D_0 | D_1 | ...], D_t = what gpupoly_matrix_sample_decomposed_window writes for the whole decomposition (row_start
// 0) of the window [col_offset, col_offset + c) under block t's seed.  The seeded-blocks sampler (sampling.hip) writes the
// src_rows x (nblk c) coefficients into scratch, its table resolving a polynomial to (block, position in the block's
// conceptual src_rows x full_ncol matrix); G^-1 works column by column, so one decompose_core over the wide scratch gives
// every block.  The launches are the sampler's (hash, sub-keys, samples) and the digit transform's: none depends on nblk.
int sample_decomposed_blocks_impl(const char *entry, bool hashed, GpuMatrix *out, int dist_type, const GpuRngSeed *seeds,
                                  const GpuHashTags *tags, size_t nblk, uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                  size_t col_offset) {
    const auto refuse = [entry](const char *what) { return set_error(std::string(entry) + what); };
    if (!out) return refuse(": null matrix");
    if (base_bits == 0 || base_bits >= 63) return refuse(": base_bits must be in 1..62");
    if (nblk == 0 || nblk > (size_t(1) << 20)) return refuse(": the block count must be 1..2^20");
    if (out->cols % nblk) return refuse(": the matrix's columns are not a multiple of the block count");
    const size_t c = out->cols / nblk;
    if (col_offset > full_ncol || c > full_ncol - col_offset) return refuse(": column window past full_ncol");
    const size_t k = window_digit_count(out, base_bits, small);
    if (src_rows > ~size_t(0) / k || out->rows != src_rows * k) return refuse(": the matrix's rows must be src_rows times the digit count");
    // the stream ids of a block's whole conceptual matrix (sample_impl's rule)
    if (full_ncol && src_rows > ((size_t(1) << 48) - 2) / full_ncol) return refuse(": matrix too large for the RNG's 48-bit stream ids");
    GpuContext *ctx = out->ctx;
    GpuMatrix src;
    src.ctx = ctx;
    src.level = out->level;
    src.rows = src_rows;
    src.cols = out->cols;
    src.bytes = src.rows * src.cols * matrix_limbs(out) * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    src.borrowed = true;  // the block below is this scope's: never swapped for packed storage
    const RngBlockWindow win{c, full_ncol, col_offset};
    CtxBlock block(ctx);
    if (matrix_polys(&src)) {  // an empty output still goes through the sampler's refusals, which launch nothing
        if (ctx_activate(ctx)) return 1;
        if (block.alloc(src.bytes)) return 1;
        src.storage = block.ptr;
    }
    if (int rc = sample_blocks_impl(entry, hashed, &src, dist_type, seeds, tags, nblk, 0, nullptr, &win)) return rc;
    if (matrix_polys(&src) == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    return decompose_core(&src, base_bits, small != 0, 0, out);
}

extern "C" int gpupoly_matrix_sample_decomposed_blocks(GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, size_t nblk,
                                                       uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                                       size_t col_offset) {
    ABI_GUARD_BEGIN
    return sample_decomposed_blocks_impl("gpupoly_matrix_sample_decomposed_blocks", false, out, dist_type, seeds, nullptr, nblk, base_bits, small,
                                         src_rows, full_ncol, col_offset);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_sample_hash_decomposed_blocks(GpuMatrix *out, int dist_type, const GpuHashTags *tags, size_t nblk,
                                                            uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                                            size_t col_offset) {
    ABI_GUARD_BEGIN
    return sample_decomposed_blocks_impl("gpupoly_matrix_sample_hash_decomposed_blocks", true, out, dist_type, nullptr, tags, nblk, base_bits,
                                         small, src_rows, full_ncol, col_offset);
    ABI_GUARD_END
}
