// serde.hip — compact wire format: coefficient-domain, CRT-reconstructed, centred integers,
// bit-packed at the matrix-wide maximum width.  Replaces the compact-bytes half of
// cuda/src/matrix/MatrixSerde.cu (ABI: cuda/include/matrix/MatrixSerde.cuh:35-58).
//
// Format (MatrixSerde.cu:280-456,1535-1627; Rust header src/matrix/gpu_dcrt_poly.rs:956-1044):
//   coefficient idx = poly*N + i occupies bits [idx*w, (idx+1)*w) of a little-endian bit
//   stream; its low w-1 bits are |x| and bit w-1 is the sign, where x is the representative
//   of the coefficient in (-Q/2, Q/2] (negative iff value > floor(Q/2)), Q = q_0..q_level;
//   w = max_coeff_bits = 1 + max bit-width of |x| over the matrix (0 for the zero matrix),
//   bytes_per_coeff = ceil(w/8), payload_len = ceil(polys*N*w/8).
//
// Device pipeline: one thread per coefficient does Garner mixed-radix CRT from the limb
// residues (inverse table built at context creation, as Runtime.cu:77-96), Horner-evaluates
// the multi-word integer, centres it, and (pass 1) contributes to the max bit-width or
// (pass 2) ORs its w bits into the zeroed payload.  Nothing is staged per coefficient in HBM:
// the value is recomputed in pass 2 (O(L^2) modmuls, cheaper than a round trip of L words).
#include "centred.h"
#include "common.h"
#include "crt.h"
#include "modarith.h"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

template <typename W, int ML>
__global__ void __launch_bounds__(256) compact_maxbits_fast_kernel(const W *__restrict__ src, size_t polys, uint32_t N, SerdeConsts sc,
                                            const uint64_t *__restrict__ garner, size_t garner_stride,
                                            const LimbConst *__restrict__ limbs, unsigned int *__restrict__ max_and_flag) {
    // grid-stride: a few thousand workgroups keep a running maximum in registers and touch the shared word once each (a
    // read of that ONE word per wave - 280 000 of them for an M3A preimage - was 0.2 of this kernel's 0.32 ms)
    const size_t total = polys * N, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    unsigned int bits = 0;
    for (size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        uint64_t lo, hi;
        bool neg;
        if (reconstruct_small<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, lo, hi, neg))
            bits = max(bits, hi ? 128u - static_cast<uint32_t>(__clzll(hi)) : (lo ? 64u - static_cast<uint32_t>(__clzll(lo)) : 0u));
        else
            max_and_flag[1] = 1u;  // some coefficient needs the general path: the host reruns with the general kernels
    }
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, __shfl_down(bits, off));
    if ((threadIdx.x & 63) == 0 && bits > __atomic_load_n(max_and_flag, __ATOMIC_RELAXED)) atomicMax(max_and_flag, bits);
}

// width <= 130 here (|x| below 2^102 at most); the block's 8 * width payload words are assembled in LDS as in the general form
template <typename W, int ML>
__global__ void __launch_bounds__(256) compact_pack_fast_kernel(const W *__restrict__ src, size_t polys, uint32_t N, SerdeConsts sc,
                                         const uint64_t *__restrict__ garner, size_t garner_stride,
                                         const LimbConst *__restrict__ limbs, uint32_t width, uint32_t *__restrict__ payload_words,
                                         size_t payload_word_count) {
    extern __shared__ uint32_t pack_words[];
    const size_t idx = item_index();
    const size_t block_first = idx - threadIdx.x;
    const uint32_t nwords = 8u * width;
    for (uint32_t w = threadIdx.x; w < nwords; w += 256) pack_words[w] = 0;
    __syncthreads();
    if (idx < polys * N) {
        uint64_t lo, hi;
        bool neg;
        (void)reconstruct_small<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, lo, hi, neg);
        // 192 bits: |x| in words 0..1, the sign bit at width - 1 (at most bit 129)
        uint64_t x0 = lo, x1 = hi, x2 = 0;
        if (neg) {
            const uint32_t sb = width - 1;
            const uint64_t bit = 1ull << (sb & 63);
            if (sb < 64) x0 |= bit;
            else if (sb < 128) x1 |= bit;
            else x2 |= bit;
        }
        const uint32_t base = threadIdx.x * width;
        uint32_t done = 0;
        while (done < width) {
            const uint32_t bit = base + done;
            const uint32_t off = bit & 31u;
            const uint32_t take = min(32u - off, width - done);
            const uint32_t wi = done >> 6, bo = done & 63u;
            const uint64_t cur = wi == 0 ? x0 : (wi == 1 ? x1 : x2), nxt = wi == 0 ? x1 : (wi == 1 ? x2 : 0ull);
            uint64_t chunk = cur >> bo;
            if (bo + take > 64) chunk |= nxt << (64 - bo);
            const uint32_t val = static_cast<uint32_t>(chunk & ((take == 32) ? 0xffffffffull : ((1ull << take) - 1)));
            if (val) atomicOr(&pack_words[bit >> 5], val << off);
            done += take;
        }
    }
    __syncthreads();
    const size_t first_word = block_first / 256 * nwords;
    for (uint32_t w = threadIdx.x; w < nwords; w += 256)
        if (first_word + w < payload_word_count) payload_words[first_word + w] = pack_words[w];
}

template <typename W, int ML>
__global__ void compact_maxbits_kernel(const W *__restrict__ src, size_t polys, uint32_t N, SerdeConsts sc,
                                       const uint64_t *__restrict__ garner, size_t garner_stride,
                                       const LimbConst *__restrict__ limbs, unsigned int *__restrict__ max_bits) {
    const size_t idx = item_index();
    unsigned int bits = 0;
    if (idx < polys * N) {
        uint64_t x[ML];
        bool neg;
        bits = reconstruct_centered<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, x, neg);
    }
    // wave-level max; the atomic only when this wave would raise the running maximum.  (One unconditional atomic per wave
    // was 280 000 read-modify-writes of ONE word for an M3A preimage - serialised in L2, 3.2 ms, the whole kernel; after the
    // first waves the plain read sees the final width and nearly every wave skips it.)
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, __shfl_down(bits, off));
    if ((threadIdx.x & 63) == 0 && bits > __atomic_load_n(max_bits, __ATOMIC_RELAXED)) atomicMax(max_bits, bits);
}

// A block of 256 coefficients fills exactly 8 * width payload words (256 * width bits, word-aligned for every width), so
// the block assembles them in LDS - 32-bit ORs on shared memory - and writes them out whole, coalesced: no global atomics
// and no memset of the payload (round 2's form ORed every coefficient's two or three pieces into global words: 0.73 ms
// for an M3A preimage against the 0.09 ms of reading it).  Widths beyond kPackLdsWidth bits per coefficient (Q above
// 2^1023) keep the global-atomic form on a zeroed payload.
static constexpr uint32_t kPackLdsWidth = 1024;  // 8 * 1024 words = 32 KB of LDS
template <typename W, int ML, bool LDS>
__global__ void __launch_bounds__(256) compact_pack_kernel(const W *__restrict__ src, size_t polys, uint32_t N, SerdeConsts sc,
                                    const uint64_t *__restrict__ garner, size_t garner_stride,
                                    const LimbConst *__restrict__ limbs, uint32_t width, uint32_t *__restrict__ payload_words,
                                    size_t payload_word_count) {
    extern __shared__ uint32_t pack_words[];  // LDS form: 8 * width words
    const size_t idx = item_index();
    const size_t block_first = idx - threadIdx.x;
    const uint32_t nwords = 8u * width;
    if constexpr (LDS) {
        for (uint32_t w = threadIdx.x; w < nwords; w += 256) pack_words[w] = 0;
        __syncthreads();
    }
    if (idx < polys * N) {
        uint64_t x[ML + 1];  // words of |x| (at most one per limb) + one for the sign bit / the shifted read below
        bool neg;
        reconstruct_centered<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, x, neg);
        // set the sign bit at position width-1
        const uint32_t sb = width - 1;
        for (int w = sc.words; w <= ML; ++w) x[w] = 0;
        if (neg) x[sb >> 6] |= 1ull << (sb & 63);
        // OR the `width` bits into the stream at bit offset idx*width, 32 bits at a time
        const size_t base = LDS ? static_cast<size_t>(threadIdx.x) * width : idx * static_cast<size_t>(width);
        uint32_t done = 0;
        while (done < width) {
            const size_t bit = base + done;
            const uint32_t off = static_cast<uint32_t>(bit & 31);
            const uint32_t take = min(32u - off, width - done);
            const uint32_t wi = done >> 6, bo = done & 63;
            uint64_t chunk = x[wi] >> bo;
            if (bo + take > 64) chunk |= x[wi + 1] << (64 - bo);
            const uint32_t val = static_cast<uint32_t>(chunk & ((take == 32) ? 0xffffffffull : ((1ull << take) - 1)));
            if (val) {
                if constexpr (LDS) atomicOr(&pack_words[bit >> 5], val << off);
                else atomicOr(&payload_words[bit >> 5], val << off);
            }
            done += take;
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        const size_t first_word = block_first / 256 * nwords;  // block_first is a multiple of 256
        for (uint32_t w = threadIdx.x; w < nwords; w += 256)
            if (first_word + w < payload_word_count) payload_words[first_word + w] = pack_words[w];
    }
}

// 32 bits of the payload starting at bit `bit` (little-endian bit stream); the payload is padded by 8 bytes
__device__ __forceinline__ uint32_t payload_bits32(const uint8_t *__restrict__ payload, size_t bit) {
    const size_t byte = bit >> 3;
    uint64_t v = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) v |= static_cast<uint64_t>(payload[byte + b]) << (8 * b);
    return static_cast<uint32_t>(v >> (bit & 7));
}

// |x| arrives as `mag_bits` bits; every limb reduces it 32 bits at a time, most significant first:
// r <- (r 2^32 + word) mod q, one multiply-high by floor(2^64 / q) per step for word-sized moduli (the first form
// reduced a 128-bit value with `%` for every byte of every limb)
template <typename W>
__global__ void compact_unpack_kernel(W *__restrict__ dst, const uint8_t *__restrict__ payload, size_t polys,
                                      uint32_t N, SerdeConsts sc, const LimbConst *__restrict__ limbs, uint32_t width) {
    const size_t idx = item_index();
    if (idx >= polys * N) return;
    const size_t poly = idx / N;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const int L = sc.limbs;
    if (width == 0) {
        for (int l = 0; l < L; ++l) dst[(poly * L + l) * N + i] = 0;
        return;
    }
    const size_t base = idx * static_cast<size_t>(width);
    const uint32_t mag_bits = width - 1;
    const size_t sbit = base + mag_bits;
    const bool neg = (payload[sbit >> 3] >> (sbit & 7)) & 1u;
    const uint32_t words = (mag_bits + 31) / 32, top_bits = mag_bits - (words - 1) * 32;  // top_bits in 1..32 (words >= 1)
    for (int l = 0; l < L; ++l) {
        const LimbConst lc = limbs[l];
        const uint64_t q = lc.q;
        uint64_t r = 0;
        for (uint32_t j = words; j-- > 0;) {
            uint32_t w = payload_bits32(payload, base + 32u * j);
            if (j == words - 1 && top_bits < 32) w &= (1u << top_bits) - 1u;
            if constexpr (sizeof(W) == 4) {
                const uint64_t x = (r << 32) | w;  // r < q < 2^31
                r = x - __umul64hi(x, lc.mu64) * q;
                if (r >= q) r -= q;
            } else {
                const u128_t x = (static_cast<u128_t>(r) << 32) | w;
                r = lc.kbits >= 32 ? barrett_reduce(x, q, lc.mu, lc.kbits) : static_cast<uint64_t>(x % q);
            }
        }
        if (mag_bits == 0) r = 0;
        if (neg && r) r = q - r;
        dst[(poly * L + l) * N + i] = static_cast<W>(r);
    }
}

extern "C" int gpu_matrix_store_compact_bytes(GpuMatrix *mat, uint8_t *payload_out, size_t payload_capacity,
                                              uint16_t *out_max_coeff_bits, uint16_t *out_bytes_per_coeff,
                                              size_t *out_payload_len) {
    ABI_GUARD_BEGIN
    if (!mat || !out_max_coeff_bits || !out_bytes_per_coeff || !out_payload_len)
        return set_error("invalid gpu_matrix_store_compact_bytes arguments");
    *out_max_coeff_bits = 0;
    *out_bytes_per_coeff = 0;
    *out_payload_len = 0;
    GpuContext *ctx = mat->ctx;
    const size_t polys = matrix_polys(mat);
    if (polys == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    // the matrix is converted to COEFF in place (MatrixSerde.cu:1108-1118); the Rust side
    // records the original tag and re-NTTs on load
    if (mat->format == GPU_POLY_FORMAT_EVAL) {
        int rc = gpu_matrix_intt_all(mat);
        if (rc) return rc;
    }
    SerdeConsts sc;
    if (build_consts(mat, sc)) return 1;
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const size_t coeffs = polys * N;
    const dim3 blocks = item_grid(coeffs, 256);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    CtxBlock max_block(ctx);
    if (max_block.alloc(2 * sizeof(unsigned int))) return 1;  // [0] running maximum of the widths, [1] "needs the general path"
    void *const d_max = max_block.ptr;
    HIP_TRY(hipMemsetAsync(d_max, 0, 2 * sizeof(unsigned int), ctx->stream));
    // fast-path-only kernels first (up to 16 limbs): preimages, trapdoors and Gaussian-sized keys never leave them
    bool fast = sc.limbs <= 16 && !ctx->env.serde_general;
    unsigned int h_mf[2] = {0, 0};
    if (fast) {
        const dim3 fast_blocks(static_cast<unsigned>(std::min<size_t>((coeffs + 255) / 256, 8192)));
#define FAST_MAXBITS(WT, ML)                                                                                             \
    MXX_LAUNCH((compact_maxbits_fast_kernel<WT, ML>), fast_blocks, dim3(256), 0, ctx->stream, static_cast<const WT *>(words_ptr(mat)), polys, N, sc, \
               ctx->d_garner, gstride, ctx->d_limbs, static_cast<unsigned int *>(d_max))
        if (ctx->wide) {
            if (sc.limbs <= 8) FAST_MAXBITS(uint64_t, 8);
            else FAST_MAXBITS(uint64_t, 16);
        } else {
            if (sc.limbs <= 8) FAST_MAXBITS(uint32_t, 8);
            else FAST_MAXBITS(uint32_t, 16);
        }
#undef FAST_MAXBITS
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_mf, d_max, sizeof(h_mf), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (h_mf[1]) {  // a coefficient beyond the fast paths: start over with the general kernels
            fast = false;
            HIP_TRY(hipMemsetAsync(d_max, 0, 2 * sizeof(unsigned int), ctx->stream));
        }
    }
#define SERDE_LAUNCH(KERNEL, WT, ...)                                                                                  \
    do {                                                                                                               \
        if (sc.limbs <= 8) MXX_LAUNCH((KERNEL<WT, 8>), blocks, dim3(256), 0, ctx->stream, __VA_ARGS__);         \
        else if (sc.limbs <= 16) MXX_LAUNCH((KERNEL<WT, 16>), blocks, dim3(256), 0, ctx->stream, __VA_ARGS__);  \
        else MXX_LAUNCH((KERNEL<WT, 64>), blocks, dim3(256), 0, ctx->stream, __VA_ARGS__);                      \
    } while (0)
    unsigned int h_max = h_mf[0];
    if (!fast) {
        if (ctx->wide)
            SERDE_LAUNCH(compact_maxbits_kernel, uint64_t, static_cast<const uint64_t *>(words_ptr(mat)), polys, N, sc, ctx->d_garner,
                         gstride, ctx->d_limbs, static_cast<unsigned int *>(d_max));
        else
            SERDE_LAUNCH(compact_maxbits_kernel, uint32_t, static_cast<const uint32_t *>(words_ptr(mat)), polys, N, sc, ctx->d_garner,
                         gstride, ctx->d_limbs, static_cast<unsigned int *>(d_max));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h_max, d_max, sizeof(h_max), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    const unsigned int width = h_max == 0 ? 0 : h_max + 1;
    if (width > 0xffffu) return set_error("centered max coeff bits exceed u16 range in gpu_matrix_store_compact_bytes");
    const unsigned int bytes_per_coeff = (width + 7) / 8;
    const size_t total_bits = coeffs * static_cast<size_t>(width);
    const size_t payload_len = (total_bits + 7) / 8;
    if (payload_len > payload_capacity) {
        // the caller learns the width and the length it needs (the reference reports only the error): a host that does not
        // want to pin the worst case - bits(Q) per coefficient - retries once with the exact size
        *out_max_coeff_bits = static_cast<uint16_t>(width);
        *out_bytes_per_coeff = static_cast<uint16_t>(bytes_per_coeff);
        *out_payload_len = payload_len;
        return set_error("payload buffer too small in gpu_matrix_store_compact_bytes");
    }
    if (payload_len > 0) {
        if (!payload_out) return set_error("null payload buffer in gpu_matrix_store_compact_bytes");
        const size_t padded = (payload_len + 3) / 4 * 4 + 4;
        CtxBlock payload_block(ctx);
        if (payload_block.alloc(padded)) return 1;
        void *const d_payload = payload_block.ptr;
        const bool in_lds = width <= kPackLdsWidth;
        if (!in_lds) HIP_TRY(hipMemsetAsync(d_payload, 0, padded, ctx->stream));
        const size_t pack_lds = in_lds ? 8u * width * sizeof(uint32_t) : 0;
        const size_t word_count = padded / 4;
#undef SERDE_LAUNCH
#define PACK_LAUNCH(WT, ML, LDSF)                                                                                       \
    MXX_LAUNCH((compact_pack_kernel<WT, ML, LDSF>), blocks, dim3(256), pack_lds, ctx->stream, static_cast<const WT *>(words_ptr(mat)), polys, N, sc, \
               ctx->d_garner, gstride, ctx->d_limbs, width, static_cast<uint32_t *>(d_payload), word_count)
#define PACK_BY_LIMBS(WT, LDSF)                       \
    do {                                              \
        if (sc.limbs <= 8) PACK_LAUNCH(WT, 8, LDSF);  \
        else if (sc.limbs <= 16) PACK_LAUNCH(WT, 16, LDSF); \
        else PACK_LAUNCH(WT, 64, LDSF);               \
    } while (0)
#define FAST_PACK(WT, ML)                                                                                                \
    MXX_LAUNCH((compact_pack_fast_kernel<WT, ML>), blocks, dim3(256), pack_lds, ctx->stream, static_cast<const WT *>(words_ptr(mat)), polys, N, sc, \
               ctx->d_garner, gstride, ctx->d_limbs, width, static_cast<uint32_t *>(d_payload), word_count)
        if (fast && in_lds) {
            if (ctx->wide) {
                if (sc.limbs <= 8) FAST_PACK(uint64_t, 8);
                else FAST_PACK(uint64_t, 16);
            } else {
                if (sc.limbs <= 8) FAST_PACK(uint32_t, 8);
                else FAST_PACK(uint32_t, 16);
            }
        } else if (ctx->wide) {
            if (in_lds) PACK_BY_LIMBS(uint64_t, true);
            else PACK_BY_LIMBS(uint64_t, false);
        } else {
            if (in_lds) PACK_BY_LIMBS(uint32_t, true);
            else PACK_BY_LIMBS(uint32_t, false);
        }
#undef FAST_PACK
#undef PACK_BY_LIMBS
#undef PACK_LAUNCH
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(payload_out, d_payload, payload_len, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *out_max_coeff_bits = static_cast<uint16_t>(width);
    *out_bytes_per_coeff = static_cast<uint16_t>(bytes_per_coeff);
    *out_payload_len = payload_len;
    return 0;
    ABI_GUARD_END
}

extern "C" int gpu_matrix_load_compact_bytes(GpuMatrix *mat, const uint8_t *payload, size_t payload_len,
                                             uint16_t max_coeff_bits) {
    ABI_GUARD_BEGIN
    if (!mat) return set_error("invalid gpu_matrix_load_compact_bytes arguments");
    GpuContext *ctx = mat->ctx;
    const size_t polys = matrix_polys(mat);
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const size_t coeffs = polys * N;
    if (max_coeff_bits == 0) {
        if (payload_len != 0) return set_error("payload_len must be zero when max_coeff_bits is zero");
    } else if (!payload && coeffs) {
        return set_error("null payload in gpu_matrix_load_compact_bytes");
    }
    const size_t expected = (coeffs * static_cast<size_t>(max_coeff_bits) + 7) / 8;
    if (payload_len != expected) return set_error("payload length mismatch in gpu_matrix_load_compact_bytes");
    mat->format = GPU_POLY_FORMAT_COEFF;
    if (coeffs == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    SerdeConsts sc;
    if (build_consts(mat, sc)) return 1;
    CtxBlock payload_block(ctx);
    if (payload_len) {
        if (payload_block.alloc(payload_len + 8)) return 1;  // payload_bits32 reads up to 4 bytes past a coefficient
        HIP_TRY(hipMemsetAsync(static_cast<uint8_t *>(payload_block.ptr) + payload_len, 0, 8, ctx->stream));
        HIP_TRY(hipMemcpyAsync(payload_block.ptr, payload, payload_len, hipMemcpyHostToDevice, ctx->stream));
    }
    void *const d_payload = payload_block.ptr;
    const dim3 blocks = item_grid(coeffs, 256);
    if (ctx->wide)
        MXX_LAUNCH(compact_unpack_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream,
                           static_cast<uint64_t *>(words_ptr(mat)), static_cast<const uint8_t *>(d_payload), polys, N, sc,
                           ctx->d_limbs, static_cast<uint32_t>(max_coeff_bits));
    else
        MXX_LAUNCH(compact_unpack_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream,
                           static_cast<uint32_t *>(words_ptr(mat)), static_cast<const uint8_t *>(d_payload), polys, N, sc,
                           ctx->d_limbs, static_cast<uint32_t>(max_coeff_bits));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like the reference; payload may be freed by the caller
    return 0;
    ABI_GUARD_END
}

// ---- many matrices per call (gpupoly_matrix_store_compact_bytes_many / _load_) -----------------------------------------
// The one-matrix entries above are launch and synchronise latency for a small matrix (three launches, two synchronises
// for a 76 x 4 preimage at n = 256).  Here up to kSerdeGroup matrices of one level share a launch: the table below is a
// kernel argument, a workgroup finds its matrix by a binary search on wave-uniform values (scalar unit, as request_of in
// preimage.hip) and then does what the one-matrix fast kernels do, at that matrix's OWN width.
constexpr uint32_t kSerdeGroup = 32;                      // 1.3 KB of table next to SerdeConsts' 1.5 KB in the 4 KB argument block
constexpr size_t kSerdeGroupBlocks = size_t(1) << 22;     // workgroups per launch (HIP: grid x block below 2^32)
constexpr size_t kLoadDirectBytes = size_t(1) << 20;      // load: payloads from this size on are copied from where they lie

struct SerdeSegments {
    uint32_t count;
    uint32_t first_block[kSerdeGroup + 1];  // matrix j owns workgroups [first_block[j], first_block[j + 1])
    uint32_t width[kSerdeGroup];            // pack / unpack: max_coeff_bits of matrix j
    void *base[kSerdeGroup];                // its words
    uint64_t coeffs[kSerdeGroup];           // polys * N
    uint64_t offset[kSerdeGroup];           // width pass: j's position in the call (its max / flag pair); pack: first 32-bit
                                            // word of its payload in the staging block; unpack: first byte
    uint64_t words[kSerdeGroup];            // pack: the 32-bit words that are j's to write (payload + padding to 8 bytes)
};

__device__ __forceinline__ uint32_t segment_of(const SerdeSegments &t, uint32_t block) {
    uint32_t lo = 0, hi = t.count;  // first_block[lo] <= block < first_block[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (block >= t.first_block[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// compact_maxbits_fast_kernel per matrix: j's workgroups stride over j's coefficients with a running maximum in registers;
// max_and_flag[2p] / [2p + 1] (p = j's position in the call) are touched only by a wave that would raise them (the reason
// is in compact_maxbits_kernel's comment)
template <typename W, int ML>
__global__ void __launch_bounds__(256) compact_maxbits_many_kernel(SerdeSegments t, uint32_t N, SerdeConsts sc,
                                            const uint64_t *__restrict__ garner, size_t garner_stride,
                                            const LimbConst *__restrict__ limbs, unsigned int *__restrict__ max_and_flag) {
    const uint32_t j = segment_of(t, blockIdx.x);
    const W *__restrict__ src = static_cast<const W *>(t.base[j]);
    const size_t total = t.coeffs[j];
    const size_t stride = static_cast<size_t>(t.first_block[j + 1] - t.first_block[j]) * 256;
    unsigned int *const mf = max_and_flag + 2 * t.offset[j];
    unsigned int bits = 0, general = 0;
    for (size_t idx = static_cast<size_t>(blockIdx.x - t.first_block[j]) * 256 + threadIdx.x; idx < total; idx += stride) {
        uint64_t lo, hi;
        bool neg;
        if (reconstruct_small<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, lo, hi, neg))
            bits = max(bits, hi ? 128u - static_cast<uint32_t>(__clzll(hi)) : (lo ? 64u - static_cast<uint32_t>(__clzll(lo)) : 0u));
        else
            general = 1u;  // this matrix needs the general path: the host reruns IT with the general kernels
    }
    for (int off = 32; off > 0; off >>= 1) {
        bits = max(bits, __shfl_down(bits, off));
        general |= __shfl_down(general, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bits > __atomic_load_n(mf, __ATOMIC_RELAXED)) atomicMax(mf, bits);
        if (general && !__atomic_load_n(mf + 1, __ATOMIC_RELAXED)) __atomic_store_n(mf + 1, 1u, __ATOMIC_RELAXED);
    }
}

// compact_pack_fast_kernel per matrix.  A matrix's first workgroup starts at its first coefficient, so every workgroup
// still assembles whole words (256 * width bits); of its last workgroup only the words below words[j] are stored - the
// payload and its zero padding to 8 bytes - because the next matrix's payload starts right there.
template <typename W, int ML>
__global__ void __launch_bounds__(256) compact_pack_many_kernel(SerdeSegments t, uint32_t N, SerdeConsts sc,
                                         const uint64_t *__restrict__ garner, size_t garner_stride,
                                         const LimbConst *__restrict__ limbs, uint32_t *__restrict__ staging_words) {
    extern __shared__ uint32_t pack_words[];
    const uint32_t j = segment_of(t, blockIdx.x);
    const W *__restrict__ src = static_cast<const W *>(t.base[j]);
    const uint32_t width = t.width[j];
    const size_t block = blockIdx.x - t.first_block[j];
    const size_t idx = block * 256 + threadIdx.x;
    const uint32_t nwords = 8u * width;
    for (uint32_t w = threadIdx.x; w < nwords; w += 256) pack_words[w] = 0;
    __syncthreads();
    if (idx < t.coeffs[j]) {
        uint64_t lo, hi;
        bool neg;
        (void)reconstruct_small<W, ML>(src, idx / N, static_cast<uint32_t>(idx % N), N, sc, garner, garner_stride, limbs, lo, hi, neg);
        uint64_t x0 = lo, x1 = hi, x2 = 0;
        if (neg) {
            const uint32_t sb = width - 1;
            const uint64_t bit = 1ull << (sb & 63);
            if (sb < 64) x0 |= bit;
            else if (sb < 128) x1 |= bit;
            else x2 |= bit;
        }
        const uint32_t base = threadIdx.x * width;
        uint32_t done = 0;
        while (done < width) {
            const uint32_t bit = base + done;
            const uint32_t off = bit & 31u;
            const uint32_t take = min(32u - off, width - done);
            const uint32_t wi = done >> 6, bo = done & 63u;
            const uint64_t cur = wi == 0 ? x0 : (wi == 1 ? x1 : x2), nxt = wi == 0 ? x1 : (wi == 1 ? x2 : 0ull);
            uint64_t chunk = cur >> bo;
            if (bo + take > 64) chunk |= nxt << (64 - bo);
            const uint32_t val = static_cast<uint32_t>(chunk & ((take == 32) ? 0xffffffffull : ((1ull << take) - 1)));
            if (val) atomicOr(&pack_words[bit >> 5], val << off);
            done += take;
        }
    }
    __syncthreads();
    const size_t first_word = block * nwords, own = t.words[j];
    uint32_t *__restrict__ out = staging_words + t.offset[j];
    for (uint32_t w = threadIdx.x; w < nwords; w += 256)
        if (first_word + w < own) out[first_word + w] = pack_words[w];
}

// compact_unpack_kernel per matrix: payload j starts at byte offset[j] of the staging block (bytes read past a payload's
// end fall into bits that are shifted out or masked, as in the one-matrix form; the block is padded by 8 bytes)
template <typename W>
__global__ void __launch_bounds__(256) compact_unpack_many_kernel(SerdeSegments t, const uint8_t *__restrict__ staging, uint32_t N,
                                                                  SerdeConsts sc, const LimbConst *__restrict__ limbs) {
    const uint32_t j = segment_of(t, blockIdx.x);
    const size_t idx = static_cast<size_t>(blockIdx.x - t.first_block[j]) * 256 + threadIdx.x;
    if (idx >= t.coeffs[j]) return;
    W *__restrict__ dst = static_cast<W *>(t.base[j]);
    const uint8_t *__restrict__ payload = staging + t.offset[j];
    const uint32_t width = t.width[j];
    const size_t poly = idx / N;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const int L = sc.limbs;
    if (width == 0) {
        for (int l = 0; l < L; ++l) dst[(poly * L + l) * N + i] = 0;
        return;
    }
    const size_t base = idx * static_cast<size_t>(width);
    const uint32_t mag_bits = width - 1;
    const size_t sbit = base + mag_bits;
    const bool neg = (payload[sbit >> 3] >> (sbit & 7)) & 1u;
    const uint32_t words = (mag_bits + 31) / 32, top_bits = mag_bits - (words - 1) * 32;
    for (int l = 0; l < L; ++l) {
        const LimbConst lc = limbs[l];
        const uint64_t q = lc.q;
        uint64_t r = 0;
        for (uint32_t k = words; k-- > 0;) {
            uint32_t w = payload_bits32(payload, base + 32u * k);
            if (k == words - 1 && top_bits < 32) w &= (1u << top_bits) - 1u;
            if constexpr (sizeof(W) == 4) {
                const uint64_t x = (r << 32) | w;
                r = x - __umul64hi(x, lc.mu64) * q;
                if (r >= q) r -= q;
            } else {
                const u128_t x = (static_cast<u128_t>(r) << 32) | w;
                r = lc.kbits >= 32 ? barrett_reduce(x, q, lc.mu, lc.kbits) : static_cast<uint64_t>(x % q);
            }
        }
        if (mag_bits == 0) r = 0;
        if (neg && r) r = q - r;
        dst[(poly * L + l) * N + i] = static_cast<W>(r);
    }
}

namespace {

// the general width / pack kernels for one matrix, launched as the one-matrix store launches them
template <typename W>
void general_maxbits(GpuContext *ctx, const GpuMatrix *mat, const SerdeConsts &sc, unsigned int *d_max) {
    const size_t polys = matrix_polys(mat), gstride = static_cast<size_t>(ctx->limb_count);
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const dim3 blocks = item_grid(polys * N, 256);
    const W *src = static_cast<const W *>(words_ptr(mat));
    if (sc.limbs <= 8) MXX_LAUNCH((compact_maxbits_kernel<W, 8>), blocks, dim3(256), 0, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, d_max);
    else if (sc.limbs <= 16) MXX_LAUNCH((compact_maxbits_kernel<W, 16>), blocks, dim3(256), 0, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, d_max);
    else MXX_LAUNCH((compact_maxbits_kernel<W, 64>), blocks, dim3(256), 0, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, d_max);
}

template <typename W, bool LDS>
void general_pack(GpuContext *ctx, const GpuMatrix *mat, const SerdeConsts &sc, uint32_t width, uint32_t *d_words, size_t word_count) {
    const size_t polys = matrix_polys(mat), gstride = static_cast<size_t>(ctx->limb_count);
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const dim3 blocks = item_grid(polys * N, 256);
    const size_t lds = LDS ? 8u * width * sizeof(uint32_t) : 0;
    const W *src = static_cast<const W *>(words_ptr(mat));
    if (sc.limbs <= 8) MXX_LAUNCH((compact_pack_kernel<W, 8, LDS>), blocks, dim3(256), lds, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, width, d_words, word_count);
    else if (sc.limbs <= 16) MXX_LAUNCH((compact_pack_kernel<W, 16, LDS>), blocks, dim3(256), lds, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, width, d_words, word_count);
    else MXX_LAUNCH((compact_pack_kernel<W, 64, LDS>), blocks, dim3(256), lds, ctx->stream, src, polys, N, sc, ctx->d_garner, gstride, ctx->d_limbs, width, d_words, word_count);
}

// a batched fast kernel over one group, by word size and limb bound
#define MANY_FAST_LAUNCH(KERNEL, limbs, grid, lds, ...)                                                                   \
    do {                                                                                                               \
        if (ctx->wide) {                                                                                               \
            if ((limbs) <= 8) MXX_LAUNCH((KERNEL<uint64_t, 8>), grid, dim3(256), lds, ctx->stream, __VA_ARGS__);       \
            else MXX_LAUNCH((KERNEL<uint64_t, 16>), grid, dim3(256), lds, ctx->stream, __VA_ARGS__);                   \
        } else {                                                                                                       \
            if ((limbs) <= 8) MXX_LAUNCH((KERNEL<uint32_t, 8>), grid, dim3(256), lds, ctx->stream, __VA_ARGS__);       \
            else MXX_LAUNCH((KERNEL<uint32_t, 16>), grid, dim3(256), lds, ctx->stream, __VA_ARGS__);                   \
        }                                                                                                              \
    } while (0)

struct ManyItem {
    GpuMatrix *mat = nullptr;
    size_t coeffs = 0, blocks = 0;  // blocks: workgroups of 256 coefficients
    bool batched = false;           // served by the segmented kernels
    unsigned int width = 0;
    size_t len = 0, offset = 0;     // payload bytes and where they start in the staging block
};

struct ManyGroup {
    int level = 0;
    size_t blocks = 0;
    std::vector<size_t> members;  // positions in the call, in argument order
};

// the checks both entries share; on success *out_ctx is the one context (null for n = 0)
int check_many(GpuMatrix *const *mats, size_t n, const char *who, GpuContext **out_ctx) {
    *out_ctx = nullptr;
    if (n == 0) return 0;
    if (!mats) return set_error(std::string("null matrix array in ") + who);
    for (size_t j = 0; j < n; ++j) {
        if (!mats[j]) return set_error(std::string("null matrix in ") + who);
        if (mats[j]->ctx != mats[0]->ctx) return set_error(std::string("matrices of different contexts in ") + who);
    }
    std::vector<const GpuMatrix *> sorted(mats, mats + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return set_error(std::string("the same matrix twice in ") + who);
    *out_ctx = mats[0]->ctx;
    return 0;
}

// batched items -> launch groups: one level per group, at most kSerdeGroup matrices and kSerdeGroupBlocks workgroups,
// argument order kept inside a level
std::vector<ManyGroup> group_by_level(const std::vector<ManyItem> &items) {
    std::vector<ManyGroup> groups;
    std::map<int, size_t> open;  // level -> its group that still takes members
    for (size_t j = 0; j < items.size(); ++j) {
        const ManyItem &it = items[j];
        if (!it.batched || it.coeffs == 0) continue;
        auto at = open.find(it.mat->level);
        if (at == open.end() || groups[at->second].members.size() == kSerdeGroup ||
            groups[at->second].blocks + it.blocks > kSerdeGroupBlocks) {
            groups.emplace_back();
            groups.back().level = it.mat->level;
            open[it.mat->level] = groups.size() - 1;
            at = open.find(it.mat->level);
        }
        groups[at->second].members.push_back(j);
        groups[at->second].blocks += it.blocks;
    }
    return groups;
}

const SerdeConsts *consts_of(std::map<int, SerdeConsts> &cache, const GpuMatrix *mat) {
    auto at = cache.find(mat->level);
    if (at == cache.end()) {
        at = cache.emplace(mat->level, SerdeConsts{}).first;
        if (build_consts(mat, at->second)) return nullptr;
    }
    return &at->second;
}

}  // namespace

extern "C" int gpupoly_matrix_store_compact_bytes_many(GpuMatrix *const *mats, size_t n, uint8_t *payload_out,
                                                       size_t payload_capacity, uint16_t *out_max_coeff_bits,
                                                       uint16_t *out_bytes_per_coeff, size_t *out_payload_offsets,
                                                       size_t *out_payload_lens, size_t *out_total_len) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_store_compact_bytes_many";
    if (!out_total_len) return set_error(std::string("null out_total_len in ") + who);
    if (n && (!out_max_coeff_bits || !out_bytes_per_coeff || !out_payload_offsets || !out_payload_lens))
        return set_error(std::string("null output array in ") + who);
    GpuContext *ctx = nullptr;
    if (check_many(mats, n, who, &ctx)) return 1;
    if (n == 0) {
        *out_total_len = 0;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const size_t gstride = static_cast<size_t>(ctx->limb_count);
    // inverse transforms first, back to back (the one-matrix entry converts in place too; the caller recorded the tags)
    for (size_t j = 0; j < n; ++j)
        if (mats[j]->format == GPU_POLY_FORMAT_EVAL) {
            const int rc = gpu_matrix_intt_all(mats[j]);
            if (rc) return rc;
        }
    std::vector<ManyItem> items(n);
    std::map<int, SerdeConsts> consts;
    for (size_t j = 0; j < n; ++j) {
        ManyItem &it = items[j];
        it.mat = mats[j];
        it.coeffs = matrix_polys(mats[j]) * N;
        it.blocks = (it.coeffs + 255) / 256;
        it.batched = mats[j]->level + 1 <= 16 && !ctx->env.serde_general && it.blocks <= kSerdeGroupBlocks;
        if (it.coeffs) {
            (void)words_ptr(mats[j]);  // a PACKED24 sample is unpacked here, before its address goes into a table
            if (!consts_of(consts, mats[j])) return 1;
        }
    }
    // ---- width pass: one launch per group, the general kernel for what the fast forms do not take; ONE copy, ONE synchronise
    CtxBlock mf_block(ctx);
    if (mf_block.alloc(2 * n * sizeof(unsigned int))) return 1;
    unsigned int *const d_mf = static_cast<unsigned int *>(mf_block.ptr);
    HIP_TRY(hipMemsetAsync(d_mf, 0, 2 * n * sizeof(unsigned int), ctx->stream));
    const std::vector<ManyGroup> groups = group_by_level(items);
    for (const ManyGroup &g : groups) {
        SerdeSegments t{};
        uint32_t at = 0;
        for (size_t j : g.members) {
            const uint32_t k = t.count++;
            t.first_block[k] = at;
            at += static_cast<uint32_t>(std::min<size_t>(items[j].blocks, 2048));  // grid-stride inside the matrix
            t.base[k] = words_ptr(mats[j]);
            t.coeffs[k] = items[j].coeffs;
            t.offset[k] = j;
        }
        t.first_block[t.count] = at;
        const SerdeConsts &sc = *consts_of(consts, mats[g.members[0]]);
        MANY_FAST_LAUNCH(compact_maxbits_many_kernel, sc.limbs, dim3(at), 0, t, N, sc, ctx->d_garner, gstride, ctx->d_limbs, d_mf);
    }
    auto general_width = [&](size_t j) {
        const SerdeConsts &sc = *consts_of(consts, mats[j]);
        if (ctx->wide) general_maxbits<uint64_t>(ctx, mats[j], sc, d_mf + 2 * j);
        else general_maxbits<uint32_t>(ctx, mats[j], sc, d_mf + 2 * j);
    };
    for (size_t j = 0; j < n; ++j)
        if (!items[j].batched && items[j].coeffs) general_width(j);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned int> h_mf(2 * n);
    HIP_TRY(hipMemcpyAsync(h_mf.data(), d_mf, 2 * n * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // matrices whose flag is up start over with the general kernels (rare: centred.h); their widths fix the offsets of
    // everything behind them, hence one more synchronise when there are any
    bool rerun = false;
    for (size_t j = 0; j < n; ++j)
        if (items[j].batched && h_mf[2 * j + 1]) {
            items[j].batched = false;
            HIP_TRY(hipMemsetAsync(d_mf + 2 * j, 0, sizeof(unsigned int), ctx->stream));
            general_width(j);
            rerun = true;
        }
    if (rerun) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_mf.data(), d_mf, 2 * n * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    // ---- widths, lengths, offsets
    size_t total = 0, next = 0;
    for (size_t j = 0; j < n; ++j) {
        ManyItem &it = items[j];
        it.width = h_mf[2 * j] == 0 ? 0 : h_mf[2 * j] + 1;
        if (it.width > 0xffffu) return set_error(std::string("centered max coeff bits exceed u16 range in ") + who);
        it.len = (it.coeffs * static_cast<size_t>(it.width) + 7) / 8;
        it.offset = next;
        total = it.offset + it.len;
        next = (total + 7) / 8 * 8;
    }
    for (size_t j = 0; j < n; ++j) {
        out_max_coeff_bits[j] = static_cast<uint16_t>(items[j].width);
        out_bytes_per_coeff[j] = static_cast<uint16_t>((items[j].width + 7) / 8);
        out_payload_offsets[j] = items[j].offset;
        out_payload_lens[j] = items[j].len;
    }
    *out_total_len = total;
    if (total > payload_capacity) return set_error(std::string("payload buffer too small in ") + who);
    if (total == 0) return 0;
    if (!payload_out) return set_error(std::string("null payload buffer in ") + who);
    // ---- pack pass into ONE staging block: every payload at its offset, padded with zeros to the next one
    CtxBlock staging_block(ctx);
    if (staging_block.alloc(next + 8)) return 1;
    uint32_t *const d_words = static_cast<uint32_t *>(staging_block.ptr);
    for (const ManyGroup &g : groups) {
        SerdeSegments t{};
        uint32_t at = 0, widest = 0;
        for (size_t j : g.members) {
            const ManyItem &it = items[j];
            if (!it.batched || it.width == 0) continue;
            const uint32_t k = t.count++;
            t.first_block[k] = at;
            at += static_cast<uint32_t>(it.blocks);
            t.width[k] = it.width;
            t.base[k] = words_ptr(mats[j]);
            t.coeffs[k] = it.coeffs;
            t.offset[k] = it.offset / 4;
            t.words[k] = (it.len + 7) / 8 * 2;
            widest = std::max(widest, it.width);
        }
        if (t.count == 0) continue;
        t.first_block[t.count] = at;
        const SerdeConsts &sc = *consts_of(consts, mats[g.members[0]]);
        MANY_FAST_LAUNCH(compact_pack_many_kernel, sc.limbs, dim3(at), 8u * widest * sizeof(uint32_t), t, N, sc, ctx->d_garner, gstride, ctx->d_limbs, d_words);
    }
    for (size_t j = 0; j < n; ++j) {
        const ManyItem &it = items[j];
        if (it.batched || it.width == 0) continue;
        const SerdeConsts &sc = *consts_of(consts, mats[j]);
        uint32_t *const slot = d_words + it.offset / 4;
        const size_t own = (it.len + 7) / 8 * 2;
        if (it.width <= kPackLdsWidth) {
            if (ctx->wide) general_pack<uint64_t, true>(ctx, mats[j], sc, it.width, slot, own);
            else general_pack<uint32_t, true>(ctx, mats[j], sc, it.width, slot, own);
        } else {
            HIP_TRY(hipMemsetAsync(slot, 0, own * 4, ctx->stream));
            if (ctx->wide) general_pack<uint64_t, false>(ctx, mats[j], sc, it.width, slot, own);
            else general_pack<uint32_t, false>(ctx, mats[j], sc, it.width, slot, own);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(payload_out, d_words, total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_load_compact_bytes_many(GpuMatrix *const *mats, size_t n, const uint8_t *const *payloads,
                                                      const size_t *payload_lens, const uint16_t *max_coeff_bits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_load_compact_bytes_many";
    if (n && (!payloads || !payload_lens || !max_coeff_bits)) return set_error(std::string("null input array in ") + who);
    GpuContext *ctx = nullptr;
    if (check_many(mats, n, who, &ctx)) return 1;
    if (n == 0) return 0;
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    // everything the one-matrix load refuses, for ALL matrices before anything is touched
    std::vector<ManyItem> items(n);
    size_t small_bytes = 0, next = 0;
    for (size_t j = 0; j < n; ++j) {
        ManyItem &it = items[j];
        it.mat = mats[j];
        it.coeffs = matrix_polys(mats[j]) * N;
        it.blocks = (it.coeffs + 255) / 256;
        it.width = max_coeff_bits[j];
        it.len = payload_lens[j];
        it.batched = it.blocks <= kSerdeGroupBlocks;
        if (it.width == 0) {
            if (it.len != 0) return set_error(std::string("payload_len must be zero when max_coeff_bits is zero in ") + who);
        } else if (!payloads[j] && it.coeffs) {
            return set_error(std::string("null payload in ") + who);
        }
        if (it.len != (it.coeffs * static_cast<size_t>(it.width) + 7) / 8)
            return set_error(std::string("payload length mismatch in ") + who);
        if (it.len < kLoadDirectBytes) small_bytes += (it.len + 7) / 8 * 8;
    }
    // staging layout: the small payloads first, gathered on the host and sent as one transfer; the large ones behind
    // them, each copied from where it lies (a host-side gather of tens of MB would cost more than the copy it saves)
    next = small_bytes;
    size_t small_at = 0;
    for (ManyItem &it : items) {
        if (it.len < kLoadDirectBytes) {
            it.offset = small_at;
            small_at += (it.len + 7) / 8 * 8;
        } else {
            it.offset = next;
            next += (it.len + 7) / 8 * 8;
        }
    }
    if (ctx_activate(ctx)) return 1;
    std::map<int, SerdeConsts> consts;
    for (size_t j = 0; j < n; ++j)
        if (items[j].coeffs && !consts_of(consts, mats[j])) return 1;
    for (size_t j = 0; j < n; ++j) mats[j]->format = GPU_POLY_FORMAT_COEFF;
    CtxBlock staging_block(ctx);
    if (staging_block.alloc(next + 8)) return 1;
    uint8_t *const d_staging = static_cast<uint8_t *>(staging_block.ptr);
    HIP_TRY(hipMemsetAsync(d_staging + next, 0, 8, ctx->stream));
    static thread_local std::vector<uint8_t> gather;
    if (small_bytes) {
        gather.assign(small_bytes, 0);
        for (size_t j = 0; j < n; ++j)
            if (items[j].len && items[j].len < kLoadDirectBytes) std::copy(payloads[j], payloads[j] + items[j].len, gather.data() + items[j].offset);
        HIP_TRY(hipMemcpyAsync(d_staging, gather.data(), small_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    for (size_t j = 0; j < n; ++j)
        if (items[j].len >= kLoadDirectBytes)
            HIP_TRY(hipMemcpyAsync(d_staging + items[j].offset, payloads[j], items[j].len, hipMemcpyHostToDevice, ctx->stream));
    for (const ManyGroup &g : group_by_level(items)) {
        SerdeSegments t{};
        uint32_t at = 0;
        for (size_t j : g.members) {
            const uint32_t k = t.count++;
            t.first_block[k] = at;
            at += static_cast<uint32_t>(items[j].blocks);
            t.width[k] = items[j].width;
            t.base[k] = words_ptr(mats[j]);
            t.coeffs[k] = items[j].coeffs;
            t.offset[k] = items[j].offset;
        }
        t.first_block[t.count] = at;
        const SerdeConsts &sc = *consts_of(consts, mats[g.members[0]]);
        if (ctx->wide) MXX_LAUNCH(compact_unpack_many_kernel<uint64_t>, dim3(at), dim3(256), 0, ctx->stream, t, static_cast<const uint8_t *>(d_staging), N, sc, ctx->d_limbs);
        else MXX_LAUNCH(compact_unpack_many_kernel<uint32_t>, dim3(at), dim3(256), 0, ctx->stream, t, static_cast<const uint8_t *>(d_staging), N, sc, ctx->d_limbs);
    }
    for (size_t j = 0; j < n; ++j) {  // beyond one launch's grid: the one-matrix kernel on its slot
        const ManyItem &it = items[j];
        if (it.batched || it.coeffs == 0) continue;
        const SerdeConsts &sc = *consts_of(consts, mats[j]);
        const dim3 blocks = item_grid(it.coeffs, 256);
        if (ctx->wide) MXX_LAUNCH(compact_unpack_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(words_ptr(mats[j])), static_cast<const uint8_t *>(d_staging + it.offset), matrix_polys(mats[j]), N, sc, ctx->d_limbs, it.width);
        else MXX_LAUNCH(compact_unpack_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(words_ptr(mats[j])), static_cast<const uint8_t *>(d_staging + it.offset), matrix_polys(mats[j]), N, sc, ctx->d_limbs, it.width);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous: the payloads may be freed on return
    return 0;
    ABI_GUARD_END
}
#undef MANY_FAST_LAUNCH

extern "C" int gpu_poly_store_compact_bytes(GpuMatrix *poly, uint8_t *payload_out, size_t payload_capacity,
                                            uint16_t *out_max_coeff_bits, uint16_t *out_bytes_per_coeff,
                                            size_t *out_payload_len) {
    return gpu_matrix_store_compact_bytes(poly, payload_out, payload_capacity, out_max_coeff_bits, out_bytes_per_coeff,
                                          out_payload_len);
}

extern "C" int gpu_poly_load_compact_bytes(GpuMatrix *poly, const uint8_t *payload, size_t payload_len,
                                           uint16_t max_coeff_bits) {
    return gpu_matrix_load_compact_bytes(poly, payload, payload_len, max_coeff_bits);
}
