// coeff_load.hip — gpupoly_matrix_load_coeff_words (extension): big-integer coefficients given as
// little-endian 64-bit words become their residues mod every limb, on the device.  The mirror image of
// gpupoly_matrix_store_coeff_words (scale_round.hip) and the device form of residues_from_biguints
// (src/poly/dcrt/gpu.rs:841-857, a BigUint % q per coefficient and limb on the CPU).
//
// Per coefficient and limb: x mod q for x = sum_w words[w] 2^(64 w), Horner from the top word.  Integers only.
//
//   32-bit words (q < 2^31).  One step takes S words = T = 2S half-words h_{T-1} .. h_0 (each below 2^32) and
//     acc = r P_T + h_{T-1} P_{T-1} + .. + h_1 P_1 + h_0,   P_j = 2^(32 j) mod q,   r the residue so far,
//   in one 64-bit accumulator, then one reduction (reduce_u64_sum: any acc < 2^64, result in [0, q)).  With r <= q - 1,
//   P_j <= q - 1 and h_j <= 2^32 - 1:
//     acc <= (q - 1)^2 + (T - 1)(2^32 - 1)(q - 1) + (2^32 - 1)
//   which for q < 2^k is below 2^(2k) + (T - 1) 2^(32 + k) + 2^32:
//     k = 31, S = 1 (T = 2):  2^62 +   2^63 + 2^32 < 2^64
//     k = 30, S = 2 (T = 4):  2^60 + 3 2^62 + 2^32 < 2^64
//     k = 29, S = 4 (T = 8):  2^58 + 7 2^61 + 2^32 < 2^64   (k = 28: 2^56 + 7 2^60 + 2^32 < 2^63)
//   S is chosen from the widest modulus of the context (steps_for_bits).  The next S would overflow: k = 31, T = 4 gives
//   2^62 + 3 2^63 > 2^64 and k = 30, T = 8 gives 2^60 + 7 2^62 > 2^64.  The bound is reached (up to
//   P_j <= q - 1, which the primes decide) by r = q - 1 followed by S words of all ones, i.e. the value
//   (q - 1) 2^(64 S) + 2^(64 S) - 1; tests/test_gpu_load_coeff_words.py loads it for every limb.  A top group with fewer
//   than S words is filled with zero words.
//
//   64-bit words (q < 2^62).  r <- (r R + (word mod q)) mod q with R = 2^64 mod q: the word is reduced first
//   (word_mod: floor(2^64 / q), estimate at most one short), so that r R + w <= (q - 1)^2 + (q - 1) < q^2 < 2^(2k), which
//   is what barrett_reduce wants of its input; the sum is below 2^124 and fits the 128-bit product type.  Nothing is lazy.
//
// Layout.  The input is coefficient-major ([row][col][k][w], 8 words_per_coeff bytes between neighbouring
// coefficients), the matrix limb-major ([row][col][limb][k]).  A workgroup takes a tile of C consecutive coefficients of
// one entry: the tile's words are one contiguous run of the input, fetched with 16-byte loads (lane i takes bytes
// [16 i, 16 i + 16) of the run: whole cache lines, each fetched once) and written to LDS at row pitch
// words_per_coeff | 1 words.  Then lane t owns coefficient t: it reads word w of its row (ds_read_b64 at a stride of
// 2 pitch dwords; pitch is odd, so the 32 lanes of a half-wave fall on 32 different bank pairs) and walks the limbs,
// G at a time so that one LDS read feeds G independent Horner chains; the store of limb l is N-strided per lane and
// contiguous across the wave.  C = 256, 128 or 64 keeps the tile at or below 64 KB (words_per_coeff <= 31, 63, 127).  One
// word per coefficient is already contiguous across lanes and is read straight from global memory, and so is anything
// above 127 words, where a tile of 64 rows no longer fits.
#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr uint32_t kStagedMaxWords = 127;
constexpr size_t kMaxPolysPerLaunch = size_t(1) << 22;  // grid.x; grid.x * 256 stays below 2^32

template <typename W>
struct LoadConsts;
template <>
struct LoadConsts<uint32_t> {
    uint32_t pw[GPUPOLY_MAX_LIMBS][8];  // pw[l][j - 1] = P_j = 2^(32 j) mod q_l, j = 1 .. 2S
};
template <>
struct LoadConsts<uint64_t> {
    uint64_t pw[GPUPOLY_MAX_LIMBS][1];  // 2^64 mod q_l
};

// words per Horner step for 32-bit limbs whose widest modulus has `bits` bits (bound in the file comment)
int steps_for_bits(uint32_t bits) { return bits <= 29 ? 4 : bits <= 30 ? 2 : 1; }

// v < 2^64 -> v mod q with mu64 = floor(2^64 / q): the quotient estimate is at most one short
__device__ __forceinline__ uint64_t word_mod(uint64_t v, uint64_t q, uint64_t mu64) {
    const uint64_t r = v - __umul64hi(v, mu64) * q;
    return r >= q ? r - q : r;
}

// S: words per step (32-bit limbs; 1 for 64-bit limbs).  STAGED: the tile goes through LDS (dynamic, C * (wpc | 1) words).
// Block (x, y) handles coefficients [y C, y C + C) of entry x, C = blockDim.x.  Every word of dst is written: coefficients
// at or above `cpp` as 0.  wpc_magic = ceil(2^32 / wpc): floor(f / wpc) = hi32(f wpc_magic) for f wpc < 2^32, and the
// tile's word index f stays below 2^15.
template <typename W, int S, bool STAGED>
__global__ void __launch_bounds__(256) load_coeff_words_kernel(W *__restrict__ dst, const uint64_t *__restrict__ src, size_t polys,
                                                               uint32_t N, uint32_t cpp, uint32_t wpc, int L,
                                                               uint32_t wpc_magic, LoadConsts<W> lc,
                                                               const LimbConst *__restrict__ limbs) {
    extern __shared__ uint64_t tile[];
    constexpr int G = sizeof(W) == 4 ? 4 : 2;  // limbs per pass over the words
    const uint32_t C = blockDim.x;
    const size_t poly = blockIdx.x;
    if (poly >= polys) return;  // whole workgroups only
    const uint32_t k0 = blockIdx.y * C;
    const uint32_t k = k0 + threadIdx.x;
    const uint64_t *row;
    if constexpr (STAGED) {
        const uint32_t pitch = wpc | 1;
        // a branch on purpose: written as the select k0 < cpp ? min(C, cpp - k0) : 0 the compiler dropped the comparison
        // (the subtraction wrapped for tiles past the input, which then read far outside it)
        if (k0 < cpp) {
            const uint32_t cnt = min(C, cpp - k0);
            const size_t base = (poly * cpp + k0) * wpc;  // first word of the run; src itself is 16-byte aligned
            const uint32_t total = cnt * wpc;             // <= 256 * 127
            const uint32_t head = static_cast<uint32_t>(base & 1);
            auto put = [&](uint32_t f, uint64_t v) {
                const uint32_t c = __umulhi(f, wpc_magic);  // f / wpc
                tile[c * pitch + (f - c * wpc)] = v;
            };
            if (head && threadIdx.x == 0) put(0, src[base]);
            const uint32_t pairs = (total - head) / 2;
            const ulonglong2 *src2 = reinterpret_cast<const ulonglong2 *>(src + base + head);
            for (uint32_t i = threadIdx.x; i < pairs; i += C) {
                const ulonglong2 v = src2[i];
                put(head + 2 * i, v.x);
                put(head + 2 * i + 1, v.y);
            }
            if (((total - head) & 1) && threadIdx.x == 0) put(total - 1, src[base + total - 1]);
        }
        __syncthreads();
        row = tile + threadIdx.x * pitch;
    } else {
        row = src + (poly * cpp + k) * wpc;  // dereferenced for k < cpp only
    }
    if (k >= N) return;
    W *out = dst + poly * static_cast<size_t>(L) * N + k;
    if (k >= cpp) {
        for (int l = 0; l < L; ++l) out[static_cast<size_t>(l) * N] = 0;
        return;
    }
    const uint32_t groups = (wpc + S - 1) / S;
    for (int l0 = 0; l0 < L; l0 += G) {
        W r[G];
        uint64_t q[G], mu64[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int l = min(l0 + g, L - 1);  // a short last pass repeats the top limb and does not store it
            r[g] = 0;
            q[g] = limbs[l].q;
            mu64[g] = limbs[l].mu64;
        }
        for (uint32_t grp = groups; grp-- > 0;) {
            uint64_t w[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const uint32_t idx = grp * S + s;
                w[s] = idx < wpc ? row[idx] : 0;  // only the top group can be short
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int l = min(l0 + g, L - 1);
                if constexpr (sizeof(W) == 4) {
                    // acc = r P_T + h_{T-1} P_{T-1} + .. + h_1 P_1 + h_0 < 2^64 (file comment)
                    uint64_t acc = static_cast<uint64_t>(r[g]) * lc.pw[l][2 * S - 1] + static_cast<uint32_t>(w[0]);
#pragma unroll
                    for (int j = 1; j < 2 * S; ++j) {
                        const uint32_t h = static_cast<uint32_t>(w[j / 2] >> (32 * (j & 1)));
                        acc += static_cast<uint64_t>(h) * lc.pw[l][j - 1];
                    }
                    r[g] = reduce_u64_sum(acc, static_cast<uint32_t>(q[g]), mu64[g]);
                } else {
                    // r R + (word mod q) < q^2 < 2^(2 kbits)
                    const u128_t x = static_cast<u128_t>(r[g]) * lc.pw[l][0] + word_mod(w[0], q[g], mu64[g]);
                    r[g] = barrett_reduce(x, q[g], limbs[l].mu, limbs[l].kbits);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (l0 + g < L) out[static_cast<size_t>(l0 + g) * N] = r[g];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 u128h;

// pw[l][j - 1] = 2^(B j) mod q_l for j = 1 .. terms, B the bits of one Horner term
template <typename W>
LoadConsts<W> build_consts(const GpuContext *ctx, int L, int terms, int term_bits) {
    LoadConsts<W> lc;
    memset(&lc, 0, sizeof(lc));
    for (int l = 0; l < L; ++l) {
        const uint64_t q = ctx->moduli[l];
        const uint64_t step = static_cast<uint64_t>((static_cast<u128h>(1) << term_bits) % q);
        uint64_t p = 1 % q;
        for (int j = 0; j < terms; ++j) {
            p = static_cast<uint64_t>(static_cast<u128h>(p) * step % q);
            lc.pw[l][j] = static_cast<W>(p);
        }
    }
    return lc;
}

struct LoadShape {
    size_t polys;
    uint32_t N, cpp, wpc;
    int L;
};

template <typename W, int S>
void launch_load(GpuContext *ctx, W *dst, const uint64_t *src, const LoadShape &sh, const LoadConsts<W> &lc) {
    const bool staged = sh.cpp > 0 && sh.wpc >= 2 && sh.wpc <= kStagedMaxWords;
    uint32_t C = !staged || sh.wpc <= 31 ? 256 : sh.wpc <= 63 ? 128 : 64;
    C = std::min(C, std::max<uint32_t>(64, (sh.N + 63) / 64 * 64));  // small rings: no wider than the ring
    const dim3 grid(static_cast<unsigned>(sh.polys), (sh.N + C - 1) / C);  // polys <= kMaxPolysPerLaunch
    const uint32_t magic = static_cast<uint32_t>(((1ull << 32) + sh.wpc - 1) / sh.wpc);  // unused at one word
    if (staged) {
        MXX_LAUNCH((load_coeff_words_kernel<W, S, true>), grid, dim3(C), static_cast<size_t>(C) * (sh.wpc | 1) * sizeof(uint64_t),
                   ctx->stream, dst, src, sh.polys, sh.N, sh.cpp, sh.wpc, sh.L, magic, lc, ctx->d_limbs);
    } else {
        MXX_LAUNCH((load_coeff_words_kernel<W, S, false>), grid, dim3(C), 0, ctx->stream, dst, src, sh.polys, sh.N, sh.cpp, sh.wpc,
                   sh.L, magic, lc, ctx->d_limbs);
    }
}

}  // namespace

extern "C" int gpupoly_matrix_load_coeff_words(GpuMatrix *mat, const uint64_t *words, size_t words_per_coeff,
                                               size_t coeffs_per_poly, int out_format) {
    ABI_GUARD_BEGIN
    // every refusal comes before the first launch and before `mat` or its tag is touched
    if (!mat) return set_error("gpupoly_matrix_load_coeff_words: null matrix");
    if (out_format != GPU_POLY_FORMAT_COEFF && out_format != GPU_POLY_FORMAT_EVAL)
        return set_error("gpupoly_matrix_load_coeff_words: invalid out_format");
    if (words_per_coeff == 0) return set_error("gpupoly_matrix_load_coeff_words: words_per_coeff must be at least 1");
    if (words_per_coeff > 0xffffffffull) return set_error("gpupoly_matrix_load_coeff_words: words_per_coeff too large");
    GpuContext *ctx = mat->ctx;
    if (coeffs_per_poly > static_cast<size_t>(ctx->N))
        return set_error("gpupoly_matrix_load_coeff_words: coeffs_per_poly is above the ring dimension " + std::to_string(ctx->N));
    if (!words && coeffs_per_poly > 0) return set_error("gpupoly_matrix_load_coeff_words: null words");
    const size_t polys = matrix_polys(mat);
    if (polys == 0) {
        mat->format = out_format;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const int L = mat->level + 1;
    const size_t poly_words = coeffs_per_poly * words_per_coeff;
    const size_t poly_res = static_cast<size_t>(L) * ctx->N;

    // the input goes through one scratch block filled by one copy; entry-aligned pieces only where that block cannot be had
    CtxBlock stage(ctx);
    size_t per_chunk = std::min(polys, kMaxPolysPerLaunch);
    if (poly_words) {
        while (stage.alloc(per_chunk * poly_words * sizeof(uint64_t))) {
            if (per_chunk == 1) return 1;
            per_chunk = (per_chunk + 1) / 2;
        }
    }
    const int S = ctx->wide ? 1 : steps_for_bits(ctx->crt_bits);
    LoadConsts<uint64_t> lc64;
    LoadConsts<uint32_t> lc32;
    if (ctx->wide) lc64 = build_consts<uint64_t>(ctx, L, 1, 64);
    else lc32 = build_consts<uint32_t>(ctx, L, 2 * S, 32);
    void *const dst = words_ptr(mat);
    for (size_t p0 = 0; p0 < polys; p0 += per_chunk) {
        const size_t pc = std::min(per_chunk, polys - p0);
        const size_t in_bytes = pc * poly_words * sizeof(uint64_t);
        if (in_bytes)
            MXX_TRACED_COPY("copy (host to device)", ctx->stream, in_bytes,
                            HIP_TRY(hipMemcpyAsync(stage.ptr, words + p0 * poly_words, in_bytes, hipMemcpyHostToDevice, ctx->stream)));
        const LoadShape sh = {pc, static_cast<uint32_t>(ctx->N), static_cast<uint32_t>(coeffs_per_poly),
                              static_cast<uint32_t>(words_per_coeff), L};
        const uint64_t *src = static_cast<const uint64_t *>(stage.ptr);
        MXX_TRACE_BYTES(static_cast<double>(in_bytes + pc * poly_res * ctx->word_bytes));
        if (ctx->wide) {
            launch_load<uint64_t, 1>(ctx, static_cast<uint64_t *>(dst) + p0 * poly_res, src, sh, lc64);
        } else {
            uint32_t *d = static_cast<uint32_t *>(dst) + p0 * poly_res;
            if (S == 4) launch_load<uint32_t, 4>(ctx, d, src, sh, lc32);
            else if (S == 2) launch_load<uint32_t, 2>(ctx, d, src, sh, lc32);
            else launch_load<uint32_t, 1>(ctx, d, src, sh, lc32);
        }
        HIP_TRY(hipGetLastError());
    }
    if (out_format == GPU_POLY_FORMAT_EVAL) {
        const int rc = launch_ntt(ctx, dst, polys * static_cast<size_t>(L), L, false);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the caller may reuse `words`
    mat->format = out_format;
    return 0;
    ABI_GUARD_END
}
