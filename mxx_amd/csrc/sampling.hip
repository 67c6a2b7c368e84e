// sampling.hip — seeded distribution sampling straight into device matrices.
// Replaces cuda/src/matrix/MatrixSampling.cu behind
// cuda/include/matrix/MatrixSampling.cuh:25-37.
//
// Every sample is a pure function of (seed, GLOBAL polynomial index row*full_ncol + col,
// coefficient index and, for the uniform distribution, limb index):
// sample_distribution_columns therefore equals the matching column slice of the full
// sample for the same seed (reference: MatrixSampling.cu:232-289, test
// src/sampler/gpu.rs:323-361).  Gaussian: a ChaCha20 stream per pair of coefficients (Karney's
// sampler takes a variable number of 16-bit draws, rng.h).  Uniform / bit / ternary: fixed-position
// draws, eight per keystream block (the reference's keying, one stream - i.e. at least
// one block - per residue, made the generator the whole cost of the call).  Integers are
// drawn once and written as residues into every limb; the result is transformed to EVAL.
#include "common.h"
#include "modarith.h"
#include "rng.h"

#include <algorithm>

static constexpr uint64_t kTagUniform = 0x6f70656e66686531ull;
static constexpr uint64_t kTagGauss = 0x6f70656e66686532ull;
static constexpr uint64_t kTagBit = 0x6f70656e66686533ull;
static constexpr uint64_t kTagTernary = 0x6f70656e66686534ull;

// uniform / bit / ternary: ONE ChaCha20 block serves eight draws (round 2 spent a block per residue: 25 ms for M2A's
// 3.5 GB operand, 0.02 of the HBM roofline, with the generator as the whole cost).  Keying, a pure function of
// (seed, global polynomial index, limb, coefficient) as before, so column windows commute (src/sampler/gpu.rs:323-361):
//   uniform : sub-key = HChaCha20(seed, tag, stream2 = limb + 1); residue of coefficient i = word (i & 7) of keystream
//             block (i >> 3) of stream (gpoly + 1, 0), reduced mod q when it is below floor(2^64 / q) q; a rejected
//             word (probability q 2^-64) is replaced by the first accepted word of the coefficient's own overflow
//             stream (gpoly + 1, i + 1) under the same sub-key;
//   bit / ternary : sub-key (seed, tag, 0); the draw of coefficient i = the same word of stream (gpoly + 1, 0).
// A thread owns eight consecutive coefficients of one (polynomial, limb) vector: one block in registers, no LDS, and
// 32 / 64 contiguous bytes stored per lane.  The sub-keys are derived once per call by a one-wave launch.
__global__ void derive_subkeys_kernel(ChaChaKey *__restrict__ keys, GpuRngSeed seed, uint64_t tag, uint32_t count, uint32_t first_stream2) {
    const uint32_t l = threadIdx.x;
    if (l < count) keys[l] = chacha_subkey(seed, static_cast<uint64_t>(first_stream2) + l, tag);
}

__device__ __forceinline__ ChaChaKey load_key(const ChaChaKey *__restrict__ keys, uint32_t l) {
    const uint4 *p = reinterpret_cast<const uint4 *>(keys + l);
    const uint4 a = p[0], b = p[1];
    ChaChaKey k;
    k.w[0] = a.x; k.w[1] = a.y; k.w[2] = a.z; k.w[3] = a.w;
    k.w[4] = b.x; k.w[5] = b.y; k.w[6] = b.z; k.w[7] = b.w;
    return k;
}

// the rare path of the uniform sampler: first accepted word of the coefficient's overflow stream
__device__ __noinline__ uint64_t uniform_overflow_draw(const ChaChaKey &key, uint64_t stream0, uint64_t stream1, uint64_t threshold) {
    for (uint32_t block = 0;; ++block) {
        uint64_t w[8];
        chacha_block_words(key, stream0, stream1, block, w);
        for (int j = 0; j < 8; ++j)
            if (w[j] < threshold) return w[j];
    }
}

template <typename W, int VEC>
__device__ __forceinline__ void store_group(W *dst, const W (&r)[8], uint32_t count) {
    if (count == 8 && VEC) {
        typedef W vec_t __attribute__((ext_vector_type(16 / sizeof(W))));
        constexpr int per = 16 / sizeof(W);
#pragma unroll
        for (int v = 0; v < 8 / per; ++v) {
            vec_t x;
#pragma unroll
            for (int e = 0; e < per; ++e) x[e] = r[v * per + e];
            __builtin_nontemporal_store(x, reinterpret_cast<vec_t *>(dst) + v);
        }
    } else {
        for (uint32_t j = 0; j < count; ++j) dst[j] = r[j];
    }
}

template <typename W>
__global__ void __launch_bounds__(256) sample_uniform_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs,
                                                             const ChaChaKey *__restrict__ keys, size_t polys, size_t local_ncol,
                                                             size_t full_ncol, size_t col_offset, uint32_t L, uint32_t N,
                                                             uint32_t groups /* ceil(N / 8) */, uint32_t l0, uint32_t Ls) {
    // limbs [l0, l0 + Ls) of every polynomial are written (all of them: l0 = 0, Ls = L); the others are left alone
    const size_t idx = item_index();
    if (idx >= polys * Ls * groups) return;
    const size_t sv = idx / groups;  // (polynomial, sampled limb)
    const uint32_t g = static_cast<uint32_t>(idx - sv * groups);
    const size_t p = sv / Ls;
    const uint32_t l = l0 + static_cast<uint32_t>(sv - p * Ls);
    const size_t vec = p * L + l;  // (polynomial, limb) vector
    const size_t row = p / local_ncol, lcol = p - row * local_ncol;
    const uint64_t gpoly = row * full_ncol + col_offset + lcol;
    const ChaChaKey key = load_key(keys, l);
    const uint64_t q = limbs[l].q, mu64 = limbs[l].mu64;
    const uint64_t threshold = mu64 * q;  // = (2^64 - 1) - (2^64 - 1) % q: q is an odd prime, so floor((2^64-1)/q) = floor(2^64/q)
    uint64_t w[8];
    chacha_block_words(key, gpoly + 1, 0, g, w);
    const uint32_t count = min(8u, N - g * 8u);
    W r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint64_t x = w[j];
        if (x >= threshold && static_cast<uint32_t>(j) < count) x = uniform_overflow_draw(key, gpoly + 1, static_cast<uint64_t>(g) * 8u + j + 1, threshold);
        uint64_t rem = x - __umul64hi(x, mu64) * q;  // quotient estimate at most one short
        rem = rem >= q ? rem - q : rem;
        r[j] = static_cast<W>(rem);
    }
    store_group<W, 1>(out + vec * N + static_cast<size_t>(g) * 8u, r, count);
}

// bit / ternary: the draw is shared by all limbs.  One thread's work for group g of polynomial p, whose draws are block g of
// stream (stream0, 0) under `key`; the plain and the block kernel differ in how they find that key and stream alone
template <typename W>
__device__ __forceinline__ void sample_small_group(W *__restrict__ out, const LimbConst *__restrict__ limbs, const ChaChaKey &key,
                                                   uint64_t stream0, size_t p, uint32_t g, uint32_t L, uint32_t N, int dist) {
    uint64_t w[8];
    chacha_block_words(key, stream0, 0, g, w);
    const uint32_t count = min(8u, N - g * 8u);
    int32_t z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (dist == GPU_MATRIX_DIST_BIT) {
            z[j] = static_cast<int32_t>(w[j] & 1ull);
        } else {
            const uint32_t pick = static_cast<uint32_t>(w[j] % 3ull);
            z[j] = pick == 0 ? 0 : (pick == 1 ? 1 : -1);
        }
    }
    for (uint32_t l = 0; l < L; ++l) {
        const W q = static_cast<W>(limbs[l].q);
        W r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = z[j] < 0 ? q - 1 : static_cast<W>(z[j]);
        store_group<W, 1>(out + (p * L + l) * N + static_cast<size_t>(g) * 8u, r, count);
    }
}

template <typename W>
__global__ void __launch_bounds__(256) sample_small_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs,
                                                           const ChaChaKey *__restrict__ keys, size_t polys, size_t local_ncol,
                                                           size_t full_ncol, size_t col_offset, uint32_t L, uint32_t N, uint32_t groups,
                                                           int dist) {
    const size_t idx = item_index();
    if (idx >= polys * groups) return;
    const size_t p = idx / groups;
    const uint32_t g = static_cast<uint32_t>(idx - p * groups);
    const size_t row = p / local_ncol, lcol = p - row * local_ncol;
    const uint64_t gpoly = row * full_ncol + col_offset + lcol;
    const ChaChaKey key = load_key(keys, 0);
    sample_small_group<W>(out, limbs, key, gpoly + 1, p, g, L, N, dist);
}

// discrete Gaussian: persistent lanes (rng.h).  An element is a PAIR of consecutive coefficients of one polynomial drawn
// one after the other from ONE stream (gpoly + 1, (i >> 1) + 1) - still a pure function of (seed, global index), column
// windows commute: the samples depend on no input.  Wave w owns pairs [w*64*per_lane, +64*per_lane); its lanes take
// them one at a time (wave_take).  Lanes finish at different times, so a lane's store is a lone 8 bytes: it goes to a
// compact int64 staging array ([poly][N]) that a coalesced pass expands into the L residues per coefficient (storing
// the residues from here cost a 32-byte HBM write per limb).
// Why pairs, and the refill policy.  With a stream per coefficient (~21 draws, ~20 steps, an empty ring at every start)
// about 25 of a wave's 64 lanes were out of draws at EVERY checkpoint and the block pass - counted: 96 % of the
// checkpoints, 1.74 blocks computed per coefficient for 0.66 consumed, ~70 % of the kernel's instructions - ran whatever
// the cadence.  A pair's stream lasts ~42 steps and wastes half as many draws, so refills can be held to every third
// checkpoint and are never forced (a lane that runs dry waits).  Same-box A/B of the group size (M3A call / M4 step):
// one coefficient per stream 7.60 ms / 0.634, pairs 7.13 / 0.647, quads 7.08 / 0.70 (a small launch lasts as long as
// its unluckiest lane's chain, which grows with the group), eight 7.2 / -.  Pairs.
#ifndef GAUSS_GROUP_LOG
#define GAUSS_GROUP_LOG 1  // two coefficients per stream (the CPU restatement's keying: oracle/oracle_sampling.c)
#endif
// UNI: every wave's chunk of groups lies inside one polynomial (the launcher checks that 64 * per_lane divides the groups
// per polynomial): its (row, column) - a 32-bit division - is then computed once per wave on the scalar unit instead of in
// every group hand-over
// SEG (with UNI): the matrix is the column-wise concatenation of independently seeded segments (rng.h, RngSegments); the
// wave's polynomial lies in one segment, whose sub-key and shape replace `key`, `full_ncol` and `col_offset` - all
// wave-uniform, read from the kernel argument on the scalar unit.
template <int SV, bool UNI = false, bool SEG = false>
__global__ void __launch_bounds__(SAMPLER_THREADS) sample_gauss_kernel(int64_t *__restrict__ stage, size_t polys,
                                    uint32_t local_ncol, size_t full_ncol, size_t col_offset, uint32_t logN,
                                    double sigma, KarneyDivisor div, ChaChaKey key, uint32_t per_lane, uint32_t fill_every,
                                    int starve_limit, SegArg<SEG> segs = SegArg<SEG>{}) {
    static_assert(!SEG || UNI, "segments need a wave's chunk inside one polynomial");
    __shared__ uint32_t ring[SAMPLER_THREADS * RNG_RING_SLOTS];  // 128 bytes per lane: 8 KB per one-wave workgroup
    const uint32_t glog = logN < GAUSS_GROUP_LOG ? logN : GAUSS_GROUP_LOG;
    const uint32_t G = 1u << glog;
    const size_t total = (polys << logN) >> glog;  // groups
    WaveChunk chunk = wave_chunk(total, per_lane);
    const uint32_t p_u = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(chunk.base >> (logN - glog))));
    const uint32_t row_u = p_u / local_ncol, lcol_u = p_u - row_u * local_ncol;
    uint64_t stream0_u = row_u * full_ncol + col_offset + lcol_u + 1;
    if constexpr (SEG) {
        const uint32_t j = rng_segment_of(segs, lcol_u);
        key = segs.key[j];
        stream0_u = static_cast<uint64_t>(row_u) * (segs.start[j + 1] - segs.start[j]) + (lcol_u - segs.start[j]) + 1;
    }
    ChaChaRng rng;
    rng_init_keyed(rng, ring, key, 0, 0, SAMPLER_THREADS);
    KarneyFsm f;
    karney_reset(f);
    karney_fix_parameters(f, 0.0, sigma, div);  // one centre and one width for the whole matrix
    const bool degenerate = div.degenerate;
    bool have = false, fin = true;
    uint32_t cnt = 0;
    size_t idx = 0;
    auto integer_ready = [&]() {
        if (f.st == KS_DONE && !fin) {
            stage[(idx << glog) + cnt] = f.result;
            ++cnt;
            if (cnt == G) fin = true;
            else karney_begin_fixed(f, degenerate);
        }
    };
    for (uint32_t step = 0;; ++step) {  // one superstep per iteration
        integer_ready();
        {
            const bool take = f.st == KS_DONE && fin;
            const uint32_t e = wave_take(chunk, take);
            if (take) {
                have = e < chunk.len;
                if (have) {
                    idx = chunk.base + e;
                    uint64_t stream0;
                    if constexpr (UNI) {
                        stream0 = stream0_u;
                    } else {
                        const uint32_t p = static_cast<uint32_t>(idx >> (logN - glog));
                        const uint32_t row = p / local_ncol, lcol = p - row * local_ncol;
                        stream0 = row * full_ncol + col_offset + lcol + 1;
                    }
                    rng_reopen(rng, stream0, (idx & ((size_t(1) << (logN - glog)) - 1)) + 1);
                    cnt = 0;
                    fin = false;
                    karney_begin_fixed(f, degenerate);
                } else {
                    f.st = KS_IDLE;
                }
            }
            if (__all(f.st == KS_IDLE)) break;
            rng_fill_wave(rng, f.st != KS_IDLE, step % fill_every == 0, starve_limit, karney_urgent(SV));
        }
        karney_heavy(f, rng);
#pragma unroll
        for (int s = 0; s < KARNEY_SUPERSTEP / SV; ++s) karney_light(f, rng);
#pragma unroll
        for (int sv = 1; sv < SV; ++sv) {
            integer_ready();
            karney_heavy(f, rng);
#pragma unroll
            for (int s = 0; s < KARNEY_SUPERSTEP / SV; ++s) karney_light(f, rng);
        }
    }
}

// ---- MXX_HIP_RNG_COMPAT=reference: the reference device RNG's own keying -----------------------
// The default keying departs from cuda/src/ChaCha.cu:138-149 + cuda/src/matrix/MatrixSampling.cu:239-289 in three
// documented ways (rng.h), so a matrix derived from a seed - the hash sampler's included - differs from the one a CUDA
// build derives.  With the switch set (read per context at creation, gpupoly_reload_env) gpu_matrix_sample_distribution
// and _columns key and consume their streams exactly as the reference does: a stream per (polynomial, coefficient) -
// and limb, for the uniform distribution -, stream0 in the 64-bit block counter, stream1 in the nonce, 64-bit draws, Karney
// on 53-bit deviates compared as doubles.  One thread per coefficient, nested loops: the slow path, for interoperability
// only.  Pure function of (seed, global polynomial index, coefficient, limb) as before: column windows commute.
struct RefRng {
    uint32_t state[16], block[16];
    uint32_t idx;
};

__device__ __forceinline__ void ref_rng_init(RefRng &r, const GpuRngSeed &seed, uint64_t s0, uint64_t s1, uint64_t s2, uint64_t tag) {
    const ChaChaKey k = chacha_subkey(seed, s2, tag);
    r.state[0] = 0x61707865u; r.state[1] = 0x3320646eu; r.state[2] = 0x79622d32u; r.state[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.state[4 + i] = k.w[i];
    r.state[12] = static_cast<uint32_t>(s0);
    r.state[13] = static_cast<uint32_t>(s0 >> 32);
    r.state[14] = static_cast<uint32_t>(s1);
    r.state[15] = static_cast<uint32_t>(s1 >> 32);
    r.idx = 8;
}

__device__ __noinline__ void ref_rng_refill(RefRng &r) {
    uint32_t x[16];
    for (int i = 0; i < 16; ++i) x[i] = r.state[i];
    chacha_rounds(x);
    for (int i = 0; i < 16; ++i) r.block[i] = x[i] + r.state[i];
    if (++r.state[12] == 0) ++r.state[13];
    r.idx = 0;
}

__device__ __forceinline__ uint64_t ref_rng_u64(RefRng &r) {
    if (r.idx >= 8) ref_rng_refill(r);
    uint32_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < 8; ++i)  // register-resident block: select instead of indexing
        if (i == r.idx) { lo = r.block[2 * i]; hi = r.block[2 * i + 1]; }
    ++r.idx;
    return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
}

__device__ __forceinline__ double ref_rng_u01(RefRng &r) { return u64_to_open01(ref_rng_u64(r)); }

__device__ bool ref_karney_h(RefRng &r) {
    double a = ref_rng_u01(r);
    if (!(a < 0.5)) return true;
    for (;;) {
        const double b = ref_rng_u01(r);
        if (!(b < a)) return false;
        a = ref_rng_u01(r);
        if (!(a < b)) return true;
    }
}

__device__ bool ref_karney_b(RefRng &r, int32_t k, double x) {
    double y = x;
    int32_t n = 0;
    const double m = static_cast<double>(2 * k + 2);
    for (;; ++n) {
        const double z = ref_rng_u01(r);
        if (!(z < y)) break;
        const double t = ref_rng_u01(r);
        if (!(t < (2.0 * static_cast<double>(k) + x) / m)) break;
        y = z;
        if (n > 4096) break;
    }
    return (n % 2) == 0;
}

__device__ int64_t ref_karney(RefRng &r, double mean, double stddev) {
    if (!(stddev > 0.0) || !isfinite(mean) || !isfinite(stddev)) return static_cast<int64_t>(llround(mean));
    const int64_t cs = static_cast<int64_t>(ceil(stddev));
    if (cs <= 0) return static_cast<int64_t>(llround(mean));
    for (int iter = 0; iter < (1 << 16); ++iter) {
        int32_t k = 0;
        while (ref_karney_h(r)) {
            if (++k > 1024) break;
        }
        int32_t n = k * (k - 1);
        while (n-- && ref_karney_h(r)) {
        }
        if (!(n < 0)) continue;
        const int64_t s = (ref_rng_u64(r) & 1ull) ? 1 : -1;
        const double di0 = stddev * static_cast<double>(k) + static_cast<double>(s) * mean;
        const int64_t i0 = static_cast<int64_t>(ceil(di0));
        const double x0 = (static_cast<double>(i0) - di0) / stddev;
        const int64_t j = static_cast<int64_t>(ref_rng_u64(r) % static_cast<uint64_t>(cs));
        const double x = x0 + static_cast<double>(j) / stddev;
        if (!(x < 1.0) || (x == 0.0 && s < 0 && k == 0)) continue;
        int32_t h = k + 1;
        while (h-- > 0 && ref_karney_b(r, k, x)) {
        }
        if (h >= 0) continue;
        return s * (i0 + j);
    }
    // 2^16 rejected trials: not reachable in practice (the reference falls back to a rounded normal here)
    const double u1 = ref_rng_u01(r), u2 = ref_rng_u01(r);
    return static_cast<int64_t>(llround(mean + stddev * (sqrt(-2.0 * det_log(u1)) * det_cos2pi(u2))));
}

template <typename W>
__global__ void __launch_bounds__(128) sample_compat_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs, size_t polys,
                                                            size_t local_ncol, size_t full_ncol, size_t col_offset, uint32_t L,
                                                            uint32_t logN, int dist, double sigma, GpuRngSeed seed, uint32_t l0,
                                                            uint32_t Ls /* uniform: limbs [l0, l0 + Ls) only */) {
    const size_t idx = item_index();
    if (idx >= (polys << logN)) return;
    const size_t p = idx >> logN;
    const uint32_t i = static_cast<uint32_t>(idx & ((size_t(1) << logN) - 1));
    const size_t row = p / local_ncol, lcol = p - row * local_ncol;
    const uint64_t gpoly = row * full_ncol + col_offset + lcol;
    RefRng r;
    if (dist == GPU_MATRIX_DIST_UNIFORM) {
        for (uint32_t l = l0; l < l0 + Ls; ++l) {
            const uint64_t q = limbs[l].q, threshold = ~0ull - (~0ull % q);
            ref_rng_init(r, seed, gpoly + 1, static_cast<uint64_t>(i) + 1, static_cast<uint64_t>(l) + 1, kTagUniform);
            uint64_t x;
            do x = ref_rng_u64(r); while (x >= threshold);
            out[((p * L + l) << logN) + i] = static_cast<W>(x % q);
        }
        return;
    }
    int64_t z;
    if (dist == GPU_MATRIX_DIST_GAUSS) {
        ref_rng_init(r, seed, gpoly + 1, static_cast<uint64_t>(i) + 1, 0, kTagGauss);
        z = ref_karney(r, 0.0, sigma);
    } else if (dist == GPU_MATRIX_DIST_BIT) {
        ref_rng_init(r, seed, gpoly + 1, static_cast<uint64_t>(i) + 1, 0, kTagBit);
        z = static_cast<int64_t>(ref_rng_u64(r) & 1ull);
    } else {
        ref_rng_init(r, seed, gpoly + 1, static_cast<uint64_t>(i) + 1, 0, kTagTernary);
        const uint64_t pick = ref_rng_u64(r) % 3ull;
        z = pick == 0 ? 0 : (pick == 1 ? 1 : -1);
    }
    for (uint32_t l = 0; l < L; ++l)
        out[((p * L + l) << logN) + i] = signed_to_residue_mu<W>(z, limbs[l].q, limbs[l].mu64);
}

// keep_coeff: leave the samples as coefficients (for a caller that decomposes them next) instead of finishing in EVAL.
// row_offset: `out` is rows [row_offset, row_offset + out->rows) of the conceptual matrix - every kernel forms the global
// polynomial index as row * full_ncol + col_offset + column, so the offset rides in col_offset.  tower_count > 0 (with
// keep_coeff, uniform only): limbs [tower_first, tower_first + tower_count) alone are sampled, the rest of `out` is not
// written (gpupoly_matrix_sample_decomposed_window reads only the towers its window touches).
int sample_impl(GpuMatrix *out, int dist, double sigma, GpuRngSeed seed, size_t full_ncol, size_t col_offset, bool keep_coeff,
                size_t row_offset, uint32_t tower_first, uint32_t tower_count) {
    if (!out) return set_error("gpu_matrix_sample_distribution: null matrix");
    if (dist < GPU_MATRIX_DIST_UNIFORM || dist > GPU_MATRIX_DIST_TERNARY)
        return set_error("gpu_matrix_sample_distribution: invalid dist_type");
    if (dist == GPU_MATRIX_DIST_GAUSS && !(sigma > 0.0))
        return set_error("gpu_matrix_sample_distribution: sigma must be positive for Gaussian sampling");
    if (col_offset > full_ncol || out->cols > full_ncol - col_offset)  // the sum col_offset + cols can wrap in size_t
        return set_error("gpu_matrix_sample_distribution_columns: column window out of range");
    // stream ids (global polynomial index + 1) are 48 bits wide in the nonce layout of rng.h: refuse what would wrap
    const size_t row_limit = full_ncol ? ((size_t(1) << 48) - 2) / full_ncol : ~size_t(0);
    if (row_offset > row_limit || out->rows > row_limit - row_offset)
        return set_error("gpu_matrix_sample_distribution: matrix too large for the RNG's 48-bit stream ids");
    GpuContext *ctx = out->ctx;
    col_offset += row_offset * full_ncol;  // from here on only the kernels' index term
    out->format = keep_coeff ? GPU_POLY_FORMAT_COEFF : GPU_POLY_FORMAT_EVAL;
    const size_t polys = matrix_polys(out);
    if (polys == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const size_t total = polys * static_cast<size_t>(ctx->N);
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(out));
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const bool subset = keep_coeff && dist == GPU_MATRIX_DIST_UNIFORM && tower_count > 0 && tower_first + tower_count <= L;
    const uint32_t l0 = subset ? tower_first : 0u, Ls = subset ? tower_count : L;
    if (ctx->env.rng_compat) {
        const dim3 blocks = item_grid(total, 128);
        MXX_TRACE_BYTES(static_cast<double>(out->bytes) / L * (dist == GPU_MATRIX_DIST_UNIFORM ? Ls : L));
        if (ctx->wide)
            MXX_LAUNCH(sample_compat_kernel<uint64_t>, blocks, dim3(128), 0, ctx->stream, static_cast<uint64_t *>(words_ptr(out)), ctx->d_limbs,
                       polys, out->cols, full_ncol, col_offset, L, ctx->logN, dist, sigma, seed, l0, Ls);
        else
            MXX_LAUNCH(sample_compat_kernel<uint32_t>, blocks, dim3(128), 0, ctx->stream, static_cast<uint32_t *>(words_ptr(out)), ctx->d_limbs,
                       polys, out->cols, full_ncol, col_offset, L, ctx->logN, dist, sigma, seed, l0, Ls);
        HIP_TRY(hipGetLastError());
        if (keep_coeff) return 0;
        if (dist == GPU_MATRIX_DIST_UNIFORM && pack24_eligible(out)) return pack24_store(out, true);
        return launch_ntt(ctx, words_ptr(out), polys * L, static_cast<int>(L), false);
    }
    if (dist == GPU_MATRIX_DIST_GAUSS) {
        if (polys >> 32) return set_error("gpu_matrix_sample_distribution: too many polynomials");
        const uint32_t glog = ctx->logN < GAUSS_GROUP_LOG ? ctx->logN : GAUSS_GROUP_LOG;
        const size_t groups = total >> glog;
        const LanePlan plan = lane_plan(groups, static_cast<size_t>(ctx->N) >> glog,
                                        sampler_per_lane(groups, reinterpret_cast<const void *>(sample_gauss_kernel<KARNEY_SERVICES>), ctx->device, ctx->env.sampler_per_lane),
                                        false, ctx->env.sampler_fill_every, kCadenceGaussMatrix, true);
        const KarneyDivisor div = karney_divisor(sigma);
        const ChaChaKey key = chacha_subkey(seed, 0, kTagGauss);
        CtxBlock stage(ctx);
        if (stage.alloc(total * sizeof(int64_t))) return 1;
        MXX_TRACE_BYTES(static_cast<double>(total) * sizeof(int64_t));  // no input: the int64 samples written once
        MXX_LAUNCH_LANES_UNI(plan, ctx->stream, (sample_gauss_kernel<1, true>), (sample_gauss_kernel<1, false>),
                             (sample_gauss_kernel<KARNEY_SERVICES, true>), (sample_gauss_kernel<KARNEY_SERVICES, false>),
                             static_cast<int64_t *>(stage.ptr), polys, static_cast<uint32_t>(out->cols), full_ncol, col_offset, ctx->logN,
                             sigma, div, key, plan.per_lane, plan.fill_every, plan.starve_limit, NoSegments{});
        return finish_staged_i64(out, stage, hipGetLastError(), "err", !keep_coeff);
    } else {
        const bool uniform = dist == GPU_MATRIX_DIST_UNIFORM;
        const uint32_t groups = (N + 7) / 8;
        const uint32_t nkeys = uniform ? L : 1u;
        CtxBlock keys(ctx);  // per call: concurrent callers on one context must not share a key table
        if (keys.alloc(sizeof(ChaChaKey) * nkeys)) return 1;
        ChaChaKey *d_keys = static_cast<ChaChaKey *>(keys.ptr);
        const uint64_t tag = uniform ? kTagUniform : (dist == GPU_MATRIX_DIST_BIT ? kTagBit : kTagTernary);
        MXX_LAUNCH(derive_subkeys_kernel, dim3(1), dim3(64), 0, ctx->stream, d_keys, seed, tag, nkeys, uniform ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        const size_t threads = polys * (uniform ? Ls : 1u) * groups;
        const dim3 blocks = item_grid(threads, 256);
#define MXX_SAMPLE(KERNEL, WORD, ...)                                                                                     \
    MXX_LAUNCH(KERNEL<WORD>, dim3(blocks), dim3(256), 0, ctx->stream, static_cast<WORD *>(words_ptr(out)), ctx->d_limbs, \
                       d_keys, polys, out->cols, full_ncol, col_offset, L, N, groups, ##__VA_ARGS__)
        MXX_TRACE_BYTES(static_cast<double>(out->bytes) / L * (uniform ? Ls : L));  // no input: the residues written once
        if (uniform) {
            if (ctx->wide) MXX_SAMPLE(sample_uniform_kernel, uint64_t, l0, Ls);
            else MXX_SAMPLE(sample_uniform_kernel, uint32_t, l0, Ls);
        } else {
            if (ctx->wide) MXX_SAMPLE(sample_small_kernel, uint64_t, dist);
            else MXX_SAMPLE(sample_small_kernel, uint32_t, dist);
        }
#undef MXX_SAMPLE
    }
    HIP_TRY(hipGetLastError());
    if (keep_coeff) return 0;
    // samples are coefficients; callers always get EVAL (MatrixSampling.cu:463-469).  Uniform samples of a context whose
    // moduli fit 3 bytes are stored packed, the transform writing the packed rows (layout.hip)
    if (dist == GPU_MATRIX_DIST_UNIFORM && pack24_eligible(out)) return pack24_store(out, true);
    return launch_ntt(ctx, words_ptr(out), polys * L, static_cast<int>(L), false);
}

// ---- several independently seeded requests in one launch (rng.h, RngSegments) ---------------------------------------
// out = [S_0 | S_1 | ...], S_j = what gpu_matrix_sample_distribution writes for a rows x seg_cols[j] matrix under seeds[j].
// Gaussian only (the perturbation p2 of batched preimage requests); finishes in EVAL like the plain entry point.
extern "C" int gpupoly_matrix_sample_distribution_segments(GpuMatrix *out, int dist_type, double sigma, const GpuRngSeed *seeds,
                                                           const size_t *seg_cols, size_t nseg) {
    ABI_GUARD_BEGIN
    if (!out) return set_error("gpupoly_matrix_sample_distribution_segments: null matrix");
    if (dist_type != GPU_MATRIX_DIST_GAUSS)
        return set_error("gpupoly_matrix_sample_distribution_segments: unsupported: only the Gaussian distribution is segmented");
    if (!(sigma > 0.0)) return set_error("gpupoly_matrix_sample_distribution_segments: sigma must be positive for Gaussian sampling");
    GpuContext *ctx = out->ctx;
    if (ctx->env.rng_compat)
        return set_error("gpupoly_matrix_sample_distribution_segments: unsupported under MXX_HIP_RNG_COMPAT=reference");
    RngSegments segs;
    if (!rng_segments_build(segs, seeds, seg_cols, nseg, kTagGauss, out->cols))
        return set_error("gpupoly_matrix_sample_distribution_segments: segments must be 1..64, non-empty and cover the matrix's columns");
    const size_t polys = matrix_polys(out);
    const uint32_t glog = ctx->logN < GAUSS_GROUP_LOG ? ctx->logN : GAUSS_GROUP_LOG;
    const size_t groups_per_poly = static_cast<size_t>(ctx->N) >> glog;
    if (groups_per_poly % SAMPLER_THREADS)
        return set_error("gpupoly_matrix_sample_distribution_segments: unsupported: ring too small for a wave per polynomial chunk");
    if (polys >> 32) return set_error("gpupoly_matrix_sample_distribution_segments: too many polynomials");
    out->format = GPU_POLY_FORMAT_EVAL;
    if (polys == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const size_t total = polys * static_cast<size_t>(ctx->N);
    const size_t groups = total >> glog;
    const LanePlan plan = lane_plan(groups, groups_per_poly,
                                    sampler_per_lane(groups, reinterpret_cast<const void *>(sample_gauss_kernel<KARNEY_SERVICES, true, true>), ctx->device, ctx->env.sampler_per_lane),
                                    true, ctx->env.sampler_fill_every, kCadenceGaussMatrix, true);
    const KarneyDivisor div = karney_divisor(sigma);
    CtxBlock stage(ctx);
    if (stage.alloc(total * sizeof(int64_t))) return 1;
    MXX_TRACE_BYTES(static_cast<double>(total) * sizeof(int64_t));
    MXX_LAUNCH_LANES(plan, ctx->stream, (sample_gauss_kernel<1, true, true>), (sample_gauss_kernel<KARNEY_SERVICES, true, true>),
                     static_cast<int64_t *>(stage.ptr), polys, static_cast<uint32_t>(out->cols), out->cols, size_t(0), ctx->logN, sigma, div,
                     ChaChaKey{}, plan.per_lane, plan.fill_every, plan.starve_limit, segs);
    return finish_staged_i64(out, stage, hipGetLastError(), "err");
    ABI_GUARD_END
}

// ---- seeded blocks: uniform / bit / ternary samples of many independently seeded requests in one call (rng.h,
// RngBlockTable) -------------------------------------------------------------------------------
// The plain kernels' shape - a thread owns eight consecutive coefficients of one (polynomial, limb) vector, one keystream
// block in registers, 32 / 64 contiguous bytes stored per lane - with the sub-key and the stream id looked up per
// polynomial.  The look-up (a division, or a binary search in the start table: dependent loads) would sit in front of
// the block function of every thread; instead the first lanes of a workgroup resolve the few polynomials its 256 items
// touch (at most 256, one at n >= 2048) into LDS, once, and every thread then reads its polynomial's block and local
// index from there: the dependent chain in front of the generator is what the plain kernel has, a 32-byte key load.
__global__ void derive_block_subkeys_kernel(ChaChaKey *__restrict__ keys, const GpuRngSeed *__restrict__ seeds, uint64_t tag, size_t nblk,
                                            uint32_t per_block, uint32_t first_stream2) {
    const size_t i = item_index();
    if (i >= nblk * per_block) return;
    const size_t t = i / per_block;
    keys[i] = chacha_subkey(seeds[t], static_cast<uint64_t>(first_stream2) + (i - t * per_block), tag);
}

// the polynomials of this workgroup's items [base, base + 256) -> refs[p - *p_first]; false: no item (the whole workgroup leaves)
__device__ __forceinline__ bool resolve_blocks(const RngBlockTable &table, size_t total, size_t per_poly, RngBlockRef *refs, size_t *p_first) {
    const size_t base = item_index() - threadIdx.x;
    if (base >= total) return false;
    const size_t last = (total - base > blockDim.x ? base + blockDim.x : total) - 1;
    *p_first = base / per_poly;
    const size_t count = last / per_poly - *p_first + 1;  // <= blockDim.x: an item belongs to one polynomial
    if (threadIdx.x < count) refs[threadIdx.x] = rng_block_of(table, *p_first + threadIdx.x);
    __syncthreads();
    return true;
}

template <typename W>
__global__ void __launch_bounds__(256) sample_uniform_blocks_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs, RngBlockTable table,
                                                                    size_t polys, uint32_t L, uint32_t N, uint32_t groups /* ceil(N / 8) */) {
    __shared__ RngBlockRef refs[256];
    const size_t total = polys * L * groups;
    size_t p_first;
    if (!resolve_blocks(table, total, static_cast<size_t>(L) * groups, refs, &p_first)) return;
    const size_t idx = item_index();
    if (idx >= total) return;
    const size_t vec = idx / groups;  // (polynomial, limb) vector
    const uint32_t g = static_cast<uint32_t>(idx - vec * groups);
    const size_t p = vec / L;
    const uint32_t l = static_cast<uint32_t>(vec - p * L);
    const RngBlockRef ref = refs[p - p_first];
    const ChaChaKey key = load_key(table.keys + static_cast<size_t>(ref.blk) * L, l);
    const uint64_t q = limbs[l].q, mu64 = limbs[l].mu64;
    const uint64_t threshold = mu64 * q;  // as in sample_uniform_kernel
    uint64_t w[8];
    chacha_block_words(key, ref.local + 1, 0, g, w);
    const uint32_t count = min(8u, N - g * 8u);
    W r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint64_t x = w[j];
        if (x >= threshold && static_cast<uint32_t>(j) < count) x = uniform_overflow_draw(key, ref.local + 1, static_cast<uint64_t>(g) * 8u + j + 1, threshold);
        uint64_t rem = x - __umul64hi(x, mu64) * q;
        rem = rem >= q ? rem - q : rem;
        r[j] = static_cast<W>(rem);
    }
    store_group<W, 1>(out + vec * N + static_cast<size_t>(g) * 8u, r, count);
}

template <typename W>
__global__ void __launch_bounds__(256) sample_small_blocks_kernel(W *__restrict__ out, const LimbConst *__restrict__ limbs, RngBlockTable table,
                                                                  size_t polys, uint32_t L, uint32_t N, uint32_t groups, int dist) {
    __shared__ RngBlockRef refs[256];
    const size_t total = polys * groups;
    size_t p_first;
    if (!resolve_blocks(table, total, groups, refs, &p_first)) return;
    const size_t idx = item_index();
    if (idx >= total) return;
    const size_t p = idx / groups;
    const uint32_t g = static_cast<uint32_t>(idx - p * groups);
    const RngBlockRef ref = refs[p - p_first];
    const ChaChaKey key = load_key(table.keys + ref.blk, 0);
    sample_small_group<W>(out, limbs, key, ref.local + 1, p, g, L, N, dist);
}

// Both block entries: the argument checks in `entry`'s name, then the table, the launches and the finish.  The seeds of
// the table come either from the caller (`seeds`: staged and copied with the starts) or from (key, tags) on the device
// (`tags`: hash_seeds_kernel writes them, hash_seed.hip; the TABLE form's offsets and bytes are staged with the starts,
// the indexed forms stage nothing).  `hashed` says which of the two the entry takes; the other is null.
// `win` (the decomposed blocks, decompose.hip): `out` is the caller's coefficient scratch, rows x (nblk * win->cols), every
// block the window [col_offset, col_offset + cols) of its own rows x full_ncol matrix (the caller has checked the window);
// `layout` and `seg_cols` are not read, and the samples stay coefficients in words: no transform, no pack, tagged COEFF.
// `sigma` (the two Gaussian entries alone; `dist_type` is then not read, `win` is null): the Gaussian leg - one sub-key per
// block, the lane kernel into an int64 staging array, the plain sampler's scatter and transform.
int sample_blocks_impl(const char *entry, bool hashed, GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, const GpuHashTags *tags,
                       size_t nblk, int layout, const size_t *seg_cols, const RngBlockWindow *win, const double *sigma) {
    constexpr size_t kMaxBlocks = size_t(1) << 20, kStreamLimit = size_t(1) << 48;
    const auto refuse = [entry](const char *what) { return set_error(std::string(entry) + what); };
    if (!out) return refuse(": null matrix");
    if (!seeds && !tags) return refuse(hashed ? ": null tags" : ": null seeds");
    if (nblk == 0 || nblk > kMaxBlocks) return refuse(": the block count must be 1..2^20");
    if (!win && layout != GPUPOLY_BLOCKS_STACKED && layout != GPUPOLY_BLOCKS_COLUMNS) return refuse(": unknown layout");
    const bool gauss = sigma != nullptr;
    if (gauss) {
        if (!(*sigma > 0.0)) return refuse(": sigma must be positive for Gaussian sampling");
    } else {
        if (dist_type == GPU_MATRIX_DIST_GAUSS)
            return refuse(win ? ": unsupported: the Gaussian distribution has no block form"
                              : ": unsupported: the Gaussian distribution goes through gpupoly_matrix_sample_distribution_segments");
        if (dist_type < GPU_MATRIX_DIST_UNIFORM || dist_type > GPU_MATRIX_DIST_TERNARY) return refuse(": invalid dist_type");
    }
    GpuContext *ctx = out->ctx;
    if (ctx->env.rng_compat) return refuse(": unsupported under MXX_HIP_RNG_COMPAT=reference");
    const size_t pairs_per_poly = static_cast<size_t>(ctx->N) >> GAUSS_GROUP_LOG;
    if (gauss && (pairs_per_poly == 0 || pairs_per_poly % SAMPLER_THREADS))
        return refuse(": unsupported: ring too small for a wave per polynomial chunk");
    const bool columns = !win && layout == GPUPOLY_BLOCKS_COLUMNS;
    // a window's shape, its place inside full_ncol and the stream ids of the conceptual matrix are the caller's checks
    if (columns) {
        if (!seg_cols) return refuse(": the columns layout needs seg_cols");
        size_t at = 0, placed = 0;  // at <= out->cols
        for (size_t j = 0; j < nblk; ++j) {
            const size_t w = seg_cols[j];
            if (w == 0) return refuse(": a block of zero columns");
            if (out->rows && w > (kStreamLimit - 1) / out->rows) return refuse(": block too large for the RNG's 48-bit stream ids");
            if (w > out->cols - at) break;
            at += w;
            ++placed;
        }
        if (placed != nblk || at != out->cols) return refuse(": the blocks' widths must sum to the matrix's columns");
    } else if (!win) {
        if (seg_cols) return refuse(": the stacked layout takes no seg_cols");
        if (out->rows != nblk) return refuse(": the stacked layout wants one row per block");
        if (out->cols >= kStreamLimit) return refuse(": block too large for the RNG's 48-bit stream ids");
    }
    size_t tag_bytes = 0;
    if (tags && hash_tags_check(entry, tags, nblk, &tag_bytes)) return 1;
    const size_t polys = matrix_polys(out);
    if (gauss && polys >> 32) return refuse(": too many polynomials");
    if (polys == 0) {
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const bool uniform = !gauss && dist_type == GPU_MATRIX_DIST_UNIFORM;
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(out)), N = static_cast<uint32_t>(ctx->N), groups = (N + 7) / 8;
    const uint32_t per_block = uniform ? L : 1u;
    // the table: [keys][seeds][starts][tag offsets and bytes]; what the host knows of it goes up in one copy out of a staging
    // vector of this thread (the caller's arrays are not read after this call returns) - seeds and starts, or starts and
    // tags, in which case the seeds are hashed on the device -, the keys are derived from the seeds on the device
    const size_t key_bytes = sizeof(ChaChaKey) * nblk * per_block, seed_words = 4 * nblk, start_words = columns ? nblk + 1 : 0;
    const size_t tag_words = tags ? hash_tags_staged_words(tags, nblk, tag_bytes) : 0;
    CtxBlock block(ctx);
    if (block.alloc(key_bytes + sizeof(uint64_t) * (seed_words + start_words + tag_words))) return 1;
    const size_t given_words = seeds ? seed_words : 0;  // the staged words begin with the seeds, or right after them
    static thread_local std::vector<uint64_t> staging;
    staging.resize(given_words + start_words + tag_words);
    if (seeds)
        for (size_t j = 0; j < nblk; ++j)
            for (int i = 0; i < 4; ++i) staging[4 * j + i] = seeds[j].words[i];
    if (columns) {
        uint64_t at = 0;
        for (size_t j = 0; j < nblk; ++j) {
            staging[given_words + j] = at;
            at += seg_cols[j];
        }
        staging[given_words + nblk] = at;
    }
    if (tag_words) hash_tags_stage(tags, nblk, tag_bytes, staging.data() + given_words + start_words);
    char *base = static_cast<char *>(block.ptr);
    ChaChaKey *d_keys = reinterpret_cast<ChaChaKey *>(base);
    uint64_t *d_words = reinterpret_cast<uint64_t *>(base + key_bytes);
    GpuRngSeed *d_seeds = reinterpret_cast<GpuRngSeed *>(d_words);
    const uint64_t *d_starts = d_words + seed_words;
    void *words = words_ptr(out);
    if (!staging.empty())
        MXX_TRACED_COPY("seeded block table (host to device)", ctx->stream, sizeof(uint64_t) * staging.size(),
                        HIP_TRY(hipMemcpyAsync(d_words + (seed_words - given_words), staging.data(), sizeof(uint64_t) * staging.size(),
                                               hipMemcpyHostToDevice, ctx->stream)));
    if (tags && launch_hash_seeds(ctx, d_seeds, tags, nblk, d_starts + start_words)) return 1;
    const uint64_t tag = gauss ? kTagGauss : uniform ? kTagUniform : (dist_type == GPU_MATRIX_DIST_BIT ? kTagBit : kTagTernary);
    MXX_LAUNCH(derive_block_subkeys_kernel, item_grid(nblk * per_block, 256), dim3(256), 0, ctx->stream, d_keys, d_seeds, tag, nblk, per_block,
               uniform ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    out->format = win ? GPU_POLY_FORMAT_COEFF : GPU_POLY_FORMAT_EVAL;
    RngBlockTable table{d_keys, columns ? d_starts : nullptr, out->cols, static_cast<uint32_t>(nblk), per_block};
    if (win) {
        table.win_cols = win->cols;
        table.full_ncol = win->full_ncol;
        table.col_offset = win->col_offset;
    }
    if (gauss) {
        // the keys are sample_impl's, chacha_subkey(seed, 0, kTagGauss), one per block (gauss_blocks.hip has the kernel)
        const size_t total = polys * static_cast<size_t>(ctx->N);
        CtxBlock stage(ctx);
        if (stage.alloc(total * sizeof(int64_t))) return 1;
        MXX_TRACE_BYTES(static_cast<double>(total) * sizeof(int64_t));  // no input to speak of: the int64 samples written once
        launch_gauss_blocks(ctx, static_cast<int64_t *>(stage.ptr), polys, table, *sigma);
        return finish_staged_i64(out, stage, hipGetLastError(), "err");  // a Gaussian sample is never stored packed
    }
    const size_t threads = polys * per_block * groups;
    const dim3 blocks = item_grid(threads, 256);
    MXX_TRACE_BYTES(static_cast<double>(out->bytes));  // no input to speak of: the residues written once
    if (uniform) {
        if (ctx->wide)
            MXX_LAUNCH(sample_uniform_blocks_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(words), ctx->d_limbs, table, polys, L, N, groups);
        else
            MXX_LAUNCH(sample_uniform_blocks_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(words), ctx->d_limbs, table, polys, L, N, groups);
    } else {
        if (ctx->wide)
            MXX_LAUNCH(sample_small_blocks_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(words), ctx->d_limbs, table, polys, L, N, groups, dist_type);
        else
            MXX_LAUNCH(sample_small_blocks_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(words), ctx->d_limbs, table, polys, L, N, groups, dist_type);
    }
    HIP_TRY(hipGetLastError());
    if (win) return 0;
    // as the plain entry finishes: samples are coefficients, callers get EVAL; a packable uniform sample is stored packed
    if (uniform && pack24_eligible(out)) return pack24_store(out, true);
    return launch_ntt(ctx, words, polys * L, static_cast<int>(L), false);
}

extern "C" int gpupoly_matrix_sample_distribution_blocks(GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, size_t nblk, int layout,
                                                         const size_t *seg_cols) {
    ABI_GUARD_BEGIN
    return sample_blocks_impl("gpupoly_matrix_sample_distribution_blocks", false, out, dist_type, seeds, nullptr, nblk, layout, seg_cols, nullptr);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_sample_hash_blocks(GpuMatrix *out, int dist_type, const GpuHashTags *tags, size_t nblk, int layout,
                                                 const size_t *seg_cols) {
    ABI_GUARD_BEGIN
    return sample_blocks_impl("gpupoly_matrix_sample_hash_blocks", true, out, dist_type, nullptr, tags, nblk, layout, seg_cols, nullptr);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_sample_gauss_blocks(GpuMatrix *out, double sigma, const GpuRngSeed *seeds, size_t nblk, int layout,
                                                  const size_t *seg_cols) {
    ABI_GUARD_BEGIN
    return sample_blocks_impl("gpupoly_matrix_sample_gauss_blocks", false, out, GPU_MATRIX_DIST_GAUSS, seeds, nullptr, nblk, layout, seg_cols,
                              nullptr, &sigma);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_sample_hash_gauss_blocks(GpuMatrix *out, double sigma, const GpuHashTags *tags, size_t nblk, int layout,
                                                       const size_t *seg_cols) {
    ABI_GUARD_BEGIN
    return sample_blocks_impl("gpupoly_matrix_sample_hash_gauss_blocks", true, out, GPU_MATRIX_DIST_GAUSS, nullptr, tags, nblk, layout,
                              seg_cols, nullptr, &sigma);
    ABI_GUARD_END
}

// ---- detmath.h where it runs (extension, test instrument) ------------------------------------------------------
// Box-Muller's log / cos(2 pi u) are fixed IEEE operation sequences compiled into the device code; this entry evaluates
// them ON THE DEVICE for caller-supplied arguments so that a test can compare them with libm / extended precision
// (tests/test_gpu_sampler_stats.py: 10^7 points, <= 2 ulp; cos(2 pi x) <= 3 ulp) - the CPU-side check alone compares the header with itself.
__global__ void detmath_eval_kernel(double *__restrict__ out, const double *__restrict__ in, size_t n, int fn) {
    const size_t i = item_index();
    if (i >= n) return;
    const double x = in[i];
    out[i] = fn == 0 ? det_log(x) : (fn == 1 ? det_cos2pi(x) : sqrt(-2.0 * det_log(x)));
}

extern "C" int gpupoly_detmath_eval(GpuContext *ctx, int fn, const double *host_in, double *host_out, size_t n) {
    ABI_GUARD_BEGIN
    if (!ctx || !host_in || !host_out) return set_error("gpupoly_detmath_eval: null argument");
    if (fn < 0 || fn > 2) return set_error("gpupoly_detmath_eval: fn must be 0 (log), 1 (cos 2 pi u) or 2 (sqrt(-2 log u))");
    if (n == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    CtxBlock din(ctx), dout(ctx);
    if (din.alloc(n * sizeof(double)) || dout.alloc(n * sizeof(double))) return 1;
    HIP_TRY(hipMemcpyAsync(din.ptr, host_in, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MXX_LAUNCH(detmath_eval_kernel, item_grid(n, 256), dim3(256), 0, ctx->stream, static_cast<double *>(dout.ptr),
               static_cast<const double *>(din.ptr), n, fn);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_out, dout.ptr, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
    ABI_GUARD_END
}

extern "C" int gpu_matrix_sample_distribution(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed) {
    ABI_GUARD_BEGIN
    if (!out) return set_error("gpu_matrix_sample_distribution: null matrix");
    return sample_impl(out, dist_type, sigma, seed, out->cols, 0, false);
    ABI_GUARD_END
}

extern "C" int gpu_matrix_sample_distribution_columns(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed,
                                                      size_t full_ncol, size_t col_offset) {
    ABI_GUARD_BEGIN
    return sample_impl(out, dist_type, sigma, seed, full_ncol, col_offset, false);
    ABI_GUARD_END
}
