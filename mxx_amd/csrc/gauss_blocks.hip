// gauss_blocks.hip - Gaussian seeded blocks: the lane kernel behind gpupoly_matrix_sample_gauss_blocks and
// gpupoly_matrix_sample_hash_gauss_blocks.  The entries, the table and the finish are
// sample_blocks_impl's (sampling.hip).
#include "common.h"
#include "rng.h"

// The block form of sample_gauss_kernel<., true, true>: the same one-wave workgroups and persistent lanes, a stream per
// pair of coefficients, the int64 staging array - with the sub-key and the stream id of the wave's polynomial looked up in
// an RngBlockTable in device memory instead of the 2 KB kernel argument.  A wave's chunk lies inside one polynomial (the
// launcher cuts per_lane down to a divisor, as for the segments), so inside one block: the look-up - a division, or the
// binary search in `starts` - runs once per wave on wave-uniform values, and the block's eight key dwords are read once
// into scalar registers; lanes then open streams (local + 1, pair + 1) under that key - exactly what the plain kernel
// opens for the block sampled alone under chacha_subkey(seed, 0, kTagGauss).  The lanes' loop is sample_gauss_kernel's,
// restated, and the kernel has this translation unit to itself: a helper shared with sample_gauss_kernel, and even a
// further kernel in sampling.hip's code object, changed the ISA text of the kernels there (tried), by which the counter
// records under profiles/ are versioned (mxx_amd/codeobj.py).
template <int SV>
__global__ void __launch_bounds__(SAMPLER_THREADS) sample_gauss_blocks_kernel(int64_t *__restrict__ stage, size_t polys, RngBlockTable table,
                                    uint32_t logN, double sigma, KarneyDivisor div, uint32_t per_lane, uint32_t fill_every,
                                    int starve_limit) {
    __shared__ uint32_t ring[SAMPLER_THREADS * RNG_RING_SLOTS];  // 128 bytes per lane: 8 KB per one-wave workgroup
    constexpr uint32_t glog = GAUSS_GROUP_LOG, G = 1u << glog;   // the launcher refuses rings below 64 pairs
    const size_t total = (polys << logN) >> glog;                // groups
    WaveChunk chunk = wave_chunk(total, per_lane);
    if (chunk.len == 0) return;  // the whole one-wave workgroup: no polynomial, so no table entry to read
    const uint32_t p_u = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(chunk.base >> (logN - glog))));
    const RngBlockRef ref = rng_block_of(table, p_u);
    const uint32_t blk_u = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(ref.blk));
    const uint64_t stream0_u = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(ref.local)))) |
                                static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(ref.local >> 32)))) << 32) + 1;
    const uint32_t *kw = reinterpret_cast<const uint32_t *>(table.keys + blk_u);
    ChaChaKey key;
#pragma unroll
    for (int i = 0; i < 8; ++i) key.w[i] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(kw[i]));
    ChaChaRng rng;
    rng_init_keyed(rng, ring, key, 0, 0, SAMPLER_THREADS);
    KarneyFsm f;
    karney_reset(f);
    karney_fix_parameters(f, 0.0, sigma, div);
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
                    rng_reopen(rng, stream0_u, (idx & ((size_t(1) << (logN - glog)) - 1)) + 1);
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

// The segments entry's plan: a wave's chunk stays inside one polynomial, i.e. inside one block, and the grid is exact (no
// empty wave).  The caller has checked that a polynomial holds a multiple of 64 pairs and that there are at most 2^32
// polynomials.
void launch_gauss_blocks(GpuContext *ctx, int64_t *stage, size_t polys, const RngBlockTable &table, double sigma) {
    const size_t pairs_per_poly = static_cast<size_t>(ctx->N) >> GAUSS_GROUP_LOG, pairs = polys * pairs_per_poly;
    const LanePlan plan = lane_plan(pairs, pairs_per_poly,
                                    sampler_per_lane(pairs, reinterpret_cast<const void *>(sample_gauss_blocks_kernel<KARNEY_SERVICES>), ctx->device,
                                                     ctx->env.sampler_per_lane),
                                    true, ctx->env.sampler_fill_every, kCadenceGaussMatrix, true);
    MXX_LAUNCH_LANES(plan, ctx->stream, (sample_gauss_blocks_kernel<1>), (sample_gauss_blocks_kernel<KARNEY_SERVICES>), stage, polys, table,
                     ctx->logN, sigma, karney_divisor(sigma), plan.per_lane, plan.fill_every, plan.starve_limit);
}
