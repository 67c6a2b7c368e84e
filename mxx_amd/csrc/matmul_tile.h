// matmul_tile.h — what the register-tiled products share: matmul_kernel (arith.hip), matmul_group_kernel
// (matmul_group.hip), matmul_sum_kernel (matmul_sum.hip).
//
// A lane holds a TR x TC tile of outputs for SV consecutive slots of one limb in lazy accumulators (64-bit for 32-bit
// words, 128-bit for 64-bit words) and reduces them once per LimbConst::lazy_terms products: at most that many products
// enter an accumulator between two reductions, wherever the including kernel's operands change.
//
// Device side: the types, the reduction, the KU rule and the accumulator clear here; the accumulate loop itself in
// matmul_tile_loop.inc.  The loop and the clear are text that a kernel includes, not functions: a __forceinline__ function
// around either is allocated registers differently (the loop: 255 instead of 153 VGPRs and one wave per SIMD instead of
// three for matmul_sum_kernel's 8-row tile), while the text compiles to the very bytes of a loop written in place
// (profiles/matmul_tile_refactor.txt).
// Host side: the tile rule for rows stacked against columns, the grid with its streamed-once hint and its limit, and the
// dispatch from a tile to its instantiation.
#pragma once
#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <type_traits>

// ---- device -------------------------------------------------------------------------------------
// VT: the SV words of a lane as one load / store; wxs: the same as a vector the non-temporal builtin takes; D: accumulator
template <typename W, int SV>
struct TileTypes {
    typedef typename std::conditional<sizeof(W) * SV == 16, uint4, typename std::conditional<sizeof(W) * SV == 8, uint2, W>::type>::type VT;
    static_assert(sizeof(VT) == sizeof(W) * SV, "vector width");
    typedef W wxs __attribute__((ext_vector_type(SV)));
    typedef typename Wide<W>::type D;
};

// inner steps whose operands are loaded before any of them is multiplied: small tiles are latency-bound (one dependent
// pair of loads per step), large ones have no registers to spare.  A kernel may set MXX_TILE_KU to a rule of its own.
template <typename W, int TR, int TC, int SV>
constexpr uint32_t kTileKU = TR * TC * SV <= 8 ? 8 : (TR * TC * SV * sizeof(W) <= 128 ? 2 : 1);

// zeroes D acc[TR][TC][SV]
#define MXX_TILE_CLEAR(acc)                                                                        \
    _Pragma("unroll") for (int r = 0; r < TR; ++r) _Pragma("unroll") for (int c = 0; c < TC; ++c) \
        _Pragma("unroll") for (int s = 0; s < SV; ++s) acc[r][c][s] = 0

// a lazy accumulator back into [0, q), q = lc.q: modarith.h's lazy_reduce under the name the tiled kernels call it by.
// The second parameter is vestigial - the call sites still pass their q, which lazy_reduce takes from lc
template <typename W>
__device__ __forceinline__ W tile_reduce(typename Wide<W>::type v, W, const LimbConst &lc) {
    return lazy_reduce<W>(v, lc);
}

// ---- host ---------------------------------------------------------------------------------------
// register tile: rows x columns of outputs (the slots per lane follow in dispatch_stacked_tile)
struct TileShape {
    uint32_t tr, tc;
};
template <typename W_, int TR_, int TC_, int SV_>
struct TileCfg {
    typedef W_ W;
    static constexpr int TR = TR_, TC = TC_, SV = SV_;
};

// the tile for `rows` (stacked) rows against `cols` columns: gpu_matrix_mul's 64-bit products, and both word widths of
// the grouped and the summed product
inline TileShape stacked_tile(const GpuContext *ctx, uint64_t rows, uint64_t cols, uint64_t L) {
    const uint64_t N = static_cast<uint64_t>(ctx->N);
    if (ctx->wide) {
        // small rings (BASELINE configs[4]: n = 256): a register tile per thread leaves most of the chip idle -
        // (2x72)*(72x4) at L = 12 is 24 waves of 4x4x2 tiles.  Below ~2 waves per SIMD of tiled work, shrink the
        // tile until the grid covers the chip (every output then re-reads its operands from L2, which is cheap there).
        const uint64_t slots = N * L;
        const uint64_t want = 1024ull * 2 * 64;  // lanes for two waves on every SIMD
        if (N >= 2 && slots / 2 * ((rows + 3) / 4) * ((cols + 3) / 4) >= want) return {rows >= 4 ? 4u : (rows >= 2 ? 2u : 1u), 4};
        if (slots * ((rows + 1) / 2) * ((cols + 1) / 2) >= want) return {2, 2};
        return {1, 1};
    }
    if (N >= 4 && rows <= 2) return {static_cast<uint32_t>(rows), 8};  // 16-byte loads: B is streamed once
    return {rows <= 4 ? 4u : 8u, 8};  // 5 and more: 8-row tiles, B is read once per 8 stacked rows
}

// f(TileCfg<W, TR, TC, SV>()) for a tile that stacked_tile chose
template <typename F>
int dispatch_stacked_tile(const GpuContext *ctx, TileShape t, F &&f) {
    if (ctx->wide) {
        if (t.tc == 4) {
            if (t.tr == 4) return f(TileCfg<uint64_t, 4, 4, 2>());
            if (t.tr == 2) return f(TileCfg<uint64_t, 2, 4, 2>());
            return f(TileCfg<uint64_t, 1, 4, 2>());
        }
        if (t.tr == 2) return f(TileCfg<uint64_t, 2, 2, 1>());
        return f(TileCfg<uint64_t, 1, 1, 1>());
    }
    if (t.tr == 1) return f(TileCfg<uint32_t, 1, 8, 4>());
    if (t.tr == 2) return f(TileCfg<uint32_t, 2, 8, 4>());
    if (t.tr == 4) return f(TileCfg<uint32_t, 4, 8, 1>());
    return f(TileCfg<uint32_t, 8, 8, 1>());
}

// the grid's y extent holds row tiles x column tiles: tile_grid_fits (grid_plan.h)

// x: slots (SV per lane), y: row tiles x column tiles (tile_grid_fits is the caller's to check), z: limbs
struct TileGrid {
    dim3 grid;
    uint32_t threads, row_tiles, col_tiles;
    // one row tile, and a B that cannot stay in the 256 MB Infinity Cache: B is then read exactly once, and non-temporal
    // loads keep it from displacing A, which every column tile re-reads (matmul_kernel has the figures)
    bool streamed;
};
template <int TR, int TC, int SV>
TileGrid tile_grid(const GpuContext *ctx, uint32_t rows, uint32_t cols, uint32_t L, size_t b_bytes) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    TileGrid g;
    g.row_tiles = (rows + TR - 1) / TR;
    g.col_tiles = (cols + TC - 1) / TC;
    g.threads = std::min<uint32_t>(256, std::max<uint32_t>(64, N / SV));
    g.grid = dim3((N / SV + g.threads - 1) / g.threads, g.row_tiles * g.col_tiles, L);
    g.streamed = g.row_tiles == 1 && b_bytes > (size_t(1) << 28);
    return g;
}
