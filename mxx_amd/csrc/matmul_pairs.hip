// matmul_pairs.hip — every left operand against ITS OWN G^-1(B_j): gpupoly_matrix_mul_decompose_pairs.
//
//   outs[j] = addends[j] (+|-) (lhss[j] * G^-1(rhss[j][:, col_start .. col_start + c))) o scalars[j]        for all j < n
//
// The slot-transfer gate targets (src/slot_transfer/bgg_pubkey_gpu.rs:371-407,409-471, one per destination slot and column
// chunk of the wave sample_gate_batch_gpu builds at :842) each decompose a column chunk of their own matrix and multiply
// it by their own left operand: slice, inverse transform, digit kernel, forward transform, product, mul_scalar, sub per
// request.  Here the windows of all requests are gathered into ONE r x (n c) coefficient matrix (one launch, the source
// pointers in a device table), ONE fused digit transform (decompose.hip) turns it into the (r k) x (n c) EVAL digit matrix,
// and one grouped product per 64 operands reads it: operand j's tiles take the column panel [j c, (j + 1) c).
//
// Grouped product: as in matmul_group_kernel a descriptor per operand rides in the kernel-argument segment and the rows of
// all operands form one stacked left factor that is never materialised - but here a row tile must not straddle two
// operands (they read different panels of B), so every operand starts a tile of its own: `first` counts stacked rows with
// each operand padded to whole tiles, and the rows of the padding repeat the operand's last row and are never stored.  The
// epilogue reduces, multiplies the PRODUCT by the scalar (matmul_group_kernel multiplies the addend), adds it to or
// subtracts it from the addend and stores into the operand's own output.
#include "matmul_tile.h"

#include <algorithm>
#include <string>
#include <vector>

struct MulPairItem {
    const void *a;       // lhss[j], words
    void *c;             // outs[j], words
    const void *addend;  // addends[j] or null
    const void *scalar;  // scalars[j] (one polynomial) or null
    uint32_t rows;       // rows_j > 0
    uint32_t first;      // first stacked row of this operand, a multiple of the tile height
    uint32_t panel;      // its column panel of the digit matrix
    uint32_t pad_;
};
constexpr size_t kMulPairMax = 64;
struct MulPairArgs {
    MulPairItem item[kMulPairMax];  // 64 x 48 bytes
};
static_assert(sizeof(MulPairArgs) <= 4096 - 128, "descriptor table must fit the kernel-argument segment");

// one window of the gather: columns [col0, col0 + c) of a matrix with `stride` columns
struct PairWindow {
    const void *src;
    uint64_t stride, col0;
};

// dst (r x (np c) polynomials) <- the np windows of `table`, panel p at columns [p c, (p + 1) c); U: the copy unit, `units`
// of them per polynomial
template <typename U>
__global__ void __launch_bounds__(256)
    gather_windows_kernel(U *__restrict__ dst, const PairWindow *__restrict__ table, size_t r, size_t np, size_t c, size_t units) {
    const size_t idx = item_index();
    if (idx >= r * np * c * units) return;
    const size_t u = idx % units, poly = idx / units;  // poly = (i * np + p) * c + cc: the destination's own order
    const size_t cc = poly % c, ip = poly / c;
    const size_t p = ip % np, i = ip / np;
    const PairWindow w = table[p];
    dst[idx] = static_cast<const U *>(w.src)[(i * w.stride + w.col0 + cc) * units + u];
}

// B = the EVAL digit matrix, inner x bcols with bcols = panels * cw; operand j reads its columns [panel_j cw, (panel_j + 1) cw)
// and writes its rows_j x cw output.  blockIdx.y = column tile * row_tiles + row tile (matmul_group_kernel's order: the row
// tiles of one operand and column tile read the same panel of B).
template <typename W, int TR, int TC, int SV, bool NTB>
__global__ void __launch_bounds__(256)
    matmul_pairs_kernel(MulPairArgs args, uint32_t items, const W *__restrict__ B, const LimbConst *__restrict__ limbs,
                        uint32_t inner, uint32_t cw, uint32_t bcols, uint32_t L, uint32_t N, uint32_t row_tiles, uint32_t negate) {
    const uint32_t limb = blockIdx.z;
    const uint32_t ct = blockIdx.y / row_tiles, rt = blockIdx.y - ct * row_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * SV;
    if (i >= N) return;
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    typedef typename TileTypes<W, SV>::VT VT;
    typedef typename TileTypes<W, SV>::wxs wxs;
    typedef typename TileTypes<W, SV>::D D;

    const size_t poly = static_cast<size_t>(L) * N;  // words per polynomial
    const size_t in_poly = static_cast<size_t>(limb) * N + i;
    // the operand of this tile (uniform per workgroup): the last one that starts at or before its first row
    uint32_t j = 0;
    for (uint32_t t = 1; t < items; ++t)
        if (args.item[t].first <= r0) j = t;
    const MulPairItem it = args.item[j];
    const uint32_t local0 = r0 - it.first;  // < it.rows: the host pads every operand to whole tiles, no tile is all padding
    const W *a_ptr[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r)
        a_ptr[r] = static_cast<const W *>(it.a) + static_cast<size_t>(min(local0 + r, it.rows - 1)) * inner * poly + in_poly;
    size_t b_off[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) b_off[c] = (static_cast<size_t>(it.panel) * cw + min(c0 + c, cw - 1)) * poly + in_poly;
    const size_t strideBk = static_cast<size_t>(bcols) * poly;

    D acc[TR][TC][SV];
    MXX_TILE_CLEAR(acc);
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
#define MXX_TILE_A(r, k) (a_ptr[r] + (k) * poly)
#define MXX_TILE_B(c, k) (B + b_off[c] + (k) * strideBk)
#include "matmul_tile_loop.inc"
    // epilogue: reduce, o scalar, addend +|- it, store into the operand's own output
    W sv[SV];
    if (it.scalar) *reinterpret_cast<VT *>(sv) = *reinterpret_cast<const VT *>(static_cast<const W *>(it.scalar) + in_poly);
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (local0 + r >= it.rows) continue;
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            if (c0 + c >= cw) continue;
            const size_t off = (static_cast<size_t>(local0 + r) * cw + c0 + c) * poly + in_poly;
            W o[SV];
#pragma unroll
            for (int s = 0; s < SV; ++s) {
                o[s] = tile_reduce<W>(acc[r][c][s], q, lc);
                if (it.scalar) o[s] = mul_mod<W>(o[s], sv[s], q, lc.mu, lc.kbits);
            }
            if (it.addend) {
                W ad[SV];
                *reinterpret_cast<VT *>(ad) = *reinterpret_cast<const VT *>(static_cast<const W *>(it.addend) + off);
#pragma unroll
                for (int s = 0; s < SV; ++s) o[s] = negate ? sub_mod<W>(ad[s], o[s], q) : add_mod<W>(ad[s], o[s], q);
            } else if (negate) {
#pragma unroll
                for (int s = 0; s < SV; ++s) o[s] = o[s] ? q - o[s] : 0;
            }
            *reinterpret_cast<VT *>(static_cast<W *>(it.c) + off) = *reinterpret_cast<const VT *>(o);
        }
    }
}

// The tile of a launch: operands of at most `max_rows` rows, `total_rows` in all, against cw columns each.  The height
// follows the tallest operand (a taller tile would be padding); for 64-bit words stacked_tile's rule of how far the work
// fills the chip is asked with all the rows of the launch.
static TileShape pairs_tile(const GpuContext *ctx, uint64_t total_rows, uint64_t max_rows, uint64_t cw, uint64_t L) {
    if (!ctx->wide) return stacked_tile(ctx, max_rows, cw, L);
    TileShape t = stacked_tile(ctx, total_rows, cw, L);
    if (t.tc == 4) t.tr = std::min<uint32_t>(t.tr, max_rows >= 4 ? 4u : (max_rows >= 2 ? 2u : 1u));
    else if (max_rows < 2) t = {1, 1};
    return t;
}

// stacked rows of a launch with every operand padded to whole tiles
static uint64_t padded_rows(const std::vector<uint32_t> &rows, uint32_t tr) {
    uint64_t total = 0;
    for (uint32_t h : rows) total += (static_cast<uint64_t>(h) + tr - 1) / tr * tr;
    return total;
}

template <typename W, int TR, int TC, int SV>
static int launch_pairs_cfg(GpuContext *ctx, MulPairArgs &args, uint32_t items, const void *b, size_t b_bytes, uint32_t inner,
                            uint32_t cw, uint32_t bcols, uint32_t L, bool negate) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    uint32_t first = 0;
    bool one_tile_each = true;
    for (uint32_t t = 0; t < items; ++t) {
        args.item[t].first = first;
        first += (args.item[t].rows + TR - 1) / TR * TR;
        one_tile_each = one_tile_each && args.item[t].rows <= TR;
    }
    const TileGrid g = tile_grid<TR, TC, SV>(ctx, first, cw, L, b_bytes);  // its y extent: checked before the first launch
    static const std::string name = std::string("matmul_pairs_kernel<") + (sizeof(W) == 4 ? "u32," : "u64,") + std::to_string(TR) + "," +
                                    std::to_string(TC) + "," + std::to_string(SV) +
                                    "> (row tiles of up to 64 operands x their own digit panel x slots per lane, scalar and addend in the epilogue)";
    ctx->last_kernel = name.c_str();
    const W *bw = static_cast<const W *>(b);
    bool streamed = false;  // the 64-bit tiles have no non-temporal instance
    if constexpr (sizeof(W) == 4) {
        // every panel is read by one row tile per column tile, and B cannot stay in the Infinity Cache (tile_grid's rule)
        if (one_tile_each && b_bytes > (size_t(1) << 28)) {
            streamed = true;
            MXX_LAUNCH((matmul_pairs_kernel<W, TR, TC, SV, true>), g.grid, dim3(g.threads), 0, ctx->stream, args, items, bw, ctx->d_limbs, inner,
                       cw, bcols, L, N, g.row_tiles, negate ? 1u : 0u);
        }
    }
    if (!streamed)
        MXX_LAUNCH((matmul_pairs_kernel<W, TR, TC, SV, false>), g.grid, dim3(g.threads), 0, ctx->stream, args, items, bw, ctx->d_limbs, inner, cw,
                   bcols, L, N, g.row_tiles, negate ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_pairs(GpuContext *ctx, MulPairArgs &args, uint32_t items, TileShape tile, const void *b, size_t b_bytes, uint32_t inner,
                        uint32_t cw, uint32_t bcols, uint32_t L, bool negate) {
    return dispatch_stacked_tile(ctx, tile, [&](auto cfg) {
        typedef decltype(cfg) T;
        return launch_pairs_cfg<typename T::W, T::TR, T::TC, T::SV>(ctx, args, items, b, b_bytes, inner, cw, bcols, L, negate);
    });
}

// dst (r x (np c), words) <- the windows of `wins`, through a device table that lives until the launch has read it
static int gather_windows(GpuContext *ctx, void *dst, const std::vector<PairWindow> &wins, size_t r, size_t c, size_t poly_bytes) {
    const size_t np = wins.size();
    CtxBlock table(ctx);  // stream-ordered: back to the cache behind the launch below
    if (table.alloc(np * sizeof(PairWindow))) return 1;
    MXX_TRACED_COPY("window table (host to device)", ctx->stream, np * sizeof(PairWindow),
                    HIP_TRY(hipMemcpyAsync(table.ptr, wins.data(), np * sizeof(PairWindow), hipMemcpyHostToDevice, ctx->stream)));
    MXX_TRACE_BYTES(2.0 * static_cast<double>(r * np * c * poly_bytes));
    const PairWindow *d_table = static_cast<const PairWindow *>(table.ptr);
    if (poly_bytes % 16 == 0) {
        const size_t units = poly_bytes / 16;
        MXX_LAUNCH(gather_windows_kernel<uint4>, item_grid(r * np * c * units, 256), dim3(256), 0, ctx->stream, static_cast<uint4 *>(dst), d_table, r,
                   np, c, units);
    } else {
        const size_t units = poly_bytes / 4;
        MXX_LAUNCH(gather_windows_kernel<uint32_t>, item_grid(r * np * c * units, 256), dim3(256), 0, ctx->stream, static_cast<uint32_t *>(dst),
                   d_table, r, np, c, units);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int gpupoly_matrix_mul_decompose_pairs(GpuMatrix *const *outs, const GpuMatrix *const *addends, const GpuMatrix *const *lhss,
                                                  const GpuMatrix *const *rhss, const GpuMatrix *const *scalars, size_t n, size_t col_start,
                                                  uint32_t base_bits, int negate) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_mul_decompose_pairs";
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    if (n == 0) return 0;
    if (!outs || !lhss || !rhss) return refuse("null array");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    for (size_t j = 0; j < n; ++j)
        if (!outs[j] || !lhss[j] || !rhss[j]) return refuse("null matrix (operand " + std::to_string(j) + ")");
    GpuContext *ctx = rhss[0]->ctx;
    const int level = rhss[0]->level;
    const size_t L = matrix_limbs(rhss[0]);
    const size_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t r = rhss[0]->rows, m = rhss[0]->cols, c = outs[0]->cols;
    const size_t inner = r * dpt * L;
    // ---- every refusal, for every j, before the first launch ----
    if (col_start > m || c > m - col_start) return refuse("column window past the right operands' columns");
    uint64_t total_rows = 0;
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *out = outs[j], *lhs = lhss[j], *rhs = rhss[j];
        const GpuMatrix *add = addends ? addends[j] : nullptr, *sc = scalars ? scalars[j] : nullptr;
        const std::string at = " (operand " + std::to_string(j) + ")";
        if (out->ctx != ctx || lhs->ctx != ctx || rhs->ctx != ctx || (add && add->ctx != ctx) || (sc && sc->ctx != ctx))
            return refuse("context mismatch" + at);
        if (out->level != level || lhs->level != level || rhs->level != level || (add && add->level != level) || (sc && sc->level != level))
            return refuse("level mismatch" + at);
        if (rhs->rows != r || rhs->cols != m) return refuse("right operand shape mismatch" + at);
        if (out->cols != c) return refuse("output width mismatch" + at);
        if (lhs->cols != inner || out->rows != lhs->rows) return refuse("shape mismatch" + at);
        if (add && (add->rows != lhs->rows || add->cols != c)) return refuse("addend shape mismatch" + at);
        if (sc && (sc->rows != 1 || sc->cols != 1)) return refuse("scalar must be 1x1" + at);
        if (lhs->format != GPU_POLY_FORMAT_EVAL || (add && add->format != GPU_POLY_FORMAT_EVAL) || (sc && sc->format != GPU_POLY_FORMAT_EVAL))
            return refuse("requires Eval format" + at);
        total_rows += lhs->rows;
    }
    for (size_t j = 0; j < n; ++j) {  // an output is written while every input is still being read
        const GpuMatrix *out = outs[j];
        for (size_t o = 0; o < n; ++o) {
            if (o != j && storage_overlaps(out, outs[o])) return refuse("an output aliases another output");
            if (storage_overlaps(out, lhss[o]) || storage_overlaps(out, rhss[o]) || (scalars && scalars[o] && storage_overlaps(out, scalars[o])))
                return refuse("an output aliases an input");
            if (addends && addends[o] && storage_overlaps(out, addends[o]) && !(o == j && same_block(out, addends[o])))
                return refuse("an output aliases an addend that is not its own block");
        }
    }
    if (total_rows > 0x7fffffffull || inner > 0xffffffffull || m > 0xffffffffull) return refuse("matrix too large");
    // the operands with rows: the others have nothing to read or write
    std::vector<size_t> act;
    for (size_t j = 0; j < n; ++j)
        if (lhss[j]->rows) act.push_back(j);
    const bool work = !act.empty() && c > 0;
    if (work && ctx_activate(ctx)) return 1;
    const size_t poly_bytes = L * static_cast<size_t>(ctx->N) * ctx->word_bytes;
    // operand groups whose digit matrix fits the budget: gpupoly_matrix_mul_decompose_many's rule (a third of what the
    // device could give us now, at least 8 GiB), or MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET; the cut is between operands
    size_t per_group = act.size();
    if (work && inner > 0) {
        size_t budget = ctx->env.mul_decompose_pairs_budget;
        if (budget == 0) {
            size_t free_b = 0, total_b = 0;
            budget = size_t(8) << 30;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::max(budget, (free_b + ctx->cached_bytes) / 3);
            else (void)hipGetLastError();
        }
        per_group = std::min(act.size(), std::max<size_t>(1, budget / inner / c / poly_bytes));
        if (per_group * c > 0xffffffffull) per_group = 0xffffffffull / c;
    }
    // launches: up to 64 operands of one group each; tile and grid extent of every one
    struct Launch {
        size_t begin, count;  // in `act`
        TileShape tile;
    };
    std::vector<Launch> launches;
    if (work) {
        for (size_t g0 = 0; g0 < act.size(); g0 += per_group)
            for (size_t l0 = g0; l0 < std::min(act.size(), g0 + per_group); l0 += kMulPairMax) {
                Launch la;
                la.begin = l0;
                la.count = std::min<size_t>(kMulPairMax, std::min(act.size(), g0 + per_group) - l0);
                std::vector<uint32_t> rows(la.count);
                uint64_t sum = 0, tallest = 0;
                for (size_t t = 0; t < la.count; ++t) {
                    rows[t] = static_cast<uint32_t>(lhss[act[l0 + t]]->rows);
                    sum += rows[t];
                    tallest = std::max<uint64_t>(tallest, rows[t]);
                }
                la.tile = pairs_tile(ctx, sum, tallest, c, L);
                const uint64_t padded = padded_rows(rows, la.tile.tr);
                if (padded > 0xffffffffull || !tile_grid_fits(padded, c, la.tile.tr, la.tile.tc)) return refuse("matrix too large");
                launches.push_back(la);
            }
    }
    // ---- accepted ----
    for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    if (!work) return 0;
    int rc = 0;
    size_t next_launch = 0;
    for (size_t g0 = 0; !rc && g0 < act.size(); g0 += per_group) {
        const size_t np = std::min(per_group, act.size() - g0);
        GpuMatrix *win = nullptr, *dec = nullptr, *evals = nullptr;
        if (inner > 0) {
            // the windows of this group, PACKED24 sources unpacked first, once (words_ptr)
            std::vector<PairWindow> wins(np), eval_wins;
            std::vector<size_t> eval_at;
            for (size_t p = 0; p < np; ++p) {
                const GpuMatrix *rhs = rhss[act[g0 + p]];
                wins[p] = PairWindow{words_ptr(rhs), m, col_start};
                if (rhs->format == GPU_POLY_FORMAT_EVAL) eval_at.push_back(p);
            }
            const bool mixed = !eval_at.empty() && eval_at.size() != np;
            if (mixed) {  // the EVAL windows alone go to the coefficient domain first; the gather below reads them there
                rc = gpu_matrix_create(ctx, level, r, eval_at.size() * c, GPU_POLY_FORMAT_EVAL, &evals);
                if (!rc) {
                    for (size_t e = 0; e < eval_at.size(); ++e) {
                        eval_wins.push_back(wins[eval_at[e]]);
                        wins[eval_at[e]] = PairWindow{words_ptr(evals), eval_at.size() * c, e * c};
                    }
                    rc = gather_windows(ctx, words_ptr(evals), eval_wins, r, c, poly_bytes);
                }
                if (!rc) rc = launch_ntt(ctx, words_ptr(evals), r * eval_at.size() * c * L, static_cast<int>(L), true);
            }
            // one gather; an all-EVAL group is tagged EVAL and the digit transform's entry takes it through ONE out-of-place
            // inverse transform (decompose_core)
            if (!rc) rc = gpu_matrix_create(ctx, level, r, np * c, (eval_at.size() == np) ? GPU_POLY_FORMAT_EVAL : GPU_POLY_FORMAT_COEFF, &win);
            if (!rc) rc = gather_windows(ctx, words_ptr(win), wins, r, c, poly_bytes);
            if (!rc) rc = gpu_matrix_create(ctx, level, inner, np * c, GPU_POLY_FORMAT_EVAL, &dec);
            if (!rc) rc = gpu_matrix_decompose_base(win, base_bits, dec);  // EVAL: the fused digit transform
        }
        for (; !rc && next_launch < launches.size() && launches[next_launch].begin < g0 + np; ++next_launch) {
            const Launch &la = launches[next_launch];
            MulPairArgs args;
            double bytes = 0.0;
            for (size_t t = 0; t < la.count; ++t) {
                const size_t j = act[la.begin + t];
                const GpuMatrix *add = addends ? addends[j] : nullptr, *sc = scalars ? scalars[j] : nullptr;
                MulPairItem &it = args.item[t];
                it.a = words_ptr(lhss[j]);
                it.c = words_ptr(outs[j]);
                it.addend = add ? words_ptr(add) : nullptr;
                it.scalar = sc ? words_ptr(sc) : nullptr;
                it.rows = static_cast<uint32_t>(lhss[j]->rows);
                it.first = 0;  // set for the tile height by the launcher
                it.panel = static_cast<uint32_t>(la.begin + t - g0);
                it.pad_ = 0;
                bytes += static_cast<double>(lhss[j]->bytes) + (sc ? static_cast<double>(sc->bytes) : 0.0) +
                         static_cast<double>(outs[j]->bytes) * (add ? 2.0 : 1.0) + static_cast<double>(inner * c * poly_bytes);
            }
            MXX_TRACE_BYTES(bytes);
            rc = launch_pairs(ctx, args, static_cast<uint32_t>(la.count), la.tile, dec ? words_ptr(dec) : nullptr, dec ? dec->bytes : 0,
                              static_cast<uint32_t>(inner), static_cast<uint32_t>(c), static_cast<uint32_t>(np * c), static_cast<uint32_t>(L),
                              negate != 0);
        }
        gpu_matrix_destroy(evals);  // stream-ordered: behind the launches that read them
        gpu_matrix_destroy(win);
        gpu_matrix_destroy(dec);
    }
    return rc;
    ABI_GUARD_END
}
