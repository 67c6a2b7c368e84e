// matmul_group.hip — several left operands against ONE G^-1(B): gpupoly_matrix_mul_decompose_many.
//
//   outs[j] = lhss[j] * G^-1(rhs) + addends[j] o scalars[j]        for all j < n
//
// The BGG multiplication gates hand the same right operand to mul_decompose again and again
// (src/bgg/encoding.rs:125-145,191-219: vector and public-key matrix against one other.pubkey.matrix;
// src/bgg/poly_encoding.rs:327-357: once per slot plus once for the key; src/io/diamond_io.rs:1924-1926,
// src/we/diamond_we.rs:456,538), each followed by `+ other.vector * plaintext`.  The digit transforms are the expensive
// half of a mul_decompose, so here G^-1(rhs) is built once per call - in as few column chunks as the memory
// budget allows - and one grouped product reads it for every operand.
//
// Grouped product: the rows of all operands form one stacked left factor that is never materialised.  A descriptor per
// operand (A, C, addend, scalar pointers, row count, first stacked row) rides in the kernel-argument segment like
// MulBatchArgs (arith.hip); a workgroup takes a TR x TC tile of stacked rows x digit-matrix columns for one limb and a
// run of slots, looks its TR rows up in the table (uniform per workgroup: scalar loads), accumulates with the shared
// register-tile loop (matmul_tile.h, which also chooses the tile and the grid) and, in the epilogue, reduces, adds addend o scalar where present and stores into the operand's own
// output at columns [c0, c0 + cw).  No stacking copy, no split copy, no mul_scalar or add launch.
#include "matmul_tile.h"

#include <algorithm>
#include <string>
#include <vector>

struct MulGroupItem {
    const void *a;       // lhss[j], words
    void *c;             // outs[j], words
    const void *addend;  // addends[j] or null
    const void *scalar;  // scalars[j] (one polynomial) or null
    uint32_t rows;       // rows_j > 0
    uint32_t first;      // first stacked row of this operand
};
constexpr size_t kMulGroupMax = 64;
struct MulGroupArgs {
    MulGroupItem item[kMulGroupMax];  // 64 x 40 bytes
};
static_assert(sizeof(MulGroupArgs) <= 4096 - 128, "descriptor table must fit the kernel-argument segment");

// B = the EVAL digit matrix of one column chunk, inner x cw.  The outputs are rows_j x out_cols; this launch writes their
// columns [col0, col0 + cw).  blockIdx.y = column tile * row_tiles + row tile: the row tiles of one column tile - they
// read the same panel of B - are neighbours in dispatch order, so all but the first find it in cache.
template <typename W, int TR, int TC, int SV, bool NTB>
__global__ void __launch_bounds__(256)
    matmul_group_kernel(MulGroupArgs args, uint32_t items, const W *__restrict__ B, const LimbConst *__restrict__ limbs,
                        uint32_t total_rows, uint32_t inner, uint32_t cw, uint32_t col0, uint32_t out_cols, uint32_t L,
                        uint32_t N, uint32_t row_tiles) {
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
    // the TR stacked rows of this tile: operand and row inside it (rows past the end repeat the last one, never stored)
    const W *a_ptr[TR];
    size_t out_off[TR];  // (row * out_cols + col0 + c0) polynomials into c / addend, + limb and slot
    uint32_t which[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const uint32_t rr = min(r0 + r, total_rows - 1);
        uint32_t j = 0;
        for (uint32_t t = 1; t < items; ++t)
            if (args.item[t].first <= rr) j = t;
        const uint32_t local = rr - args.item[j].first;
        which[r] = j;
        a_ptr[r] = static_cast<const W *>(args.item[j].a) + static_cast<size_t>(local) * inner * poly + in_poly;
        out_off[r] = (static_cast<size_t>(local) * out_cols + col0 + c0) * poly + in_poly;
    }
    size_t b_off[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) b_off[c] = static_cast<size_t>(min(c0 + c, cw - 1)) * poly + in_poly;
    const size_t strideBk = static_cast<size_t>(cw) * poly;

    D acc[TR][TC][SV];
    MXX_TILE_CLEAR(acc);
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
#define MXX_TILE_A(r, k) (a_ptr[r] + (k) * poly)
#define MXX_TILE_B(c, k) (B + b_off[c] + (k) * strideBk)
#include "matmul_tile_loop.inc"
    // epilogue: reduce, + addend o scalar, store into the operand's own output
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (r0 + r >= total_rows) continue;
        const MulGroupItem it = args.item[which[r]];
        W sv[SV];
        if (it.scalar) *reinterpret_cast<VT *>(sv) = *reinterpret_cast<const VT *>(static_cast<const W *>(it.scalar) + in_poly);
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            if (c0 + c >= cw) continue;
            const size_t off = out_off[r] + static_cast<size_t>(c) * poly;
            W o[SV];
#pragma unroll
            for (int s = 0; s < SV; ++s) o[s] = tile_reduce<W>(acc[r][c][s], q, lc);
            if (it.addend) {
                W ad[SV];
                *reinterpret_cast<VT *>(ad) = *reinterpret_cast<const VT *>(static_cast<const W *>(it.addend) + off);
#pragma unroll
                for (int s = 0; s < SV; ++s) {
                    const W t = it.scalar ? mul_mod<W>(ad[s], sv[s], q, lc.mu, lc.kbits) : ad[s];
                    o[s] = add_mod<W>(o[s], t, q);
                }
            }
            *reinterpret_cast<VT *>(static_cast<W *>(it.c) + off) = *reinterpret_cast<const VT *>(o);
        }
    }
}

template <typename W, int TR, int TC, int SV>
static int launch_group_cfg(GpuContext *ctx, const MulGroupArgs &args, uint32_t items, uint32_t total_rows, const void *b,
                            size_t b_bytes, uint32_t inner, uint32_t cw, uint32_t col0, uint32_t out_cols, uint32_t L) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const TileGrid g = tile_grid<TR, TC, SV>(ctx, total_rows, cw, L, b_bytes);  // its y extent: checked before the first launch
    static const std::string name = std::string("matmul_group_kernel<") + (sizeof(W) == 4 ? "u32," : "u64,") + std::to_string(TR) + "," +
                                    std::to_string(TC) + "," + std::to_string(SV) +
                                    "> (stacked rows of up to 64 operands x digit columns x slots per lane, addend o scalar in the epilogue)";
    ctx->last_kernel = name.c_str();
    const W *bw = static_cast<const W *>(b);
    bool streamed = false;  // the 64-bit tiles have no non-temporal instance
    if constexpr (sizeof(W) == 4) {
        if (g.streamed) {
            streamed = true;
            MXX_LAUNCH((matmul_group_kernel<W, TR, TC, SV, true>), g.grid, dim3(g.threads), 0, ctx->stream, args, items, bw, ctx->d_limbs,
                       total_rows, inner, cw, col0, out_cols, L, N, g.row_tiles);
        }
    }
    if (!streamed)
        MXX_LAUNCH((matmul_group_kernel<W, TR, TC, SV, false>), g.grid, dim3(g.threads), 0, ctx->stream, args, items, bw, ctx->d_limbs,
                   total_rows, inner, cw, col0, out_cols, L, N, g.row_tiles);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_group(GpuContext *ctx, const MulGroupArgs &args, uint32_t items, uint32_t total_rows, const void *b, size_t b_bytes,
                        uint32_t inner, uint32_t cw, uint32_t col0, uint32_t out_cols, uint32_t L) {
    return dispatch_stacked_tile(ctx, stacked_tile(ctx, total_rows, cw, L), [&](auto cfg) {
        typedef decltype(cfg) T;
        return launch_group_cfg<typename T::W, T::TR, T::TC, T::SV>(ctx, args, items, total_rows, b, b_bytes, inner, cw, col0, out_cols, L);
    });
}

extern "C" int gpupoly_matrix_mul_decompose_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                                 const GpuMatrix *const *addends, const GpuMatrix *const *scalars, size_t n,
                                                 const GpuMatrix *rhs, uint32_t base_bits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_mul_decompose_many";
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    if (n == 0) return 0;
    if (!outs || !lhss) return refuse("null array");
    if (!rhs) return refuse("null rhs");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    GpuContext *ctx = rhs->ctx;
    const int level = rhs->level;
    const size_t L = matrix_limbs(rhs);
    const size_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t inner = rhs->rows * dpt * L, cols = rhs->cols;
    // ---- every refusal, for every j, before the first launch ----
    uint64_t total_rows = 0;
    for (size_t j = 0; j < n; ++j) {
        GpuMatrix *out = outs[j];
        const GpuMatrix *lhs = lhss[j], *add = addends ? addends[j] : nullptr, *sc = scalars ? scalars[j] : nullptr;
        const std::string at = " (operand " + std::to_string(j) + ")";
        if (!out || !lhs) return refuse("null matrix" + at);
        if (sc && !add) return refuse("a scalar without an addend" + at);
        if (out->ctx != ctx || lhs->ctx != ctx || (add && add->ctx != ctx) || (sc && sc->ctx != ctx)) return refuse("context mismatch" + at);
        if (out->level != level || lhs->level != level || (add && add->level != level) || (sc && sc->level != level))
            return refuse("level mismatch" + at);
        if (lhs->cols != inner || out->rows != lhs->rows || out->cols != cols) return refuse("shape mismatch" + at);
        if (add && (add->rows != lhs->rows || add->cols != cols)) return refuse("addend shape mismatch" + at);
        if (sc && (sc->rows != 1 || sc->cols != 1)) return refuse("scalar must be 1x1" + at);
        if (lhs->format != GPU_POLY_FORMAT_EVAL || (add && add->format != GPU_POLY_FORMAT_EVAL) || (sc && sc->format != GPU_POLY_FORMAT_EVAL))
            return refuse("requires Eval format" + at);
        total_rows += lhs->rows;
    }
    for (size_t j = 0; j < n; ++j) {  // an output is written while every input is still being read
        const GpuMatrix *out = outs[j];
        if (storage_overlaps(out, rhs)) return refuse("an output aliases rhs");
        for (size_t o = 0; o < n; ++o) {
            if (o != j && storage_overlaps(out, outs[o])) return refuse("an output aliases another output");
            if (storage_overlaps(out, lhss[o]) || (addends && addends[o] && storage_overlaps(out, addends[o])) ||
                (scalars && scalars[o] && storage_overlaps(out, scalars[o])))
                return refuse("an output aliases an input");
        }
    }
    if (total_rows > 0xffffffffull || inner > 0xffffffffull || cols > 0xffffffffull) return refuse("matrix too large");
    // groups of up to 64 operands with rows: one descriptor table and one launch each per column chunk
    std::vector<std::vector<size_t>> members;
    std::vector<uint32_t> group_rows;
    for (size_t j = 0; j < n; ++j) {
        if (lhss[j]->rows == 0) continue;
        if (members.empty() || members.back().size() == kMulGroupMax) {
            members.emplace_back();
            group_rows.push_back(0);
        }
        members.back().push_back(j);
        group_rows.back() += static_cast<uint32_t>(lhss[j]->rows);
    }
    const bool work = total_rows > 0 && cols > 0;
    if (work && ctx_activate(ctx)) return 1;
    const size_t poly_bytes = L * static_cast<size_t>(ctx->N) * ctx->word_bytes;
    // column chunks of the digit matrix: mul_tensor_identity_impl's budget rule (a third of what the device could give us
    // now, at least 8 GiB), or MXX_HIP_MUL_DECOMPOSE_MANY_BUDGET
    size_t chunk = cols;
    if (work && inner > 0) {
        size_t budget = ctx->env.mul_decompose_many_budget;
        if (budget == 0) {
            size_t free_b = 0, total_b = 0;
            budget = size_t(8) << 30;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::max(budget, (free_b + ctx->cached_bytes) / 3);
            else (void)hipGetLastError();
        }
        chunk = std::min(cols, std::max<size_t>(1, budget / (inner * poly_bytes)));
    }
    if (work) {  // the grid's y extent holds row tiles x column tiles, for the full chunks and for the last one
        const size_t widths[2] = {chunk, cols % chunk};
        for (size_t cwid : widths)
            for (uint32_t rows_g : group_rows) {
                if (cwid == 0) continue;
                const TileShape t = stacked_tile(ctx, rows_g, cwid, L);
                if (!tile_grid_fits(rows_g, cwid, t.tr, t.tc)) return refuse("matrix too large");
            }
    }
    // ---- accepted ----
    for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    if (!work) return 0;
    // PACKED24 operands are unpacked here, once (words_ptr)
    std::vector<MulGroupArgs> groups(members.size());
    std::vector<double> group_bytes(members.size(), 0.0);  // left operands and scalars, read once per launch
    std::vector<size_t> group_add_rows(members.size(), 0);  // rows with an addend: read once, like the output is written
    for (size_t g = 0; g < members.size(); ++g) {
        uint32_t first = 0;
        for (size_t m = 0; m < members[g].size(); ++m) {
            const size_t j = members[g][m];
            const GpuMatrix *add = addends ? addends[j] : nullptr, *sc = scalars ? scalars[j] : nullptr;
            MulGroupItem &it = groups[g].item[m];
            it.a = words_ptr(lhss[j]);
            it.c = words_ptr(outs[j]);
            it.addend = add ? words_ptr(add) : nullptr;
            it.scalar = sc ? words_ptr(sc) : nullptr;
            it.rows = static_cast<uint32_t>(lhss[j]->rows);
            it.first = first;
            first += it.rows;
            group_bytes[g] += static_cast<double>(lhss[j]->bytes) + (sc ? static_cast<double>(sc->bytes) : 0.0);
            if (add) group_add_rows[g] += add->rows;
        }
    }
    int rc = 0;
    for (size_t c0 = 0; !rc && c0 < cols; c0 += chunk) {
        const size_t cw = std::min(chunk, cols - c0);
        GpuMatrix *slice = nullptr, *dec = nullptr;
        if (inner > 0) {
            if (cw != cols) {
                rc = gpu_matrix_create(ctx, level, rhs->rows, cw, rhs->format, &slice);
                if (!rc) rc = gpu_matrix_copy_block(slice, rhs, 0, 0, 0, c0, rhs->rows, cw);
            }
            if (!rc) rc = gpu_matrix_create(ctx, level, inner, cw, GPU_POLY_FORMAT_EVAL, &dec);
            if (!rc) rc = gpu_matrix_decompose_base(slice ? slice : rhs, base_bits, dec);  // EVAL: the fused digit transform
        }
        for (size_t g = 0; !rc && g < groups.size(); ++g) {
            MXX_TRACE_BYTES(group_bytes[g] + (dec ? static_cast<double>(dec->bytes) : 0.0) +
                            static_cast<double>(group_rows[g] + group_add_rows[g]) * cw * poly_bytes);
            rc = launch_group(ctx, groups[g], static_cast<uint32_t>(members[g].size()), group_rows[g], dec ? words_ptr(dec) : nullptr, dec ? dec->bytes : 0,
                              static_cast<uint32_t>(inner), static_cast<uint32_t>(cw), static_cast<uint32_t>(c0),
                              static_cast<uint32_t>(cols), static_cast<uint32_t>(L));
        }
        gpu_matrix_destroy(slice);  // stream-ordered: behind the launches that read them
        gpu_matrix_destroy(dec);
    }
    return rc;
    ABI_GUARD_END
}
