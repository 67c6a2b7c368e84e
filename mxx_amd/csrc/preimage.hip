// preimage.hip — several preimage requests in one ABI call: against ONE trapdoor (gpupoly_trapdoor_preimage_many) or
// each against one of several (gpupoly_trapdoor_preimage_keyed, at the end of this file).
//
// The body of `preimage` (src/sampler/trapdoor/gpu.rs:228-369, :423-474) over the column-wise concatenation of up to 64
// requests per group, each with its own seed triple (the gpupoly_*_segments samplers key every element by its position
// inside its own request, so a request's output is the matrix it would get alone).  Per group:
//   P = [p1; p2]       one stacked matrix, every request padded to a multiple of d columns; p2 is sampled into P's
//                      bottom rows, p1 (from [R;E] p2) into its top rows - row views, no copies
//   A P                one product: the residues of left p1 + right p2, without slicing A
//   u - A P            gather-subtract: reads every target through a pointer table, skips the padding columns
//   z                  the G-sampler over the perturbed syndromes, [R;E] z one product
//   outs[j]            scatter-assemble: [P_top + [R;E] z ; P_bottom + z], written straight into each caller's output
// The mirror's sequence (mxx_amd/trapdoor.py, `_preimage_segments`) adds a concatenation of the targets, two
// drop-padding passes, two products for the image, a sum, a difference, two row-block sums and a split.
#include "matmul_tile.h"
#include "rng.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace {

constexpr size_t kGroupMax = RNG_MAX_SEGMENTS;  // requests per group: one segment table per sampler launch
constexpr size_t kGroupBytes = size_t(1) << 30;  // cap on a group's p2 block (trapdoor.py: BATCH_BYTES)

// the requests of one group as a kernel argument: request j owns columns [start[j], start[j + 1]) of the group's
// target-shaped matrices and columns [pad_start[j], pad_start[j] + start[j + 1] - start[j]) of the padded ones
struct RequestTable {
    uint32_t count;
    uint32_t start[kGroupMax + 1];
    uint32_t pad_start[kGroupMax];
    void *ptr[kGroupMax];  // request j's target (gather) or output (scatter): rows x (start[j + 1] - start[j])
};

__device__ __forceinline__ uint32_t request_of(const RequestTable &t, uint32_t col) {
    uint32_t lo = 0, hi = t.count;  // start[lo] <= col < start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (col >= t.start[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename W, int VN>
struct Words {
    typedef typename std::conditional<VN == 1, W, typename std::conditional<sizeof(W) == 4, uint4, ulonglong2>::type>::type V;
    static_assert(sizeof(V) == sizeof(W) * VN, "vector width");
};

// out[r, c] = target_j[r, c - start[j]] - ap[r, pad_start[j] + c - start[j]]  (out: rows x start[count], ap: rows x ap_cols).
// blockIdx.y/z = the output polynomial, blockIdx.x strides its words VN per lane (16 bytes when VN > 1).
template <typename W, int VN>
__global__ void preimage_gather_sub_kernel(W *__restrict__ out, const W *__restrict__ ap, RequestTable req,
                                           const LimbConst *__restrict__ limbs, size_t rows, size_t ap_cols, uint32_t logN,
                                           size_t words_per_poly) {
    typedef typename Words<W, VN>::V V;
    const size_t cols = req.start[req.count];
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= rows * cols) return;
    const size_t r = entry / cols;
    const uint32_t c = static_cast<uint32_t>(entry - r * cols);
    const uint32_t j = request_of(req, c);
    const uint32_t lc = c - req.start[j];
    const size_t tcols = req.start[j + 1] - req.start[j];
    const W *t = static_cast<const W *>(req.ptr[j]) + (r * tcols + lc) * words_per_poly;
    const W *a = ap + (r * ap_cols + req.pad_start[j] + lc) * words_per_poly;
    W *o = out + (r * cols + c) * words_per_poly;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < words_per_poly;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const W q = static_cast<W>(limbs[w0 >> logN].q);  // VN divides N: one limb per vector
        W tv[VN], av[VN], ov[VN];
        *reinterpret_cast<V *>(tv) = *reinterpret_cast<const V *>(t + w0);
        *reinterpret_cast<V *>(av) = *reinterpret_cast<const V *>(a + w0);
#pragma unroll
        for (int v = 0; v < VN; ++v) ov[v] = sub_mod<W>(tv[v], av[v], q);
        *reinterpret_cast<V *>(o + w0) = *reinterpret_cast<const V *>(ov);
    }
}

// out_j[r, c - start[j]] = p[r, pad_start[j] + c - start[j]] + (r < top ? rez[r, c] : z[r - top, c])
// (p: rows x p_cols, rez: top x start[count], z: (rows - top) x start[count]); grid as above
template <typename W, int VN>
__global__ void preimage_scatter_kernel(RequestTable req, const W *__restrict__ p, const W *__restrict__ rez,
                                        const W *__restrict__ z, const LimbConst *__restrict__ limbs, size_t top, size_t rows,
                                        size_t p_cols, uint32_t logN, size_t words_per_poly) {
    typedef typename Words<W, VN>::V V;
    const size_t cols = req.start[req.count];
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= rows * cols) return;
    const size_t r = entry / cols;
    const uint32_t c = static_cast<uint32_t>(entry - r * cols);
    const uint32_t j = request_of(req, c);
    const uint32_t lc = c - req.start[j];
    const size_t ocols = req.start[j + 1] - req.start[j];
    const W *pp = p + (r * p_cols + req.pad_start[j] + lc) * words_per_poly;
    const W *s = r < top ? rez + (r * cols + c) * words_per_poly : z + ((r - top) * cols + c) * words_per_poly;
    W *o = static_cast<W *>(req.ptr[j]) + (r * ocols + lc) * words_per_poly;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < words_per_poly;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const W q = static_cast<W>(limbs[w0 >> logN].q);
        W pv[VN], sv[VN], ov[VN];
        *reinterpret_cast<V *>(pv) = *reinterpret_cast<const V *>(pp + w0);
        *reinterpret_cast<V *>(sv) = *reinterpret_cast<const V *>(s + w0);
#pragma unroll
        for (int v = 0; v < VN; ++v) ov[v] = add_mod<W>(pv[v], sv[v], q);
        *reinterpret_cast<V *>(o + w0) = *reinterpret_cast<const V *>(ov);
    }
}

// grid over `entries` polynomials of `words_per_poly` words, VN words per lane (column_blocks' shape, matrix.hip)
static bool poly_grid(size_t entries, size_t words_per_poly, int vn, dim3 &grid) {
    const size_t vecs = words_per_poly / vn;
    size_t gy, gz;
    if (!fold_yz(entries, gy, gz)) return false;
    grid = dim3(static_cast<unsigned>(std::min<size_t>((vecs + 255) / 256, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    return true;
}

template <typename W>
static int launch_gather_sub(GpuContext *ctx, GpuMatrix *out, const GpuMatrix *ap, const RequestTable &req) {
    const size_t wpp = matrix_limbs(out) * static_cast<size_t>(ctx->N), entries = out->rows * out->cols;
    // 16 bytes per lane where a limb vector holds whole 16-byte words (every ring the segmented samplers take);
    // a word per lane below that
    const int vn = (static_cast<size_t>(ctx->N) * sizeof(W)) % 16 == 0 ? static_cast<int>(16 / sizeof(W)) : 1;
    dim3 grid;
    if (!poly_grid(entries, wpp, vn, grid)) return set_error("gpupoly_trapdoor_preimage_many: matrix too large");
    MXX_TRACE_BYTES(3.0 * entries * wpp * sizeof(W));
    if (vn == 1)
        MXX_LAUNCH((preimage_gather_sub_kernel<W, 1>), grid, dim3(256), 0, ctx->stream, static_cast<W *>(words_ptr(out)),
                   static_cast<const W *>(words_ptr(ap)), req, ctx->d_limbs, out->rows, ap->cols, ctx->logN, wpp);
    else
        MXX_LAUNCH((preimage_gather_sub_kernel<W, 16 / sizeof(W)>), grid, dim3(256), 0, ctx->stream, static_cast<W *>(words_ptr(out)),
                   static_cast<const W *>(words_ptr(ap)), req, ctx->d_limbs, out->rows, ap->cols, ctx->logN, wpp);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
static int launch_scatter(GpuContext *ctx, const RequestTable &req, const GpuMatrix *p, const GpuMatrix *rez, const GpuMatrix *z) {
    const size_t wpp = matrix_limbs(p) * static_cast<size_t>(ctx->N), entries = p->rows * req.start[req.count];
    const int vn = (static_cast<size_t>(ctx->N) * sizeof(W)) % 16 == 0 ? static_cast<int>(16 / sizeof(W)) : 1;
    dim3 grid;
    if (!poly_grid(entries, wpp, vn, grid)) return set_error("gpupoly_trapdoor_preimage_many: matrix too large");
    MXX_TRACE_BYTES(3.0 * entries * wpp * sizeof(W));
    if (vn == 1)
        MXX_LAUNCH((preimage_scatter_kernel<W, 1>), grid, dim3(256), 0, ctx->stream, req, static_cast<const W *>(words_ptr(p)),
                   static_cast<const W *>(words_ptr(rez)), static_cast<const W *>(words_ptr(z)), ctx->d_limbs, rez->rows, p->rows,
                   p->cols, ctx->logN, wpp);
    else
        MXX_LAUNCH((preimage_scatter_kernel<W, 16 / sizeof(W)>), grid, dim3(256), 0, ctx->stream, req,
                   static_cast<const W *>(words_ptr(p)), static_cast<const W *>(words_ptr(rez)), static_cast<const W *>(words_ptr(z)),
                   ctx->d_limbs, rez->rows, p->rows, p->cols, ctx->logN, wpp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the keyed few-row product: out[:, c] = lhs_k(c) * rhs[:, c] -------------------------------------------------------
// The columns of rhs (inner x cols) and out (rows x cols, rows <= 8: d or 2d) fall into runs; run k owns columns
// [col_start[k], col_start[k + 1]) and has a left operand of its own (rows x inner): the requests of one trapdoor.  A
// column tile never crosses a run, so a workgroup has ONE left operand and the shared register-tile loop (matmul_tile.h)
// with its lazy-accumulation rule serves as it stands; run k owns the column tiles [tile_start[k], tile_start[k + 1]).
// The residues are canonical, so every run's columns equal gpu_matrix_mul's for that run alone, bit for bit.
struct KeyedLhs {
    uint32_t count;                      // runs with columns
    uint32_t col_start[kGroupMax + 1];   // col_start[count] = cols
    uint32_t tile_start[kGroupMax + 1];  // tile_start[count] = all column tiles
    const void *lhs[kGroupMax];          // words, rows x inner
};
static_assert(sizeof(KeyedLhs) <= 4096 - 128, "the run table must fit the kernel-argument segment");

// blockIdx.y = column tile * row_tiles + row tile, x: slots (SV per lane), z: limbs - matmul_group_kernel's grid
template <typename W, int TR, int TC, int SV>
__global__ void __launch_bounds__(256)
    matmul_keyed_kernel(KeyedLhs keys, W *__restrict__ C, const W *__restrict__ B, const LimbConst *__restrict__ limbs, uint32_t rows,
                        uint32_t inner, uint32_t cols, uint32_t L, uint32_t N, uint32_t row_tiles) {
    constexpr bool NTB = false;  // few columns: B is never beyond the Infinity Cache
    const uint32_t limb = blockIdx.z;
    const uint32_t ct = blockIdx.y / row_tiles, rt = blockIdx.y - ct * row_tiles;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * SV;
    if (i >= N) return;
    uint32_t lo = 0, hi = keys.count;  // tile_start[lo] <= ct < tile_start[hi]: request_of's search, wave-uniform
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ct >= keys.tile_start[mid]) lo = mid;
        else hi = mid;
    }
    const uint32_t r0 = rt * TR, c0 = keys.col_start[lo] + (ct - keys.tile_start[lo]) * TC, cend = keys.col_start[lo + 1];
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    typedef typename TileTypes<W, SV>::VT VT;
    typedef typename TileTypes<W, SV>::wxs wxs;
    typedef typename TileTypes<W, SV>::D D;

    const size_t poly = static_cast<size_t>(L) * N;  // words per polynomial
    const size_t in_poly = static_cast<size_t>(limb) * N + i;
    // rows past the end repeat the last row, columns past the run's end its last column: computed, never stored
    const W *a_ptr[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r)
        a_ptr[r] = static_cast<const W *>(keys.lhs[lo]) + static_cast<size_t>(min(r0 + r, rows - 1)) * inner * poly + in_poly;
    size_t b_off[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) b_off[c] = static_cast<size_t>(min(c0 + c, cend - 1)) * poly + in_poly;
    const size_t strideBk = static_cast<size_t>(cols) * poly;

    D acc[TR][TC][SV];
    MXX_TILE_CLEAR(acc);
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
#define MXX_TILE_A(r, k) (a_ptr[r] + (k) * poly)
#define MXX_TILE_B(c, k) (B + b_off[c] + (k) * strideBk)
#include "matmul_tile_loop.inc"
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (r0 + r >= rows) continue;
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            if (c0 + c >= cend) continue;
            W o[SV];
#pragma unroll
            for (int s = 0; s < SV; ++s) o[s] = tile_reduce<W>(acc[r][c][s], q, lc);
            *reinterpret_cast<VT *>(C + (static_cast<size_t>(r0 + r) * cols + c0 + c) * poly + in_poly) = *reinterpret_cast<const VT *>(o);
        }
    }
}

// the key runs of one group of requests, host side: run k = the group's adjacent requests of one key
struct KeyRuns {
    size_t count = 0;
    uint32_t start[kGroupMax + 1];      // first column of run k in the target-shaped matrices
    uint32_t pad_start[kGroupMax + 1];  // ... in the padded ones
    const GpuMatrix *re[kGroupMax], *a[kGroupMax];
};

static uint64_t keyed_col_tiles(const uint32_t *col_start, size_t runs, uint32_t tc) {
    uint64_t tiles = 0;
    for (size_t k = 0; k < runs; ++k) tiles += (col_start[k + 1] - col_start[k] + tc - 1) / tc;
    return tiles;
}

// whether the grid of the keyed product of `rows` rows over these runs fits (checked before a call's first launch)
static bool keyed_grid_fits(const GpuContext *ctx, size_t rows, const uint32_t *col_start, size_t runs, size_t L) {
    const TileShape t = stacked_tile(ctx, rows, col_start[runs], L);
    return (rows + t.tr - 1) / t.tr * keyed_col_tiles(col_start, runs, t.tc) <= 65535;
}

template <typename W, int TR, int TC, int SV>
static int launch_keyed_cfg(GpuContext *ctx, GpuMatrix *out, const GpuMatrix *const *lhs, const uint32_t *col_start, size_t runs,
                            const GpuMatrix *rhs) {
    const uint32_t rows = static_cast<uint32_t>(out->rows), inner = static_cast<uint32_t>(rhs->rows),
                   cols = static_cast<uint32_t>(rhs->cols), L = static_cast<uint32_t>(matrix_limbs(out));
    KeyedLhs keys{};
    keys.count = static_cast<uint32_t>(runs);
    uint32_t tiles = 0;
    double lhs_bytes = 0.0;
    for (size_t k = 0; k < runs; ++k) {
        keys.col_start[k] = col_start[k];
        keys.tile_start[k] = tiles;
        keys.lhs[k] = words_ptr(lhs[k]);
        tiles += (col_start[k + 1] - col_start[k] + TC - 1) / TC;
        lhs_bytes += static_cast<double>(lhs[k]->bytes);
    }
    for (size_t k = runs; k <= kGroupMax; ++k) {
        keys.col_start[k] = cols;
        keys.tile_start[k] = tiles;
    }
    TileGrid g = tile_grid<TR, TC, SV>(ctx, rows, cols, L, rhs->bytes);
    g.grid.y = g.row_tiles * tiles;
    if (g.grid.y > 65535) return set_error("gpupoly_trapdoor_preimage_keyed: matrix too large");
    static const std::string name = std::string("matmul_keyed_kernel<") + (sizeof(W) == 4 ? "u32," : "u64,") + std::to_string(TR) + "," +
                                    std::to_string(TC) + "," + std::to_string(SV) + "> (a left operand per column run, few rows)";
    ctx->last_kernel = name.c_str();
    MXX_TRACE_BYTES(lhs_bytes + static_cast<double>(rhs->bytes) + static_cast<double>(out->bytes));
    MXX_LAUNCH((matmul_keyed_kernel<W, TR, TC, SV>), g.grid, dim3(g.threads), 0, ctx->stream, keys, static_cast<W *>(words_ptr(out)),
               static_cast<const W *>(words_ptr(rhs)), ctx->d_limbs, rows, inner, cols, L, static_cast<uint32_t>(ctx->N), g.row_tiles);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out (rows x cols) = per run k: lhs[k] (rows x inner) * rhs[:, col_start[k] .. col_start[k + 1]); every run has columns
static int launch_matmul_keyed(GpuContext *ctx, GpuMatrix *out, const GpuMatrix *const *lhs, const uint32_t *col_start, size_t runs,
                               const GpuMatrix *rhs) {
    const int rc = dispatch_stacked_tile(ctx, stacked_tile(ctx, out->rows, rhs->cols, matrix_limbs(out)), [&](auto cfg) {
        typedef decltype(cfg) T;  // u32 words take the 8-row tile from 5 rows on (2d rows at d = 3, 4)
        return launch_keyed_cfg<typename T::W, T::TR, T::TC, T::SV>(ctx, out, lhs, col_start, runs, rhs);
    });
    if (rc == 0) out->format = GPU_POLY_FORMAT_EVAL;
    return rc;
}

// a temporary of the context's allocator, released stream-ordered when the scope ends (error paths included)
struct TempMatrix {
    GpuMatrix *m = nullptr;
    TempMatrix() = default;
    TempMatrix(const TempMatrix &) = delete;
    TempMatrix &operator=(const TempMatrix &) = delete;
    ~TempMatrix() { release(); }
    int make(GpuContext *ctx, int level, size_t rows, size_t cols) {
        return gpu_matrix_create(ctx, level, rows, cols, GPU_POLY_FORMAT_EVAL, &m);
    }
    void release() {
        gpu_matrix_destroy(m);
        m = nullptr;
    }
};

// rows [row, row + rows) of m as a matrix that shares its storage (gpupoly_matrix_row_view without the allocation)
static GpuMatrix row_block(const GpuMatrix *m, size_t row, size_t rows) {
    const size_t poly_bytes = matrix_limbs(m) * static_cast<size_t>(m->ctx->N) * m->ctx->word_bytes;
    char *base = static_cast<char *>(words_ptr(m));
    GpuMatrix v = *m;
    v.rows = rows;
    v.storage = rows && m->cols ? base + row * m->cols * poly_bytes : nullptr;
    v.bytes = rows * m->cols * poly_bytes;
    v.borrowed = true;
    return v;
}

// the shared byte-range test (common.h: nothing is unpacked for it); a matrix without entries overlaps nothing, itself included
static bool words_overlap(const GpuMatrix *a, const GpuMatrix *b) { return a->bytes && b->bytes && storage_overlaps(a, b); }

static int fail(const std::string &msg) { return set_error("gpupoly_trapdoor_preimage_many: " + msg); }

struct PreimageCall {
    GpuContext *ctx;
    const GpuMatrix *re, *a;
    const GpuP1CovarianceCache *cache;
    uint32_t base_bits;
    double sigma_large;
    size_t d, dk;
    const char *entry = "gpupoly_trapdoor_preimage_many";  // named in this call's errors
};

// gpupoly_trapdoor_preimage_keyed: what one group adds - its key runs, and the device table of its segments' caches
struct KeyedGroup {
    KeyRuns runs;
    const P1KeyEntry *d_keys;
};

// one group of requests (all with columns): the sequence of launches described at the top of this file
// `keyed`: the group's requests belong to several trapdoors - the three products take a left operand per key run and the
// p1 sampler a covariance cache per segment; call.re, call.a and call.cache then stand for what all keys share
static int preimage_group(const PreimageCall &call, const GpuMatrix *const *targets, const GpuRngSeed *seeds,
                          GpuMatrix *const *outs, const std::vector<size_t> &group, const KeyedGroup *keyed = nullptr) {
    GpuContext *ctx = call.ctx;
    const int level = call.re->level;
    const size_t top = 2 * call.d, ng = group.size();
    std::vector<size_t> cols(ng), pads(ng);
    std::vector<GpuRngSeed> seed_p2(ng), seed_p1(ng), seed_z(ng);
    RequestTable gather{}, scatter{};
    gather.count = scatter.count = static_cast<uint32_t>(ng);
    size_t at = 0, pad_at = 0;
    for (size_t g = 0; g < ng; ++g) {
        const size_t j = group[g];
        cols[g] = targets[j]->cols;
        pads[g] = (cols[g] + call.d - 1) / call.d * call.d;
        seed_p2[g] = seeds[3 * j];
        seed_p1[g] = seeds[3 * j + 1];
        seed_z[g] = seeds[3 * j + 2];
        gather.start[g] = scatter.start[g] = static_cast<uint32_t>(at);
        gather.pad_start[g] = scatter.pad_start[g] = static_cast<uint32_t>(pad_at);
        gather.ptr[g] = words_ptr(targets[j]);
        scatter.ptr[g] = words_ptr(outs[j]);
        at += cols[g];
        pad_at += pads[g];
    }
    if (pad_at >> 32) return set_error(std::string(call.entry) + ": a group of requests wider than 2^32 columns");
    for (size_t g = ng; g <= kGroupMax; ++g) gather.start[g] = scatter.start[g] = static_cast<uint32_t>(at);
    for (size_t g = ng; g < kGroupMax; ++g) {
        gather.pad_start[g] = scatter.pad_start[g] = static_cast<uint32_t>(pad_at);
        gather.ptr[g] = scatter.ptr[g] = nullptr;
    }
    // P = [p1; p2]: p2 into the bottom rows, [R;E] p2 (to the coefficient domain) feeds p1 into the top rows
    TempMatrix p, tp2, ap, perturbed, z, rez;
    int rc = p.make(ctx, level, top + call.dk, pad_at);
    if (rc) return rc;
    GpuMatrix p1 = row_block(p.m, 0, top), p2 = row_block(p.m, top, call.dk);
    rc = gpupoly_matrix_sample_distribution_segments(&p2, GPU_MATRIX_DIST_GAUSS, call.sigma_large, seed_p2.data(), pads.data(), ng);
    if (rc) return rc;
    if ((rc = tp2.make(ctx, level, top, pad_at))) return rc;
    rc = keyed ? launch_matmul_keyed(ctx, tp2.m, keyed->runs.re, keyed->runs.pad_start, keyed->runs.count, &p2)
               : gpu_matrix_mul(tp2.m, call.re, &p2);
    if (rc || (rc = gpu_matrix_intt_all(tp2.m))) return rc;
    rc = keyed ? sample_p1_keyed_segments(call.cache, keyed->d_keys, tp2.m, seed_p1.data(), pads.data(), ng, &p1)
               : gpupoly_matrix_sample_p1_full_cached_segments(call.cache, tp2.m, seed_p1.data(), pads.data(), ng, &p1);
    if (rc) return rc;
    tp2.release();
    p.m->format = GPU_POLY_FORMAT_EVAL;  // both row blocks were written in EVAL form
    // the image A P in one product, then u - A P over the targets' columns only
    if ((rc = ap.make(ctx, level, call.d, pad_at))) return rc;
    rc = keyed ? launch_matmul_keyed(ctx, ap.m, keyed->runs.a, keyed->runs.pad_start, keyed->runs.count, p.m) : gpu_matrix_mul(ap.m, call.a, p.m);
    if (rc) return rc;
    if ((rc = perturbed.make(ctx, level, call.d, at))) return rc;
    rc = ctx->wide ? launch_gather_sub<uint64_t>(ctx, perturbed.m, ap.m, gather) : launch_gather_sub<uint32_t>(ctx, perturbed.m, ap.m, gather);
    if (rc) return rc;
    ap.release();
    // z = G-sampler over the perturbed syndromes (EVAL), [R;E] z
    if ((rc = z.make(ctx, level, call.dk, at))) return rc;
    rc = gpupoly_matrix_gauss_samp_gq_arb_base_segments(perturbed.m, call.base_bits, call.cache->sigma, call.cache->dgg_stddev,
                                                        seed_z.data(), cols.data(), ng, z.m);
    if (rc) return rc;
    perturbed.release();
    if ((rc = rez.make(ctx, level, top, at))) return rc;
    rc = keyed ? launch_matmul_keyed(ctx, rez.m, keyed->runs.re, keyed->runs.start, keyed->runs.count, z.m) : gpu_matrix_mul(rez.m, call.re, z.m);
    if (rc) return rc;
    // x_j = [p1 + [R;E] z ; p2 + z], straight into the callers' outputs
    return ctx->wide ? launch_scatter<uint64_t>(ctx, scatter, p.m, rez.m, z.m) : launch_scatter<uint32_t>(ctx, scatter, p.m, rez.m, z.m);
}

}  // namespace

extern "C" int gpupoly_trapdoor_preimage_many(const GpuMatrix *re, const GpuP1CovarianceCache *cache,
                                              const GpuMatrix *public_matrix, uint32_t base_bits,
                                              const GpuMatrix *const *targets, size_t n, const GpuRngSeed *seeds,
                                              GpuMatrix *const *outs) {
    ABI_GUARD_BEGIN
    // ---- every check before the first launch: a refused call launches nothing and writes no output, not even a tag
    if (!re || !cache || !public_matrix) return fail("null trapdoor, covariance cache or public matrix");
    if (n == 0) return 0;
    if (!targets || !seeds || !outs) return fail("null targets, seeds or outputs");
    GpuContext *ctx = re->ctx;
    const int level = re->level;
    if (cache->ctx != ctx || public_matrix->ctx != ctx) return fail("context mismatch");
    if (cache->level != level || public_matrix->level != level) return fail("level mismatch");
    if (base_bits == 0 || base_bits >= 63) return fail("invalid base_bits");
    const size_t d = public_matrix->rows, L = matrix_limbs(re);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t top = 2 * d, dk = d * dpt * L;
    if (d == 0 || re->rows != top || re->cols != dk || public_matrix->cols != top + dk || cache->d != d || cache->m != top)
        return fail("shape mismatch: needs [R; E] 2d x dk, A d x (2d + dk) and a covariance cache of dimension d");
    if (re->format != GPU_POLY_FORMAT_EVAL || public_matrix->format != GPU_POLY_FORMAT_EVAL)
        return fail("[R; E] and the public matrix must be in EVAL form");
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *t = targets[j], *o = outs[j];
        if (!t || !o) return fail("null target or output " + std::to_string(j));
        if (t->ctx != ctx || o->ctx != ctx) return fail("context mismatch in request " + std::to_string(j));
        if (t->level != level || o->level != level) return fail("level mismatch in request " + std::to_string(j));
        if (t->rows != d) return fail("target " + std::to_string(j) + " must have d rows");
        if (o->rows != top + dk || o->cols != t->cols)
            return fail("output " + std::to_string(j) + " must be (2d + dk) x its target's columns");
        if (t->format != GPU_POLY_FORMAT_EVAL) return fail("target " + std::to_string(j) + " must be in EVAL form");
        if (t->cols >> 31) return fail("target " + std::to_string(j) + " too wide");
    }
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *o = outs[j];
        bool alias = words_overlap(o, re) || words_overlap(o, public_matrix);
        for (size_t i = 0; i < n && !alias; ++i) alias = words_overlap(o, targets[i]) || (i != j && words_overlap(o, outs[i]));
        if (alias) return fail("output " + std::to_string(j) + " aliases an input or another output");
    }
    // what the segmented samplers cover (include/gpupoly.h); the caller issues such requests one by one
    if ((static_cast<size_t>(ctx->N) >> 1) % SAMPLER_THREADS)
        return fail("unsupported: ring dimension not a multiple of 128 (segmented samplers)");
    if (cache->m > 8) return fail("unsupported: trapdoor dimension above 4 (no p1 lane kernel)");
    if (ctx->env.p1_simple) return fail("unsupported under MXX_HIP_P1=simple (the p1 lane kernel is switched off)");
    if (dpt > 4) return fail("unsupported: more than four digits per tower (G-sampler lane kernel)");
    if (ctx->env.rng_compat) return fail("unsupported under MXX_HIP_RNG_COMPAT=reference");
    // the widths as trapdoor.py evaluates them: c = cache->sigma, s = cache->s, large = sqrt(s^2 - c^2)
    const double sigma_large = std::sqrt(cache->s * cache->s - cache->sigma * cache->sigma);
    if (!(sigma_large > 0.0) || !(cache->sigma > 0.0)) return fail("invalid Gaussian widths in the covariance cache");
    if (ctx_activate(ctx)) return 1;
    // ---- groups of at most 64 requests with columns, p2 capped at 1 GiB (trapdoor.py: preimage_many)
    const PreimageCall call{ctx, re, public_matrix, cache, base_bits, sigma_large, d, dk};
    const size_t poly_bytes = L * static_cast<size_t>(ctx->N) * ctx->word_bytes;
    std::vector<size_t> group;
    size_t group_bytes = 0;
    for (size_t j = 0; j < n; ++j) {
        if (targets[j]->cols == 0) continue;  // a zero-column request: a zero-column output, nothing to launch
        const size_t bytes = dk * ((targets[j]->cols + d - 1) / d * d) * poly_bytes;
        if (!group.empty() && (group.size() == kGroupMax || group_bytes + bytes > kGroupBytes)) {
            const int rc = preimage_group(call, targets, seeds, outs, group);
            if (rc) return rc;
            group.clear();
            group_bytes = 0;
        }
        group.push_back(j);
        group_bytes += bytes;
    }
    if (!group.empty()) {
        const int rc = preimage_group(call, targets, seeds, outs, group);
        if (rc) return rc;
    }
    for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    return 0;
    ABI_GUARD_END
}

// ---- requests of several trapdoors in one call ---------------------------------------------------------------------------
// Only the linear algebra and the perturbation's conditional Gaussians depend on the key: p2 and the G-sampler do not read
// it, the p1 sampler reads it through the three arrays of its covariance cache, the three products through [R;E] and A.
// So the requests are ordered by key (stable) and cut into groups exactly as above - a boundary may fall inside a key's
// run - and a group runs preimage_group's sequence once, whatever the number of keys in it: the products as
// matmul_keyed_kernel over the group's key runs, p1 as the sampler's KEYED form, which finds segment j's cache in a
// device table.  That table (one P1KeyEntry per segment, 64 per group, all groups of the call in one block from the
// context's allocator) is filled by one staged copy before the first group and released stream-ordered.
extern "C" int gpupoly_trapdoor_preimage_keyed(const GpuMatrix *const *res, const GpuP1CovarianceCache *const *caches,
                                               const GpuMatrix *const *public_matrices, size_t nkeys, uint32_t base_bits,
                                               const uint32_t *key_of, const GpuMatrix *const *targets, size_t n,
                                               const GpuRngSeed *seeds, GpuMatrix *const *outs) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_trapdoor_preimage_keyed";
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    // ---- every check, for every key and every request, before the first launch
    if (nkeys > 0 && (!res || !caches || !public_matrices)) return refuse("null array of trapdoors, covariance caches or public matrices");
    if (n > 0 && (!key_of || !targets || !seeds || !outs)) return refuse("null key_of, targets, seeds or outputs");
    if (nkeys == 0 && n > 0) return refuse("requests without keys");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    for (size_t k = 0; k < nkeys; ++k)
        if (!res[k] || !caches[k] || !public_matrices[k])
            return refuse("null trapdoor, covariance cache or public matrix in key " + std::to_string(k));
    if (nkeys == 0) return 0;
    GpuContext *ctx = res[0]->ctx;
    const int level = res[0]->level;
    const size_t d = public_matrices[0]->rows, L = matrix_limbs(res[0]);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t top = 2 * d, dk = d * dpt * L;
    for (size_t k = 0; k < nkeys; ++k) {
        const GpuMatrix *re = res[k], *a = public_matrices[k];
        const GpuP1CovarianceCache *cache = caches[k];
        const std::string at = " in key " + std::to_string(k);
        if (re->ctx != ctx || cache->ctx != ctx || a->ctx != ctx) return refuse("context mismatch" + at);
        if (re->level != level || cache->level != level || a->level != level) return refuse("level mismatch" + at);
        if (a->rows != d) return refuse("keys of different trapdoor dimension d" + at);
        if (d == 0 || re->rows != top || re->cols != dk || a->cols != top + dk || cache->d != d || cache->m != top)
            return refuse("shape mismatch" + at + ": needs [R; E] 2d x dk, A d x (2d + dk) and a covariance cache of dimension d");
        if (re->format != GPU_POLY_FORMAT_EVAL || a->format != GPU_POLY_FORMAT_EVAL)
            return refuse("[R; E] and the public matrix must be in EVAL form" + at);
    }
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *t = targets[j], *o = outs[j];
        const std::string js = std::to_string(j);
        if (key_of[j] >= nkeys) return refuse("key_of[" + js + "] out of range");
        if (!t || !o) return refuse("null target or output " + js);
        if (t->ctx != ctx || o->ctx != ctx) return refuse("context mismatch in request " + js);
        if (t->level != level || o->level != level) return refuse("level mismatch in request " + js);
    }
    // shared storage is named as such, whatever shape the overlapping view has: before the shape checks
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *o = outs[j];
        bool alias = false;
        for (size_t k = 0; k < nkeys && !alias; ++k) alias = words_overlap(o, res[k]) || words_overlap(o, public_matrices[k]);
        for (size_t i = 0; i < n && !alias; ++i) alias = words_overlap(o, targets[i]) || (i != j && words_overlap(o, outs[i]));
        if (alias) return refuse("output " + std::to_string(j) + " aliases a key's [R; E] or A, a target or another output");
    }
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *t = targets[j], *o = outs[j];
        const std::string js = std::to_string(j);
        if (t->rows != d) return refuse("target " + js + " must have d rows");
        if (o->rows != top + dk || o->cols != t->cols) return refuse("output " + js + " must be (2d + dk) x its target's columns");
        if (t->format != GPU_POLY_FORMAT_EVAL) return refuse("target " + js + " must be in EVAL form");
        if (t->cols >> 31) return refuse("target " + js + " too wide");
    }
    // what the segmented samplers cover, as in the one-key entry; the caller then issues one call per key
    if ((static_cast<size_t>(ctx->N) >> 1) % SAMPLER_THREADS)
        return refuse("unsupported: ring dimension not a multiple of 128 (segmented samplers)");
    if (top > 8) return refuse("unsupported: trapdoor dimension above 4 (no p1 lane kernel)");
    if (ctx->env.p1_simple) return refuse("unsupported under MXX_HIP_P1=simple (the p1 lane kernel is switched off)");
    if (dpt > 4) return refuse("unsupported: more than four digits per tower (G-sampler lane kernel)");
    if (ctx->env.rng_compat) return refuse("unsupported under MXX_HIP_RNG_COMPAT=reference");
    for (size_t k = 1; k < nkeys; ++k)  // sigma_large and c_scale are single launch scalars
        if (caches[k]->sigma != caches[0]->sigma || caches[k]->s != caches[0]->s || caches[k]->dgg_stddev != caches[0]->dgg_stddev)
            return refuse("unsupported: the covariance caches of key 0 and key " + std::to_string(k) + " carry different widths");
    const GpuP1CovarianceCache *cache0 = caches[0];
    const double sigma_large = std::sqrt(cache0->s * cache0->s - cache0->sigma * cache0->sigma);
    if (!(sigma_large > 0.0) || !(cache0->sigma > 0.0)) return refuse("invalid Gaussian widths in the covariance caches");
    // ---- by key (stable), then groups as in the one-key entry: at most 64 requests with columns, p2 capped at 1 GiB
    std::vector<size_t> order;
    for (size_t j = 0; j < n; ++j)
        if (targets[j]->cols) order.push_back(j);  // a zero-column request: a zero-column output, nothing to launch
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return key_of[x] < key_of[y]; });
    const size_t poly_bytes = L * static_cast<size_t>(ctx->N) * ctx->word_bytes;
    std::vector<std::vector<size_t>> groups;
    size_t group_bytes = 0;
    for (size_t j : order) {
        const size_t bytes = dk * ((targets[j]->cols + d - 1) / d * d) * poly_bytes;
        if (groups.empty() || groups.back().size() == kGroupMax || group_bytes + bytes > kGroupBytes) {
            groups.emplace_back();
            group_bytes = 0;
        }
        groups.back().push_back(j);
        group_bytes += bytes;
    }
    // a group's key runs and, per segment, its cache; the grids of the three products must fit
    std::vector<KeyedGroup> keyed(groups.size());
    std::vector<P1KeyEntry> table(groups.size() * kGroupMax, P1KeyEntry{nullptr, nullptr, nullptr});
    for (size_t g = 0; g < groups.size(); ++g) {
        KeyRuns &runs = keyed[g].runs;
        uint64_t at = 0, pad_at = 0;
        for (size_t m = 0; m < groups[g].size(); ++m) {
            const size_t j = groups[g][m];
            const uint32_t key = key_of[j];
            if (m == 0 || key != key_of[groups[g][m - 1]]) {
                runs.start[runs.count] = static_cast<uint32_t>(at);
                runs.pad_start[runs.count] = static_cast<uint32_t>(pad_at);
                runs.re[runs.count] = res[key];
                runs.a[runs.count] = public_matrices[key];
                ++runs.count;
            }
            table[g * kGroupMax + m] = P1KeyEntry{caches[key]->sqrt_var, caches[key]->update_coeff, caches[key]->karney_div};
            at += targets[j]->cols;
            pad_at += (targets[j]->cols + d - 1) / d * d;
        }
        if (pad_at >> 32) return refuse("a group of requests wider than 2^32 columns");
        runs.start[runs.count] = static_cast<uint32_t>(at);
        runs.pad_start[runs.count] = static_cast<uint32_t>(pad_at);
        if (!keyed_grid_fits(ctx, top, runs.pad_start, runs.count, L) || !keyed_grid_fits(ctx, d, runs.pad_start, runs.count, L) ||
            !keyed_grid_fits(ctx, top, runs.start, runs.count, L))
            return refuse("matrix too large");
    }
    if (groups.empty()) {
        for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    CtxBlock d_table(ctx);
    if (d_table.alloc(table.size() * sizeof(P1KeyEntry))) return 1;
    MXX_TRACED_COPY("covariance cache table (host to device)", ctx->stream, table.size() * sizeof(P1KeyEntry),
                    HIP_TRY(hipMemcpyAsync(d_table.ptr, table.data(), table.size() * sizeof(P1KeyEntry), hipMemcpyHostToDevice, ctx->stream)));
    PreimageCall call{ctx, res[0], public_matrices[0], cache0, base_bits, sigma_large, d, dk};
    call.entry = who;
    for (size_t g = 0; g < groups.size(); ++g) {
        keyed[g].d_keys = static_cast<const P1KeyEntry *>(d_table.ptr) + g * kGroupMax;
        const int rc = preimage_group(call, targets, seeds, outs, groups[g], &keyed[g]);
        if (rc) return rc;
    }
    for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    return 0;
    ABI_GUARD_END
}
