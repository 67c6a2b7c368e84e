// common.h — private structures of libgpupoly (host side).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <map>
#include <unordered_map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gpupoly.h"
#include "grid_plan.h"

constexpr size_t GPUPOLY_MAX_LIMBS = 64;  // cuda/include/Runtime.cuh:51 of the reference

// Per-limb constants, one array entry per prime, resident in HBM and read
// through the scalar cache (uniform per workgroup).
struct LimbConst {
    uint64_t q;          // modulus
    uint64_t mu;         // Barrett constant: floor(2^(2*kbits)/q)   (kbits = bits(q))
    uint64_t mu64;       // floor(2^64/q) (u32 path: lazy 64-bit sum reduction)
    uint64_t n_inv;      // N^-1 mod q
    uint64_t n_inv_sh;   // Shoup companion of n_inv (2^32 or 2^64 scaled, by word width)
    uint64_t mu32;       // floor(2^32/q) (u32 path: fold lazy NTT values back to [0,2q))
    uint64_t inv_last_w;     // inv[1] * N^-1 mod q : last inverse-NTT stage with N^-1 folded in
    uint64_t inv_last_w_sh;  // its Shoup companion
    uint32_t kbits;      // bits(q)
    uint32_t lazy_terms; // how many q^2-bounded products fit the accumulator
};

// Environment switches, read ONCE per context at gpu_context_create (not per launch: a preimage call
// at n = 256 is ~30 launches and each getenv scans the environment under libc's lock).
// gpupoly_reload_env() re-reads them for every live context (tests flip them between calls).
struct EnvSwitches {
    int ntt_path = 0;             // MXX_HIP_NTT_PATH: 0 auto, 1 lds, 2 generic, 3 global
    int ntt14 = 0;                // MXX_HIP_NTT14: 0 grouped signed, 1 whole-vector kernel, 2 grouped unsigned
    bool decompose_fused = true;  // MXX_HIP_DECOMPOSE_FUSED=0 disables digits-in-the-NTT-load
    char matmul_path = 0;         // MXX_HIP_MATMUL_PATH: 0 auto, 'r' reg, 'l' lds, 'd' dma, 'w' dma32 (wide tile), 'm' mfma
    int matmul_tile = 0;          // MXX_HIP_MATMUL_TILE=RCS[p] (tuning: rows, cols, slots per lane of the register tile, p = loads ahead)
    bool gsamp_simple = false;    // MXX_HIP_GSAMP=simple
    bool gsamp_no_uni = false;    // MXX_HIP_GSAMP=nouni: the lane kernel's per-element tower look-up even when chunks are uniform (A/B, tests)
    bool p1_simple = false;       // MXX_HIP_P1=simple
    int sampler_per_lane = 0;     // MXX_HIP_SAMPLER_PER_LANE (0 = sized for one resident round)
    int sampler_fill_every = 0;   // MXX_HIP_SAMPLER_FILL_EVERY = 1..8: keystream refill cadence of the Gaussian lane kernels in checkpoints (0 = per kernel default)
    bool ntt64_int = false;       // MXX_HIP_NTT64=int: 64-bit words keep the integer butterflies (A/B, tests)
    int ntt_phase = 0;            // MXX_HIP_NTT_PHASE: phase mask of the forward 2^14 transform, GPUPOLY_PHASE_TIMING builds only (ntt14.h)
    bool serde_general = false;   // MXX_HIP_SERDE=general: compact store always through the kernels that carry the general Garner path (tests, A/B)
    bool rng_compat = false;      // MXX_HIP_RNG_COMPAT=reference: sample_distribution* keyed exactly as the reference's device RNG (sampling.hip)
    bool pack24 = true;           // MXX_HIP_PACK24=0|off: uniform samples stay in 4-byte words (layout.hip)
    int skinny24 = 0;             // MXX_HIP_SKINNY24: 0 auto, 1 = "0" never (matmul_kernel reads packed B, the A/B baseline), 2 = force[:TC,G,WPE,MAP]
    int skinny24_shape = 0;       // the shape after "force:" (matmul_skinny24.hip; 0: the default shape)
    size_t mul_decompose_many_budget = 0;  // MXX_HIP_MUL_DECOMPOSE_MANY_BUDGET=<bytes>: digit-matrix budget of gpupoly_matrix_mul_decompose_many
                                           // alone (0 = a third of the free memory, at least 8 GiB; tests reach its column chunks with it)
    size_t mul_decompose_pairs_budget = 0;  // MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET=<bytes>: the same for gpupoly_matrix_mul_decompose_pairs,
                                            // which cuts its call into groups of operands (matmul_pairs.hip)
    size_t gadget_scalar_budget = 0;  // MXX_HIP_GADGET_SCALAR_BUDGET=<bytes>: digit-polynomial table budget of
                                      // gpupoly_matrix_mul_decompose_gadget_scalar_many alone (0 = the same rule; tests reach its tower groups with it)
    size_t ggh15_lookup_budget = 0;  // MXX_HIP_GGH15_LOOKUP_BUDGET=<bytes>: scratch cap of a slot group of gpupoly_matrix_ggh15_lookup
                                     // (0 = the target builders' 1 GiB; tests reach several groups with it)
    size_t lwe_lookup_budget = 0;  // MXX_HIP_LWE_LOOKUP_BUDGET=<bytes>: scratch cap of a slot group of gpupoly_matrix_lwe_lookup (likewise)
    size_t slot_eval_budget = 0;   // MXX_HIP_SLOT_EVAL_BUDGET=<bytes>: scratch cap of an output group of gpupoly_matrix_slot_transfer_eval (likewise)
    size_t bgg_encode_budget = 0;  // MXX_HIP_BGG_ENCODE_BUDGET=<bytes>: scratch cap of a slot group of gpupoly_matrix_bgg_encode_slots (likewise)
    size_t commit_lut_budget = 0;  // MXX_HIP_COMMIT_LUT_BUDGET=<bytes>: digit-scratch cap of a row group of gpupoly_matrix_commit_lut_messages (likewise)
    char mul_sum_path = 0;        // MXX_HIP_MUL_SUM_PATH: 0 auto, 't' the term-table tile kernel at every height, 's' products into
                                  // scratch + one combine pass per term above 8 rows (matmul_sum.hip; A/B, tests)
    size_t crt_recompose_chunk_bytes = size_t(256) << 20;  // MXX_HIP_CRT_RECOMPOSE_CHUNK_BYTES=<bytes>: scratch cap of
                                  // gpupoly_matrix_crt_recompose_rounded, which works through whole slots per chunk (at least one
                                  // slot whatever the cap; tests reach its chunks with it)
    void load();
};

struct GpuContext {
    EnvSwitches env;
    int device = 0;
    std::vector<int> gpu_ids;
    uint32_t logN = 0;
    int N = 0;
    int level = 0;  // top level = limb_count-1
    uint32_t dnum = 0;
    int limb_count = 0;
    bool wide = false;  // true: uint64_t residues
    int word_bytes = 4;
    uint32_t crt_bits = 0;  // max bit width over the moduli
    std::vector<uint64_t> moduli;
    hipStream_t stream = nullptr;
    // device tables
    LimbConst *d_limbs = nullptr;  // [limb_count]
    LimbConst *d_limbs_r = nullptr;  // u32 words: the same with n_inv / inv_last_w (+ companions) multiplied by 2^32 mod q,
                                     // for the inverse transform that multiplies in its load (Montgomery product, ntt14.h)
    void *d_tw_fwd = nullptr;      // [limb][N] words, fwd[bitrev(i)] = psi^i
    void *d_tw_fwd_sh = nullptr;   // Shoup companions
    void *d_tw_inv = nullptr;      // inv[bitrev(i)] = psi^-i
    void *d_tw_inv_sh = nullptr;
    void *d_tw2_fwd = nullptr;     // [limb][N] pairs {-w mod 2^W, Shoup(w)} for the lazy forward kernel
    void *d_tw2_inv = nullptr;     // [limb][N] pairs {w, Shoup(w)} for the lazy inverse kernel
    bool lazy_ok = false;          // every modulus < 2^(W-7): lazy LDS kernels are valid
    bool tight_ok = false;         // 32-bit words, moduli of 26..28 bits: the lazy kernels' TIGHT forms (ntt_lds.h)
    void *d_tw2s_inv = nullptr;    // u32 words, moduli < 2^24: inverse pairs {centred w, floor(w 2^32 / q)} as int32 (ntt14.h)
    bool signed_ok = false;
    // 64-bit words, every modulus below 2^51: the double-precision transforms of ntt_f64.h
    void *d_twf_fwd = nullptr, *d_twf_inv = nullptr;  // [limb][N] {w, w / q} as doubles
    void *d_flimbs = nullptr;                         // [limb] F64Limb
    bool f64_ok = false;
    uint64_t *d_garner = nullptr;  // [limb][limb] : inverse of q_j mod q_i for j<i
    std::vector<uint64_t> garner_inv;  // host copy
    std::vector<LimbConst> limbs;      // host copy
    // bench timer
    hipEvent_t timer_start = nullptr, timer_stop = nullptr;
    std::vector<hipEvent_t> marks;  // lazily created timing marks
    std::mutex mutex;
    bool pool_ok = false;  // cache freed blocks (stream-ordered reuse)
    std::mutex alloc_mutex;
    std::multimap<size_t, void *> free_blocks;      // size -> block
    std::unordered_map<void *, size_t> live_blocks;  // block -> size
    size_t cached_bytes = 0, cache_limit = 0;
    // name of the kernel the product dispatcher launched last on this context (a string literal or a function-local
    // static: bench.py labels its roofline with what actually ran, gpupoly_context_last_kernel)
    std::atomic<const char *> last_kernel{""};
    bool pack24_ok = false;  // 32-bit words, every modulus below 2^24, N % 4 == 0: matrices may hold GPU_MATRIX_LAYOUT_PACKED24
    // guards every matrix's layout tag and storage swap (layout.hip) and the launches that read packed storage, so that
    // no thread frees packed bytes another thread is about to hand to a kernel
    std::mutex layout_mutex;
    // base_bits -> device table [limb_count][dpt] of {(2^base_bits mod q_l)^e, its Shoup companion}: built on the first
    // gadget product for that base (gadget_products.hip), under `mutex`, freed with the context
    std::map<uint32_t, void *> gadget_weights;
    // {base_bits, limbs, C mod q_0, ...} -> device table [l][t][e'][e] of {delta mod q_l, its Shoup companion} for the
    // constant C of gpupoly_matrix_mul_decompose_gadget_const_many (gadget_scalar.hip): built on the first call with that
    // constant, under `mutex`, freed with the context; a bounded number of them is kept
    std::map<std::vector<uint64_t>, void *> gadget_const_tables;
    // {word bytes, limbs, level offset, active levels, scale, p_0, ...} -> the device tables of the nested-RNS gadget
    // (nested_rns.hip): built on the first call with those arguments, under `mutex`, freed with the context; a bounded
    // number of bounded size is kept
    std::map<std::vector<uint64_t>, void *> nested_rns_tables;
};

// the layout tag of a matrix's storage, copyable (local views copy a GpuMatrix) and read without the lock on the fast path
struct LayoutTag {
    std::atomic<int> v{GPU_MATRIX_LAYOUT_WORDS};
    LayoutTag() = default;
    LayoutTag(const LayoutTag &o) : v(o.v.load(std::memory_order_acquire)) {}
    LayoutTag &operator=(const LayoutTag &o) {
        v.store(o.v.load(std::memory_order_acquire), std::memory_order_release);
        return *this;
    }
};

struct GpuMatrix {
    GpuContext *ctx = nullptr;
    int level = 0;
    size_t rows = 0, cols = 0;
    int format = GPU_POLY_FORMAT_EVAL;
    // words [rows*cols][level+1][N], or with layout PACKED24 [rows*cols][level+1][3N] bytes (residue i at bytes
    // [3i, 3i+3), little-endian).  Never touched directly: words_ptr() / packed24_ptr() (layout.hip)
    void *storage = nullptr;
    size_t bytes = 0;  // of the words layout, whatever the storage holds now
    LayoutTag layout;
    bool borrowed = false;  // a row-block view of another matrix (gpupoly_matrix_row_view): data is not freed with it
    GpuMatrix *parent = nullptr;  // row views (gpupoly_matrix_row_view): the matrix whose storage they share
    int views = 0;                // live row views of this matrix (under ctx->layout_mutex): it is then never packed
};

struct GpuEventSet {
    std::vector<hipEvent_t> events;
    int device = 0;
    void *staging = nullptr;  // host-visible staging released after the wait
    GpuContext *ctx = nullptr;
    void *dev_staging = nullptr;
};

struct GpuP1CovarianceCache {
    GpuContext *ctx = nullptr;
    int level = 0;
    size_t d = 0, m = 0, n = 0;
    double sigma = 0, s = 0, dgg_stddev = 0;
    double *sqrt_var = nullptr;      // [coeff][row]
    double *update_coeff = nullptr;  // [coeff][sampled_row][updated_row]
    void *karney_div = nullptr;      // [coeff][row] KarneyDivisor of sqrt_var (rng.h)
};

// one covariance cache's arrays as the keyed p1 sampler reads them from its device table (trapdoor.hip)
struct P1KeyEntry {
    const double *sqrt_var;
    const double *update_coeff;
    const void *karney_div;
};

// ---- one thread per item -----------------------------------------------------------------------
// item_grid() and the other launch-grid rules: grid_plan.h (no HIP dependency, so a host program can check them)
#if defined(__HIPCC__)
__device__ __forceinline__ size_t item_index() {
    return (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
}
#endif

// every kernel launch of the library goes through this (bench.py prints launches per step for the launch-bound
// small-ring chain: gpupoly_launch_count)
extern std::atomic<uint64_t> g_kernel_launches;
// Launch trace (gpupoly_trace_begin / gpupoly_trace_end, runtime.hip): while it is on, every launch is bracketed by two
// hipEvents on the stream it is launched on and recorded with its kernel's name, grid and - where the launcher states
// them with MXX_TRACE_BYTES - the algorithmic bytes of its operands (each read once + written once).  bench.py composes
// the roofline of a multi-kernel call (a preimage, a chain step) from it.  Off: one relaxed load per launch.
extern std::atomic<int> g_trace_on;
void trace_launch_begin(const char *name, hipStream_t stream, dim3 grid, dim3 block);
void trace_launch_end(hipStream_t stream);
void trace_set_bytes(double bytes);
#define MXX_TRACE_BYTES(b)                                                                        \
    do {                                                                                          \
        if (g_trace_on.load(std::memory_order_relaxed)) trace_set_bytes(static_cast<double>(b)); \
    } while (0)
#define MXX_LAUNCH(kern, grid, block, lds, strm, ...)                          \
    do {                                                                       \
        g_kernel_launches.fetch_add(1, std::memory_order_relaxed);             \
        const bool mxx_tr_ = g_trace_on.load(std::memory_order_relaxed) != 0;  \
        if (mxx_tr_) trace_launch_begin(#kern, strm, grid, block);             \
        hipLaunchKernelGGL(kern, grid, block, lds, strm, __VA_ARGS__);         \
        if (mxx_tr_) trace_launch_end(strm);                                   \
    } while (0)
// a runtime copy / memset on the context's stream, traced like a launch (the statement is the HIP_TRY'd call)
#define MXX_TRACED_COPY(name, strm, bytes, stmt)                               \
    do {                                                                       \
        const bool mxx_tr_ = g_trace_on.load(std::memory_order_relaxed) != 0;  \
        if (mxx_tr_) {                                                         \
            trace_set_bytes(static_cast<double>(bytes));                       \
            trace_launch_begin(name, strm, dim3(0), dim3(0));                  \
        }                                                                      \
        stmt;                                                                  \
        if (mxx_tr_) trace_launch_end(strm);                                   \
    } while (0)

// ---- error plumbing ---------------------------------------------------------
int set_error(const char *msg);
int set_error(const std::string &msg);
int set_error(hipError_t err, const char *what);

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t _e = (expr);                                \
        if (_e != hipSuccess) return set_error(_e, #expr);     \
    } while (0)

// Kernels that ask for more than 64 KB of dynamic LDS must opt in, once per (kernel set, device).  `lds` is a property of
// the kernel set: every launch of these kernels asks for the same amount.
template <auto... KERNELS>
static int lds_opt_in(const GpuContext *ctx, size_t lds) {
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (lds <= 64 * 1024 || (configured.load() & bit)) return 0;
    for (const void *f : {reinterpret_cast<const void *>(KERNELS)...})
        HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    configured.fetch_or(bit);
    return 0;
}

// roctx range around an ABI entry (rocprofv3 --marker-trace attributes kernels to the FFI call that launched them).
// Active under rocprofv3 (ROCP_TOOL_LIBRARIES is set by it) or with MXX_HIP_ROCTX=1; one predictable branch otherwise.
extern int (*g_roctx_push)(const char *);
extern int (*g_roctx_pop)();
void roctx_init_once();
struct RoctxScope {
    bool on;
    explicit RoctxScope(const char *name) {
        roctx_init_once();
        on = g_roctx_push != nullptr;
        if (on) g_roctx_push(name);
    }
    ~RoctxScope() {
        if (on) g_roctx_pop();
    }
};

// every extern "C" body is wrapped so no exception crosses the ABI
#define ABI_GUARD_BEGIN try { RoctxScope roctx_scope_(__func__);
#define ABI_GUARD_END                                                         \
    }                                                                         \
    catch (const std::exception &e) { return set_error(e.what()); }           \
    catch (...) { return set_error("unknown exception in libgpupoly"); }

// ---- helpers ------------------------------------------------------------------
inline size_t matrix_polys(const GpuMatrix *m) { return m->rows * m->cols; }
inline size_t matrix_limbs(const GpuMatrix *m) { return static_cast<size_t>(m->level) + 1; }
inline size_t matrix_words(const GpuMatrix *m) { return matrix_polys(m) * matrix_limbs(m) * static_cast<size_t>(m->ctx->N); }

// ---- storage layout (layout.hip) -------------------------------------------------------------------
// the storage as 4-byte / 8-byte words: a PACKED24 matrix is unpacked first, once, on its context's stream (the matrix
// stays in words afterwards).  Throws on failure (ABI_GUARD turns that into the library's error).
void *words_ptr(const GpuMatrix *m);
// m's storage as it is now and (*packed) whether that is PACKED24, for the kernels that read either layout.  The caller
// holds ctx->layout_mutex from this call until its launch is enqueued (words_ptr must not be called meanwhile).
const void *packed24_ptr(const GpuMatrix *m, bool *packed);
inline size_t packed24_bytes(const GpuMatrix *m) { return m->bytes / 4 * 3; }
// [storage, storage + bytes held now) of two matrices overlap (row views share their parent's storage)
inline bool storage_overlaps(const GpuMatrix *x, const GpuMatrix *y) {
    if (x == y) return true;
    if (!x->storage || !y->storage || x->bytes == 0 || y->bytes == 0) return false;
    const size_t xb = x->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24 ? packed24_bytes(x) : x->bytes;
    const size_t yb = y->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24 ? packed24_bytes(y) : y->bytes;
    const char *xs = static_cast<const char *>(x->storage), *ys = static_cast<const char *>(y->storage);
    return xs < ys + yb && ys < xs + xb;
}
// ---- the operand overlap rule (include/gpupoly.h, conventions) -------------------------------------------------------
// x and y are the very same block: the same object, or a view with the same start and byte length
inline bool same_block(const GpuMatrix *x, const GpuMatrix *y) {
    return x == y || (x->storage == y->storage && x->bytes == y->bytes);
}
// the point-wise entries: an operand may be out's very block (every word is read and written by the same thread); any
// other overlap would be read after it is written
inline bool partial_overlap(const GpuMatrix *out, const GpuMatrix *operand) {
    return storage_overlaps(out, operand) && !same_block(out, operand);
}
// rows [row, row + rows) of m - the block a row-block writer fills - overlap y.  Nothing is unpacked: a PACKED24 matrix
// has no views (gpupoly_matrix_row_view unpacks its parent, and a viewed matrix is never packed), so only m itself
// shares its storage and the whole of it stands for the block
inline bool row_block_overlaps(const GpuMatrix *m, size_t row, size_t rows, const GpuMatrix *y) {
    if (m->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24) return rows && m->cols && storage_overlaps(m, y);
    if (!m->storage) return false;
    const size_t poly_bytes = matrix_limbs(m) * static_cast<size_t>(m->ctx->N) * m->ctx->word_bytes;
    GpuMatrix block;
    block.storage = static_cast<char *>(m->storage) + row * m->cols * poly_bytes;
    block.bytes = rows * m->cols * poly_bytes;
    return storage_overlaps(&block, y);
}
// whether a fresh uniform sample into m may be stored PACKED24
bool pack24_eligible(const GpuMatrix *m);
// m's words (EVAL after the caller's transform) -> PACKED24 storage in a new block; the words block is freed on the stream.
// `ntt`: run the forward transform on the way (fused into the 2^14 transform's store where it exists)
int pack24_store(GpuMatrix *m, bool ntt);

// sampling.hip: fills `out` with samples; keep_coeff leaves them in the coefficient domain
// row_offset: `out` holds rows [row_offset, row_offset + out->rows) of the conceptual matrix; tower_count > 0 (uniform
// only, whose limbs are keyed separately): only limbs [tower_first, tower_first + tower_count) are written
int sample_impl(GpuMatrix *out, int dist, double sigma, GpuRngSeed seed, size_t full_ncol, size_t col_offset, bool keep_coeff,
                size_t row_offset = 0, uint32_t tower_first = 0, uint32_t tower_count = 0);

// sampling.hip: the seeded-blocks sampler behind gpupoly_matrix_sample_distribution_blocks / _hash_blocks (seeds or tags,
// the other null).  With `win` it fills a caller's coefficient scratch for the decomposed blocks (decompose.hip): `out` is
// rows x (nblk * cols), block j columns [j cols, (j + 1) cols) = the window [col_offset, col_offset + cols) of a rows x
// full_ncol matrix under block j's seed; left in the coefficient domain, in words
struct RngBlockWindow {
    size_t cols, full_ncol, col_offset;
};
int sample_blocks_impl(const char *entry, bool hashed, GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, const GpuHashTags *tags,
                       size_t nblk, int layout, const size_t *seg_cols, const RngBlockWindow *win, const double *sigma = nullptr);
// decompose.hip: both decomposed-blocks entries in `entry`'s name (seeds or tags, the other null)
int sample_decomposed_blocks_impl(const char *entry, bool hashed, GpuMatrix *out, int dist_type, const GpuRngSeed *seeds,
                                  const GpuHashTags *tags, size_t nblk, uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                  size_t col_offset);

// hash_seed.hip: tags to seeds on the device.  hash_tags_check refuses a malformed GpuHashTags in `entry`'s name and tells
// the TABLE form's byte count; the TABLE form's offsets and bytes are staged as hash_tags_staged_words 8-byte words (none in
// the indexed forms) which the caller copies to `d_staged` on the stream before launch_hash_seeds writes d_seeds[0 .. ntags)
int hash_tags_check(const char *entry, const GpuHashTags *tags, size_t ntags, size_t *table_bytes);
size_t hash_tags_staged_words(const GpuHashTags *tags, size_t ntags, size_t table_bytes);
void hash_tags_stage(const GpuHashTags *tags, size_t ntags, size_t table_bytes, uint64_t *staging);
int launch_hash_seeds(GpuContext *ctx, GpuRngSeed *d_seeds, const GpuHashTags *tags, size_t ntags, const uint64_t *d_staged);

int ctx_activate(const GpuContext *ctx);                   // hipSetDevice
bool ctx_is_registered(const GpuContext *ctx);             // still a live context of this process (runtime.hip's registry)
int ctx_alloc(GpuContext *ctx, size_t bytes, void **out);  // stream-ordered
void ctx_free(GpuContext *ctx, void *ptr);                 // stream-ordered
// a stream-ordered block that goes back to the context's cache when the scope ends (error paths
// included) unless ownership is handed on with release()
struct CtxBlock {
    GpuContext *ctx;
    void *ptr = nullptr;
    explicit CtxBlock(GpuContext *c) : ctx(c) {}
    CtxBlock(const CtxBlock &) = delete;
    CtxBlock &operator=(const CtxBlock &) = delete;
    ~CtxBlock() {
        if (ptr) ctx_free(ctx, ptr);
    }
    int alloc(size_t bytes) { return ctx_alloc(ctx, bytes, &ptr); }
    void *release() {
        void *p = ptr;
        ptr = nullptr;
        return p;
    }
};
int matrix_check_same_shape(const GpuMatrix *a, const GpuMatrix *b, const char *who);
// *src <- the words of `mat` in the coefficient domain, `mat` (residues and tag) left as it is: its own words for a COEFF
// matrix; for an EVAL matrix a copy in `scratch`, inverse-transformed on the context's stream (matrix.hip).  The read-out
// entries use it (readout.hip); scale_round.hip and norm.hip still carry the same block inline
int coeff_domain_source(const GpuMatrix *mat, CtxBlock &scratch, const void **src);

// internal launchers shared across translation units
int launch_ntt(GpuContext *ctx, void *data, size_t vectors, int limbs_per_poly, bool inverse);
// tuned LDS kernels (ntt_lds_u32.hip / ntt_lds_u64.hip over the ring table of ntt_rings.h); return -1 when no tuned kernel covers logN
int launch_ntt_lds_u32(GpuContext *ctx, uint32_t *data, size_t vectors, uint32_t L, bool inverse);
int launch_ntt_digits_u32(GpuContext *ctx, uint32_t *out, const uint32_t *coeff, size_t out_vectors, uint32_t L,
                          uint32_t src_cols, uint32_t towers, uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0 = 0);
int launch_ntt_lds_u64(GpuContext *ctx, uint64_t *data, size_t vectors, uint32_t L, bool inverse);
int launch_ntt_digits_u64(GpuContext *ctx, uint64_t *out, const uint64_t *coeff, size_t out_vectors, uint32_t L,
                          uint32_t src_cols, uint32_t towers, uint32_t dpt, uint32_t base_bits, size_t k, uint32_t td0 = 0);
// out <- INTT(in o w), w one resident EVAL-form ring element [L][N]; -1: no fused kernel for this context
int launch_intt_oop_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, size_t vectors, uint32_t L);
int launch_ntt_add_u32(GpuContext *ctx, uint32_t *out, const uint32_t *src, const uint32_t *add, size_t vectors, uint32_t L);
int launch_mul_intt_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, const uint32_t *w, size_t vectors, uint32_t L);
int launch_matmul(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);
// forward 2^14 transform of `in` (words) into PACKED24 rows at `out` (3N bytes per vector); -1: no fused kernel here
int launch_ntt_fwd_pack24_u32(GpuContext *ctx, uint32_t *out, const uint32_t *in, size_t vectors, uint32_t L);
int launch_matmul_skinny24(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, bool small_grid);  // -1: not a one-row product against packed B
int skinny24_parse_shape(const char *s);  // "TC,G,WPE,MAP" -> EnvSwitches::skinny24_shape, 0: not a shape
int launch_matmul_dma_u32(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);  // -1: shape not supported
int launch_matmul_dma32_u32(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);  // 32 slots x 32x32 tile, 16 waves
int launch_matmul_mfma_u32(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);  // -1: shape / moduli not supported
int launch_copy_block(GpuMatrix *out, const GpuMatrix *src, size_t dst_row, size_t dst_col, size_t src_row,
                      size_t src_col, size_t rows, size_t cols, bool add);
// trapdoor.hip: gpupoly_matrix_sample_p1_full_cached_segments with segment j's cache arrays in d_keys[j] (device memory)
int sample_p1_keyed_segments(const GpuP1CovarianceCache *cache, const P1KeyEntry *d_keys, const GpuMatrix *tp2,
                             const GpuRngSeed *seeds, const size_t *seg_cols, size_t nseg, GpuMatrix *out);
int launch_scatter_i64(GpuMatrix *out, const int64_t *vals);  // int64 [poly][N] -> residues in every limb
// The staged finish of the Gaussian lane samplers: `stage` holds the int64 samples [poly][N] of `out`, `launch_err` is
// hipGetLastError() after the lane kernel.  Scatters, frees the stage, transforms and tags EVAL; a launch error is
// reported under `what` after the stage is freed (the Gaussian matrix sites pass "err", the text their HIP_TRY(err) has
// always put in front of the HIP error; p1 names its kernel).  transform = false: the samples stay coefficients, the tag
// is the caller's.
int finish_staged_i64(GpuMatrix *out, CtxBlock &stage, hipError_t launch_err, const char *what, bool transform = true);
