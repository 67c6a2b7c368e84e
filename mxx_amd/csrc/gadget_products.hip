// gadget_products.hip — products with the gadget matrix G_d = I_d (x) g that never build it:
// gpupoly_matrix_mul_gadget, gpupoly_matrix_gadget_mul.
//
//   mul_gadget:  out[:, dst_col .. dst_col + cols) = addend block +/- (lhs * G_d[:, gadget_col .. gadget_col + cols)) o scalar
//   gadget_mul:  out = addend +/- G_d * rhs
//
// Every BGG+ relation of the reference's callers holds such a product: A - G x and its column chunks
// (src/lookup/lwe/pubkey_gpu.rs:205-210, src/lookup/ggh15/pubkey_gpu.rs:393-395,474, src/io/diamond_io/utils.rs:612-616,
// src/we/diamond_we.rs:223-227, src/sampler/trapdoor/gpu.rs:212), s G (src/bgg/sampler_gpu.rs:149, src/bgg/sampler.rs:165)
// and the recomposition G D (src/lookup/ggh15/pubkey_gpu.rs:505, src/commit/wee25.rs:718).  Through gpu_matrix_fill_gadget
// that is d x dk polynomials of L N words of which d k limb VECTORS of N words are non-zero - entry (j, j k + t dpt + e) is
// the constant (2^base_bits)^e in limb t and 0 in every other limb - followed by a generic mul_scalar / mul and an add, sub
// or neg over all of it.
//
// Both kernels work on limb vectors (the N contiguous words of one (entry, limb)): hit or miss, the block row, tower, digit
// and weight are uniform per workgroup and live on the scalar side; lanes move 16 bytes each.  The weights
// (2^base_bits mod q_l)^e with their Shoup companions come from a per-context table built on the first call for a base.
#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <string>
#include <vector>

struct GadgetWeight {
    uint64_t w, wsh;  // (2^base_bits mod q_l)^e mod q_l and floor(w 2^W / q_l), W the word width
};

// what a launch of mul_gadget_kernel covers
struct GadgetBlock {
    uint32_t rows, cols, out_cols, dst_col;  // the block: rows x cols at column dst_col of an out that is out_cols wide
    uint32_t d, gadget_col;                  // G_d and the first of its columns
    uint32_t L, N, dpt, k;
    int small, negate;
    int hits_only;  // addend is out's very block: only the vectors G makes non-zero are visited
};

template <typename W, int VN>
struct VecOf {
    typedef typename std::conditional<sizeof(W) * VN == 16, uint4, W>::type type;
};

// the limb vector of this workgroup (grid y, z; grid x runs along the vector)
__device__ __forceinline__ uint32_t limb_vector_index() { return blockIdx.z * gridDim.y + blockIdx.y; }

// One workgroup = one chunk of one limb vector of out's block.  `addend` may be `out` (no __restrict__): a word is then read
// and written by the same thread.  lhs null: the identity.
template <typename W, int VN>
__global__ void __launch_bounds__(256)
    mul_gadget_kernel(W *out, const W *addend, const W *__restrict__ lhs, const W *__restrict__ scalar, const GadgetWeight *__restrict__ table,
                      const LimbConst *__restrict__ limbs, GadgetBlock b, uint32_t vectors) {
    const uint32_t v = limb_vector_index();
    if (v >= vectors) return;
    // ---- uniform: which (row, column, limb), hit or miss, the weight ----
    uint32_t i, c, l;
    if (b.hits_only && !lhs) {  // one hit row per column
        c = b.small ? v / b.L : v;
        l = b.small ? v - c * b.L : 0;
        i = (b.gadget_col + c) / b.k;
    } else if (b.hits_only && !b.small) {  // one hit limb per entry
        i = v / b.cols;
        c = v - i * b.cols;
        l = 0;
    } else {
        const uint32_t p = v / b.L;
        l = v - p * b.L;
        i = p / b.cols;
        c = p - i * b.cols;
    }
    const uint32_t gc = b.gadget_col + c;
    const uint32_t j = gc / b.k, loc = gc - j * b.k;
    const uint32_t t = b.small ? 0 : loc / b.dpt, e = loc - t * b.dpt;
    if (b.hits_only && !b.small) l = t;
    const bool hit = (b.small || t == l) && (lhs || i == j);
    const size_t o_off = ((static_cast<size_t>(i) * b.out_cols + b.dst_col + c) * b.L + l) * b.N;
    const W q = static_cast<W>(limbs[l].q);
    const uint64_t mu = limbs[l].mu;
    const uint32_t kbits = limbs[l].kbits;
    const GadgetWeight gw = table[l * b.dpt + e];
    const W w = static_cast<W>(gw.w), wsh = static_cast<W>(gw.wsh);
    const W *a = lhs ? lhs + ((static_cast<size_t>(i) * b.d + j) * b.L + l) * b.N : nullptr;
    const W *sc = scalar ? scalar + static_cast<size_t>(l) * b.N : nullptr;
    typedef typename VecOf<W, VN>::type VT;

    for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) * VN; s < b.N; s += gridDim.x * blockDim.x * VN) {
        W o[VN];
        if (hit) {
            W x[VN], y[VN];
            if (a) *reinterpret_cast<VT *>(x) = *reinterpret_cast<const VT *>(a + s);
            if (sc) *reinterpret_cast<VT *>(y) = *reinterpret_cast<const VT *>(sc + s);
            if (addend) *reinterpret_cast<VT *>(o) = *reinterpret_cast<const VT *>(addend + o_off + s);
#pragma unroll
            for (int u = 0; u < VN; ++u) {
                W val = a ? mul_shoup<W>(x[u], w, wsh, q) : w;
                if (sc) val = mul_mod<W>(val, y[u], q, mu, kbits);
                if (b.negate) val = val ? static_cast<W>(q - val) : static_cast<W>(0);
                o[u] = addend ? add_mod<W>(o[u], val, q) : val;
            }
        } else {
            if (addend) *reinterpret_cast<VT *>(o) = *reinterpret_cast<const VT *>(addend + o_off + s);
            else {
#pragma unroll
                for (int u = 0; u < VN; ++u) o[u] = 0;
            }
        }
        *reinterpret_cast<VT *>(out + o_off + s) = *reinterpret_cast<const VT *>(o);
    }
}

// One workgroup = one chunk of one limb vector of out (d x c): limb l of entry (j, col) is the base-2^base_bits recomposition
// of limb l of the dpt rows j k + l dpt + e of rhs (small: rows j dpt + e), by Horner with B = 2^base_bits mod q_l.
template <typename W, int VN>
__global__ void __launch_bounds__(256)
    gadget_mul_kernel(W *out, const W *addend, const W *__restrict__ rhs, const GadgetWeight *__restrict__ table,
                      const LimbConst *__restrict__ limbs, uint32_t c, uint32_t L, uint32_t N, uint32_t dpt, uint32_t k, int small, int negate,
                      uint32_t vectors) {
    const uint32_t v = limb_vector_index();
    if (v >= vectors) return;
    const uint32_t p = v / L, l = v - p * L;
    const uint32_t j = p / c, col = p - j * c;
    const W q = static_cast<W>(limbs[l].q);
    W B = 0, Bsh = 0;
    if (dpt > 1) {
        const GadgetWeight gw = table[l * dpt + 1];
        B = static_cast<W>(gw.w);
        Bsh = static_cast<W>(gw.wsh);
    }
    const size_t row0 = static_cast<size_t>(j) * k + (small ? 0 : static_cast<size_t>(l) * dpt);
    const size_t row_stride = static_cast<size_t>(c) * L * N;  // words between the same (column, limb) of consecutive rows
    const W *r0 = rhs + ((row0 * c + col) * L + l) * N;
    const size_t o_off = static_cast<size_t>(v) * N;
    typedef typename VecOf<W, VN>::type VT;

    for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) * VN; s < N; s += gridDim.x * blockDim.x * VN) {
        W acc[VN], o[VN];
        *reinterpret_cast<VT *>(acc) = *reinterpret_cast<const VT *>(r0 + (dpt - 1) * row_stride + s);
        if (addend) *reinterpret_cast<VT *>(o) = *reinterpret_cast<const VT *>(addend + o_off + s);
        for (uint32_t e = dpt - 1; e-- > 0;) {
            W x[VN];
            *reinterpret_cast<VT *>(x) = *reinterpret_cast<const VT *>(r0 + e * row_stride + s);
#pragma unroll
            for (int u = 0; u < VN; ++u) acc[u] = add_mod<W>(mul_shoup<W>(acc[u], B, Bsh, q), x[u], q);
        }
#pragma unroll
        for (int u = 0; u < VN; ++u) {
            W val = acc[u];
            if (negate) val = val ? static_cast<W>(q - val) : static_cast<W>(0);
            o[u] = addend ? add_mod<W>(o[u], val, q) : val;
        }
        *reinterpret_cast<VT *>(out + o_off + s) = *reinterpret_cast<const VT *>(o);
    }
}

namespace {

// the context's weight table for `base_bits`, [limb_count][dpt]: built and uploaded on the first call (synchronous, once),
// kept until the context goes.  dpt follows the context's crt_bits, so one table serves every level.
int gadget_table(GpuContext *ctx, uint32_t base_bits, const GadgetWeight **out) {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    auto it = ctx->gadget_weights.find(base_bits);
    if (it != ctx->gadget_weights.end()) {
        *out = static_cast<const GadgetWeight *>(it->second);
        return 0;
    }
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const int shift = ctx->wide ? 64 : 32;
    std::vector<GadgetWeight> host(static_cast<size_t>(ctx->limb_count) * dpt);
    std::vector<uint64_t> w(dpt);
    for (int l = 0; l < ctx->limb_count; ++l) {
        const uint64_t q = ctx->moduli[l];
        base_powers(q, base_bits, dpt, w.data());
        for (uint32_t e = 0; e < dpt; ++e)
            host[static_cast<size_t>(l) * dpt + e] = {w[e], static_cast<uint64_t>((static_cast<u128_t>(w[e]) << shift) / q)};
    }
    void *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, host.size() * sizeof(GadgetWeight)));
    const hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(GadgetWeight), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return set_error(e, "gadget weight table upload");
    }
    ctx->gadget_weights.emplace(base_bits, dev);
    *out = static_cast<const GadgetWeight *>(dev);
    return 0;
}

// the grid, x = chunks of a limb vector and (y, z) = limb vectors: vector_grid and kMaxVectors (grid_plan.h)

template <typename W>
int launch_mul_gadget(GpuContext *ctx, void *out, const void *addend, const void *lhs, const void *scalar, const GadgetWeight *table,
                      const GadgetBlock &b, uint32_t vectors) {
    constexpr uint32_t VN = 16 / sizeof(W);
    W *o = static_cast<W *>(out);
    const W *ad = static_cast<const W *>(addend), *a = static_cast<const W *>(lhs), *sc = static_cast<const W *>(scalar);
    if (b.N % VN == 0) {
        const VectorGrid g = vector_grid(vectors, b.N, VN);
        MXX_LAUNCH((mul_gadget_kernel<W, VN>), g.grid, g.block, 0, ctx->stream, o, ad, a, sc, table, ctx->d_limbs, b, vectors);
    } else {
        const VectorGrid g = vector_grid(vectors, b.N, 1);
        MXX_LAUNCH((mul_gadget_kernel<W, 1>), g.grid, g.block, 0, ctx->stream, o, ad, a, sc, table, ctx->d_limbs, b, vectors);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int launch_gadget_mul(GpuContext *ctx, void *out, const void *addend, const void *rhs, const GadgetWeight *table, uint32_t c, uint32_t L,
                      uint32_t dpt, uint32_t k, int small, int negate, uint32_t vectors) {
    constexpr uint32_t VN = 16 / sizeof(W);
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    W *o = static_cast<W *>(out);
    const W *ad = static_cast<const W *>(addend), *r = static_cast<const W *>(rhs);
    if (N % VN == 0) {
        const VectorGrid g = vector_grid(vectors, N, VN);
        MXX_LAUNCH((gadget_mul_kernel<W, VN>), g.grid, g.block, 0, ctx->stream, o, ad, r, table, ctx->d_limbs, c, L, N, dpt, k, small, negate,
                   vectors);
    } else {
        const VectorGrid g = vector_grid(vectors, N, 1);
        MXX_LAUNCH((gadget_mul_kernel<W, 1>), g.grid, g.block, 0, ctx->stream, o, ad, r, table, ctx->d_limbs, c, L, N, dpt, k, small, negate,
                   vectors);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int mul_gadget_impl(GpuMatrix *out, size_t dst_col, const GpuMatrix *lhs, const GpuMatrix *scalar, size_t gadget_col, size_t cols,
                    const GpuMatrix *addend, int negate, uint32_t base_bits, int small) {
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_mul_gadget: " + what); };
    // ---- every refusal before the launch ----
    if (!out) return refuse("null output");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    GpuContext *ctx = out->ctx;
    const struct {
        const GpuMatrix *m;
        const char *name;
    } operands[] = {{lhs, "lhs"}, {scalar, "scalar"}, {addend, "addend"}};
    for (const auto &op : operands) {
        if (!op.m) continue;
        if (op.m->ctx != ctx) return refuse(std::string("context mismatch (") + op.name + ")");
        if (op.m->level != out->level) return refuse(std::string("level mismatch (") + op.name + ")");
    }
    const size_t L = matrix_limbs(out);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (lhs && lhs->rows != out->rows) return refuse("shape mismatch: lhs->rows != out->rows");
    const size_t d = lhs ? lhs->cols : out->rows;
    if (dst_col > out->cols || cols > out->cols - dst_col) return refuse("column block out of range: dst_col + cols > out->cols");
    if (d > 0xffffffffull / k) return refuse("matrix too large");
    if (gadget_col > d * k || cols > d * k - gadget_col) return refuse("gadget window out of range: gadget_col + cols > d*k");
    if (scalar && (scalar->rows != 1 || scalar->cols != 1)) return refuse("the scalar must be 1x1");
    if (addend && (addend->rows != out->rows || addend->cols != out->cols)) return refuse("addend shape mismatch");
    for (const auto &op : operands)
        if (op.m && op.m->format != GPU_POLY_FORMAT_EVAL) return refuse(std::string("requires Eval format (") + op.name + ")");
    const bool whole = dst_col == 0 && cols == out->cols;
    if (!whole && out->format != GPU_POLY_FORMAT_EVAL) return refuse("a partial column block needs an output already in Eval format");
    if (addend && partial_overlap(out, addend)) return refuse("the addend overlaps the output without being the same block");
    if (lhs && storage_overlaps(out, lhs)) return refuse("the output overlaps lhs");
    if (scalar && storage_overlaps(out, scalar)) return refuse("the output overlaps the scalar");
    if (out->rows > 0xffffffffull || out->cols > 0xffffffffull) return refuse("matrix too large");
    if (static_cast<u128_t>(out->rows) * cols * L > kMaxVectors) return refuse("matrix too large");
    // ---- accepted ----
    out->format = GPU_POLY_FORMAT_EVAL;
    if (out->rows == 0 || cols == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const GadgetWeight *table = nullptr;
    if (gadget_table(ctx, base_bits, &table)) return 1;
    // PACKED24 operands are unpacked here (words_ptr)
    void *const o = words_ptr(out);
    const void *ad = addend ? words_ptr(addend) : nullptr;
    const void *a = lhs ? words_ptr(lhs) : nullptr;
    const void *sc = scalar ? words_ptr(scalar) : nullptr;
    GadgetBlock b;
    b.rows = static_cast<uint32_t>(out->rows);
    b.cols = static_cast<uint32_t>(cols);
    b.out_cols = static_cast<uint32_t>(out->cols);
    b.dst_col = static_cast<uint32_t>(dst_col);
    b.d = static_cast<uint32_t>(d);
    b.gadget_col = static_cast<uint32_t>(gadget_col);
    b.L = static_cast<uint32_t>(L);
    b.N = static_cast<uint32_t>(ctx->N);
    b.dpt = dpt;
    b.k = static_cast<uint32_t>(k);
    b.small = small ? 1 : 0;
    b.negate = negate ? 1 : 0;
    b.hits_only = ad == o ? 1 : 0;
    // limb vectors the launch visits, and those of them G makes non-zero
    const uint64_t per_entry = small ? L : 1;  // hit limbs of a hit entry
    const uint64_t hits = (lhs ? static_cast<uint64_t>(out->rows) : 1) * cols * per_entry;
    const uint64_t vectors = b.hits_only ? hits : static_cast<uint64_t>(out->rows) * cols * L;
    // algorithmic bytes: a hit reads its lhs and addend vectors and is written; in one pass over the block a miss is written
    // and reads the addend's vector; the scalar's L vectors are read once
    const double vec_bytes = static_cast<double>(ctx->N) * ctx->word_bytes;
    MXX_TRACE_BYTES(vec_bytes * (static_cast<double>(hits) * ((lhs ? 1 : 0) + (ad ? 1 : 0)) + static_cast<double>(vectors) +
                                 static_cast<double>(vectors - hits) * (ad ? 1 : 0) + (sc ? static_cast<double>(L) : 0)));
    return ctx->wide ? launch_mul_gadget<uint64_t>(ctx, o, ad, a, sc, table, b, static_cast<uint32_t>(vectors))
                     : launch_mul_gadget<uint32_t>(ctx, o, ad, a, sc, table, b, static_cast<uint32_t>(vectors));
}

int gadget_mul_impl(GpuMatrix *out, const GpuMatrix *rhs, const GpuMatrix *addend, int negate, uint32_t base_bits, int small) {
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_gadget_mul: " + what); };
    if (!out || !rhs) return refuse("null matrix");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    GpuContext *ctx = out->ctx;
    if (rhs->ctx != ctx) return refuse("context mismatch (rhs)");
    if (rhs->level != out->level) return refuse("level mismatch (rhs)");
    if (addend && addend->ctx != ctx) return refuse("context mismatch (addend)");
    if (addend && addend->level != out->level) return refuse("level mismatch (addend)");
    const size_t L = matrix_limbs(out);
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = small ? dpt : static_cast<size_t>(dpt) * L;
    if (out->rows > 0xffffffffull / k || out->cols > 0xffffffffull) return refuse("matrix too large");
    if (rhs->rows != out->rows * k || rhs->cols != out->cols) return refuse("shape mismatch: rhs must be (out->rows * k) x out->cols");
    if (addend && (addend->rows != out->rows || addend->cols != out->cols)) return refuse("addend shape mismatch");
    if (addend && addend->format != rhs->format) return refuse("rhs and addend differ in format");
    if (addend && partial_overlap(out, addend)) return refuse("the addend overlaps the output without being the same block");
    if (storage_overlaps(out, rhs)) return refuse("the output overlaps rhs");
    if (static_cast<u128_t>(out->rows) * out->cols * L > kMaxVectors) return refuse("matrix too large");
    // ---- accepted ----
    out->format = rhs->format;
    if (out->rows == 0 || out->cols == 0) return 0;
    if (ctx_activate(ctx)) return 1;
    const GadgetWeight *table = nullptr;
    if (gadget_table(ctx, base_bits, &table)) return 1;
    void *const o = words_ptr(out);
    const void *ad = addend ? words_ptr(addend) : nullptr;
    const void *r = words_ptr(rhs);
    const uint64_t vectors = static_cast<uint64_t>(out->rows) * out->cols * L;
    // each output limb vector reads dpt vectors of rhs and the addend's, and is written once
    MXX_TRACE_BYTES(static_cast<double>(vectors) * ctx->N * ctx->word_bytes * (dpt + 1 + (ad ? 1 : 0)));
    return ctx->wide ? launch_gadget_mul<uint64_t>(ctx, o, ad, r, table, static_cast<uint32_t>(out->cols), static_cast<uint32_t>(L), dpt,
                                                   static_cast<uint32_t>(k), small ? 1 : 0, negate ? 1 : 0, static_cast<uint32_t>(vectors))
                     : launch_gadget_mul<uint32_t>(ctx, o, ad, r, table, static_cast<uint32_t>(out->cols), static_cast<uint32_t>(L), dpt,
                                                   static_cast<uint32_t>(k), small ? 1 : 0, negate ? 1 : 0, static_cast<uint32_t>(vectors));
}

}  // namespace

extern "C" int gpupoly_matrix_mul_gadget(GpuMatrix *out, size_t dst_col, const GpuMatrix *lhs, const GpuMatrix *scalar_1x1, size_t gadget_col,
                                         size_t cols, const GpuMatrix *addend, int negate, uint32_t base_bits, int small) {
    ABI_GUARD_BEGIN
    return mul_gadget_impl(out, dst_col, lhs, scalar_1x1, gadget_col, cols, addend, negate, base_bits, small);
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_gadget_mul(GpuMatrix *out, const GpuMatrix *rhs, const GpuMatrix *addend, int negate, uint32_t base_bits,
                                         int small) {
    ABI_GUARD_BEGIN
    return gadget_mul_impl(out, rhs, addend, negate, base_bits, small);
    ABI_GUARD_END
}
