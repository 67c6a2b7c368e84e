// gadget_scalar.hip — the LargeScalarMul gate without G or its digit matrix:
// gpupoly_matrix_mul_decompose_gadget_scalar_many, gpupoly_matrix_mul_decompose_gadget_const_many.
//
//   outs[j] = addends[j] +/- lhss[j] * G^-1(G_dj o c)
//
// Every Evaluable of the reference writes the gate as `lhs.mul_decompose(&(gadget_matrix(d) * scalar))`
// (src/bgg/public_key.rs:134-140, src/bgg/encoding.rs:191-200, src/bgg/poly_encoding.rs:431-461, src/bgg/naive_vec.rs:441,607).
// Entry (j, (j, t, e)) of G o c is c B^e in limb t and 0 in every other limb, and digits are taken per tower, so
//
//   G^-1(G_d o c) = I_d (x) blockdiag_{t<L}(D_t),   D_t[e'][e] = digit e' of (c_t[i] B^e mod q_t), coefficient by coefficient,
//
// written into every limb and transformed: L dpt^2 digit polynomials instead of (d L dpt)^2, and
//
//   out[i, (j, t, e)] = sum_{e' < dpt} lhs[i, (j, t, e')] * D_t[e'][e]          (every limb, every slot).
//
// For a constant c every D_t[e'][e] is a constant below 2^base_bits, its own transform: the constant entry builds the
// L^2 dpt^2 weights (delta mod q_l, with Shoup companions) on the host and one launch streams lhs once and out once.  For a
// ring element a table kernel writes the L dpt^2 digit polynomials, the existing forward transform runs over them, and a
// product kernel holds its dpt^2 table words per lane in registers while it walks the rows of every operand.
//
// A "block row" below is one (operand row i, block column j): the k = dpt L consecutive polynomials (i, (j, ., .)) of an
// operand, which start at polynomial (i d + j) k - so neither kernel needs d.
#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr uint32_t kScalarOpsMax = 64;  // operands per launch

struct ScalarWeight {
    uint64_t w, wsh;  // delta mod q_l and floor(w 2^W / q_l), W the word width
};

// the operands of one launch, by value in the kernel-argument segment
struct ScalarOps {
    const void *lhs[kScalarOpsMax];
    void *out[kScalarOpsMax];
    const void *addend[kScalarOpsMax];   // null: none; may be out's very block
    uint32_t first[kScalarOpsMax + 1];  // prefix sum of block rows
};
static_assert(sizeof(ScalarOps) <= 4096 - 128, "operand table must fit the kernel-argument segment");

template <typename W, int VN>
struct ScalarVec {
    typedef typename std::conditional<sizeof(W) * VN == 16, uint4, W>::type type;
};

template <typename W>
__device__ __forceinline__ W epilogue(W val, int negate, bool has_addend, W a, W q) {
    if (negate) val = val ? static_cast<W>(q - val) : static_cast<W>(0);
    return has_addend ? add_mod<W>(a, val, q) : val;
}

}  // namespace

// ---- constant scalar -------------------------------------------------------------------------------------------------
// One workgroup = one chunk of the dpt limb vectors (block row, (t, .), l): dpt vectors in, dpt vectors out.  The operand,
// the offsets and the dpt^2 weights are uniform per workgroup.  DPT 0: any dpt, the inputs are read again per output.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256)
    gadget_const_kernel(ScalarOps ops, uint32_t count, const ScalarWeight *__restrict__ table, const LimbConst *__restrict__ limbs, uint32_t L,
                        uint32_t N, uint32_t dpt_rt, int negate, uint32_t units) {
    const uint32_t unit = blockIdx.z * gridDim.y + blockIdx.y;
    if (unit >= units) return;
    const uint32_t R = unit / (L * L), rem = unit - R * L * L;
    const uint32_t t = rem / L, l = rem - t * L;
    uint32_t o = 0;
    while (o + 1 < count && ops.first[o + 1] <= R) ++o;
    const uint32_t r = R - ops.first[o];
    const uint32_t dpt = DPT ? DPT : dpt_rt;
    const size_t stride = static_cast<size_t>(L) * N;  // words between the same limb of consecutive polynomials
    const size_t base = ((static_cast<size_t>(r) * dpt * L + static_cast<size_t>(t) * dpt) * L + l) * N;
    const W *a = static_cast<const W *>(ops.lhs[o]) + base;
    const W *ad = ops.addend[o] ? static_cast<const W *>(ops.addend[o]) + base : nullptr;  // may be `out` (no __restrict__)
    W *out = static_cast<W *>(ops.out[o]) + base;
    const ScalarWeight *tw = table + (static_cast<size_t>(l) * L + t) * dpt * dpt;  // [e'][e]
    const W q = static_cast<W>(limbs[l].q);
    typedef typename ScalarVec<W, VN>::type VT;

    if constexpr (DPT > 0) {
        W w[DPT][DPT], wsh[DPT][DPT];
#pragma unroll
        for (int ep = 0; ep < DPT; ++ep)
#pragma unroll
            for (int e = 0; e < DPT; ++e) {
                const ScalarWeight sw = tw[ep * DPT + e];
                w[ep][e] = static_cast<W>(sw.w);
                wsh[ep][e] = static_cast<W>(sw.wsh);
            }
        for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) * VN; s < N; s += gridDim.x * blockDim.x * VN) {
            W x[DPT][VN];
#pragma unroll
            for (int ep = 0; ep < DPT; ++ep) *reinterpret_cast<VT *>(x[ep]) = *reinterpret_cast<const VT *>(a + ep * stride + s);
#pragma unroll
            for (int e = 0; e < DPT; ++e) {
                W y[VN];
                if (ad) *reinterpret_cast<VT *>(y) = *reinterpret_cast<const VT *>(ad + e * stride + s);
#pragma unroll
                for (int u = 0; u < VN; ++u) {
                    W acc = mul_shoup<W>(x[0][u], w[0][e], wsh[0][e], q);
#pragma unroll
                    for (int ep = 1; ep < DPT; ++ep) acc = add_mod<W>(acc, mul_shoup<W>(x[ep][u], w[ep][e], wsh[ep][e], q), q);
                    y[u] = epilogue<W>(acc, negate, ad != nullptr, ad ? y[u] : static_cast<W>(0), q);
                }
                *reinterpret_cast<VT *>(out + e * stride + s) = *reinterpret_cast<const VT *>(y);
            }
        }
    } else {
        for (uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) * VN; s < N; s += gridDim.x * blockDim.x * VN) {
            for (uint32_t e = 0; e < dpt; ++e) {
                W acc[VN], y[VN];
#pragma unroll
                for (int u = 0; u < VN; ++u) acc[u] = 0;
                for (uint32_t ep = 0; ep < dpt; ++ep) {
                    const ScalarWeight sw = tw[ep * dpt + e];
                    W x[VN];
                    *reinterpret_cast<VT *>(x) = *reinterpret_cast<const VT *>(a + ep * stride + s);
#pragma unroll
                    for (int u = 0; u < VN; ++u) acc[u] = add_mod<W>(acc[u], mul_shoup<W>(x[u], static_cast<W>(sw.w), static_cast<W>(sw.wsh), q), q);
                }
                if (ad) *reinterpret_cast<VT *>(y) = *reinterpret_cast<const VT *>(ad + e * stride + s);
#pragma unroll
                for (int u = 0; u < VN; ++u) y[u] = epilogue<W>(acc[u], negate, ad != nullptr, ad ? y[u] : static_cast<W>(0), q);
                *reinterpret_cast<VT *>(out + e * stride + s) = *reinterpret_cast<const VT *>(y);
            }
        }
    }
}

// ---- ring-element scalar ---------------------------------------------------------------------------------------------
// The digit polynomials of towers [t0, t0 + towers) in COEFF form, every limb: table[((tl dpt + e') dpt + e) L + l][i] =
// digit e' of (c_t[i] B^e mod q_t), t = t0 + tl, with decompose_kernel's masks and its rule for a digit above a narrow modulus.
// item = (tower, coefficient): c_t[i] is read once and multiplied by B from one e to the next.
template <typename W>
__global__ void gadget_scalar_table_kernel(W *__restrict__ table, const W *__restrict__ coeff, const LimbConst *__restrict__ limbs, uint32_t L,
                                           uint32_t N, uint32_t dpt, uint32_t base_bits, uint32_t t0, uint32_t towers) {
    const size_t idx = item_index();
    if (idx >= static_cast<size_t>(towers) * N) return;
    const uint32_t i = static_cast<uint32_t>(idx % N);
    const uint32_t tl = static_cast<uint32_t>(idx / N), t = t0 + tl;
    const LimbConst lc = limbs[t];
    const W q = static_cast<W>(lc.q);
    const W B = static_cast<W>((1ull << base_bits) % lc.q);  // base_bits < 63
    const uint32_t src_bits = lc.kbits;
    W v = coeff[static_cast<size_t>(t) * N + i];
    for (uint32_t e = 0; e < dpt; ++e) {
        const uint64_t residue = static_cast<uint64_t>(v);
        for (uint32_t ep = 0; ep < dpt; ++ep) {
            const uint32_t shift = ep * base_bits;
            uint64_t mask = 0;
            if (shift < src_bits) {
                const uint32_t rem = src_bits - shift;
                const uint32_t db = base_bits < rem ? base_bits : rem;
                mask = db >= 64 ? ~0ull : ((1ull << db) - 1);
            }
            const uint64_t digit = shift >= 64 ? 0 : ((residue >> shift) & mask);
            const size_t poly = (static_cast<size_t>(tl) * dpt + ep) * dpt + e;
            for (uint32_t l = 0; l < L; ++l) {
                const uint64_t ql = limbs[l].q;
                table[(poly * L + l) * N + i] = static_cast<W>(digit >= ql ? digit % ql : digit);
            }
        }
        v = mul_mod<W>(v, B, q, lc.mu, lc.kbits);
    }
}

// grid (slot chunk, (tower of the group, limb), row group).  A lane keeps the dpt^2 table words of its VN slots in registers
// (DPT 1..4) and walks the block rows of its group through the operand table: dpt words in, dpt words out per row.  The sum
// of the dpt <= 4 products is reduced once.  DPT 0: any dpt; table and inputs are read again per output and the sum is
// reduced every 4 terms.
template <typename W, int VN, int DPT>
__global__ void __launch_bounds__(256)
    gadget_scalar_kernel(ScalarOps ops, uint32_t count, const W *__restrict__ table, const LimbConst *__restrict__ limbs, uint32_t L, uint32_t N,
                         uint32_t dpt_rt, uint32_t t0, int negate, uint32_t block_rows, uint32_t rows_per_group) {
    typedef typename Wide<W>::type D;
    typedef typename ScalarVec<W, VN>::type VT;
    const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) * VN;
    if (s >= N) return;
    const uint32_t tl = blockIdx.y / L, l = blockIdx.y - tl * L, t = t0 + tl;
    const uint32_t dpt = DPT ? DPT : dpt_rt;
    const LimbConst lc = limbs[l];
    const W q = static_cast<W>(lc.q);
    const size_t stride = static_cast<size_t>(L) * N;
    const W *tb = table + (static_cast<size_t>(tl) * dpt * dpt * L + l) * N + s;  // word (e', e) at tb + (e' dpt + e) stride
    const uint32_t R0 = blockIdx.z * rows_per_group;
    const uint32_t R1 = min(block_rows, R0 + rows_per_group);
    uint32_t o = 0;

    W T[DPT ? DPT : 1][DPT ? DPT : 1][VN];
    if constexpr (DPT > 0) {
#pragma unroll
        for (int ep = 0; ep < DPT; ++ep)
#pragma unroll
            for (int e = 0; e < DPT; ++e) *reinterpret_cast<VT *>(T[ep][e]) = *reinterpret_cast<const VT *>(tb + (ep * DPT + e) * stride);
    }
    for (uint32_t R = R0; R < R1; ++R) {
        while (o + 1 < count && ops.first[o + 1] <= R) ++o;
        const uint32_t r = R - ops.first[o];
        const size_t base = ((static_cast<size_t>(r) * dpt * L + static_cast<size_t>(t) * dpt) * L + l) * N + s;
        const W *a = static_cast<const W *>(ops.lhs[o]) + base;
        const W *ad = ops.addend[o] ? static_cast<const W *>(ops.addend[o]) + base : nullptr;  // may be `out`
        W *out = static_cast<W *>(ops.out[o]) + base;
        if constexpr (DPT > 0) {
            W x[DPT][VN];
#pragma unroll
            for (int ep = 0; ep < DPT; ++ep) *reinterpret_cast<VT *>(x[ep]) = *reinterpret_cast<const VT *>(a + ep * stride);
#pragma unroll
            for (int e = 0; e < DPT; ++e) {
                W y[VN];
                if (ad) *reinterpret_cast<VT *>(y) = *reinterpret_cast<const VT *>(ad + e * stride);
#pragma unroll
                for (int u = 0; u < VN; ++u) {
                    D acc = static_cast<D>(x[0][u]) * T[0][e][u];
#pragma unroll
                    for (int ep = 1; ep < DPT; ++ep) acc += static_cast<D>(x[ep][u]) * T[ep][e][u];
                    y[u] = epilogue<W>(lazy_reduce<W>(acc, lc), negate, ad != nullptr, ad ? y[u] : static_cast<W>(0), q);
                }
                *reinterpret_cast<VT *>(out + e * stride) = *reinterpret_cast<const VT *>(y);
            }
        } else {
            for (uint32_t e = 0; e < dpt; ++e) {
                W res[VN], y[VN];
#pragma unroll
                for (int u = 0; u < VN; ++u) res[u] = 0;
                for (uint32_t ep0 = 0; ep0 < dpt; ep0 += 4) {
                    D acc[VN];
#pragma unroll
                    for (int u = 0; u < VN; ++u) acc[u] = 0;
                    const uint32_t ep1 = min(dpt, ep0 + 4);
                    for (uint32_t ep = ep0; ep < ep1; ++ep) {  // at most 4 terms between reductions
                        W x[VN], w[VN];
                        *reinterpret_cast<VT *>(x) = *reinterpret_cast<const VT *>(a + ep * stride);
                        *reinterpret_cast<VT *>(w) = *reinterpret_cast<const VT *>(tb + (static_cast<size_t>(ep) * dpt + e) * stride);
#pragma unroll
                        for (int u = 0; u < VN; ++u) acc[u] += static_cast<D>(x[u]) * w[u];
                    }
#pragma unroll
                    for (int u = 0; u < VN; ++u) res[u] = add_mod<W>(res[u], lazy_reduce<W>(acc[u], lc), q);
                }
                if (ad) *reinterpret_cast<VT *>(y) = *reinterpret_cast<const VT *>(ad + e * stride);
#pragma unroll
                for (int u = 0; u < VN; ++u) y[u] = epilogue<W>(res[u], negate, ad != nullptr, ad ? y[u] : static_cast<W>(0), q);
                *reinterpret_cast<VT *>(out + e * stride) = *reinterpret_cast<const VT *>(y);
            }
        }
    }
}

namespace {

constexpr uint64_t kMaxUnits = 65535ull * 65535ull;

// the operands of an accepted call that have block rows, in launches of up to kScalarOpsMax
struct ScalarLaunch {
    ScalarOps ops = {};
    uint32_t count = 0, block_rows = 0;
    double bytes = 0;  // lhs read once, out written once, the addend read once
};

template <typename W, int VN>
int launch_const_vn(GpuContext *ctx, const ScalarLaunch &g, const ScalarWeight *table, uint32_t L, uint32_t dpt, int negate) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const uint32_t units = g.block_rows * L * L;
    // grid: x = chunks of a limb vector (each lane one access per pass, up to four passes), (y, z) = units
    const uint32_t lanes = (N + VN - 1) / VN;
    const uint32_t threads = std::min<uint32_t>(256, (lanes + 63) / 64 * 64);
    const uint32_t gx = (lanes + threads * 4 - 1) / (threads * 4);
    size_t gy, gz;
    (void)fold_yz(units, gy, gz);  // grid_plan.h; units <= kMaxUnits: checked with the refusals
    const dim3 grid(gx, static_cast<unsigned>(gy), static_cast<unsigned>(gz)), block(threads);
    MXX_TRACE_BYTES(g.bytes);
#define MXX_CONST(D)                                                                                                                     \
    MXX_LAUNCH((gadget_const_kernel<W, VN, D>), grid, block, 0, ctx->stream, g.ops, g.count, table, ctx->d_limbs, L, N, dpt, negate, units)
    switch (dpt) {
        case 1: MXX_CONST(1); break;
        case 2: MXX_CONST(2); break;
        case 3: MXX_CONST(3); break;
        case 4: MXX_CONST(4); break;
        default: MXX_CONST(0); break;
    }
#undef MXX_CONST
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int launch_const(GpuContext *ctx, const ScalarLaunch &g, const ScalarWeight *table, uint32_t L, uint32_t dpt, int negate) {
    constexpr int VN = 16 / sizeof(W);
    if (ctx->N % VN == 0) return launch_const_vn<W, VN>(ctx, g, table, L, dpt, negate);
    return launch_const_vn<W, 1>(ctx, g, table, L, dpt, negate);  // a limb vector narrower than 16 bytes
}

template <typename W, int VN>
int launch_product_vn(GpuContext *ctx, const ScalarLaunch &g, const void *table, uint32_t L, uint32_t dpt, uint32_t t0, uint32_t towers,
                      int negate) {
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const uint32_t lanes = (N + VN - 1) / VN;
    const uint32_t threads = std::min<uint32_t>(256, (lanes + 63) / 64 * 64);
    const uint32_t gx = (lanes + threads - 1) / threads, gy = towers * L;
    // row groups: enough workgroups to cover the chip several times, each keeping its table words for as many rows as that allows
    const uint64_t want = 4096;
    uint32_t groups = static_cast<uint32_t>(std::min<uint64_t>(g.block_rows, std::max<uint64_t>(1, want / (static_cast<uint64_t>(gx) * gy))));
    groups = std::min<uint32_t>(groups, 65535);
    const uint32_t rpg = (g.block_rows + groups - 1) / groups;
    groups = (g.block_rows + rpg - 1) / rpg;
    const dim3 grid(gx, gy, groups), block(threads);
    MXX_TRACE_BYTES(g.bytes * towers / L + static_cast<double>(towers) * dpt * dpt * L * N * sizeof(W));
#define MXX_PRODUCT(D)                                                                                                                       \
    MXX_LAUNCH((gadget_scalar_kernel<W, VN, D>), grid, block, 0, ctx->stream, g.ops, g.count, static_cast<const W *>(table), ctx->d_limbs, L, N, \
               dpt, t0, negate, g.block_rows, rpg)
    switch (dpt) {
        case 1: MXX_PRODUCT(1); break;
        case 2: MXX_PRODUCT(2); break;
        case 3: MXX_PRODUCT(3); break;
        case 4: MXX_PRODUCT(4); break;
        default: MXX_PRODUCT(0); break;
    }
#undef MXX_PRODUCT
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int launch_product(GpuContext *ctx, const ScalarLaunch &g, const void *table, uint32_t L, uint32_t dpt, uint32_t t0, uint32_t towers, int negate) {
    constexpr int VN = 16 / sizeof(W);
    if (ctx->N % VN == 0) return launch_product_vn<W, VN>(ctx, g, table, L, dpt, t0, towers, negate);
    return launch_product_vn<W, 1>(ctx, g, table, L, dpt, t0, towers, negate);
}

// Everything both entries refuse, for every j, before anything is launched.  `scalar` null: the constant entry, whose
// context and level are lhss[0]'s.
int check_call(const char *who, GpuMatrix *const *outs, const GpuMatrix *const *lhss, const GpuMatrix *const *addends, size_t n,
               const GpuMatrix *scalar, uint32_t base_bits, GpuContext **ctx_out, uint64_t *block_rows_out) {
    auto refuse = [&](const std::string &what) { return set_error(std::string(who) + ": " + what); };
    if (!outs || !lhss) return refuse("null array");
    if (base_bits == 0 || base_bits >= 63) return refuse("invalid base_bits");
    for (size_t j = 0; j < n; ++j)
        if (!outs[j] || !lhss[j]) return refuse("null matrix (operand " + std::to_string(j) + ")");
    GpuContext *ctx = scalar ? scalar->ctx : lhss[0]->ctx;
    const int level = scalar ? scalar->level : lhss[0]->level;
    if (level < 0 || level >= ctx->limb_count) return refuse("level out of range");
    const size_t L = static_cast<size_t>(level) + 1;
    const size_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const size_t k = dpt * L;
    if (scalar && (scalar->rows != 1 || scalar->cols != 1)) return refuse("the scalar must be 1x1");
    if (scalar && scalar->format != GPU_POLY_FORMAT_EVAL && scalar->format != GPU_POLY_FORMAT_COEFF) return refuse("the scalar's format is unknown");
    uint64_t block_rows = 0;
    for (size_t j = 0; j < n; ++j) {
        const GpuMatrix *out = outs[j], *lhs = lhss[j], *add = addends ? addends[j] : nullptr;
        const std::string at = " (operand " + std::to_string(j) + ")";
        if (out->ctx != ctx || lhs->ctx != ctx || (add && add->ctx != ctx)) return refuse("context mismatch" + at);
        if (out->level != level || lhs->level != level || (add && add->level != level)) return refuse("level mismatch" + at);
        if (lhs->cols % k) return refuse("lhs->cols is not a multiple of the digit count k" + at);
        if (out->rows != lhs->rows || out->cols != lhs->cols) return refuse("shape mismatch: the output has lhs's shape" + at);
        if (add && (add->rows != lhs->rows || add->cols != lhs->cols)) return refuse("addend shape mismatch" + at);
        if (lhs->format != GPU_POLY_FORMAT_EVAL || (add && add->format != GPU_POLY_FORMAT_EVAL)) return refuse("requires Eval format" + at);
        if (lhs->rows > 0xffffffffull || lhs->cols > 0xffffffffull) return refuse("matrix too large" + at);
        block_rows += static_cast<uint64_t>(lhs->rows) * (lhs->cols / k);
        if (block_rows * L * L > kMaxUnits || block_rows > 0xffffffffull) return refuse("matrix too large" + at);
    }
    for (size_t j = 0; j < n; ++j) {  // an output is written while every input is still being read
        const GpuMatrix *out = outs[j];
        const std::string at = " (operand " + std::to_string(j) + ")";
        if (scalar && storage_overlaps(out, scalar)) return refuse("an output overlaps the scalar" + at);
        for (size_t o = 0; o < n; ++o) {
            if (storage_overlaps(out, lhss[o])) return refuse("an output overlaps an lhs" + at);
            if (o != j && storage_overlaps(out, outs[o])) return refuse("an output overlaps another output" + at);
            const GpuMatrix *add = addends ? addends[o] : nullptr;
            if (!add) continue;
            if (o == j ? partial_overlap(out, add) : storage_overlaps(out, add))
                return refuse("an addend overlaps an output without being that output's own block" + at);
        }
    }
    *ctx_out = ctx;
    *block_rows_out = block_rows;
    return 0;
}

// tags the outputs, unpacks PACKED24 operands (words_ptr) and fills the launches
void accept_call(GpuMatrix *const *outs, const GpuMatrix *const *lhss, const GpuMatrix *const *addends, size_t n, size_t k, bool work,
                 std::vector<ScalarLaunch> *launches) {
    for (size_t j = 0; j < n; ++j) outs[j]->format = GPU_POLY_FORMAT_EVAL;
    if (!work) return;
    for (size_t j = 0; j < n; ++j) {
        const uint32_t rows = static_cast<uint32_t>(lhss[j]->rows * (lhss[j]->cols / k));
        if (rows == 0) continue;
        if (launches->empty() || launches->back().count == kScalarOpsMax) launches->emplace_back();
        ScalarLaunch &g = launches->back();
        const GpuMatrix *add = addends ? addends[j] : nullptr;
        g.ops.lhs[g.count] = words_ptr(lhss[j]);
        g.ops.out[g.count] = words_ptr(outs[j]);
        g.ops.addend[g.count] = add ? words_ptr(add) : nullptr;
        g.ops.first[g.count] = g.block_rows;
        g.block_rows += rows;
        g.ops.first[++g.count] = g.block_rows;
        g.bytes += static_cast<double>(lhss[j]->bytes) * (add ? 3 : 2);
    }
}

uint64_t digit_of(uint64_t residue, uint32_t ep, uint32_t base_bits, uint32_t src_bits) {  // decompose_kernel's masks
    const uint32_t shift = ep * base_bits;
    if (shift >= src_bits || shift >= 64) return 0;
    const uint32_t db = std::min(base_bits, src_bits - shift);
    return (residue >> shift) & (db >= 64 ? ~0ull : ((1ull << db) - 1));
}

constexpr size_t kConstTablesMax = 256;  // constants a context keeps tables for

// The weights of the constant C at L limbs: delta(t, e', e) = digit e' of (C B^e mod q_t), stored mod every q_l with its Shoup
// companion, [l][t][e'][e].  Like the gadget weight table they are built and uploaded on the first call for that constant
// (synchronous, once) and kept by the context - a circuit multiplies by the same few constants gate after gate - so later
// calls only launch.  Past kConstTablesMax constants the table goes through `scratch`, stream-ordered, for this call alone.
int const_table(GpuContext *ctx, uint32_t L, uint32_t dpt, uint32_t base_bits, const uint64_t *words, size_t count, CtxBlock *scratch,
                const ScalarWeight **out) {
    std::vector<uint64_t> key(2 + L);
    key[0] = base_bits;
    key[1] = L;
    for (uint32_t t = 0; t < L; ++t) key[2 + t] = words_mod(words, count, ctx->moduli[t]);
    std::lock_guard<std::mutex> lock(ctx->mutex);
    auto it = ctx->gadget_const_tables.find(key);
    if (it != ctx->gadget_const_tables.end()) {
        *out = static_cast<const ScalarWeight *>(it->second);
        return 0;
    }
    const int shift = ctx->wide ? 64 : 32;
    std::vector<ScalarWeight> host(static_cast<size_t>(L) * L * dpt * dpt);
    std::vector<uint64_t> cb(dpt);  // C B^e mod q_t
    for (uint32_t t = 0; t < L; ++t) {
        base_powers(ctx->moduli[t], base_bits, dpt, cb.data(), key[2 + t]);
        for (uint32_t e = 0; e < dpt; ++e) {
            for (uint32_t ep = 0; ep < dpt; ++ep) {
                const uint64_t digit = digit_of(cb[e], ep, base_bits, ctx->limbs[t].kbits);
                for (uint32_t l = 0; l < L; ++l) {
                    const uint64_t ql = ctx->moduli[l];
                    const uint64_t w = digit >= ql ? digit % ql : digit;
                    host[((static_cast<size_t>(l) * L + t) * dpt + ep) * dpt + e] = {w, static_cast<uint64_t>((static_cast<u128_t>(w) << shift) / ql)};
                }
            }
        }
    }
    const size_t bytes = host.size() * sizeof(ScalarWeight);
    if (ctx->gadget_const_tables.size() >= kConstTablesMax) {
        if (scratch->alloc(bytes)) return 1;
        HIP_TRY(hipMemcpyAsync(scratch->ptr, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // `host` goes out of scope
        *out = static_cast<const ScalarWeight *>(scratch->ptr);
        return 0;
    }
    void *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, bytes));
    const hipError_t e = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return set_error(e, "gadget constant table upload");
    }
    ctx->gadget_const_tables.emplace(std::move(key), dev);
    *out = static_cast<const ScalarWeight *>(dev);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_mul_decompose_gadget_const_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                                              const GpuMatrix *const *addends, size_t n, const uint64_t *const_words,
                                                              size_t words_per_const, int negate, uint32_t base_bits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_mul_decompose_gadget_const_many";
    if (n == 0) return 0;
    if (!const_words || words_per_const == 0) return set_error(std::string(who) + ": null const_words or words_per_const = 0");
    GpuContext *ctx = nullptr;
    uint64_t block_rows = 0;
    if (check_call(who, outs, lhss, addends, n, nullptr, base_bits, &ctx, &block_rows)) return 1;
    const uint32_t L = static_cast<uint32_t>(lhss[0]->level) + 1;
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    // ---- accepted ----
    const bool work = block_rows > 0;
    if (work && ctx_activate(ctx)) return 1;
    std::vector<ScalarLaunch> launches;
    accept_call(outs, lhss, addends, n, static_cast<size_t>(dpt) * L, work, &launches);
    if (!work) return 0;
    CtxBlock scratch(ctx);
    const ScalarWeight *tb = nullptr;
    if (const_table(ctx, L, dpt, base_bits, const_words, words_per_const, &scratch, &tb)) return 1;
    for (const ScalarLaunch &g : launches) {
        const int rc = ctx->wide ? launch_const<uint64_t>(ctx, g, tb, L, dpt, negate ? 1 : 0) : launch_const<uint32_t>(ctx, g, tb, L, dpt, negate ? 1 : 0);
        if (rc) return rc;
    }
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_mul_decompose_gadget_scalar_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                                               const GpuMatrix *const *addends, size_t n, const GpuMatrix *scalar_1x1, int negate,
                                                               uint32_t base_bits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_mul_decompose_gadget_scalar_many";
    if (n == 0) return 0;
    if (!scalar_1x1) return set_error(std::string(who) + ": null scalar");
    GpuContext *ctx = nullptr;
    uint64_t block_rows = 0;
    if (check_call(who, outs, lhss, addends, n, scalar_1x1, base_bits, &ctx, &block_rows)) return 1;
    const uint32_t L = static_cast<uint32_t>(scalar_1x1->level) + 1;
    const uint32_t dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    // ---- accepted ----
    const bool work = block_rows > 0;
    if (work && ctx_activate(ctx)) return 1;
    std::vector<ScalarLaunch> launches;
    accept_call(outs, lhss, addends, n, static_cast<size_t>(dpt) * L, work, &launches);
    if (!work) return 0;
    // the scalar's coefficient residues: its own words, or an inverse transform into scratch
    const size_t poly_bytes = static_cast<size_t>(L) * N * ctx->word_bytes;
    const void *coeff = words_ptr(scalar_1x1);
    CtxBlock scratch(ctx);
    if (scalar_1x1->format == GPU_POLY_FORMAT_EVAL) {
        if (scratch.alloc(poly_bytes)) return 1;
        MXX_TRACED_COPY("copy (device to device)", ctx->stream, 2.0 * poly_bytes,
                        HIP_TRY(hipMemcpyAsync(scratch.ptr, coeff, poly_bytes, hipMemcpyDeviceToDevice, ctx->stream)));
        if (int rc = launch_ntt(ctx, scratch.ptr, L, static_cast<int>(L), true)) return rc;
        coeff = scratch.ptr;
    }
    // the table of a tower is dpt^2 polynomials; towers per group by gpupoly_matrix_mul_decompose's budget rule (a third of
    // what the device could give us now, at least 8 GiB) or MXX_HIP_GADGET_SCALAR_BUDGET
    const size_t tower_bytes = static_cast<size_t>(dpt) * dpt * poly_bytes;
    size_t budget = ctx->env.gadget_scalar_budget;
    if (budget == 0) {
        size_t free_b = 0, total_b = 0;
        budget = size_t(8) << 30;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::max(budget, (free_b + ctx->cached_bytes) / 3);
        else (void)hipGetLastError();
    }
    const uint32_t per_group = static_cast<uint32_t>(std::min<size_t>(L, std::max<size_t>(1, budget / tower_bytes)));
    CtxBlock table(ctx);
    if (table.alloc(per_group * tower_bytes)) return 1;
    for (uint32_t t0 = 0; t0 < L; t0 += per_group) {
        const uint32_t towers = std::min(per_group, L - t0);
        const dim3 blocks = item_grid(static_cast<size_t>(towers) * N, 256);
        MXX_TRACE_BYTES(static_cast<double>(towers) * (N * ctx->word_bytes + tower_bytes));
        if (ctx->wide)
            MXX_LAUNCH(gadget_scalar_table_kernel<uint64_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint64_t *>(table.ptr),
                       static_cast<const uint64_t *>(coeff), ctx->d_limbs, L, N, dpt, base_bits, t0, towers);
        else
            MXX_LAUNCH(gadget_scalar_table_kernel<uint32_t>, blocks, dim3(256), 0, ctx->stream, static_cast<uint32_t *>(table.ptr),
                       static_cast<const uint32_t *>(coeff), ctx->d_limbs, L, N, dpt, base_bits, t0, towers);
        HIP_TRY(hipGetLastError());
        if (int rc = launch_ntt(ctx, table.ptr, static_cast<size_t>(towers) * dpt * dpt * L, static_cast<int>(L), false)) return rc;
        for (const ScalarLaunch &g : launches) {
            const int rc = ctx->wide ? launch_product<uint64_t>(ctx, g, table.ptr, L, dpt, t0, towers, negate ? 1 : 0)
                                     : launch_product<uint32_t>(ctx, g, table.ptr, L, dpt, t0, towers, negate ? 1 : 0);
            if (rc) return rc;
        }
    }
    return 0;
    ABI_GUARD_END
}
