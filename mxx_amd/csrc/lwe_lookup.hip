// lwe_lookup.hip — the online side of the LWE public lookup for S slots of one gate and one output column chunk in one call:
// gpupoly_matrix_lwe_lookup.
//
// The evaluator's public_lookup_poly_gpu (src/lookup/lwe/poly_encoding_gpu.rs:419-453) is a plain loop over the slots around
// public_lookup_slot_gpu (src/lookup/lwe/encoding_gpu.rs:225-370), which per slot s and column chunk forms two products - the
// stored K_high chunk under c_b, the decomposed hash sample K_low under the input vector c_z (compute_wave, :142-188) -, takes
// both through compact bytes, concatenates the chunks per family and adds the two families (:190-223):
//
//   out_s[:, dst_col .. dst_col + c) = c_b_s K_high_s + c_z_s G^-1(U_s[:, col_start .. col_start + c)),
//
// c_b_s r x w, K_high_s w x c, c_z_s r x m_g, U_s the d x m_g uniform matrix under hash_seed_for_matrix(key, tag_s),
// tag_s = "LWE_R_G_<gate>_<lut>_<entry_s>_slot<slot>".  Everything is exact arithmetic on canonical residues, so one sum over
// the w + m_g terms equals the reference's two products and one addition bit for bit.  Per group of slots: one staged copy
// of the slots' table (output, c_b, K_high and c_z pointers), the decomposed-blocks sample [D_0 | D_1 | ...] and ONE kernel
// that forms every output word in one lazy accumulator - the w terms against K_high_s, the m_g terms against D_s, the left
// words read in place through the table - folded every LimbConst::lazy_terms terms wherever they fall, reduced once and
// stored once at dst_col of outs[s].  It is ggh15_lookup.hip's main kernel without weights, first word or left-factor
// pre-pass.  Nothing is uploaded, launched or awaited per slot.
#include "common.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

// the group's device table: [S] output pointers, [S] c_b pointers, [S] K_high pointers, [S] c_z pointers
struct LweLookupArgs {
    const void *v;  // m_g x (S c): slot s at columns [s c, (s + 1) c)
    const uint64_t *table;
    size_t m_g, w, out_cols, dst_col, entries;
    uint32_t S, r, c, L, logN, row_tiles, col_tiles;
};

// A block's tile: rows [r0, r0 + TR) x chunk columns [c0, c0 + TC) of slot s (blockIdx.y/z), blockIdx.x strides the
// polynomial's L N words VN per lane (16 bytes, or one word where a limb vector is narrower; VN divides N: one limb per
// vector).  A lane keeps the TR left words of a term in registers for all TC columns, and every word of K_high_s and D_s is
// loaded by one tile only (TR = r where r <= 2).  Rows and columns past the end repeat the last one and are never stored.
// The TR x TC x VN sums share one count of pending terms - LazyAcc's rule (row_targets.h) with the count kept once; the
// sums start at 0, a residue.
template <typename W, int VN, int TR, int TC>
__global__ void __launch_bounds__(256) lwe_lookup_kernel(LweLookupArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const uint32_t per_slot = a.row_tiles * a.col_tiles;
    const size_t s = entry / per_slot;
    const uint32_t rest = static_cast<uint32_t>(entry - s * per_slot);
    const uint32_t rt = rest / a.col_tiles, ct = rest - rt * a.col_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN;
    W *out = reinterpret_cast<W *>(a.table[s]);
    const W *cb = reinterpret_cast<const W *>(a.table[a.S + s]);
    const W *ksrc = reinterpret_cast<const W *>(a.table[2 * static_cast<size_t>(a.S) + s]);
    const W *cz = reinterpret_cast<const W *>(a.table[3 * static_cast<size_t>(a.S) + s]);
    size_t row[TR], cc[TC];
#pragma unroll
    for (int i = 0; i < TR; ++i) row[i] = min(r0 + i, a.r - 1);
#pragma unroll
    for (int j = 0; j < TC; ++j) cc[j] = min(c0 + j, a.c - 1);
    const size_t v_stride = static_cast<size_t>(a.S) * a.c * wpp, k_stride = static_cast<size_t>(a.c) * wpp;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const LimbConst lc = limbs[w0 >> a.logN];
        const uint32_t lazy = lc.lazy_terms;
        uint32_t pending = 0;
        D acc[TR][TC][VN];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j)
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[i][j][x] = 0;
        auto fold = [&]() {
#pragma unroll
            for (int i = 0; i < TR; ++i)
#pragma unroll
                for (int j = 0; j < TC; ++j)
#pragma unroll
                    for (int x = 0; x < VN; ++x) acc[i][j][x] = lazy_reduce<W>(acc[i][j][x], lc);
            pending = 0;
        };
        // `count` terms lhs[row, rho] * B[rho, column]: lhs has `count` columns, B's column j is at b[j] + rho * stride
        auto stream = [&](const W *lhs, size_t count, const W *(&b)[TC], size_t stride) {
            for (size_t rho = 0; rho < count; ++rho) {
                W av[TR][VN], bv[TC][VN];
#pragma unroll
                for (int i = 0; i < TR; ++i) *reinterpret_cast<V *>(av[i]) = *reinterpret_cast<const V *>(lhs + (row[i] * count + rho) * wpp + w0);
#pragma unroll
                for (int j = 0; j < TC; ++j) *reinterpret_cast<V *>(bv[j]) = *reinterpret_cast<const V *>(b[j] + rho * stride + w0);
                if (pending >= lazy) fold();
#pragma unroll
                for (int i = 0; i < TR; ++i)
#pragma unroll
                    for (int j = 0; j < TC; ++j)
#pragma unroll
                        for (int x = 0; x < VN; ++x) acc[i][j][x] += static_cast<D>(av[i][x]) * bv[j][x];
                ++pending;
            }
        };
        const W *kb[TC], *vb[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            kb[j] = ksrc + cc[j] * wpp;
            vb[j] = static_cast<const W *>(a.v) + (s * a.c + cc[j]) * wpp;
        }
        stream(cb, a.w, kb, k_stride);
        stream(cz, a.m_g, vb, v_stride);
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            if (r0 + i >= a.r) continue;
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                if (c0 + j >= a.c) continue;
                W o[VN];
#pragma unroll
                for (int x = 0; x < VN; ++x) o[x] = lazy_reduce<W>(acc[i][j][x], lc);
                *reinterpret_cast<V *>(out + (static_cast<size_t>(r0 + i) * a.out_cols + a.dst_col + (c0 + j)) * wpp + w0) = *reinterpret_cast<const V *>(o);
            }
        }
    }
}

// what one accepted call works with: S slots; c_b r x w, K_high w x c, c_z r x m_g, outputs r x out_cols written at dst_col
struct LweLookupCall : RowCall {
    size_t S, r, m_g, w, c, out_cols, col_start, dst_col;
    size_t cap;  // a group's scratch
};

// Everything both entries refuse, for every slot, before anything is launched.  `digits` null: the sampling entry, whose
// tags are checked; otherwise the combine entry with [D_0 | D_1 | ...] given.
int check_call(const char *who, GpuMatrix *const *outs, size_t S, size_t dst_col, const GpuMatrix *const *c_bs, const GpuMatrix *const *k_highs,
               const GpuMatrix *const *c_zs, const GpuMatrix *digits, bool full, size_t col_start, uint32_t base_bits, const GpuHashTags *tags,
               LweLookupCall *call) {
    const Refuse refuse{who};
    if (!outs || !c_bs || !k_highs || !c_zs) return refuse("null array");
    if (!full && !digits) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, S, [](size_t s) { return "null output" + slot_at(s); })) return rc;
    for (size_t s = 0; s < S; ++s)
        if (!c_bs[s] || !k_highs[s] || !c_zs[s]) return refuse("null operand" + slot_at(s));
    if (int rc = refuse_base_level(refuse, c_zs[0], base_bits, full, call)) return rc;
    const size_t r = c_zs[0]->rows, m_g = c_zs[0]->cols, w = k_highs[0]->rows, c = k_highs[0]->cols, out_cols = outs[0]->cols;
    if (m_g % call->k != 0) return refuse("shape mismatch: the input vectors have d * digits per tower * limbs columns");
    for (size_t s = 0; s < S; ++s) {
        const std::string at = slot_at(s);
        for (const GpuMatrix *m : {c_bs[s], k_highs[s], c_zs[s]})
            if (int rc = refuse_foreign(refuse, m, *call, at)) return rc;
        if (k_highs[s]->cols != c) return refuse("the K_high chunks differ in width" + at);
        if (k_highs[s]->rows != w) return refuse("shape mismatch: a K_high chunk is w x chunk columns" + at);
        if (c_bs[s]->rows != r || c_bs[s]->cols != w) return refuse("shape mismatch: a c_b is r x w" + at);
        if (c_zs[s]->rows != r || c_zs[s]->cols != m_g) return refuse("shape mismatch: an input vector is r x m_g" + at);
        for (const GpuMatrix *m : {c_bs[s], k_highs[s], c_zs[s]})
            if (m->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + at);
    }
    if (col_start > m_g || c > m_g - col_start) return refuse("column chunk past the operands' columns");
    if (r > 0xffffffffull || c > 0xffffffffull || S > 0xffffffffull || out_cols > 0xffffffffull || (c && S > ~size_t(0) / c)) return refuse("matrix too large");
    if (digits)
        if (int rc = refuse_operand(refuse, digits, *call, m_g, S * c, "shape mismatch: the digits are m_g x (slots * chunk columns)")) return rc;
    if (int rc = refuse_outputs(refuse, outs, S, *call, slot_at, [&](const GpuMatrix *out) -> const char * {
            if (out->cols != out_cols) return "the outputs differ in width";
            return out->rows != r ? "shape mismatch: an output is r x output columns" : nullptr;
        }))
        return rc;
    if (dst_col > out_cols || c > out_cols - dst_col) return refuse("column block past the outputs' columns");
    if (!(dst_col == 0 && c == out_cols))
        for (size_t s = 0; s < S; ++s)
            if (outs[s]->format != GPU_POLY_FORMAT_EVAL) return refuse("a partial column block needs an output already in Eval format" + slot_at(s));
    call->S = S, call->r = r, call->m_g = m_g, call->w = w, call->c = c, call->out_cols = out_cols, call->col_start = col_start, call->dst_col = dst_col;
    call->cap = call->ctx->env.lwe_lookup_budget ? call->ctx->env.lwe_lookup_budget : kRowGroupBytes;
    // an output is written while every operand is still being read, and by no other slot
    const GpuMatrix *operands[1] = {digits};
    static const char *const names[1] = {"the digits"};
    if (int rc = refuse_tags_overlap(refuse, full ? tags : nullptr, S, outs, S, operands, names, digits ? 1 : 0)) return rc;
    const std::string overlap = slot_operands_overlap(outs, S, {c_bs, k_highs, c_zs});
    return overlap.empty() ? 0 : refuse(overlap);
}

// the column tile and the row tile of a call, and the tiles per slot
struct LweLookupTiles {
    int tr, tc;
    uint32_t row_tiles, col_tiles;
};
LweLookupTiles lookup_tiles(const LweLookupCall &call) {
    LweLookupTiles t;
    t.tr = call.r >= 2 ? 2 : 1;
    t.tc = call.c >= 3 ? 4 : call.c == 2 ? 2 : 1;
    t.row_tiles = static_cast<uint32_t>((call.r + t.tr - 1) / t.tr);
    t.col_tiles = static_cast<uint32_t>((call.c + t.tc - 1) / t.tc);
    return t;
}
bool grid_fits(const LweLookupCall &call, size_t Sg) {
    const LweLookupTiles t = lookup_tiles(call);
    return Sg * t.row_tiles * t.col_tiles <= size_t(65535) * 65535;
}

template <typename W, int VN>
int launch_main(GpuContext *ctx, const LweLookupArgs &a, const LweLookupTiles &t, dim3 grid, dim3 block) {
#define MXX_LWE_LOOKUP_TILE(R, Cc) \
    if (t.tr == R && t.tc == Cc) MXX_LAUNCH((lwe_lookup_kernel<W, VN, R, Cc>), grid, block, 0, ctx->stream, a, ctx->d_limbs)
    MXX_LWE_LOOKUP_TILE(1, 1);
    MXX_LWE_LOOKUP_TILE(1, 2);
    MXX_LWE_LOOKUP_TILE(1, 4);
    MXX_LWE_LOOKUP_TILE(2, 1);
    MXX_LWE_LOOKUP_TILE(2, 2);
    MXX_LWE_LOOKUP_TILE(2, 4);
#undef MXX_LWE_LOOKUP_TILE
    HIP_TRY(hipGetLastError());
    return 0;
}

// slots [s0, s0 + Sg) with their digits at `v` (m_g x (Sg c) words): the table in one staged copy, the kernel
int combine_group(const LweLookupCall &call, GpuMatrix *const *outs, const GpuMatrix *const *c_bs, const GpuMatrix *const *k_highs,
                  const GpuMatrix *const *c_zs, size_t s0, size_t Sg, const void *v) {
    GpuContext *ctx = call.ctx;
    static thread_local std::vector<uint64_t> staging;
    staging.resize(4 * Sg);
    for (size_t s = 0; s < Sg; ++s) {
        staging[s] = reinterpret_cast<uint64_t>(words_ptr(outs[s0 + s]));
        staging[Sg + s] = reinterpret_cast<uint64_t>(words_ptr(c_bs[s0 + s]));
        staging[2 * Sg + s] = reinterpret_cast<uint64_t>(words_ptr(k_highs[s0 + s]));
        staging[3 * Sg + s] = reinterpret_cast<uint64_t>(words_ptr(c_zs[s0 + s]));
    }
    CtxBlock block(ctx);
    if (upload_table(block, "LWE lookup slot table (host to device)", staging)) return 1;
    const size_t wpp = static_cast<size_t>(call.L) << ctx->logN, poly_bytes = wpp * ctx->word_bytes;
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    const LweLookupTiles t = lookup_tiles(call);
    LweLookupArgs a;
    a.v = v, a.table = static_cast<const uint64_t *>(block.ptr);
    a.m_g = call.m_g, a.w = call.w, a.out_cols = call.out_cols, a.dst_col = call.dst_col;
    a.entries = Sg * t.row_tiles * t.col_tiles;
    a.S = static_cast<uint32_t>(Sg), a.r = static_cast<uint32_t>(call.r), a.c = static_cast<uint32_t>(call.c);
    a.L = call.L, a.logN = ctx->logN, a.row_tiles = t.row_tiles, a.col_tiles = t.col_tiles;
    const size_t vecs = wpp / vn;
    size_t gy, gz;
    (void)fold_yz(a.entries, gy, gz);  // grid_plan.h; the count was held to 65535 x 65535 with the refusals (grid_fits)
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // [K_high_s; D_s] read once per row tile, [c_b_s | c_z_s] once per column tile, the outputs' block written once
    MXX_TRACE_BYTES(static_cast<double>(Sg) * poly_bytes *
                    (static_cast<double>(t.row_tiles) * (call.m_g + call.w) * call.c + static_cast<double>(t.col_tiles) * call.r * (call.m_g + call.w) +
                     static_cast<double>(call.r) * call.c));
    if (ctx->wide && vn > 1) return launch_main<uint64_t, 2>(ctx, a, t, grid, dim3(threads));
    if (ctx->wide) return launch_main<uint64_t, 1>(ctx, a, t, grid, dim3(threads));
    if (vn > 1) return launch_main<uint32_t, 4>(ctx, a, t, grid, dim3(threads));
    return launch_main<uint32_t, 1>(ctx, a, t, grid, dim3(threads));
}

// after the refusals: the outputs' tags, then (*go) whether anything is left to launch; PACKED24 operands unpacked once
int accept(const LweLookupCall &call, GpuMatrix *const *outs, const GpuMatrix *const *c_bs, const GpuMatrix *const *k_highs,
           const GpuMatrix *const *c_zs, const GpuMatrix *digits, bool *go) {
    for (size_t s = 0; s < call.S; ++s) outs[s]->format = GPU_POLY_FORMAT_EVAL;
    *go = call.r != 0 && call.c != 0;
    if (!*go) return 0;
    if (ctx_activate(call.ctx)) return 1;
    for (size_t s = 0; s < call.S; ++s) words_ptr(c_bs[s]), words_ptr(k_highs[s]), words_ptr(c_zs[s]), words_ptr(outs[s]);
    if (digits) words_ptr(digits);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_lwe_lookup(GpuMatrix *const *outs, size_t nslots_S, size_t dst_col, const GpuMatrix *const *c_bs,
                                         const GpuMatrix *const *k_highs, const GpuMatrix *const *c_zs, size_t col_start, uint32_t base_bits,
                                         const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lwe_lookup";
    const size_t S = nslots_S;
    if (S == 0) return 0;
    LweLookupCall call;
    if (check_call(who, outs, S, dst_col, c_bs, k_highs, c_zs, nullptr, true, col_start, base_bits, tags, &call)) return 1;
    GpuContext *ctx = call.ctx;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // a slot's scratch: its digits m_g x c
    const size_t v_bytes = call.m_g * call.c * poly_bytes;
    const size_t slot_bytes = std::max<size_t>(v_bytes, 1);
    const size_t per_group = rows_per_group(S, slot_bytes, call.cap);
    if (!grid_fits(call, per_group)) return set_error(std::string(who) + ": too many output tiles in one group");
    // ---- accepted ----
    bool go;
    if (accept(call, outs, c_bs, k_highs, c_zs, nullptr, &go)) return 1;
    if (!go) return 0;
    CtxBlock digits(ctx);
    if (digits.alloc(per_group * v_bytes)) return 1;
    return for_row_groups(
        S, slot_bytes, tags,
        [&](size_t s0, size_t Sg, const GpuHashTags &part) {
            GpuMatrix v = scratch_matrix(ctx, call.level, call.m_g, Sg * call.c, digits.ptr);
            if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Sg, base_bits, 0, call.m_g / call.k,
                                                       call.m_g, col_start))
                return rc;
            return combine_group(call, outs, c_bs, k_highs, c_zs, s0, Sg, digits.ptr);
        },
        call.cap);
    ABI_GUARD_END
}

// The same with the digits [D_0 | D_1 | ...] given instead of sampled: the table copy and the kernel alone, one group.
// A test instrument (tests/test_gpu_lwe_lookup.py reaches the lazy accumulator's bound with operands no sampler gives).
extern "C" int gpupoly_matrix_lwe_lookup_combine(GpuMatrix *const *outs, size_t nslots_S, size_t dst_col, const GpuMatrix *const *c_bs,
                                                 const GpuMatrix *const *k_highs, const GpuMatrix *const *c_zs, size_t col_start,
                                                 uint32_t base_bits, const GpuMatrix *digits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_lwe_lookup_combine";
    const size_t S = nslots_S;
    if (S == 0) return 0;
    LweLookupCall call;
    if (check_call(who, outs, S, dst_col, c_bs, k_highs, c_zs, digits, false, col_start, base_bits, nullptr, &call)) return 1;
    if (!grid_fits(call, S)) return set_error(std::string(who) + ": too many output tiles in one group");
    bool go;
    if (accept(call, outs, c_bs, k_highs, c_zs, digits, &go)) return 1;
    if (!go) return 0;
    return combine_group(call, outs, c_bs, k_highs, c_zs, 0, S, words_ptr(digits));
    ABI_GUARD_END
}
