// slot_transfer_eval.hip — stage 2 of the slot-transfer online evaluation for S outputs of one gate and one output column
// chunk in one call: gpupoly_matrix_slot_transfer_eval.
//
// The evaluator's output_slot_for_params and slot_reduce_output_slot_for_params (src/slot_transfer/bgg_poly_encoding.rs:119-248,
// :250-386; the device path is src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786, one one-row product per task and chunk
// behind the plain `for dst_slot` loop of evaluate_slot_transfer_slots_gpu, :748-786) compute, per destination slot s with
// terms t,
//
//   out_s = c_b0 Pg_s + sum_t x^shift_t o kappa_t o ( c_in_t G^-1(A_s) + mu_t o ((c_b0 P0_src_t) P1_s) ),
//
// c_b0 r x w0 shared by every slot, Pg_s the stored gate preimage (w0 x m_g), P0_src (w0 x w1) and P1_s (w1 x m_g) the stored slot
// preimages, A_s the d x m_g uniform matrix under hash_seed_for_matrix(key, "slot_transfer_slot_a_<s>"), mu_t the constant
// coefficient of the source plaintext, kappa_t the optional scalar; slot_transfer has one term per output with shift 0,
// slot_reduce num_slots terms with shift = the source index and kappa = 1.  Everything is exact ring arithmetic on canonical
// residues, so the products re-associate without changing a bit.  Stage 1 - the caller's, with the library's product entries
// - is mid_src = c_b0 P0_src, once per DISTINCT source.  Stage 2, this file, per column chunk:
//
//   LhsA_s = sum_t (kappa_t x^shift_t) o c_in_t           r x m_g
//   LhsB_s = sum_t (kappa_t mu_t x^shift_t) o mid_src_t   r x w1
//   out_s[:, chunk] = c_b0 Pg_s[:, chunk] + LhsA_s D_s + LhsB_s P1_s[:, chunk],      D_s = G^-1(A_s[:, chunk]).
//
// Per group of outputs: one staged copy of the table (per output: the output, Pg, P1 and A-segment pointers, the term range;
// per term: the c_in and mid pointers, the shift mod 2N and per limb the weights kappa mod q_l and kappa mu mod q_l, computed on
// the host, slot_weights.h), the decomposed-blocks sample [D_0 | D_1 | ...], one pre-pass kernel that writes LhsA and LhsB
// with canonical residues, and ONE main kernel - lwe_lookup_kernel's register tile with three streams into one lazy
// accumulator.  An output whose only term has shift 0 and scalar 1 gets no A segment: its table entry points at c_in itself.
// Nothing is uploaded, launched or awaited per output or per term.
#include "common.h"
#include "modarith.h"
#include "monomial_factor.h"
#include "row_targets.h"
#include "slot_weights.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

// The group's device table, 8-byte words.  Sg outputs, Tg terms:
//   [0, Sg) outputs  [Sg, 2 Sg) Pg  [2 Sg, 3 Sg) P1  [3 Sg, 4 Sg) the A segment's left words (LhsA's rows or c_in itself)
//   [4 Sg, 5 Sg + 1) the outputs' first terms within the group  [5 Sg + 1, 6 Sg + 1) 1 where the A segment is c_in in place
//   then [Tg] c_in pointers, [Tg] mid pointers, [Tg] shifts mod 2N, [Tg][L][2] weights {kappa, kappa mu} mod q_l
struct SlotTable {
    const uint64_t *words;
    uint32_t S, T, L;
    __host__ __device__ size_t outs() const { return 0; }
    __host__ __device__ size_t pg() const { return S; }
    __host__ __device__ size_t p1() const { return 2 * static_cast<size_t>(S); }
    __host__ __device__ size_t lhs_a() const { return 3 * static_cast<size_t>(S); }
    __host__ __device__ size_t first_term() const { return 4 * static_cast<size_t>(S); }
    __host__ __device__ size_t in_place() const { return 5 * static_cast<size_t>(S) + 1; }
    __host__ __device__ size_t c_in() const { return 6 * static_cast<size_t>(S) + 1; }
    __host__ __device__ size_t mid() const { return c_in() + T; }
    __host__ __device__ size_t shift() const { return c_in() + 2 * static_cast<size_t>(T); }
    __host__ __device__ size_t weights() const { return c_in() + 3 * static_cast<size_t>(T); }
    __host__ __device__ size_t size() const { return weights() + 2 * static_cast<size_t>(T) * L; }
};

struct LhsArgs {
    SlotTable table;
    void *lhs_b;  // (Sg r) x w1; LhsA's rows are reached through the table
    const void *tw;
    size_t polys_a, polys_b, entries;  // r m_g and r w1 polynomials per output; entries = Sg * (tiles_a + tiles_b)
    uint32_t tiles_a, tiles_b, N, logN, slot_blocks;
};

// The pre-pass.  blockIdx.y/z = (output, tile of PT polynomials of its A segment, then of its B segment), blockIdx.x = limb *
// slot_blocks + slot block: a thread owns SV consecutive evaluation slots of PT polynomials of one limb
// (monomial_sum_eval_kernel's shape).  Per term the factor weight * psi^(shift (2 bitrev(k) + 1)) is formed once - the table
// gather skipped when the shift is 0 - and multiplies the tile; the raw products are accumulated lazily, folded every
// lazy_terms of them and reduced once.  A tile past the segment's last polynomial re-reads the last one and is not stored.
template <typename W, int SV, int PT>
__global__ void __launch_bounds__(256) slot_eval_lhs_kernel(LhsArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, SV>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const uint32_t limb = blockIdx.x / a.slot_blocks, sb = blockIdx.x - limb * a.slot_blocks;
    const uint32_t k0 = (sb * blockDim.x + threadIdx.x) * SV;
    if (k0 >= a.N) return;
    const uint32_t per_out = a.tiles_a + a.tiles_b;
    const size_t s = entry / per_out;
    const uint32_t tile = static_cast<uint32_t>(entry - s * per_out);
    const bool seg_b = tile >= a.tiles_a;
    const uint64_t *tb = a.table.words;
    if (!seg_b && tb[a.table.in_place() + s]) return;  // the main kernel reads c_in itself
    const size_t polys = seg_b ? a.polys_b : a.polys_a;
    const size_t p0 = static_cast<size_t>(seg_b ? tile - a.tiles_a : tile) * PT;
    const size_t wpp = static_cast<size_t>(a.table.L) << a.logN;
    const LimbConst lc = limbs[limb];
    const W q = static_cast<W>(lc.q);
    const W *twl = static_cast<const W *>(a.tw) + static_cast<size_t>(limb) * a.N;
    size_t off[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) off[p] = min(p0 + p, polys - 1) * wpp + (static_cast<size_t>(limb) << a.logN) + k0;
    uint32_t odd[SV];
#pragma unroll
    for (int x = 0; x < SV; ++x) odd[x] = 2u * bitrev_n(k0 + x, a.logN) + 1u;
    D acc[PT][SV];
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int x = 0; x < SV; ++x) acc[p][x] = 0;
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
    const size_t t_end = tb[a.table.first_term() + s + 1];
    for (size_t t = tb[a.table.first_term() + s]; t < t_end; ++t) {
        const W *src = reinterpret_cast<const W *>(tb[(seg_b ? a.table.mid() : a.table.c_in()) + t]);
        W v[PT][SV];
#pragma unroll
        for (int p = 0; p < PT; ++p) *reinterpret_cast<V *>(v[p]) = *reinterpret_cast<const V *>(src + off[p]);
        const uint32_t sh = static_cast<uint32_t>(tb[a.table.shift() + t]);
        const W weight = static_cast<W>(tb[a.table.weights() + 2 * (t * a.table.L + limb) + (seg_b ? 1 : 0)]);
        W f[SV];
#pragma unroll
        for (int x = 0; x < SV; ++x) f[x] = sh ? mul_mod<W>(weight, monomial_factor<W>(twl, sh, odd[x], a.N, a.logN, q), q, lc.mu, lc.kbits) : weight;
        if (pending >= lazy) {
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int x = 0; x < SV; ++x) acc[p][x] = lazy_reduce<W>(acc[p][x], lc);
            pending = 0;
        }
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int x = 0; x < SV; ++x) acc[p][x] += static_cast<D>(v[p][x]) * f[x];
        ++pending;
    }
    W *dst = seg_b ? static_cast<W *>(a.lhs_b) + s * a.polys_b * wpp : reinterpret_cast<W *>(tb[a.table.lhs_a() + s]);
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if (p0 + p >= polys) continue;
        W o[SV];
#pragma unroll
        for (int x = 0; x < SV; ++x) o[x] = lazy_reduce<W>(acc[p][x], lc);
        *reinterpret_cast<V *>(dst + off[p]) = *reinterpret_cast<const V *>(o);
    }
}

struct EvalArgs {
    SlotTable table;
    const void *c_b0;   // r x w0
    const void *lhs_b;  // (Sg r) x w1
    const void *v;      // m_g x (Sg c): output s at columns [s c, (s + 1) c)
    size_t m_g, w0, w1, out_cols, dst_col, entries;
    uint32_t r, c, logN, row_tiles, col_tiles;
};

// A block's tile: rows [r0, r0 + TR) x chunk columns [c0, c0 + TC) of output s (blockIdx.y/z), blockIdx.x strides the
// polynomial's L N words VN per lane (16 bytes, or one word where a limb vector is narrower; VN divides N: one limb per
// vector) - lwe_lookup_kernel's tile with three streams: the w0 terms of c_b0 against Pg_s, the m_g terms of the A segment
// against D_s, the w1 terms of LhsB_s against P1_s.  A lane keeps the TR left words of a term in registers for all TC
// columns, and every word of Pg_s, D_s and P1_s is loaded by one tile only (TR = r where r <= 2).  Rows and columns past the
// end repeat the last one and are never stored.  The TR x TC x VN sums share one count of pending terms - LazyAcc's rule
// (row_targets.h) with the count kept once; the sums start at 0, a residue.
template <typename W, int VN, int TR, int TC>
__global__ void __launch_bounds__(256) slot_eval_kernel(EvalArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const uint32_t per_slot = a.row_tiles * a.col_tiles;
    const size_t s = entry / per_slot;
    const uint32_t rest = static_cast<uint32_t>(entry - s * per_slot);
    const uint32_t rt = rest / a.col_tiles, ct = rest - rt * a.col_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const size_t wpp = static_cast<size_t>(a.table.L) << a.logN;
    const uint64_t *tb = a.table.words;
    W *out = reinterpret_cast<W *>(tb[a.table.outs() + s]);
    const W *pg = reinterpret_cast<const W *>(tb[a.table.pg() + s]);
    const W *p1 = reinterpret_cast<const W *>(tb[a.table.p1() + s]);
    const W *lhs_a = reinterpret_cast<const W *>(tb[a.table.lhs_a() + s]);
    const W *lhs_b = static_cast<const W *>(a.lhs_b) + s * a.r * a.w1 * wpp;
    size_t row[TR], cc[TC];
#pragma unroll
    for (int i = 0; i < TR; ++i) row[i] = min(r0 + i, a.r - 1);
#pragma unroll
    for (int j = 0; j < TC; ++j) cc[j] = min(c0 + j, a.c - 1);
    const size_t v_stride = static_cast<size_t>(a.table.S) * a.c * wpp, k_stride = static_cast<size_t>(a.c) * wpp;
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
        const W *gb[TC], *vb[TC], *pb[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            gb[j] = pg + cc[j] * wpp;
            vb[j] = static_cast<const W *>(a.v) + (s * a.c + cc[j]) * wpp;
            pb[j] = p1 + cc[j] * wpp;
        }
        stream(static_cast<const W *>(a.c_b0), a.w0, gb, k_stride);
        stream(lhs_a, a.m_g, vb, v_stride);
        stream(lhs_b, a.w1, pb, k_stride);
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

inline std::string term_at(size_t t) { return " (term " + std::to_string(t) + ")"; }

// what one accepted call works with: S outputs, T terms; c_b0 r x w0, Pg w0 x c, P1 w1 x c, c_in r x m_g, mid r x w1, outputs
// r x out_cols written at dst_col
struct SlotEvalCall : RowCall {
    size_t S, T, r, m_g, w0, w1, c, out_cols, col_start, dst_col;
    size_t cap;  // a group's scratch
};

// Everything both entries refuse, for every output and term, before anything is launched.  `digits` null: the sampling
// entry, whose tags are checked; otherwise the combine entry with [D_0 | D_1 | ...] given.
int check_call(const char *who, GpuMatrix *const *outs, size_t S, size_t dst_col, const GpuMatrix *c_b0, const GpuMatrix *const *gate_preimages,
               const GpuMatrix *const *b1_preimages, const GpuSlotTerm *terms, const size_t *term_offsets, const uint64_t *mu_words,
               size_t words_per_mu, const GpuMatrix *digits, bool full, size_t col_start, uint32_t base_bits, const GpuHashTags *tags,
               SlotEvalCall *call) {
    const Refuse refuse{who};
    if (!outs || !gate_preimages || !b1_preimages || !terms || !term_offsets || !mu_words) return refuse("null array");
    if (!c_b0) return refuse("null operand");
    if (!full && !digits) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (int rc = refuse_null_outputs(refuse, outs, S, [](size_t s) { return "null output" + slot_at(s); })) return rc;
    for (size_t s = 0; s < S; ++s)
        if (!gate_preimages[s] || !b1_preimages[s]) return refuse("null operand" + slot_at(s));
    if (term_offsets[0] != 0) return refuse("term_offsets must start at 0");
    for (size_t s = 0; s < S; ++s) {
        if (term_offsets[s + 1] < term_offsets[s]) return refuse("term_offsets must not decrease" + slot_at(s));
        if (term_offsets[s + 1] == term_offsets[s]) return refuse("an output without terms" + slot_at(s));
    }
    const size_t T = term_offsets[S];
    for (size_t t = 0; t < T; ++t)
        if (!terms[t].c_in || !terms[t].mid) return refuse("null operand" + term_at(t));
    if (words_per_mu == 0) return refuse("words_per_mu = 0");
    if (int rc = refuse_base_level(refuse, c_b0, base_bits, full, call)) return rc;
    const size_t r = c_b0->rows, w0 = c_b0->cols, m_g = terms[0].c_in->cols, w1 = b1_preimages[0]->rows, c = gate_preimages[0]->cols,
                 out_cols = outs[0]->cols;
    if (c_b0->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
    // m_g is read off the first term's input vector, k off c_b0's context: the two must be of one context and level first
    if (int rc = refuse_foreign(refuse, terms[0].c_in, *call, term_at(0))) return rc;
    if (m_g % call->k != 0) return refuse("shape mismatch: the input vectors have d * digits per tower * limbs columns");
    for (size_t s = 0; s < S; ++s) {
        const std::string at = slot_at(s);
        for (const GpuMatrix *m : {gate_preimages[s], b1_preimages[s]})
            if (int rc = refuse_foreign(refuse, m, *call, at)) return rc;
        if (gate_preimages[s]->cols != c || b1_preimages[s]->cols != c) return refuse("the preimage chunks differ in width" + at);
        if (gate_preimages[s]->rows != w0) return refuse("shape mismatch: a gate preimage chunk is w0 x chunk columns" + at);
        if (b1_preimages[s]->rows != w1) return refuse("shape mismatch: a slot preimage chunk is w1 x chunk columns" + at);
        for (const GpuMatrix *m : {gate_preimages[s], b1_preimages[s]})
            if (m->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + at);
    }
    for (size_t t = 0; t < T; ++t) {
        const std::string at = term_at(t);
        for (const GpuMatrix *m : {terms[t].c_in, terms[t].mid})
            if (int rc = refuse_foreign(refuse, m, *call, at)) return rc;
        if (terms[t].c_in->rows != r || terms[t].c_in->cols != m_g) return refuse("shape mismatch: an input vector is r x m_g" + at);
        if (terms[t].mid->rows != r || terms[t].mid->cols != w1) return refuse("shape mismatch: a stage-1 product is r x w1" + at);
        for (const GpuMatrix *m : {terms[t].c_in, terms[t].mid})
            if (m->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + at);
    }
    if (m_g % call->k != 0) return refuse("shape mismatch: the input vectors have d * digits per tower * limbs columns");
    if (col_start > m_g || c > m_g - col_start) return refuse("column chunk past the operands' columns");
    if (r > 0xffffffffull || c > 0xffffffffull || S > 0xffffffffull || T > 0xffffffffull || out_cols > 0xffffffffull || (c && S > ~size_t(0) / c))
        return refuse("matrix too large");
    if (digits)
        if (int rc = refuse_operand(refuse, digits, *call, m_g, S * c, "shape mismatch: the digits are m_g x (outputs * chunk columns)")) return rc;
    if (int rc = refuse_outputs(refuse, outs, S, *call, slot_at, [&](const GpuMatrix *out) -> const char * {
            if (out->cols != out_cols) return "the outputs differ in width";
            return out->rows != r ? "shape mismatch: an output is r x output columns" : nullptr;
        }))
        return rc;
    if (dst_col > out_cols || c > out_cols - dst_col) return refuse("column block past the outputs' columns");
    if (!(dst_col == 0 && c == out_cols))
        for (size_t s = 0; s < S; ++s)
            if (outs[s]->format != GPU_POLY_FORMAT_EVAL) return refuse("a partial column block needs an output already in Eval format" + slot_at(s));
    call->S = S, call->T = T, call->r = r, call->m_g = m_g, call->w0 = w0, call->w1 = w1, call->c = c, call->out_cols = out_cols;
    call->col_start = col_start, call->dst_col = dst_col;
    call->cap = call->ctx->env.slot_eval_budget ? call->ctx->env.slot_eval_budget : kRowGroupBytes;
    // an output is written while every operand is still being read, and by no other output
    const GpuMatrix *operands[2] = {c_b0, digits};
    static const char *const names[2] = {"c_b0", "the digits"};
    if (int rc = refuse_tags_overlap(refuse, full ? tags : nullptr, S, outs, S, operands, names, digits ? 2 : 1)) return rc;
    std::vector<const GpuMatrix *> of_terms(2 * T);
    for (size_t t = 0; t < T; ++t) of_terms[2 * t] = terms[t].c_in, of_terms[2 * t + 1] = terms[t].mid;
    const std::string overlap = slot_operands_overlap(outs, S, {gate_preimages, b1_preimages}, of_terms.data(), of_terms.size());
    return overlap.empty() ? 0 : refuse(overlap);
}

// the column tile and the row tile of a call, and the tiles per output
struct EvalTiles {
    int tr, tc;
    uint32_t row_tiles, col_tiles;
};
EvalTiles eval_tiles(const SlotEvalCall &call) {
    EvalTiles t;
    t.tr = call.r >= 2 ? 2 : 1;
    t.tc = call.c >= 3 ? 4 : call.c == 2 ? 2 : 1;
    t.row_tiles = static_cast<uint32_t>((call.r + t.tr - 1) / t.tr);
    t.col_tiles = static_cast<uint32_t>((call.c + t.tc - 1) / t.tc);
    return t;
}
constexpr int kLhsTile = 4;  // polynomials per thread of the pre-pass: one factor serves them all
size_t lhs_tiles(size_t polys) { return (polys + kLhsTile - 1) / kLhsTile; }
bool grid_fits(const SlotEvalCall &call, size_t Sg) {
    const EvalTiles t = eval_tiles(call);
    const size_t limit = size_t(65535) * 65535;
    const size_t pre = lhs_tiles(call.r * call.m_g) + lhs_tiles(call.r * call.w1);
    return Sg * t.row_tiles * t.col_tiles <= limit && (pre == 0 || Sg <= limit / pre);
}

template <typename W, int VN>
int launch_main(GpuContext *ctx, const EvalArgs &a, const EvalTiles &t, dim3 grid, dim3 block) {
#define MXX_SLOT_EVAL_TILE(R, Cc) \
    if (t.tr == R && t.tc == Cc) MXX_LAUNCH((slot_eval_kernel<W, VN, R, Cc>), grid, block, 0, ctx->stream, a, ctx->d_limbs)
    MXX_SLOT_EVAL_TILE(1, 1);
    MXX_SLOT_EVAL_TILE(1, 2);
    MXX_SLOT_EVAL_TILE(1, 4);
    MXX_SLOT_EVAL_TILE(2, 1);
    MXX_SLOT_EVAL_TILE(2, 2);
    MXX_SLOT_EVAL_TILE(2, 4);
#undef MXX_SLOT_EVAL_TILE
    HIP_TRY(hipGetLastError());
    return 0;
}

// outputs [s0, s0 + Sg) with their digits at `v` (m_g x (Sg c) words): the table in one staged copy, the pre-pass into
// `lhs_a` ((Sg r) x m_g words) and `lhs_b` ((Sg r) x w1 words), the main kernel
int combine_group(const SlotEvalCall &call, GpuMatrix *const *outs, const GpuMatrix *c_b0, const GpuMatrix *const *gate_preimages,
                  const GpuMatrix *const *b1_preimages, const GpuSlotTerm *terms, const size_t *term_offsets, const uint64_t *mu_words,
                  size_t words_per_mu, size_t s0, size_t Sg, const void *v, void *lhs_a, void *lhs_b) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, t0 = term_offsets[s0], Tg = term_offsets[s0 + Sg] - t0;
    const size_t wpp = L << ctx->logN, poly_bytes = wpp * ctx->word_bytes;
    const uint64_t mask = 2ull * static_cast<uint64_t>(ctx->N) - 1ull;
    SlotTable tab{nullptr, static_cast<uint32_t>(Sg), static_cast<uint32_t>(Tg), call.L};
    static thread_local std::vector<uint64_t> staging;
    staging.resize(tab.size());
    for (size_t s = 0; s < Sg; ++s) {
        const size_t first = term_offsets[s0 + s], count = term_offsets[s0 + s + 1] - first;
        const bool in_place = count == 1 && (terms[first].shift & mask) == 0 && terms[first].scalar == 1;
        staging[tab.outs() + s] = reinterpret_cast<uint64_t>(words_ptr(outs[s0 + s]));
        staging[tab.pg() + s] = reinterpret_cast<uint64_t>(words_ptr(gate_preimages[s0 + s]));
        staging[tab.p1() + s] = reinterpret_cast<uint64_t>(words_ptr(b1_preimages[s0 + s]));
        staging[tab.lhs_a() + s] = in_place ? reinterpret_cast<uint64_t>(words_ptr(terms[first].c_in))
                                            : reinterpret_cast<uint64_t>(static_cast<char *>(lhs_a) + s * call.r * call.m_g * poly_bytes);
        staging[tab.first_term() + s] = first - t0;
        staging[tab.in_place() + s] = in_place ? 1 : 0;
    }
    staging[tab.first_term() + Sg] = Tg;
    for (size_t t = 0; t < Tg; ++t) {
        const GpuSlotTerm &term = terms[t0 + t];
        staging[tab.c_in() + t] = reinterpret_cast<uint64_t>(words_ptr(term.c_in));
        staging[tab.mid() + t] = reinterpret_cast<uint64_t>(words_ptr(term.mid));
        staging[tab.shift() + t] = term.shift & mask;
        slot_eval::term_weights(term.scalar, mu_words + (t0 + t) * words_per_mu, words_per_mu, ctx->moduli.data(), L, &staging[tab.weights() + 2 * t * L]);
    }
    CtxBlock block(ctx);
    if (upload_table(block, "slot-transfer evaluation table (host to device)", staging)) return 1;
    tab.words = static_cast<const uint64_t *>(block.ptr);
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;

    LhsArgs la;
    la.table = tab, la.lhs_b = lhs_b, la.tw = ctx->d_tw_fwd;
    la.polys_a = call.r * call.m_g, la.polys_b = call.r * call.w1;
    la.tiles_a = static_cast<uint32_t>(lhs_tiles(la.polys_a)), la.tiles_b = static_cast<uint32_t>(lhs_tiles(la.polys_b));
    la.entries = Sg * (static_cast<size_t>(la.tiles_a) + la.tiles_b);
    la.N = static_cast<uint32_t>(ctx->N), la.logN = ctx->logN;
    if (la.entries) {  // m_g = 0 and w1 = 0: nothing to prepare
        const uint32_t lanes = static_cast<uint32_t>(ctx->N / vn);
        const uint32_t threads = std::min<uint32_t>(256, (lanes + 63) / 64 * 64);
        la.slot_blocks = (lanes + threads - 1) / threads;
        size_t gy, gz;
        (void)fold_yz(la.entries, gy, gz);  // grid_plan.h; the count was held to 65535 x 65535 with the refusals (grid_fits)
        const dim3 grid(static_cast<unsigned>(la.slot_blocks * L), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
        // every term's c_in and mid read once, LhsA and LhsB written once (an in-place A segment is neither read nor written)
        double moved = 0;
        for (size_t s = 0; s < Sg; ++s) {
            const double count = static_cast<double>(staging[tab.first_term() + s + 1] - staging[tab.first_term() + s]);
            moved += (count + 1) * (static_cast<double>(la.polys_b) + (staging[tab.in_place() + s] ? 0.0 : static_cast<double>(la.polys_a)));
        }
        MXX_TRACE_BYTES(moved * poly_bytes);
        if (ctx->wide && vn > 1) MXX_LAUNCH((slot_eval_lhs_kernel<uint64_t, 2, kLhsTile>), grid, dim3(threads), 0, ctx->stream, la, ctx->d_limbs);
        else if (ctx->wide) MXX_LAUNCH((slot_eval_lhs_kernel<uint64_t, 1, kLhsTile>), grid, dim3(threads), 0, ctx->stream, la, ctx->d_limbs);
        else if (vn > 1) MXX_LAUNCH((slot_eval_lhs_kernel<uint32_t, 4, kLhsTile>), grid, dim3(threads), 0, ctx->stream, la, ctx->d_limbs);
        else MXX_LAUNCH((slot_eval_lhs_kernel<uint32_t, 1, kLhsTile>), grid, dim3(threads), 0, ctx->stream, la, ctx->d_limbs);
        HIP_TRY(hipGetLastError());
    }

    const EvalTiles t = eval_tiles(call);
    EvalArgs a;
    a.table = tab, a.c_b0 = words_ptr(c_b0), a.lhs_b = lhs_b, a.v = v;
    a.m_g = call.m_g, a.w0 = call.w0, a.w1 = call.w1, a.out_cols = call.out_cols, a.dst_col = call.dst_col;
    a.entries = Sg * t.row_tiles * t.col_tiles;
    a.r = static_cast<uint32_t>(call.r), a.c = static_cast<uint32_t>(call.c), a.logN = ctx->logN;
    a.row_tiles = t.row_tiles, a.col_tiles = t.col_tiles;
    const size_t vecs = wpp / vn;
    size_t gy, gz;
    (void)fold_yz(a.entries, gy, gz);  // grid_plan.h; the count was held to 65535 x 65535 with the refusals (grid_fits)
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // [Pg_s; D_s; P1_s] read once per row tile, [c_b0 | LhsA_s | LhsB_s] once per column tile, the outputs' block written once
    const double inner = static_cast<double>(call.w0) + call.m_g + call.w1;
    MXX_TRACE_BYTES(static_cast<double>(Sg) * poly_bytes *
                    (static_cast<double>(t.row_tiles) * inner * call.c + static_cast<double>(t.col_tiles) * call.r * inner + static_cast<double>(call.r) * call.c));
    if (ctx->wide && vn > 1) return launch_main<uint64_t, 2>(ctx, a, t, grid, dim3(threads));
    if (ctx->wide) return launch_main<uint64_t, 1>(ctx, a, t, grid, dim3(threads));
    if (vn > 1) return launch_main<uint32_t, 4>(ctx, a, t, grid, dim3(threads));
    return launch_main<uint32_t, 1>(ctx, a, t, grid, dim3(threads));
}

// after the refusals: the outputs' tags, then (*go) whether anything is left to launch; PACKED24 operands unpacked once
int accept(const SlotEvalCall &call, GpuMatrix *const *outs, const GpuMatrix *c_b0, const GpuMatrix *const *gate_preimages,
           const GpuMatrix *const *b1_preimages, const GpuSlotTerm *terms, const GpuMatrix *digits, bool *go) {
    for (size_t s = 0; s < call.S; ++s) outs[s]->format = GPU_POLY_FORMAT_EVAL;
    *go = call.r != 0 && call.c != 0;
    if (!*go) return 0;
    if (ctx_activate(call.ctx)) return 1;
    words_ptr(c_b0);
    for (size_t s = 0; s < call.S; ++s) words_ptr(gate_preimages[s]), words_ptr(b1_preimages[s]), words_ptr(outs[s]);
    for (size_t t = 0; t < call.T; ++t) words_ptr(terms[t].c_in), words_ptr(terms[t].mid);
    if (digits) words_ptr(digits);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_slot_transfer_eval(GpuMatrix *const *outs, size_t nouts_S, size_t dst_col, const GpuMatrix *c_b0,
                                                 const GpuMatrix *const *gate_preimages, const GpuMatrix *const *b1_preimages,
                                                 const GpuSlotTerm *terms, const size_t *term_offsets, const uint64_t *mu_words,
                                                 size_t words_per_mu, size_t col_start, uint32_t base_bits, const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_slot_transfer_eval";
    const size_t S = nouts_S;
    if (S == 0) return 0;
    SlotEvalCall call;
    if (check_call(who, outs, S, dst_col, c_b0, gate_preimages, b1_preimages, terms, term_offsets, mu_words, words_per_mu, nullptr, true, col_start,
                   base_bits, tags, &call))
        return 1;
    GpuContext *ctx = call.ctx;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // an output's scratch: its digits m_g x c and its left factors r x (m_g + w1)
    const size_t v_bytes = call.m_g * call.c * poly_bytes, a_bytes = call.r * call.m_g * poly_bytes, b_bytes = call.r * call.w1 * poly_bytes;
    const size_t slot_bytes = std::max<size_t>(v_bytes + a_bytes + b_bytes, 1);
    const size_t per_group = rows_per_group(S, slot_bytes, call.cap);
    if (!grid_fits(call, per_group)) return set_error(std::string(who) + ": too many output tiles in one group");
    // ---- accepted ----
    bool go;
    if (accept(call, outs, c_b0, gate_preimages, b1_preimages, terms, nullptr, &go)) return 1;
    if (!go) return 0;
    CtxBlock digits(ctx), lhs_a(ctx), lhs_b(ctx);
    if (digits.alloc(per_group * v_bytes)) return 1;
    if (lhs_a.alloc(per_group * a_bytes)) return 1;
    if (lhs_b.alloc(per_group * b_bytes)) return 1;
    return for_row_groups(
        S, slot_bytes, tags,
        [&](size_t s0, size_t Sg, const GpuHashTags &part) {
            GpuMatrix v = scratch_matrix(ctx, call.level, call.m_g, Sg * call.c, digits.ptr);
            if (int rc = sample_decomposed_blocks_impl(who, true, &v, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Sg, base_bits, 0, call.m_g / call.k,
                                                       call.m_g, col_start))
                return rc;
            return combine_group(call, outs, c_b0, gate_preimages, b1_preimages, terms, term_offsets, mu_words, words_per_mu, s0, Sg, digits.ptr,
                                 lhs_a.ptr, lhs_b.ptr);
        },
        call.cap);
    ABI_GUARD_END
}

// The same with the digits [D_0 | D_1 | ...] given instead of sampled: the table copy, the pre-pass and the main kernel alone,
// one group.  A test instrument (tests/test_gpu_slot_transfer_eval.py reaches the lazy accumulator's bound with operands no
// sampler gives).
extern "C" int gpupoly_matrix_slot_transfer_eval_combine(GpuMatrix *const *outs, size_t nouts_S, size_t dst_col, const GpuMatrix *c_b0,
                                                         const GpuMatrix *const *gate_preimages, const GpuMatrix *const *b1_preimages,
                                                         const GpuSlotTerm *terms, const size_t *term_offsets, const uint64_t *mu_words,
                                                         size_t words_per_mu, size_t col_start, uint32_t base_bits, const GpuMatrix *digits) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_slot_transfer_eval_combine";
    const size_t S = nouts_S;
    if (S == 0) return 0;
    SlotEvalCall call;
    if (check_call(who, outs, S, dst_col, c_b0, gate_preimages, b1_preimages, terms, term_offsets, mu_words, words_per_mu, digits, false, col_start,
                   base_bits, nullptr, &call))
        return 1;
    if (!grid_fits(call, S)) return set_error(std::string(who) + ": too many output tiles in one group");
    bool go;
    if (accept(call, outs, c_b0, gate_preimages, b1_preimages, terms, digits, &go)) return 1;
    if (!go) return 0;
    GpuContext *ctx = call.ctx;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    CtxBlock lhs_a(ctx), lhs_b(ctx);
    if (lhs_a.alloc(S * call.r * call.m_g * poly_bytes)) return 1;
    if (lhs_b.alloc(S * call.r * call.w1 * poly_bytes)) return 1;
    return combine_group(call, outs, c_b0, gate_preimages, b1_preimages, terms, term_offsets, mu_words, words_per_mu, 0, S, words_ptr(digits), lhs_a.ptr,
                         lhs_b.ptr);
    ABI_GUARD_END
}
