// commit_lut.hip — the message blocks of T LUT rows of the commitment-based public lookup in one call:
// gpupoly_matrix_commit_lut_messages.
//
// The commit evaluator's message stream (build_msg_stream_for_lut_eval, src/lookup/commit_eval.rs:417-522) holds one d x m_b
// block per LUT row of every lookup gate, and the reference builds each on its own (:461-517):
//
//   R_t        = sample_hash(key, "R_<g>_<idx_t>", d, m_b)
//   canceler_t = (B_1 V_t + R_t) o iota_t,          iota_t = (idx_t + 1)^-1 mod q_l in limb l
//   msg_t      = [ A_out_g - G_d o y_t | 0 ] + R_t - P_g G^-1(canceler_t),          P_g = A_in,g + A_one,g
//
// with m_g = d k, m_b = d (k + 2), V_t the verifier slice the row names and y_t a constant polynomial.  Column (j, tw, e) of
// G_d o y_t is (y_t mod q_tw) B^e mod q_tw in every slot of limb tw of row j and zero elsewhere.  Per group of rows: the
// stacked block sample [R_0 | R_1 | ...], one elementwise kernel that forms every canceler word from B_1 V (one product per
// call, of B_1 as it is), the decomposition of the d x (Tg m_b) cancelers, and ONE register-tiled product whose left operand
// is chosen per row through the table - P_g read in place - and whose epilogue negates the reduced sum, adds R_t and, in the
// first m_g columns, A_out's word and the negated gadget constant where it hits, and stores every word once straight into
// its output.  The rows' pointers and constants go up in one staged copy per group; G is never filled, nothing of size
// d x m_b is built per row, and nothing is uploaded, launched or awaited per row.
#include "common.h"
#include "grid_plan.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

// the group's device table: [T] output pointers, [T] P_g pointers, [T] A_out pointers, [T] verifier slots,
// [T][L] iota_t mod q_l, [T][k] (y_t mod q_tw) B^e mod q_tw at tw dpt + e
struct CommitLutArgs {
    const void *r;       // d x (T m_b): [R_0 | R_1 | ...]
    const void *digits;  // m_g x (T m_b): row t at columns [t m_b, (t + 1) m_b)
    const uint64_t *table;
    size_t m_g, m_b, k, entries;
    uint32_t T, d, L, logN, dpt, row_tiles, col_tiles;
};

__device__ __forceinline__ const uint64_t *commit_iota(const CommitLutArgs &a) { return a.table + 4 * static_cast<size_t>(a.T); }
__device__ __forceinline__ const uint64_t *commit_gy(const CommitLutArgs &a) { return commit_iota(a) + static_cast<size_t>(a.T) * a.L; }

struct CancelerArgs {
    const void *bv;  // d x (nV m_b) = B_1 verifier
    const void *r;   // d x (T m_b)
    void *c;         // d x (T m_b)
    const uint64_t *table;
    size_t m_b, nV, entries;
    uint32_t T, d, L, logN;
};

// C[i, t m_b + j] = (BV[i, vslot_t m_b + j] + R[i, t m_b + j]) o iota_t for the block's polynomial (i, t, j), VN words per
// lane: every word read and written once, 16 bytes at a time (VN divides N: one limb per vector)
template <typename W, int VN>
__global__ void __launch_bounds__(256) commit_canceler_kernel(CancelerArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const size_t per_row = static_cast<size_t>(a.T) * a.m_b;
    const size_t i = entry / per_row, rest = entry - i * per_row;
    const size_t t = rest / a.m_b, j = rest - t * a.m_b;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN;
    const size_t vslot = a.table[3 * static_cast<size_t>(a.T) + t];
    const uint64_t *iota = a.table + 4 * static_cast<size_t>(a.T) + t * a.L;
    const W *bv = static_cast<const W *>(a.bv) + (i * a.nV * a.m_b + vslot * a.m_b + j) * wpp;
    const W *r = static_cast<const W *>(a.r) + entry * wpp;
    W *c = static_cast<W *>(a.c) + entry * wpp;
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.logN);
        const LimbConst lc = limbs[l];
        const W q = static_cast<W>(lc.q), f = static_cast<W>(iota[l]);
        W bw[VN], rw[VN], ow[VN];
        *reinterpret_cast<V *>(bw) = *reinterpret_cast<const V *>(bv + w0);
        *reinterpret_cast<V *>(rw) = *reinterpret_cast<const V *>(r + w0);
#pragma unroll
        for (int x = 0; x < VN; ++x) ow[x] = lazy_reduce<W>(static_cast<D>(add_mod<W>(bw[x], rw[x], q)) * f, lc);
        *reinterpret_cast<V *>(c + w0) = *reinterpret_cast<const V *>(ow);
    }
}

// A block's tile: rows [r0, r0 + TR) x columns [c0, c0 + TC) of row t's d x m_b block (blockIdx.y/z), blockIdx.x strides the
// polynomial's L N words VN per lane.  A lane keeps the TR words of P_g of a term in registers for all TC columns; every
// word of the digits is loaded by one tile only where TR covers d (d <= 4).  Rows and columns past the end repeat the last
// one and are never stored.  The TR x TC x VN sums share one count of pending terms - LazyAcc's rule (row_targets.h) with
// the count kept once; they start at 0, a residue, and fold every lazy_terms terms, so a modulus that leaves room for
// fewer terms is reduced in every window.  Epilogue: q - sum (0 stays 0) + R_t's word, and in columns below m_g + A_out's
// word and - gy where (row, limb) is the column's (j, tw); one store per word into outs[t].
template <typename W, int VN, int TR, int TC>
__global__ void __launch_bounds__(256) commit_lut_combine_kernel(CommitLutArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const uint32_t per_row = a.row_tiles * a.col_tiles;
    const size_t t = entry / per_row;
    const uint32_t rest = static_cast<uint32_t>(entry - t * per_row);
    const uint32_t rt = rest / a.col_tiles, ct = rest - rt * a.col_tiles;
    const uint32_t r0 = rt * TR, c0 = ct * TC;
    const size_t wpp = static_cast<size_t>(a.L) << a.logN;
    const size_t T = a.T, tc = T * a.m_b;  // columns of the group's scratch matrices
    W *out = reinterpret_cast<W *>(a.table[t]);
    const W *lhs = reinterpret_cast<const W *>(a.table[T + t]);
    const W *aout = reinterpret_cast<const W *>(a.table[2 * T + t]);
    const uint64_t *gy = commit_gy(a) + t * a.k;
    size_t row[TR], cc[TC];
#pragma unroll
    for (int i = 0; i < TR; ++i) row[i] = min(r0 + i, a.d - 1);
#pragma unroll
    for (int j = 0; j < TC; ++j) cc[j] = c0 + j < a.m_b ? c0 + j : a.m_b - 1;
    const size_t d_stride = tc * wpp;  // words from one digit row to the next
    for (size_t w0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; w0 < wpp;
         w0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        const uint32_t l = static_cast<uint32_t>(w0 >> a.logN);
        const LimbConst lc = limbs[l];
        const W q = static_cast<W>(lc.q);
        const uint32_t lazy = lc.lazy_terms;
        uint32_t pending = 0;
        D acc[TR][TC][VN];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j)
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[i][j][x] = 0;
        const W *ap[TR], *bp[TC];
#pragma unroll
        for (int i = 0; i < TR; ++i) ap[i] = lhs + row[i] * a.m_g * wpp + w0;
#pragma unroll
        for (int j = 0; j < TC; ++j) bp[j] = static_cast<const W *>(a.digits) + (t * a.m_b + cc[j]) * wpp + w0;
        for (size_t rho = 0; rho < a.m_g; ++rho) {
            W av[TR][VN], bv[TC][VN];
#pragma unroll
            for (int i = 0; i < TR; ++i) *reinterpret_cast<V *>(av[i]) = *reinterpret_cast<const V *>(ap[i] + rho * wpp);
#pragma unroll
            for (int j = 0; j < TC; ++j) *reinterpret_cast<V *>(bv[j]) = *reinterpret_cast<const V *>(bp[j] + rho * d_stride);
            if (pending >= lazy) {
#pragma unroll
                for (int i = 0; i < TR; ++i)
#pragma unroll
                    for (int j = 0; j < TC; ++j)
#pragma unroll
                        for (int x = 0; x < VN; ++x) acc[i][j][x] = lazy_reduce<W>(acc[i][j][x], lc);
                pending = 0;
            }
#pragma unroll
            for (int i = 0; i < TR; ++i)
#pragma unroll
                for (int j = 0; j < TC; ++j)
#pragma unroll
                    for (int x = 0; x < VN; ++x) acc[i][j][x] += static_cast<D>(av[i][x]) * bv[j][x];
            ++pending;
        }
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            if (r0 + i >= a.d) continue;
            const size_t ri = r0 + i;
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                if (c0 + j >= a.m_b) continue;
                const size_t col = c0 + j;
                W rv[VN], o[VN];
                *reinterpret_cast<V *>(rv) = *reinterpret_cast<const V *>(static_cast<const W *>(a.r) + (ri * tc + t * a.m_b + col) * wpp + w0);
#pragma unroll
                for (int x = 0; x < VN; ++x) {
                    const W p = lazy_reduce<W>(acc[i][j][x], lc);
                    o[x] = add_mod<W>(rv[x], p ? q - p : 0, q);
                }
                if (col < a.m_g) {
                    W ov[VN];
                    *reinterpret_cast<V *>(ov) = *reinterpret_cast<const V *>(aout + (ri * a.m_g + col) * wpp + w0);
                    const size_t jb = col / a.k;
                    const uint32_t kk = static_cast<uint32_t>(col - jb * a.k);
                    // the negated constant q - gy <= q: adding q leaves a residue as it is
                    const bool hit = ri == jb && l == kk / a.dpt;
                    const W g = hit ? static_cast<W>(q - static_cast<W>(gy[kk])) : 0;
#pragma unroll
                    for (int x = 0; x < VN; ++x) o[x] = add_mod<W>(add_mod<W>(o[x], ov[x], q), g, q);
                }
                *reinterpret_cast<V *>(out + (ri * a.m_b + col) * wpp + w0) = *reinterpret_cast<const V *>(o);
            }
        }
    }
}

// what one accepted call works with: T rows of d x m_b outputs over ngates gates
struct CommitLutCall : RowCall {
    size_t T, d, m_g, m_b, nV;
    size_t cap;  // a group's digit scratch
};

uint64_t inverse_mod(uint64_t v, uint64_t q) {  // q prime, v in [1, q)
    u128_t r = 1, b = v;
    for (uint64_t e = q - 2; e; e >>= 1) {
        if (e & 1) r = r * b % q;
        b = b * b % q;
    }
    return static_cast<uint64_t>(r);
}

// Everything both entries refuse, for every row, before anything is launched.  `full`: the sampling entry, whose b_1,
// verifier, vslot, idx and tags are checked; otherwise the combine entry with [R_0 | ...] and the digits given.
int check_call(const char *who, GpuMatrix *const *outs, size_t T, const GpuMatrix *b_1, const GpuMatrix *verifier, const uint64_t *vslot,
               const GpuMatrix *r_stacked, const GpuMatrix *digits, const GpuMatrix *const *pubkey_sums, const GpuMatrix *const *a_outs,
               size_t ngates, const uint32_t *gate_of_row, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *idx,
               const GpuHashTags *tags, bool full, CommitLutCall *call) {
    const Refuse refuse{who};
    auto gate_at = [](size_t g) { return " (gate " + std::to_string(g) + ")"; };
    if (!outs || !pubkey_sums || !a_outs || !gate_of_row || !y_words || (full && (!vslot || !idx))) return refuse("null array");
    if (full ? (!b_1 || !verifier) : (!r_stacked || !digits)) return refuse("null operand");
    if (full && !tags) return refuse("null tags");
    if (ngates == 0) return refuse("no gates");
    if (int rc = refuse_null_outputs(refuse, outs, T, null_row)) return rc;
    for (size_t g = 0; g < ngates; ++g)
        if (!pubkey_sums[g] || !a_outs[g]) return refuse("null operand" + gate_at(g));
    if (words_per_y == 0) return refuse("words_per_y = 0");
    if (int rc = refuse_base_level(refuse, a_outs[0], base_bits, full, call)) return rc;
    const size_t d = a_outs[0]->rows, k = call->k;
    if (d > 0xffffffffull / (k + 2)) return refuse("matrix too large");
    const size_t m_g = d * k, m_b = d * (k + 2);
    if (m_b && T > (~size_t(0) >> 1) / m_b) return refuse("matrix too large");
    for (size_t g = 0; g < ngates; ++g) {
        const std::string at = gate_at(g);
        for (const GpuMatrix *m : {pubkey_sums[g], a_outs[g]}) {
            if (int rc = refuse_foreign(refuse, m, *call, at)) return rc;
            if (m->rows != d || m->cols != m_g) return refuse("shape mismatch: pubkey_sums[g] and a_outs[g] are d x (d * digits per tower * limbs)" + at);
            if (m->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + at);
        }
    }
    for (size_t t = 0; t < T; ++t)
        if (gate_of_row[t] >= ngates) return refuse("gate_of_row past the gates" + row_at(t));
    size_t nV = 0;
    if (full) {
        if (int rc = refuse_operand(refuse, b_1, *call, d, m_b, "shape mismatch: b_1 is d x m_b, m_b = d * (digits per tower * limbs + 2)")) return rc;
        if (int rc = refuse_foreign(refuse, verifier, *call)) return rc;
        if (verifier->rows != m_b || m_b == 0 || verifier->cols == 0 || verifier->cols % m_b != 0)
            return refuse("shape mismatch: verifier is m_b x (a positive multiple of m_b)");
        if (verifier->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
        nV = verifier->cols / m_b;
        for (size_t t = 0; t < T; ++t)
            if (vslot[t] >= nV) return refuse("vslot past the verifier's blocks" + row_at(t));
        for (size_t t = 0; t < T; ++t)
            for (uint32_t l = 0; l < call->L; ++l) {
                const uint64_t q = call->ctx->moduli[l];
                if ((idx[t] % q + 1) % q == 0) return refuse("idx + 1 has no inverse mod q_" + std::to_string(l) + row_at(t));
            }
    } else {
        if (int rc = refuse_operand(refuse, r_stacked, *call, d, T * m_b, "shape mismatch: r_stacked is d x (rows * m_b)")) return rc;
        if (int rc = refuse_operand(refuse, digits, *call, m_g, T * m_b, "shape mismatch: the digits are m_g x (rows * m_b)")) return rc;
    }
    if (T > 0xffffffffull) return refuse("matrix too large");
    if (int rc = refuse_outputs(refuse, outs, T, *call, row_at, [&](const GpuMatrix *out) -> const char * {
            return out->rows != d || out->cols != m_b ? "shape mismatch: an output is d x m_b, m_b = d * (digits per tower * limbs + 2)" : nullptr;
        }))
        return rc;
    call->T = T, call->d = d, call->m_g = m_g, call->m_b = m_b, call->nV = nV;
    call->cap = call->ctx->env.commit_lut_budget ? call->ctx->env.commit_lut_budget : kRowGroupBytes;
    // an output is written while every operand is still being read, and by no other row
    const GpuMatrix *operands[2] = {full ? b_1 : r_stacked, full ? verifier : digits};
    static const char *const full_names[2] = {"b_1", "the verifier"};
    static const char *const given_names[2] = {"r_stacked", "the digits"};
    if (int rc = refuse_tags_overlap(refuse, full ? tags : nullptr, T, outs, T, operands, full ? full_names : given_names, 2)) return rc;
    std::vector<const GpuMatrix *> per_gate;
    per_gate.insert(per_gate.end(), pubkey_sums, pubkey_sums + ngates);
    per_gate.insert(per_gate.end(), a_outs, a_outs + ngates);
    const std::string overlap = slot_operands_overlap(outs, T, {}, per_gate.data(), per_gate.size());
    if (!overlap.empty()) return refuse("overlap: an output overlaps a gate's operand");
    return 0;
}

// the row tile and the column tile of a call (m_b >= 3 wherever d >= 1), and the tiles per row
struct CommitLutTiles {
    int tr, tc;
    uint32_t row_tiles, col_tiles;
};
CommitLutTiles combine_tiles(const CommitLutCall &call) {
    CommitLutTiles t;
    t.tr = call.d >= 3 ? 4 : call.d == 2 ? 2 : 1;
    t.tc = t.tr == 4 ? 2 : 4;
    t.row_tiles = static_cast<uint32_t>((call.d + t.tr - 1) / t.tr);
    t.col_tiles = static_cast<uint32_t>((call.m_b + t.tc - 1) / t.tc);
    return t;
}
bool grid_fits(const CommitLutCall &call, size_t Tg) {
    const CommitLutTiles t = combine_tiles(call);
    size_t gy, gz;
    return fold_yz(Tg * t.row_tiles * t.col_tiles, gy, gz) && fold_yz(Tg * call.d * call.m_b, gy, gz);
}

// the grid of a kernel whose blockIdx.y/z is one of `entries` polynomials (or tiles) and whose blockIdx.x strides the words
void words_grid(const GpuContext *ctx, uint32_t L, size_t entries, dim3 *grid, dim3 *block) {
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    const size_t vecs = (static_cast<size_t>(L) << ctx->logN) / vn;
    size_t gy = 1, gz = 1;
    (void)fold_yz(entries, gy, gz);  // grid_plan.h; the counts were held to its range with the refusals (grid_fits)
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    *grid = dim3(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    *block = dim3(threads);
}

template <typename W, int VN>
int launch_combine_tiles(GpuContext *ctx, const CommitLutArgs &a, const CommitLutTiles &t, dim3 grid, dim3 block) {
#define MXX_COMMIT_LUT_TILE(R, Cc) \
    if (t.tr == R && t.tc == Cc) MXX_LAUNCH((commit_lut_combine_kernel<W, VN, R, Cc>), grid, block, 0, ctx->stream, a, ctx->d_limbs)
    MXX_COMMIT_LUT_TILE(1, 4);
    MXX_COMMIT_LUT_TILE(2, 4);
    MXX_COMMIT_LUT_TILE(4, 2);
#undef MXX_COMMIT_LUT_TILE
    HIP_TRY(hipGetLastError());
    return 0;
}

// the table of rows [t0, t0 + Tg) in one staged copy
int upload_rows(const CommitLutCall &call, CtxBlock &block, GpuMatrix *const *outs, const uint64_t *vslot, const GpuMatrix *const *pubkey_sums,
                const GpuMatrix *const *a_outs, const uint32_t *gate_of_row, const uint64_t *y_words, size_t words_per_y, const uint64_t *idx,
                size_t t0, size_t Tg) {
    GpuContext *ctx = call.ctx;
    const size_t L = call.L, dpt = call.dpt, k = call.k;
    static thread_local std::vector<uint64_t> staging, bpow;
    staging.assign(4 * Tg + Tg * L + Tg * k, 0);
    bpow.resize(k);  // B^e mod q_l at l dpt + e, once for the group's rows
    for (size_t l = 0; l < L; ++l) base_powers(ctx->moduli[l], call.base_bits, dpt, bpow.data() + l * dpt);
    uint64_t *iota = staging.data() + 4 * Tg, *gy = iota + Tg * L;
    for (size_t t = 0; t < Tg; ++t) {
        const size_t g = gate_of_row[t0 + t];
        staging[t] = reinterpret_cast<uint64_t>(words_ptr(outs[t0 + t]));
        staging[Tg + t] = reinterpret_cast<uint64_t>(words_ptr(pubkey_sums[g]));
        staging[2 * Tg + t] = reinterpret_cast<uint64_t>(words_ptr(a_outs[g]));
        if (vslot) staging[3 * Tg + t] = vslot[t0 + t];
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = ctx->moduli[l];
            if (idx) iota[t * L + l] = inverse_mod((idx[t0 + t] % q + 1) % q, q);
            const u128_t yv = words_mod(y_words + (t0 + t) * words_per_y, words_per_y, q);
            for (size_t e = l * dpt; e < (l + 1) * dpt; ++e) gy[t * k + e] = static_cast<uint64_t>(yv * bpow[e] % q);
        }
    }
    return upload_table(block, "commit LUT row table (host to device)", staging);
}

// rows [t0, t0 + Tg) with [R_0 | ...] at `r` (d x (Tg m_b) words) and their digits at `digits` (m_g x (Tg m_b) words),
// the table already on the device: the combine kernel
int combine_group(const CommitLutCall &call, const uint64_t *table, size_t Tg, const void *r, const void *digits) {
    GpuContext *ctx = call.ctx;
    const CommitLutTiles t = combine_tiles(call);
    CommitLutArgs a;
    a.r = r, a.digits = digits, a.table = table;
    a.m_g = call.m_g, a.m_b = call.m_b, a.k = call.k;
    a.entries = Tg * t.row_tiles * t.col_tiles;
    a.T = static_cast<uint32_t>(Tg), a.d = static_cast<uint32_t>(call.d), a.L = call.L, a.logN = ctx->logN, a.dpt = call.dpt;
    a.row_tiles = t.row_tiles, a.col_tiles = t.col_tiles;
    dim3 grid, block;
    words_grid(ctx, call.L, a.entries, &grid, &block);
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    const double poly_bytes = static_cast<double>(static_cast<size_t>(call.L) << ctx->logN) * ctx->word_bytes;
    // the digits read once per row tile, P_g once per column tile, R_t and A_out's block read once, the outputs written once
    MXX_TRACE_BYTES(static_cast<double>(Tg) * poly_bytes *
                    (static_cast<double>(t.row_tiles) * call.m_g * call.m_b + static_cast<double>(t.col_tiles) * call.d * call.m_g +
                     2.0 * call.d * call.m_b + static_cast<double>(call.d) * call.m_g));
    static const std::string name = "commit_lut_combine_kernel (per-row P_g x digits, register tile; negation, R_t, A_out and gadget constant in the epilogue)";
    ctx->last_kernel = name.c_str();
    if (ctx->wide && vn > 1) return launch_combine_tiles<uint64_t, 2>(ctx, a, t, grid, block);
    if (ctx->wide) return launch_combine_tiles<uint64_t, 1>(ctx, a, t, grid, block);
    if (vn > 1) return launch_combine_tiles<uint32_t, 4>(ctx, a, t, grid, block);
    return launch_combine_tiles<uint32_t, 1>(ctx, a, t, grid, block);
}

// C = (BV[:, vslot block] + R) o iota for the group's rows, elementwise
int canceler_group(const CommitLutCall &call, const uint64_t *table, size_t Tg, const void *bv, const void *r, void *c) {
    GpuContext *ctx = call.ctx;
    CancelerArgs a;
    a.bv = bv, a.r = r, a.c = c, a.table = table;
    a.m_b = call.m_b, a.nV = call.nV, a.entries = call.d * Tg * call.m_b;
    a.T = static_cast<uint32_t>(Tg), a.d = static_cast<uint32_t>(call.d), a.L = call.L, a.logN = ctx->logN;
    dim3 grid, block;
    words_grid(ctx, call.L, a.entries, &grid, &block);
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    MXX_TRACE_BYTES(3.0 * static_cast<double>(a.entries) * (static_cast<size_t>(call.L) << ctx->logN) * ctx->word_bytes);
    if (ctx->wide && vn > 1) MXX_LAUNCH((commit_canceler_kernel<uint64_t, 2>), grid, block, 0, ctx->stream, a, ctx->d_limbs);
    else if (ctx->wide) MXX_LAUNCH((commit_canceler_kernel<uint64_t, 1>), grid, block, 0, ctx->stream, a, ctx->d_limbs);
    else if (vn > 1) MXX_LAUNCH((commit_canceler_kernel<uint32_t, 4>), grid, block, 0, ctx->stream, a, ctx->d_limbs);
    else MXX_LAUNCH((commit_canceler_kernel<uint32_t, 1>), grid, block, 0, ctx->stream, a, ctx->d_limbs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// after the refusals: the outputs' tags, then (*go) whether anything is left to launch; PACKED24 operands unpacked once
int accept(const CommitLutCall &call, GpuMatrix *const *outs, const GpuMatrix *const *pubkey_sums, const GpuMatrix *const *a_outs, size_t ngates,
           std::initializer_list<const GpuMatrix *> fixed, bool *go) {
    for (size_t t = 0; t < call.T; ++t) outs[t]->format = GPU_POLY_FORMAT_EVAL;
    *go = call.d != 0;
    if (!*go) return 0;
    if (ctx_activate(call.ctx)) return 1;
    for (size_t t = 0; t < call.T; ++t) words_ptr(outs[t]);
    for (size_t g = 0; g < ngates; ++g) words_ptr(pubkey_sums[g]), words_ptr(a_outs[g]);
    for (const GpuMatrix *m : fixed) words_ptr(m);
    return 0;
}

}  // namespace

extern "C" int gpupoly_matrix_commit_lut_messages(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *b_1, const GpuMatrix *verifier,
                                                  const uint64_t *vslot, const GpuMatrix *const *pubkey_sums, const GpuMatrix *const *a_outs,
                                                  size_t ngates, const uint32_t *gate_of_row, uint32_t base_bits, const uint64_t *y_words,
                                                  size_t words_per_y, const uint64_t *idx, const GpuHashTags *tags) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_commit_lut_messages";
    const size_t T = nrows_T;
    if (T == 0) return 0;
    CommitLutCall call;
    if (check_call(who, outs, T, b_1, verifier, vslot, nullptr, nullptr, pubkey_sums, a_outs, ngates, gate_of_row, base_bits, y_words, words_per_y,
                   idx, tags, true, &call))
        return 1;
    GpuContext *ctx = call.ctx;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // a row's digit scratch is m_g x m_b; its R_t and its canceler are d x m_b each
    const size_t block_bytes = call.d * call.m_b * poly_bytes;
    const size_t row_bytes = std::max<size_t>(call.m_g * call.m_b * poly_bytes, 1);
    const size_t per_group = rows_per_group(T, row_bytes, call.cap);
    if (!grid_fits(call, per_group)) return set_error(std::string(who) + ": too many output tiles in one group");
    // ---- accepted ----
    bool go;
    if (accept(call, outs, pubkey_sums, a_outs, ngates, {b_1, verifier}, &go)) return 1;
    if (!go) return 0;
    CtxBlock bv(ctx), r(ctx), c(ctx), digits(ctx);
    if (bv.alloc(call.d * call.nV * call.m_b * poly_bytes) || r.alloc(per_group * block_bytes) || c.alloc(per_group * block_bytes) ||
        digits.alloc(per_group * row_bytes))
        return 1;
    // every B_1 V_t at once: one product of b_1, as it is, against the verifier
    GpuMatrix bvm = scratch_matrix(ctx, call.level, call.d, call.nV * call.m_b, bv.ptr);
    if (int rc = launch_matmul(&bvm, b_1, verifier)) return rc;
    std::vector<size_t> seg_cols;
    return for_row_groups(
        T, row_bytes, tags,
        [&](size_t t0, size_t Tg, const GpuHashTags &part) {
            CtxBlock table(ctx);
            if (upload_rows(call, table, outs, vslot, pubkey_sums, a_outs, gate_of_row, y_words, words_per_y, idx, t0, Tg)) return 1;
            GpuMatrix rm = scratch_matrix(ctx, call.level, call.d, Tg * call.m_b, r.ptr);
            seg_cols.assign(Tg, call.m_b);
            if (int rc = sample_blocks_impl(who, true, &rm, GPU_MATRIX_DIST_UNIFORM, nullptr, &part, Tg, GPUPOLY_BLOCKS_COLUMNS, seg_cols.data(), nullptr))
                return rc;
            const uint64_t *d_table = static_cast<const uint64_t *>(table.ptr);
            if (int rc = canceler_group(call, d_table, Tg, bv.ptr, r.ptr, c.ptr)) return rc;
            GpuMatrix cm = scratch_matrix(ctx, call.level, call.d, Tg * call.m_b, c.ptr);
            GpuMatrix dm = scratch_matrix(ctx, call.level, call.m_g, Tg * call.m_b, digits.ptr);
            if (int rc = gpu_matrix_decompose_base(&cm, base_bits, &dm)) return rc;
            return combine_group(call, d_table, Tg, r.ptr, digits.ptr);
        },
        call.cap);
    ABI_GUARD_END
}

// The same with [R_0 | R_1 | ...] and the digits given instead of sampled, multiplied and decomposed: the table copy and the
// combine kernel alone, one group.  A test instrument (tests/test_gpu_commit_lut.py reaches the lazy accumulator's bound with
// operands no sampler gives).
extern "C" int gpupoly_matrix_commit_lut_messages_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *r_stacked,
                                                          const GpuMatrix *digits, const GpuMatrix *const *pubkey_sums,
                                                          const GpuMatrix *const *a_outs, size_t ngates, const uint32_t *gate_of_row,
                                                          uint32_t base_bits, const uint64_t *y_words, size_t words_per_y) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_commit_lut_messages_combine";
    const size_t T = nrows_T;
    if (T == 0) return 0;
    CommitLutCall call;
    if (check_call(who, outs, T, nullptr, nullptr, nullptr, r_stacked, digits, pubkey_sums, a_outs, ngates, gate_of_row, base_bits, y_words,
                   words_per_y, nullptr, nullptr, false, &call))
        return 1;
    if (!grid_fits(call, T)) return set_error(std::string(who) + ": too many output tiles in one group");
    bool go;
    if (accept(call, outs, pubkey_sums, a_outs, ngates, {r_stacked, digits}, &go)) return 1;
    if (!go) return 0;
    CtxBlock table(call.ctx);
    if (upload_rows(call, table, outs, nullptr, pubkey_sums, a_outs, gate_of_row, y_words, words_per_y, nullptr, 0, T)) return 1;
    return combine_group(call, static_cast<const uint64_t *>(table.ptr), T, words_ptr(r_stacked), words_ptr(digits));
    ABI_GUARD_END
}
