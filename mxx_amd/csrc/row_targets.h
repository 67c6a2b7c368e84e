// row_targets.h — the scaffold of the target builders (lut_targets.hip, lwe_targets.hip, wee25_targets.hip): many preimage
// targets in one call.  Host side: what an accepted call works with, the refusals every entry makes (each file's check_call
// keeps its own order, shape sentences and position suffix), the rows of a call in groups under one scratch cap with
// their tags cut per group, one staged table per group, the outputs' overlap rule and the one launcher of a combine
// kernel.  Device side: what the two combine kernels share - the output polynomial of a block and the lazy accumulator.  A
// builder adds its formula: its operands' checks, its table's rows and its kernel's terms.  The online lookups
// (ggh15_lookup.hip, lwe_lookup.hip) stand on the same host scaffold with slots for rows, and share the rule for operands
// that every slot brings of its own.  Every kernel of the three
// files compiles to the bytes it had before it was written on top of this (profiles/row_targets_refactor.txt), and some
// pieces have the form they have for that reason; each says so.
#pragma once

#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// ---- host: an accepted call and its refusals ------------------------------------------------------
// what every accepted call works with; k = dpt L gadget columns per source row
struct RowCall {
    const char *who;
    GpuContext *ctx;
    int level;
    uint32_t L, dpt, base_bits;
    size_t k;
};

// a call over the column chunk [col_start, col_start + c) of d x m operands, m = d k: the outputs are d x c
struct ChunkCall : RowCall {
    size_t d, m, c, col_start;
};

struct Refuse {
    const char *who;
    int operator()(const std::string &what) const { return set_error(std::string(who) + ": " + what); }
};

// where row t's output stands, for a message, and the whole message for a null one
inline std::string row_at(size_t t) { return " (row " + std::to_string(t) + ")"; }
inline std::string null_row(size_t t) { return "null output (row " + std::to_string(t) + ")"; }

// `null_at(j)`: the message for a null outs[j]
template <typename Text>
int refuse_null_outputs(const Refuse &refuse, GpuMatrix *const *outs, size_t count, Text null_at) {
    for (size_t j = 0; j < count; ++j)
        if (!outs[j]) return refuse(null_at(j));
    return 0;
}

// base_bits, the level of `first` - the operand whose context and level the call takes - and, for an entry that samples,
// the reference's keying, which has no block form; fills the base of `call`
inline int refuse_base_level(const Refuse &refuse, const GpuMatrix *first, uint32_t base_bits, bool samples, RowCall *call) {
    if (base_bits == 0 || base_bits >= 63) return refuse("base_bits must be in 1..62");
    GpuContext *ctx = first->ctx;
    if (first->level < 0 || first->level >= ctx->limb_count) return refuse("level out of range");
    if (ctx->env.rng_compat && samples) return refuse("unsupported under MXX_HIP_RNG_COMPAT=reference");
    const uint32_t L = static_cast<uint32_t>(first->level) + 1, dpt = (ctx->crt_bits + base_bits - 1) / base_bits;
    *call = RowCall{refuse.who, ctx, first->level, L, dpt, base_bits, static_cast<size_t>(dpt) * L};
    return 0;
}

inline int refuse_foreign(const Refuse &refuse, const GpuMatrix *mat, const RowCall &call, const std::string &at = std::string()) {
    if (mat->ctx != call.ctx) return refuse("context mismatch" + at);
    if (mat->level != call.level) return refuse("level mismatch" + at);
    return 0;
}

// `shape`: the caller's "shape mismatch: ..." sentence for what rows x cols are
inline int refuse_form(const Refuse &refuse, const GpuMatrix *mat, size_t rows, size_t cols, const char *shape) {
    if (mat->rows != rows || mat->cols != cols) return refuse(shape);
    if (mat->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format");
    return 0;
}

inline int refuse_operand(const Refuse &refuse, const GpuMatrix *mat, const RowCall &call, size_t rows, size_t cols, const char *shape) {
    if (int rc = refuse_foreign(refuse, mat, call)) return rc;
    return refuse_form(refuse, mat, rows, cols, shape);
}

// every output's context and level, then `shape(out)`: what is wrong with its size, or null
template <typename At, typename Shape>
int refuse_outputs(const Refuse &refuse, GpuMatrix *const *outs, size_t count, const RowCall &call, At at, Shape shape) {
    for (size_t j = 0; j < count; ++j) {
        const std::string where = at(j);
        if (int rc = refuse_foreign(refuse, outs[j], call, where)) return rc;
        if (const char *what = shape(outs[j])) return refuse(what + where);
    }
    return 0;
}

// the chunk within the operands' columns, the sizes within the kernels' 32-bit fields, T outputs of d x c
inline int refuse_chunk_outputs(const Refuse &refuse, GpuMatrix *const *outs, size_t T, const ChunkCall &call) {
    if (call.col_start > call.m || call.c > call.m - call.col_start) return refuse("column chunk past the operands' columns");
    if (call.d > 0xffffffffull || call.c > 0xffffffffull || T > 0xffffffffull) return refuse("matrix too large");
    return refuse_outputs(refuse, outs, T, call, row_at, [&](const GpuMatrix *out) -> const char * {
        if (out->cols != call.c) return "the outputs differ in width";
        return out->rows != call.d ? "shape mismatch: an output is d x chunk columns" : nullptr;
    });
}

// An output is written while every operand is still being read, and by no other row: no overlap with an operand or with
// another output.  The outputs' blocks are sorted by address, so T rows cost T log T comparisons.  Returns what to refuse
// with ("" when nothing overlaps); `names[j]` says what operand j is called in the message
inline std::string row_outputs_overlap(GpuMatrix *const *outs, size_t T, const GpuMatrix *const *operands, const char *const *names, size_t noperands) {
    std::vector<std::pair<const char *, const char *>> blocks;
    std::vector<const GpuMatrix *> seen(outs, outs + T);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return "overlap: an output is given twice";
    for (size_t t = 0; t < T; ++t) {
        const GpuMatrix *out = outs[t];
        for (size_t j = 0; j < noperands; ++j)
            if (storage_overlaps(out, operands[j])) return std::string("overlap: an output overlaps ") + names[j] + row_at(t);
        if (out->storage && out->bytes) {
            const char *s = static_cast<const char *>(out->storage);
            const size_t held = out->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24 ? packed24_bytes(out) : out->bytes;
            blocks.emplace_back(s, s + held);
        }
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t j = 1; j < blocks.size(); ++j)
        if (blocks[j].first < blocks[j - 1].second) return "overlap: an output overlaps another output";
    return "";
}

// the last refusals of every entry: the T tags (null: an entry that does not sample), then the overlap rule
inline int refuse_tags_overlap(const Refuse &refuse, const GpuHashTags *tags, size_t T, GpuMatrix *const *outs, size_t count,
                               const GpuMatrix *const *operands, const char *const *names, size_t noperands) {
    size_t tag_bytes = 0;
    if (tags && hash_tags_check(refuse.who, tags, T, &tag_bytes)) return 1;
    const std::string overlap = row_outputs_overlap(outs, count, operands, names, noperands);
    return overlap.empty() ? 0 : refuse(overlap);
}

// ---- the lookups (ggh15_lookup.hip, lwe_lookup.hip): S slots, each with operands of its own ------------------------
inline std::string slot_at(size_t s) { return " (slot " + std::to_string(s) + ")"; }

inline size_t held_bytes(const GpuMatrix *m) {
    return m->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24 ? packed24_bytes(m) : m->bytes;
}

// an output overlaps one of the per-slot operands (`kinds`: arrays of S matrices; the same matrix may stand for several
// slots): the operands' blocks sorted by start with the furthest end so far, one search per output.  `more`: `nmore` further
// operands that do not come one per slot (slot_transfer_eval.hip's terms)
inline std::string slot_operands_overlap(GpuMatrix *const *outs, size_t S, std::initializer_list<const GpuMatrix *const *> kinds,
                                         const GpuMatrix *const *more = nullptr, size_t nmore = 0) {
    std::vector<std::pair<const char *, const char *>> blocks;
    std::vector<const GpuMatrix *> given;
    auto give = [&](const GpuMatrix *m) {
        given.push_back(m);
        if (m->storage && m->bytes) blocks.emplace_back(static_cast<const char *>(m->storage), static_cast<const char *>(m->storage) + held_bytes(m));
    };
    for (size_t s = 0; s < S; ++s)
        for (const GpuMatrix *const *kind : kinds) give(kind[s]);
    for (size_t j = 0; j < nmore; ++j) give(more[j]);
    std::sort(given.begin(), given.end());
    std::sort(blocks.begin(), blocks.end());
    for (size_t j = 1; j < blocks.size(); ++j) blocks[j].second = std::max(blocks[j].second, blocks[j - 1].second);
    for (size_t t = 0; t < S; ++t) {
        const GpuMatrix *out = outs[t];
        if (std::binary_search(given.begin(), given.end(), out)) return "overlap: an output overlaps a slot's operand" + slot_at(t);
        if (!out->storage || !out->bytes) continue;
        const char *lo = static_cast<const char *>(out->storage), *hi = lo + held_bytes(out);
        // the blocks that start below the output's end: the furthest of their ends reaches past its start
        const auto it = std::lower_bound(blocks.begin(), blocks.end(), std::make_pair(hi, static_cast<const char *>(nullptr)));
        if (it != blocks.begin() && (it - 1)->second > lo) return "overlap: an output overlaps a slot's operand" + slot_at(t);
    }
    return "";
}

// ---- host: groups of rows, their scratch and their table ------------------------------------------
constexpr size_t kRowGroupBytes = size_t(1) << 30;  // cap on a group's scratch [V_0 | ...] (preimage.hip's rule for p2)

// rows per group: the scratch of row_bytes per row stays under the cap (one row at least), within the block sampler's 2^20
inline size_t rows_per_group(size_t T, size_t row_bytes, size_t cap = kRowGroupBytes) {
    return std::min<size_t>(std::min<size_t>(T, size_t(1) << 20), std::max<size_t>(1, cap / row_bytes));
}

// a borrowed rows x cols EVAL matrix over `words` (scratch of one call: never swapped for packed storage)
inline GpuMatrix scratch_matrix(GpuContext *ctx, int level, size_t rows, size_t cols, void *words) {
    GpuMatrix m;
    m.ctx = ctx;
    m.level = level;
    m.rows = rows;
    m.cols = cols;
    m.format = GPU_POLY_FORMAT_EVAL;
    m.bytes = rows * cols * (static_cast<size_t>(level) + 1) * static_cast<size_t>(ctx->N) * static_cast<size_t>(ctx->word_bytes);
    m.storage = words;
    m.borrowed = true;
    return m;
}

// the tags of rows [t0, t0 + Tg): `offsets` backs the TABLE form's cut and must outlive the returned value's use
inline GpuHashTags hash_tags_rows(const GpuHashTags *tags, size_t t0, size_t Tg, std::vector<size_t> &offsets) {
    GpuHashTags part = *tags;
    if (tags->form == GPUPOLY_TAGS_TABLE) {
        offsets.resize(Tg + 1);
        for (size_t j = 0; j <= Tg; ++j) offsets[j] = tags->tag_offsets[t0 + j] - tags->tag_offsets[t0];
        part.tag_offsets = offsets.data();
        if (tags->tags) part.tags = tags->tags + tags->tag_offsets[t0];
    } else {
        part.first_index = tags->first_index + t0;
    }
    return part;
}

// body(t0, Tg, the tags of rows [t0, t0 + Tg)) for every group of rows_per_group(T, row_bytes, cap) rows, until one fails
template <typename Body>
int for_row_groups(size_t T, size_t row_bytes, const GpuHashTags *tags, Body &&body, size_t cap = kRowGroupBytes) {
    const size_t per_group = rows_per_group(T, row_bytes, cap);
    std::vector<size_t> offsets;
    for (size_t t0 = 0; t0 < T; t0 += per_group) {
        const size_t Tg = std::min(per_group, T - t0);
        if (int rc = body(t0, Tg, hash_tags_rows(tags, t0, Tg, offsets))) return rc;
    }
    return 0;
}

// a group's table: `staging` goes up in one traced copy to the start of `block`, allocated here with `extra_words` more
// 8-byte words behind it.  The caller's arrays were read into `staging`; they are not read after the call returns
inline int upload_table(CtxBlock &block, const char *label, const std::vector<uint64_t> &staging, size_t extra_words = 0) {
    const size_t bytes = sizeof(uint64_t) * staging.size();
    if (block.alloc(bytes + sizeof(uint64_t) * extra_words)) return 1;
    hipStream_t stream = block.ctx->stream;
    MXX_TRACED_COPY(label, stream, bytes, HIP_TRY(hipMemcpyAsync(block.ptr, staging.data(), bytes, hipMemcpyHostToDevice, stream)));
    return 0;
}

// ---- the combine kernels: one block column per output polynomial --------------------------------
// what both kernels know of a launch: Tg rows of d x c outputs over the chunk.  It is the LAST member of their argument
// structs, not a base of them: a base's fields would come first and move every other argument's offset in the segment
struct CombineShape {
    size_t m, col_start, k, entries;
    uint32_t T, d, c, L, dpt, logN;
};
inline CombineShape combine_shape(const ChunkCall &call, size_t Tg) {
    return {call.m, call.col_start, call.k, Tg * call.d * call.c, static_cast<uint32_t>(Tg), static_cast<uint32_t>(call.d),
            static_cast<uint32_t>(call.c), call.L, call.dpt, call.ctx->logN};
}

template <typename W_, int VN_, int DPT_>
struct CombineCfg {
    typedef W_ W;
    static constexpr int VN = VN_, DPT = DPT_;
};

// launch(CombineCfg<W, VN, DPT>(), grid, block) enqueues kernel<W, VN, DPT>: blockIdx.y/z = the output polynomial,
// blockIdx.x strides its L N words VN per lane - 16 bytes, or one word where a limb vector is narrower - and DPT is the
// digit count up to 4, else 0.  `bytes`: what the launch moves, for the trace.  The four (W, VN) pairs stand in the order
// in which the kernels' instances are to be emitted: another order moves every kernel's code within the object file
template <typename F>
int launch_combine(const char *who, GpuContext *ctx, double bytes, size_t entries, uint32_t L, uint32_t logN, uint32_t dpt, F &&launch) {
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    const size_t wpp = static_cast<size_t>(L) << logN, vecs = wpp / vn;
    size_t gy, gz;
    if (!fold_yz(entries, gy, gz)) return set_error(std::string(who) + ": too many target polynomials in one group");
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    MXX_TRACE_BYTES(bytes);
    auto digits = [&](auto w, auto lanes) {
        typedef decltype(w) W;
        constexpr int VN = decltype(lanes)::value;
        switch (dpt) {
            case 1: launch(CombineCfg<W, VN, 1>(), grid, dim3(threads)); break;
            case 2: launch(CombineCfg<W, VN, 2>(), grid, dim3(threads)); break;
            case 3: launch(CombineCfg<W, VN, 3>(), grid, dim3(threads)); break;
            case 4: launch(CombineCfg<W, VN, 4>(), grid, dim3(threads)); break;
            default: launch(CombineCfg<W, VN, 0>(), grid, dim3(threads)); break;
        }
    };
    if (ctx->wide && vn > 1) digits(uint64_t(), std::integral_constant<int, 2>());
    else if (ctx->wide) digits(uint64_t(), std::integral_constant<int, 1>());
    else if (vn > 1) digits(uint32_t(), std::integral_constant<int, 4>());
    else digits(uint32_t(), std::integral_constant<int, 1>());
    HIP_TRY(hipGetLastError());
    return 0;
}

// Inside `launch`: MXX_LAUNCH of kernel<W, VN, DPT> for `cfg` with the rest of MXX_LAUNCH's arguments.  The trace records
// the launch under MXX_LAUNCH's argument as written, and a trace tells the digit-count instances apart by it, so the
// digit count stands there as a literal: "(kernel<W, VN, 2>)"
#define MXX_COMBINE_ONE(kernel, D, ...) \
    if constexpr (decltype(cfg)::DPT == D) MXX_LAUNCH((kernel<W, VN, D>), __VA_ARGS__)
#define MXX_LAUNCH_COMBINE(kernel, cfg, ...)          \
    do {                                              \
        typedef typename decltype(cfg)::W W;          \
        constexpr int VN = decltype(cfg)::VN;         \
        MXX_COMBINE_ONE(kernel, 1, __VA_ARGS__);      \
        MXX_COMBINE_ONE(kernel, 2, __VA_ARGS__);      \
        MXX_COMBINE_ONE(kernel, 3, __VA_ARGS__);      \
        MXX_COMBINE_ONE(kernel, 4, __VA_ARGS__);      \
        MXX_COMBINE_ONE(kernel, 0, __VA_ARGS__);      \
    } while (0)

// VN words of type W as one 16-byte vector (VN == 1: the word itself)
template <typename W, int VN>
struct CombineVec {
    typedef typename std::conditional<VN == 1, W, typename std::conditional<sizeof(W) == 4, uint4, ulonglong2>::type>::type V;
    static_assert(sizeof(V) == sizeof(W) * VN, "vector width");
};

// the output polynomial of a block: entry (i, cc) of row t, chunk column cc = global column col = (jb, tw, .); wpp words per
// polynomial; column pc of the tc columns that the group's scratch matrices hold
struct CombineEntry {
    size_t t, i, cc, col, jb, wpp, tc, pc;
    uint32_t tw;
};
// `entry`: the block's, static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y, below the shape's count.  `dpt`: the
// kernel's DPT, or the shape's where that is 0.  The kernel takes both: with the early return or the choice of dpt in
// here, some instances compile to other code (DPT 1 with the choice; 64-bit words with the return).  So does the kernels'
// loop over a lane's words once its start and its step are functions, and it stays written out in both
__device__ __forceinline__ CombineEntry combine_entry(const CombineShape &s, size_t entry, uint32_t dpt) {
    CombineEntry e;
    const size_t per_row = static_cast<size_t>(s.d) * s.c;
    e.t = entry / per_row;
    const size_t rest = entry - e.t * per_row;
    e.i = rest / s.c;
    e.cc = rest - e.i * s.c;
    e.col = s.col_start + e.cc;
    e.jb = e.col / s.k;
    e.tw = static_cast<uint32_t>(e.col - e.jb * s.k) / dpt;
    e.wpp = static_cast<size_t>(s.L) << s.logN;
    e.tc = static_cast<size_t>(s.T) * s.c;
    e.pc = e.t * s.c + e.cc;
    return e;
}

// One output word's sum: a residue (the first word, or a folded sum) and then terms of at most (q - 1)^2 each, in 64 bits
// for 32-bit words and 128 bits for 64-bit words, folded back into [0, q) every `lazy` = LimbConst::lazy_terms terms - the
// bound that figure is computed for - and once at the end
template <typename W>
struct LazyAcc {
    typedef typename Wide<W>::type D;
    D acc;
    uint32_t pending = 0;
    const uint32_t lazy;
    const LimbConst &lc;
    __device__ __forceinline__ LazyAcc(W first, uint32_t lazy_terms, const LimbConst &limb) : acc(first), lazy(lazy_terms), lc(limb) {}
    __device__ __forceinline__ void fold() {
        acc = lazy_reduce<W>(acc, lc);
        pending = 0;
    }
    __device__ __forceinline__ void add(D term) {
        if (pending >= lazy) fold();
        acc += term;
        ++pending;
    }
    __device__ __forceinline__ W result() {
        fold();
        return static_cast<W>(acc);
    }
};
