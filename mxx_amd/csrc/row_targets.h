// row_targets.h — what the per-row target builders share on the host (lut_targets.hip, lwe_targets.hip): the rows of a call
// go in groups under one scratch cap, their constants are reduced from little-endian words, their tags are cut per group
// and their outputs obey one overlap rule.
#pragma once

#include "common.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

constexpr size_t kRowGroupBytes = size_t(1) << 30;  // cap on a group's digit scratch [V_0 | ...] (preimage.hip's rule for p2)

// rows per group: the digit scratch of row_bytes per row stays under the cap (one row at least), within the block sampler's 2^20
inline size_t rows_per_group(size_t T, size_t row_bytes) {
    return std::min<size_t>(std::min<size_t>(T, size_t(1) << 20), std::max<size_t>(1, kRowGroupBytes / row_bytes));
}

// C mod q for the little-endian words of C (gpupoly_matrix_load_coeff_words's rule)
inline uint64_t words_mod(const uint64_t *words, size_t count, uint64_t q) {
    unsigned __int128 r = 0;
    for (size_t i = count; i-- > 0;) r = ((r << 64) | words[i]) % q;  // r < q < 2^62
    return static_cast<uint64_t>(r);
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
            if (storage_overlaps(out, operands[j])) return std::string("overlap: an output overlaps ") + names[j] + " (row " + std::to_string(t) + ")";
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

// VN words of type W as one 16-byte vector (VN == 1: the word itself)
template <typename W, int VN>
struct CombineVec {
    typedef typename std::conditional<VN == 1, W, typename std::conditional<sizeof(W) == 4, uint4, ulonglong2>::type>::type V;
    static_assert(sizeof(V) == sizeof(W) * VN, "vector width");
};
