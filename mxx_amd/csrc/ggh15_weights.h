// ggh15_weights.h — host side of gpupoly_matrix_ggh15_lookup (ggh15_lookup.hip): the weights of the gy term.  Column
// (j, tw, e) of G_d times the constant y has one non-zero residue, (y mod q_tw) B^e mod q_tw, B = 2^base_bits, whose digits are
// constants - their own transform - so the term is sum_{e' < dpt} weight[l][e'] * mid_gy[:, (j, tw, e')] in every limb l, with
// weight[l][e'] = digit e' of that residue, cut at bits(q_tw) as the decomposition cuts it, reduced mod q_l (a digit of a
// wide tower can exceed a narrow modulus).  Plain C++ (no HIP types), so that it is tested as a stand-alone host program.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ggh15 {

typedef unsigned __int128 u128;

inline uint32_t bit_length(uint64_t q) {
    uint32_t bits = 0;
    for (; q; q >>= 1) ++bits;
    return bits;
}

// out[l * dpt + e'] for l < L, e' < dpt; v = y mod q_tw (below q_tw), 0 < base_bits < 63, q_tw < 2^62
inline void gy_weights(uint64_t v, uint64_t q_tw, uint32_t base_bits, uint32_t dpt, uint32_t e, const uint64_t *moduli, size_t L, uint64_t *out) {
    const uint64_t B = (1ull << base_bits) % q_tw;
    for (uint32_t i = 0; i < e; ++i) v = static_cast<uint64_t>(static_cast<u128>(v) * B % q_tw);
    const uint32_t src_bits = bit_length(q_tw);
    for (uint32_t ep = 0; ep < dpt; ++ep) {
        const uint64_t shift = static_cast<uint64_t>(ep) * base_bits;
        uint64_t digit = 0;
        if (shift < src_bits) {  // src_bits <= 62: the shift is defined
            const uint32_t left = src_bits - static_cast<uint32_t>(shift);
            const uint32_t db = base_bits < left ? base_bits : left;
            digit = (v >> shift) & ((1ull << db) - 1);
        }
        for (size_t l = 0; l < L; ++l) out[l * dpt + ep] = digit % moduli[l];
    }
}

}  // namespace ggh15
