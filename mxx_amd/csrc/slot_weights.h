// slot_weights.h — host side of gpupoly_matrix_slot_transfer_eval (slot_transfer_eval.hip): the two weights of a term in every
// limb.  A term's input vector is multiplied by the scalar kappa and its stage-1 product by kappa * mu, mu the constant
// coefficient of the source plaintext: a big integer given as little-endian 64-bit words (gpupoly_matrix_load_coeff_words's
// rule), reduced mod every q_l.  Plain C++ (no HIP types), so that it is tested as a stand-alone host program.
#pragma once

#include <cstddef>
#include <cstdint>

namespace slot_eval {

typedef unsigned __int128 u128;

// the integer of `count` little-endian words mod q, 0 < q < 2^62
inline uint64_t words_mod(const uint64_t *words, size_t count, uint64_t q) {
    u128 r = 0;
    for (size_t i = count; i-- > 0;) r = ((r << 64) | words[i]) % q;  // r < q: the shifted value stays below 2^126
    return static_cast<uint64_t>(r);
}

// out[2 l] = kappa mod q_l, out[2 l + 1] = kappa * mu mod q_l for l < L
inline void term_weights(uint64_t kappa, const uint64_t *mu_words, size_t words_per_mu, const uint64_t *moduli, size_t L, uint64_t *out) {
    for (size_t l = 0; l < L; ++l) {
        const uint64_t q = moduli[l];
        const uint64_t k = kappa % q;
        out[2 * l] = k;
        out[2 * l + 1] = static_cast<uint64_t>(static_cast<u128>(k) * words_mod(mu_words, words_per_mu, q) % q);
    }
}

}  // namespace slot_eval
