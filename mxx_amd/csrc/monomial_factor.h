// monomial_factor.h — the EVAL-form factor of a monomial, shared by monomial.hip and slot_transfer_eval.hip: slot k of limb l
// holds a(psi_l^(2 bitrev(k) + 1)), so the product by x^s is the point-wise product by psi_l^(s (2 bitrev(k) + 1) mod 2N), which the
// forward twiddle table holds (d_tw_fwd[l][bitrev(i)] = psi_l^i).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t bitrev_n(uint32_t x, uint32_t logN) { return logN ? __brev(x) >> (32u - logN) : 0u; }

// psi^(s * odd) of one limb, odd = 2 bitrev(slot) + 1: the table entry, negated in the upper half of the exponents (psi^N = -1;
// a power of psi is never 0)
template <typename W>
__device__ __forceinline__ W monomial_factor(const W *__restrict__ tw, uint32_t s, uint32_t odd, uint32_t N, uint32_t logN, W q) {
    const uint32_t e = (s * odd) & (2u * N - 1u);  // wraps mod 2^32, a multiple of 2N
    const W f = tw[bitrev_n(e & (N - 1u), logN)];
    return (e & N) ? static_cast<W>(q - f) : f;
}
