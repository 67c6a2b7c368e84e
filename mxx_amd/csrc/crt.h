// crt.h — Garner mixed-radix CRT of one coefficient, in registers.  Shared by the compact store (serde.hip) and the exact
// scale-and-round / coefficient-word store (scale_round.hip).
//
// ML bounds the limb count at compile time (8, 16 or 64).  Up to 16 limbs every loop is unrolled and guarded by the
// runtime count, so that the digit and word arrays stay in registers; the 64-limb form keeps plain loops (its arrays live
// in scratch memory).
#pragma once

#include "common.h"
#include "modarith.h"

// Garner: digits v_k of x = v_0 + v_1 q_0 + v_2 q_0 q_1 + ... (v_k < q_k) from its residues r_k = x mod q_k, k < L,
// v_k = (r_k - (v_0 + v_1 q_0 + ...)) / (q_0 .. q_{k-1}) mod q_k computed incrementally.  `res` and `v` may be the same
// array.  garner[k * garner_stride + j] = q_j^-1 mod q_k (j < k); limbs[k] carries q_k's Barrett constants.  The products
// go through Barrett instead of a 128-bit `%`.
template <typename W, int ML>
__device__ __forceinline__ void crt_garner_digits(const uint64_t *res, uint64_t *v, int L, const uint64_t *q,
                                                  const uint64_t *__restrict__ garner, size_t garner_stride,
                                                  const LimbConst *__restrict__ limbs) {
    auto garner_step = [&](int k, int j, uint64_t t, uint64_t qk, uint64_t mu, uint32_t kb) {
        uint64_t vj = v[j];
        if (vj >= qk) vj %= qk;  // only when an earlier modulus is wider than this one
        const uint64_t d = t >= vj ? t - vj : t + qk - vj;
        const uint64_t g = garner[k * garner_stride + j];
        if constexpr (sizeof(W) == 4) return static_cast<uint64_t>(barrett_reduce(d * g, static_cast<uint32_t>(qk), mu, kb));
        else return barrett_reduce(static_cast<u128_t>(d) * g, qk, mu, kb);
    };
    if constexpr (ML <= 16) {  // fully unrolled, guarded: everything stays in registers
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) {
                const uint64_t qk = q[k], mu = limbs[k].mu;
                const uint32_t kb = limbs[k].kbits;
                uint64_t t = res[k];
#pragma unroll
                for (int j = 0; j < ML; ++j)
                    if (j < k) t = garner_step(k, j, t, qk, mu, kb);
                v[k] = t;
            }
    } else {
        for (int k = 0; k < L; ++k) {
            const uint64_t qk = q[k], mu = limbs[k].mu;
            const uint32_t kb = limbs[k].kbits;
            uint64_t t = res[k];
            for (int j = 0; j < k; ++j) t = garner_step(k, j, t, qk, mu, kb);
            v[k] = t;
        }
    }
}

// Horner over the digits: x = (..(v_{L-1} q_{L-2} + v_{L-2}) q_{L-3} + ..) q_0 + v_0 as WC little-endian 64-bit words
// (WC >= the words of q_0 .. q_{L-1}; every word below WC is written).
template <int ML>
__device__ __forceinline__ void crt_horner_words(const uint64_t *v, int L, const uint64_t *q, int WC, uint64_t *x) {
    for (int w = 0; w < WC; ++w) x[w] = 0;
    auto horner_step = [&](int k) {
        const uint64_t m = q[k];
        u128_t carry = v[k];
        for (int w = 0; w < WC; ++w) {
            const u128_t p = static_cast<u128_t>(x[w]) * m + carry;
            x[w] = static_cast<uint64_t>(p);
            carry = p >> 64;
        }
    };
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = ML - 1; k >= 0; --k) {
            if (k == L - 1) x[0] = v[k];
            else if (k < L - 1) horner_step(k);
        }
    } else {
        x[0] = v[L - 1];
        for (int k = L - 2; k >= 0; --k) horner_step(k);
    }
}
