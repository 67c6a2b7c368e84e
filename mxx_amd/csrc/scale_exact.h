// scale_exact.h — the pieces of the exact scale-and-round that its two users share: scale_round.hip
// (one t for the whole matrix) and crt_recompose.hip (t = the limb a level is decoded for).
//
// Device side: arithmetic mod the auxiliary prime m = 2^64 - 59, the word reduction by floor(2^64 / q) and the residue
// load of one coefficient.  Host side: the small multi-word helpers that build the per-call constants.
#pragma once

#include "common.h"

#include <vector>

constexpr uint64_t kAuxM = 0xFFFFFFFFFFFFFFC5ull;  // 2^64 - 59, prime; 2^64 = 59 (mod m)

#if defined(__HIPCC__)
#include "modarith.h"

// x mod m for x < 2^128: x = hi 2^64 + lo = 59 hi + lo (mod m), twice
__device__ __forceinline__ uint64_t aux_reduce(u128_t x) {
    const u128_t y = static_cast<u128_t>(static_cast<uint64_t>(x >> 64)) * 59u + static_cast<uint64_t>(x);  // < 2^70
    const uint64_t lo = static_cast<uint64_t>(y), hi = static_cast<uint64_t>(y >> 64);                       // hi < 64
    uint64_t r = lo + hi * 59u;
    if (r < lo) r += 59u;  // wrapped past 2^64: r < 3776 here
    return r >= kAuxM ? r - kAuxM : r;
}
__device__ __forceinline__ uint64_t aux_mul(uint64_t a, uint64_t b) { return aux_reduce(static_cast<u128_t>(a) * b); }
__device__ __forceinline__ uint64_t aux_add(uint64_t a, uint64_t b) {  // a, b < m
    const uint64_t r = a + b;
    return (r < a || r >= kAuxM) ? r - kAuxM : r;
}
__device__ __forceinline__ uint64_t aux_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + (kAuxM - b); }

// v < 2^64 -> v mod q with floor(2^64 / q): the quotient estimate is at most one short
__device__ __forceinline__ uint64_t reduce_word(uint64_t v, uint64_t q, uint64_t mu64) {
    uint64_t r = v - __umul64hi(v, mu64) * q;
    return r >= q ? r - q : r;
}

template <typename W, int ML>
__device__ __forceinline__ void load_residues(const W *src, size_t poly, uint32_t i, uint32_t N, int L, uint64_t *res) {
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) res[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    } else {
        for (int k = 0; k < L; ++k) res[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    }
}
#endif  // __HIPCC__

// ---- host ----------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 u128h;

inline uint64_t h_mulmod64(uint64_t a, uint64_t b, uint64_t m) { return static_cast<uint64_t>(static_cast<u128h>(a) * b % m); }

inline uint64_t h_powmod64(uint64_t b, uint64_t e, uint64_t m) {
    uint64_t r = 1 % m;
    for (b %= m; e; e >>= 1, b = h_mulmod64(b, b, m))
        if (e & 1) r = h_mulmod64(r, b, m);
    return r;
}

// little-endian words of q_0 .. q_{L-1}
inline std::vector<uint64_t> h_product_words(const std::vector<uint64_t> &moduli, int L) {
    std::vector<uint64_t> Q(1, 1);
    for (int l = 0; l < L; ++l) {
        u128h carry = 0;
        for (size_t w = 0; w < Q.size(); ++w) {
            const u128h p = static_cast<u128h>(Q[w]) * moduli[l] + carry;
            Q[w] = static_cast<uint64_t>(p);
            carry = p >> 64;
        }
        if (carry) Q.push_back(static_cast<uint64_t>(carry));
    }
    return Q;
}

// floor(x / 2)
inline std::vector<uint64_t> h_half_words(const std::vector<uint64_t> &x) {
    std::vector<uint64_t> half(x.size(), 0);
    for (size_t w = 0; w < x.size(); ++w) half[w] = (x[w] >> 1) | (w + 1 < x.size() ? x[w + 1] << 63 : 0);
    return half;
}

inline uint64_t h_words_mod(const std::vector<uint64_t> &x, uint64_t m) {
    u128h r = 0;
    for (size_t w = x.size(); w-- > 0;) r = ((r << 64) | x[w]) % m;
    return static_cast<uint64_t>(r);
}
