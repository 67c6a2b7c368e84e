// centred.h — one coefficient's centred representative from its limb residues, in registers.  Shared by the compact
// store (serde.hip) and the centred infinity norm (norm.hip).
//
// x is the representative of the coefficient in (-Q/2, Q/2], Q = q_0 .. q_level (odd): reconstruct_centered returns |x| as
// little-endian words and its sign, with two O(L) fast paths for small |x| ahead of the general Garner path;
// reconstruct_small holds only the fast paths and reports whether they applied.
#pragma once

#include "common.h"
#include "crt.h"
#include "modarith.h"

static constexpr int kMaxWords = 64;  // up to 4096-bit Q

struct SerdeConsts {
    int limbs;
    int words;                    // 64-bit words per reconstructed coefficient
    uint64_t q[GPUPOLY_MAX_LIMBS];
    uint64_t modulus[kMaxWords];  // Q, little-endian words
    uint64_t half[kMaxWords];     // floor(Q/2)
};

// residues of coefficient (poly, i) -> |x| words (little-endian), sign; returns bit width of |x|.
// ML bounds the limb count at compile time (8, 16 or 64) so that the mixed-radix digits and the words of x stay in
// registers for the sizes that matter (the unbounded form kept two 64-entry arrays in scratch memory).
// Fast path: the matrices that are serialised most - preimages, trapdoors, Gaussian-sized keys - hold SMALL integers:
// if every limb's residue is the residue of the centred limb-0 value c (|c| <= q_0 / 2), then x = c, by uniqueness of
// the CRT representative in (-Q/2, Q/2]; that is an O(L) comparison instead of the O(L^2) Garner recurrence.
// General path: Garner's products go through Barrett (mu of every limb from the context) instead of a 128-bit `%`.
template <typename W, int ML>
__device__ __forceinline__ uint32_t reconstruct_centered(const W *__restrict__ src, size_t poly, uint32_t i, uint32_t N,
                                                         const SerdeConsts &sc, const uint64_t *__restrict__ garner,
                                                         size_t garner_stride, const LimbConst *__restrict__ limbs,
                                                         uint64_t *x, bool &negative) {
    const int L = sc.limbs, WC = sc.words;
    uint64_t res[ML];
    if constexpr (ML <= 16) {
#pragma unroll
        for (int k = 0; k < ML; ++k)
            if (k < L) res[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    } else {
        for (int k = 0; k < L; ++k) res[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    }
    {
        const uint64_t q0 = sc.q[0];
        const bool neg0 = res[0] > (q0 >> 1);
        const uint64_t mag = neg0 ? q0 - res[0] : res[0];  // |c|
        bool small = true;
        auto same = [&](int k) {
            const uint64_t qk = sc.q[k];
            return mag < qk && res[k] == (neg0 ? qk - mag : mag);
        };
        if constexpr (ML <= 16) {
#pragma unroll
            for (int k = 1; k < ML; ++k)
                if (k < L) small = small && same(k);
        } else {
            for (int k = 1; k < L; ++k) small = small && same(k);
        }
        if (small) {
            for (int w = 0; w < WC; ++w) x[w] = 0;
            x[0] = mag;
            negative = neg0 && mag != 0;
            return mag ? 64u - static_cast<uint32_t>(__clzll(mag)) : 0u;
        }
    }
    // Second fast path: |x| < q_0 q_1 / 2 - a preimage's entries (perturbations of width ~2^27 against 24-bit limbs) overflow
    // limb 0 alone but not two limbs.  The candidate is the centred two-limb CRT value c2 (one Garner step, one double-width
    // word); if every further limb holds c2's residue then x = c2, again by uniqueness of the representative in
    // (-Q/2, Q/2] (|c2| <= q_0 q_1 / 2 < Q / 2 from three limbs on; with two limbs c2 IS the general result).  O(L) instead
    // of the O(L^2) recurrence below: the width and pack passes over an M3A preimage went from 3.4 + 2.0 ms to the
    // time of reading the matrix (bench.py, compact_bytes).
    if (L >= 2) {
        typedef typename Wide<W>::type D;
        const uint64_t q0 = sc.q[0], q1 = sc.q[1];
        const uint64_t r0m = res[0] >= q1 ? res[0] % q1 : res[0];
        const uint64_t dd = res[1] >= r0m ? res[1] - r0m : res[1] + q1 - r0m;
        const uint64_t v1 = static_cast<uint64_t>(barrett_reduce(static_cast<D>(dd) * static_cast<D>(garner[garner_stride]), static_cast<W>(q1), limbs[1].mu, limbs[1].kbits));
        const D q01 = static_cast<D>(q0) * q1;
        const D val = static_cast<D>(res[0]) + static_cast<D>(v1) * q0;  // in [0, q_0 q_1)
        const bool neg2 = val > (q01 >> 1);
        const D mag2 = neg2 ? q01 - val : val;
        bool ok = true;
        auto same2 = [&](int k) {
            const uint64_t qk = sc.q[k];
            const uint32_t kb = limbs[k].kbits;
            const bool fits = 2 * kb >= 8 * sizeof(D) || (mag2 >> (2 * kb)) == 0;  // Barrett's range: mag2 < 2^(2 bits(q_k))
            const uint64_t r = static_cast<uint64_t>(barrett_reduce(mag2, static_cast<W>(qk), limbs[k].mu, kb));
            return fits && res[k] == ((neg2 && r) ? qk - r : r);
        };
        if constexpr (ML <= 16) {
#pragma unroll
            for (int k = 2; k < ML; ++k)
                if (k < L) ok = ok && same2(k);
        } else {
            for (int k = 2; k < L; ++k) ok = ok && same2(k);
        }
        if (ok) {
            for (int w = 0; w < WC; ++w) x[w] = 0;
            x[0] = static_cast<uint64_t>(mag2);
            uint64_t hi = 0;
            if constexpr (sizeof(D) > 8) hi = static_cast<uint64_t>(mag2 >> 64);
            if (WC > 1) x[1] = hi;
            negative = neg2 && mag2 != 0;
            if (hi) return 128u - static_cast<uint32_t>(__clzll(hi));
            return x[0] ? 64u - static_cast<uint32_t>(__clzll(x[0])) : 0u;
        }
    }
    uint64_t v[ML];
    crt_garner_digits<W, ML>(res, v, L, sc.q, garner, garner_stride, limbs);
    crt_horner_words<ML>(v, L, sc.q, WC, x);
    // centre: negative iff x > floor(Q/2)
    int cmp = 0;
    for (int w = WC - 1; w >= 0; --w) {
        if (x[w] != sc.half[w]) {
            cmp = x[w] > sc.half[w] ? 1 : -1;
            break;
        }
    }
    negative = cmp > 0;
    if (negative) {
        uint64_t borrow = 0;
        for (int w = 0; w < WC; ++w) {
            const uint64_t a = sc.modulus[w], b = x[w];
            const uint64_t d = a - b - borrow;
            borrow = (a < b + borrow) || (b + borrow < b) ? 1 : 0;
            x[w] = d;
        }
    }
    for (int w = WC - 1; w >= 0; --w)
        if (x[w]) return static_cast<uint32_t>(w) * 64u + (64u - static_cast<uint32_t>(__clzll(x[w])));
    return 0;
}

// ---- fast-path-only forms ----------------------------------------------------------------------------------------------
// The matrices that get serialised (preimages, trapdoors, Gaussian-sized keys) never leave the two fast paths of
// reconstruct_centered, but kernels that also carry the general Garner path pay for it in registers (102 / 73 VGPRs, the
// word array indexed dynamically in scratch): 0.45 + 0.66 ms for an M3A preimage against 0.09 ms of reading it.  These
// forms hold ONLY the fast paths - a coefficient is |x| < q_0 / 2 or |x| < q_0 q_1 / 2, checked against every further
// limb - and raise a flag for anything else; the host then reruns the general kernels (never, for the matrices above).
template <typename W, int ML>
__device__ __forceinline__ bool reconstruct_small(const W *__restrict__ src, size_t poly, uint32_t i, uint32_t N,
                                                  const SerdeConsts &sc, const uint64_t *__restrict__ garner,
                                                  size_t garner_stride, const LimbConst *__restrict__ limbs,
                                                  uint64_t &mag_lo, uint64_t &mag_hi, bool &negative) {
    static_assert(ML <= 16, "fast forms are unrolled over the limbs");
    typedef typename Wide<W>::type D;
    const int L = sc.limbs;
    uint64_t res[ML];
#pragma unroll
    for (int k = 0; k < ML; ++k)
        if (k < L) res[k] = static_cast<uint64_t>(src[(poly * L + k) * N + i]);
    const uint64_t q0 = sc.q[0];
    {
        const bool neg0 = res[0] > (q0 >> 1);
        const uint64_t mag = neg0 ? q0 - res[0] : res[0];
        bool small = true;
#pragma unroll
        for (int k = 1; k < ML; ++k)
            if (k < L) {
                const uint64_t qk = sc.q[k];
                small = small && mag < qk && res[k] == (neg0 ? qk - mag : mag);
            }
        if (small) {
            mag_lo = mag;
            mag_hi = 0;
            negative = neg0 && mag != 0;
            return true;
        }
    }
    if (L < 2) return false;
    const uint64_t q1 = sc.q[1];
    const uint64_t r0m = res[0] >= q1 ? res[0] % q1 : res[0];
    const uint64_t dd = res[1] >= r0m ? res[1] - r0m : res[1] + q1 - r0m;
    const uint64_t v1 = static_cast<uint64_t>(barrett_reduce(static_cast<D>(dd) * static_cast<D>(garner[garner_stride]), static_cast<W>(q1), limbs[1].mu, limbs[1].kbits));
    const D q01 = static_cast<D>(q0) * q1;
    const D val = static_cast<D>(res[0]) + static_cast<D>(v1) * q0;
    const bool neg2 = val > (q01 >> 1);
    const D mag2 = neg2 ? q01 - val : val;
    bool ok = true;
#pragma unroll
    for (int k = 2; k < ML; ++k)
        if (k < L) {
            const uint64_t qk = sc.q[k];
            const uint32_t kb = limbs[k].kbits;
            const bool fits = 2 * kb >= 8 * sizeof(D) || (mag2 >> (2 * kb)) == 0;
            const uint64_t r = static_cast<uint64_t>(barrett_reduce(mag2, static_cast<W>(qk), limbs[k].mu, kb));
            ok = ok && fits && res[k] == ((neg2 && r) ? qk - r : r);
        }
    mag_lo = static_cast<uint64_t>(mag2);
    mag_hi = 0;
    if constexpr (sizeof(D) > 8) mag_hi = static_cast<uint64_t>(mag2 >> 64);
    negative = neg2 && mag2 != 0;
    return ok;
}

static int build_consts(const GpuMatrix *mat, SerdeConsts &sc) {
    const GpuContext *ctx = mat->ctx;
    const int L = mat->level + 1;
    sc.limbs = L;
    // Q = product of the active moduli, little-endian 64-bit words
    std::vector<uint64_t> Q(1, 1);
    for (int l = 0; l < L; ++l) {
        sc.q[l] = ctx->moduli[l];
        unsigned __int128 carry = 0;
        for (size_t w = 0; w < Q.size(); ++w) {
            unsigned __int128 p = static_cast<unsigned __int128>(Q[w]) * ctx->moduli[l] + carry;
            Q[w] = static_cast<uint64_t>(p);
            carry = p >> 64;
        }
        if (carry) Q.push_back(static_cast<uint64_t>(carry));
    }
    if (Q.size() > static_cast<size_t>(kMaxWords)) return set_error("compact bytes: modulus exceeds 4096 bits");
    sc.words = static_cast<int>(Q.size());
    for (int w = 0; w < kMaxWords; ++w) {
        sc.modulus[w] = w < sc.words ? Q[w] : 0;
    }
    for (int w = 0; w < kMaxWords; ++w) {
        const uint64_t lo = sc.modulus[w] >> 1;
        const uint64_t hi = (w + 1 < kMaxWords) ? (sc.modulus[w + 1] & 1ull) << 63 : 0;
        sc.half[w] = lo | hi;
    }
    return 0;
}
