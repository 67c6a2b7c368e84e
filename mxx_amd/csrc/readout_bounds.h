// readout_bounds.h — host side of the bit / small-integer read-out (readout.hip): a bound B in [0, Q] given as
// little-endian 64-bit words -> its mixed-radix digits over the basis q_0 .. q_{L-1},
//   B = d_0 + d_1 q_0 + d_2 q_0 q_1 + ..  (d_k < q_k),   d_k = B / (q_0 .. q_{k-1}) mod q_k,
// the form in which the kernels compare a coefficient's Garner digits with it (top digit first), and the range checks
// of the entries.  Plain C++ (no HIP types), so that it is tested as a stand-alone host program.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace readout {

constexpr int kMaxLimbs = 64;

typedef unsigned __int128 u128;

struct BoundDigits {
    uint64_t d[kMaxLimbs];  // digits of B; all zero when B = Q
    int is_q;               // B = Q: every coefficient lies below it ("no upper bound")
};

// little-endian words without their high zero words (0 -> no words)
inline std::vector<uint64_t> trimmed(const uint64_t *w, size_t n) {
    while (n > 0 && w[n - 1] == 0) --n;
    return std::vector<uint64_t>(w, w + n);
}

// q_0 .. q_{L-1} as little-endian words
inline std::vector<uint64_t> product_words(const uint64_t *q, int L) {
    std::vector<uint64_t> Q(1, 1);
    for (int l = 0; l < L; ++l) {
        u128 carry = 0;
        for (size_t w = 0; w < Q.size(); ++w) {
            const u128 p = static_cast<u128>(Q[w]) * q[l] + carry;
            Q[w] = static_cast<uint64_t>(p);
            carry = p >> 64;
        }
        if (carry) Q.push_back(static_cast<uint64_t>(carry));
    }
    return Q;
}

// -1, 0, 1 as a < b, a == b, a > b (either may carry high zero words)
inline int compare_words(const uint64_t *a, size_t na, const uint64_t *b, size_t nb) {
    const std::vector<uint64_t> x = trimmed(a, na), y = trimmed(b, nb);
    if (x.size() != y.size()) return x.size() < y.size() ? -1 : 1;
    for (size_t w = x.size(); w-- > 0;)
        if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
    return 0;
}

// x <- x / m, returns x mod m (m > 0)
inline uint64_t divmod_word(std::vector<uint64_t> &x, uint64_t m) {
    u128 r = 0;
    for (size_t w = x.size(); w-- > 0;) {
        const u128 cur = (r << 64) | x[w];
        x[w] = static_cast<uint64_t>(cur / m);
        r = cur % m;
    }
    return static_cast<uint64_t>(r);
}

// a - b for a >= b, as words of a's length
inline std::vector<uint64_t> sub_words(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    std::vector<uint64_t> out(a.size(), 0);
    uint64_t borrow = 0;
    for (size_t w = 0; w < a.size(); ++w) {
        const uint64_t bw = w < b.size() ? b[w] : 0;
        const uint64_t d = a[w] - bw - borrow;
        borrow = (a[w] < bw || (a[w] == bw && borrow)) ? 1 : 0;
        out[w] = d;
    }
    return out;
}

// The digits of the bound `words` (nwords little-endian words, high zero words allowed) over q_0 .. q_{L-1}.
// Returns 0 and fills `out`, or 1 with `out` untouched when the bound lies above Q = q_0 .. q_{L-1} (non-zero words
// above Q's words included) or the basis is not 1 .. kMaxLimbs non-zero moduli.
inline int bound_digits(const uint64_t *words, size_t nwords, const uint64_t *q, int L, BoundDigits *out) {
    if (L < 1 || L > kMaxLimbs) return 1;
    for (int k = 0; k < L; ++k)
        if (q[k] == 0) return 1;
    const std::vector<uint64_t> Q = product_words(q, L);
    const int c = compare_words(words, nwords, Q.data(), Q.size());
    if (c > 0) return 1;
    BoundDigits b;
    for (int k = 0; k < kMaxLimbs; ++k) b.d[k] = 0;
    b.is_q = c == 0;
    if (!b.is_q) {
        std::vector<uint64_t> x = trimmed(words, nwords);
        for (int k = 0; k < L && !x.empty(); ++k) b.d[k] = divmod_word(x, q[k]);
    }
    *out = b;
    return 0;
}

// min(2^e, Q) as a bound (e < 64 * (words of Q) + 64)
inline BoundDigits power_of_two_bound(unsigned e, const uint64_t *q, int L) {
    const std::vector<uint64_t> Q = product_words(q, L);
    std::vector<uint64_t> p(e / 64 + 1, 0);
    p[e / 64] = uint64_t(1) << (e % 64);
    BoundDigits b;
    if (compare_words(p.data(), p.size(), Q.data(), Q.size()) >= 0) bound_digits(Q.data(), Q.size(), q, L, &b);
    else bound_digits(p.data(), p.size(), q, L, &b);
    return b;
}

// max(Q - 2^e, 0) as a bound
inline BoundDigits q_minus_power_of_two_bound(unsigned e, const uint64_t *q, int L) {
    const std::vector<uint64_t> Q = product_words(q, L);
    std::vector<uint64_t> p(e / 64 + 1, 0);
    p[e / 64] = uint64_t(1) << (e % 64);
    std::vector<uint64_t> x(1, 0);
    if (compare_words(p.data(), p.size(), Q.data(), Q.size()) < 0) x = sub_words(Q, p);
    BoundDigits b;
    bound_digits(x.data(), x.size(), q, L, &b);
    return b;
}

// floor(Q / 2) + 1 as a bound: a coefficient at or above it has a negative centred representative
inline BoundDigits half_plus_one_bound(const uint64_t *q, int L) {
    std::vector<uint64_t> h = product_words(q, L);
    for (size_t w = 0; w < h.size(); ++w) h[w] = (h[w] >> 1) | (w + 1 < h.size() ? h[w + 1] << 63 : 0);
    for (size_t w = 0; w < h.size(); ++w)
        if (++h[w] != 0) break;  // no carry out of the top word: floor(Q/2) + 1 <= Q
    BoundDigits b;
    bound_digits(h.data(), h.size(), q, L, &b);
    return b;
}

// q_0 .. q_{k-1} mod 2^64 for every k < L (1 for k = 0), and Q mod 2^64 in *q_low
inline void wrapping_prefix_products(const uint64_t *q, int L, uint64_t *pw, uint64_t *q_low) {
    uint64_t p = 1;
    for (int k = 0; k < L; ++k) {
        pw[k] = p;
        p *= q[k];
    }
    *q_low = p;
}

}  // namespace readout
