// nested_rns.hip — the nested-RNS gadget vector, its decomposition and the p-residues of a matrix on the device
// (extension).
//
// gpupoly_matrix_fill_nested_rns_gadget and gpupoly_matrix_nested_rns_decompose replace nested_rns_gadget_vector and
// nested_rns_gadget_decomposed (src/gadgets/arith/nested_rns/encoding.rs:240-338), which the reference runs as a serial
// host loop over BigUints (map_nested_rns_values, :121-139); gpupoly_matrix_nested_rns_residues is the slot-wise form of
// encode_nested_rns_poly_with_offset (:401-420).
//
// With pairwise coprime p_0..p_{D-1}, P their product, the window limbs off .. off+A-1 of the matrix's L limbs:
//   rdiv(a, b) = floor((a + floor(b/2)) / b),   inv_j = ((P/p_j) mod p_j)^-1 mod p_j,
//   terms(x_0..x_{D-1}):  y_j = (x_j mod p_j) inv_j mod p_j,  w = rdiv(sum_j rdiv(y_j scale, p_j), scale)   (:196-214)
//   slot(a, x) in limb l = ((sum_j y_j (P/p_j mod q_l) - w (P mod q_l)) (rc_a mod q_l)) mod q_l               (:222-238)
//   rc_a = (Q_act/q_a) ((Q_act/q_a) mod q_a)^-1, an integer below Q_act: rc_a mod q_l is a product of residues.
// rc_a is 0 in the window's other limbs, so a digit row of window index a is zero there and needs a table only for the
// NZ = L - A + 1 limbs outside the window and limb off+a.
//
// Per set of arguments the context keeps one block of device tables (built on the first call, like the gadget constant
// tables): per p_j the reciprocals, x -> y and x -> rdiv(y scale, p_j); per limb the constants above; the gadget vector's
// A(D+1) x L words; and T[a][i][s] = slot(a, s) in the i-th non-zero limb of a, s < S = max(p_max, D+1), built by a
// small kernel.  A digit of the decomposition is some y_d < p_d or w <= D, so every output word is a read of T.
//
// Main kernel: block y = window index a, whose T slice sits in LDS where it fits 64 KB (global reads otherwise); a lane
// owns 16 bytes of coefficients of one (entry, a), takes r mod p_j by the precomputed reciprocal, looks up y_j and the
// partial sum, and stores the L vectors of digit row j at once, zeros included; w's row follows.  Lanes run along the
// coefficient: every store instruction of a wave is one contiguous run of a (row, limb) vector.
//
// An EVAL source is inverse-transformed in a copy.  An EVAL result over the full window of several limbs transforms no
// zero: the kernel stores limb a of a's rows alone into scratch, the forward transform runs over that, and a second
// kernel spreads it over `out` with the zeros.  Other windows store COEFF words and transform `out` whole.
#include "common.h"
#include "modarith.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace {

constexpr size_t kTablesMax = 64;                // argument sets a context keeps tables for
constexpr size_t kTableBytesMax = size_t(64) << 20;  // a larger block serves its call alone
constexpr size_t kLdsBytes = 64 * 1024;          // T slice of one window index held in LDS up to this

struct PMod {
    uint64_t m64;  // floor(2^64 / p)
    uint32_t m32;  // floor(2^32 / p)
    uint32_t p;
    uint32_t ofs;  // of p's rows in the x tables
    uint32_t pad;
};

// where the pieces of one table block lie, from the arguments alone
struct TableLayout {
    size_t pm, rtab, ytab, ph, pmq, rc, gvals, T, bytes;
    uint32_t D, S, NZ, SP;
    TableLayout(const uint64_t *p, size_t D_, size_t Lm, size_t A, size_t wb) {
        D = static_cast<uint32_t>(D_);
        uint64_t pmax = 0, sp = 0;
        for (size_t j = 0; j < D_; ++j) {
            pmax = std::max(pmax, p[j]);
            sp += p[j];
        }
        S = static_cast<uint32_t>(std::max<uint64_t>(pmax, D_ + 1));
        SP = static_cast<uint32_t>(sp);
        NZ = static_cast<uint32_t>(Lm - A + 1);
        size_t at = 0;
        auto take = [&](size_t bytes_) {
            const size_t here = at;
            at += (bytes_ + 15) / 16 * 16;
            return here;
        };
        pm = take(D_ * sizeof(PMod));
        rtab = take(sp * 8);
        ytab = take(sp * 2);
        ph = take(D_ * Lm * 8);
        pmq = take(Lm * 8);
        rc = take(A * Lm * 8);
        gvals = take(A * (D_ + 1) * Lm * wb);
        T = take(A * static_cast<size_t>(NZ) * S * wb);
        bytes = at;
    }
};

struct Tables {
    const PMod *pm;
    const uint64_t *rtab;
    const uint16_t *ytab;
    const uint64_t *ph, *pmq, *rc;
    const void *gvals;
    void *T;
    uint32_t D, S, NZ;
};

Tables tables_at(void *base, const TableLayout &lay) {
    char *b = static_cast<char *>(base);
    Tables t;
    t.pm = reinterpret_cast<const PMod *>(b + lay.pm);
    t.rtab = reinterpret_cast<const uint64_t *>(b + lay.rtab);
    t.ytab = reinterpret_cast<const uint16_t *>(b + lay.ytab);
    t.ph = reinterpret_cast<const uint64_t *>(b + lay.ph);
    t.pmq = reinterpret_cast<const uint64_t *>(b + lay.pmq);
    t.rc = reinterpret_cast<const uint64_t *>(b + lay.rc);
    t.gvals = b + lay.gvals;
    t.T = b + lay.T;
    t.D = lay.D;
    t.S = lay.S;
    t.NZ = lay.NZ;
    return t;
}

template <typename W, int VN>
struct WordVec {
    typedef typename std::conditional<sizeof(W) * VN == 16, uint4, W>::type type;
};

// r mod p by the reciprocal: the quotient estimate is at most one short
__device__ __forceinline__ uint32_t mod_p(uint32_t r, const PMod &pm) {
    const uint32_t x = r - __umulhi(r, pm.m32) * pm.p;
    return x >= pm.p ? x - pm.p : x;
}
__device__ __forceinline__ uint32_t mod_p(uint64_t r, const PMod &pm) {
    const uint32_t x = static_cast<uint32_t>(r - __umul64hi(r, pm.m64) * pm.p);
    return x >= pm.p ? x - pm.p : x;
}

// the i-th non-zero limb of window index a: the limbs below the window, limb off + a, the limbs above the window
__device__ __forceinline__ uint32_t nz_limb(uint32_t i, uint32_t a, uint32_t off, uint32_t A) {
    return i < off ? i : (i == off ? off + a : i + A - 1);
}

// T[a][i][s] = slot(a, s) in limb nz_limb(i, a); one thread per word
template <typename W>
__global__ void __launch_bounds__(256) nrns_table_kernel(W *__restrict__ T, Tables tb, size_t words, uint32_t Lm, uint32_t off, uint32_t A,
                                                         uint64_t scale, const LimbConst *__restrict__ limbs) {
    const size_t idx = item_index();
    if (idx >= words) return;
    const uint32_t s = static_cast<uint32_t>(idx % tb.S);
    const size_t rest = idx / tb.S;
    const uint32_t i = static_cast<uint32_t>(rest % tb.NZ), a = static_cast<uint32_t>(rest / tb.NZ);
    const uint32_t l = nz_limb(i, a, off, A);
    const LimbConst lc = limbs[l];
    const W q = static_cast<W>(lc.q);
    uint64_t sum = 0;
    W acc = 0;
    for (uint32_t j = 0; j < tb.D; ++j) {
        const PMod pm = tb.pm[j];
        const uint32_t x = s % pm.p;
        const uint64_t y = tb.ytab[pm.ofs + x];
        sum += tb.rtab[pm.ofs + x];
        acc = add_mod<W>(acc, mul_mod<W>(static_cast<W>(y % lc.q), static_cast<W>(tb.ph[j * Lm + l]), q, lc.mu, lc.kbits), q);
    }
    const uint64_t w = (sum + scale / 2) / scale;  // at most D
    const W wp = mul_mod<W>(static_cast<W>(w % lc.q), static_cast<W>(tb.pmq[l]), q, lc.mu, lc.kbits);
    const W v = sub_mod<W>(acc, wp, q);
    T[idx] = mul_mod<W>(v, static_cast<W>(tb.rc[a * Lm + l]), q, lc.mu, lc.kbits);
}

struct MainArgs {
    const PMod *pm;
    const uint64_t *rtab;
    const uint16_t *ytab;
    const void *T;
    uint32_t D, S, NZ, Lm, off, A, cols;
    uint32_t logN, log_cv;  // log2 of the vectors per polynomial
    size_t items;           // (entry, vector) pairs of one window index
    uint64_t scale, scale_m, half;  // scale_m = floor(2^64 / scale) (2^64 - 1 for scale 1), half = floor(scale / 2)
};

// grid y = window index a, x strides over the (entry, vector) items of a.  out is [rows A (D+1)][cols][Lm][N], src the
// coefficient-domain words of the source, [rows][cols][Lm][N].
// COMPACT (the full window only, where limb a is the one non-zero limb of a's rows): out is instead the scratch
// [rows][D+1][cols][A][N] that holds that limb alone - vector v of it is of limb v mod A, the order the transform
// launchers expect - and nrns_expand_kernel spreads it over the matrix after the forward transform.
template <typename W, int VN, bool LDS, bool COMPACT>
__global__ void __launch_bounds__(256) nrns_decompose_kernel(W *__restrict__ out, const W *__restrict__ src, MainArgs g) {
    typedef typename WordVec<W, VN>::type VT;
    extern __shared__ __align__(16) unsigned char nrns_lds[];
    const uint32_t a = blockIdx.y;
    const size_t slice = static_cast<size_t>(g.NZ) * g.S;
    const W *tab = static_cast<const W *>(g.T) + a * slice;
    if constexpr (LDS) {
        W *sh = reinterpret_cast<W *>(nrns_lds);
        for (size_t i = threadIdx.x; i < slice; i += blockDim.x) sh[i] = tab[i];
        __syncthreads();
        tab = sh;
    }
    const uint32_t N = 1u << g.logN;
    const uint32_t cw = g.D + 1;
    const size_t poly_words = static_cast<size_t>(g.Lm) * N;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < g.items; t += stride) {
        const size_t entry = t >> g.log_cv;
        const uint32_t k0 = static_cast<uint32_t>(t - (entry << g.log_cv)) * VN;
        size_t row, col;
        if (entry <= 0xffffffffull) {
            const uint32_t e32 = static_cast<uint32_t>(entry);
            row = e32 / g.cols;
            col = e32 % g.cols;
        } else {
            row = entry / g.cols;
            col = entry % g.cols;
        }
        W r[VN];
        *reinterpret_cast<VT *>(r) = *reinterpret_cast<const VT *>(src + entry * poly_words + static_cast<size_t>(g.off + a) * N + k0);
        // words of digit row d of this entry: ((row A cw + a cw + d) cols + col) poly_words
        W *o = COMPACT ? out + ((row * cw * g.cols + col) * g.A + a) * N + k0 : out + ((row * g.A + a) * cw * g.cols + col) * poly_words + k0;
        const size_t row_step = COMPACT ? static_cast<size_t>(g.cols) * g.A * N : static_cast<size_t>(g.cols) * poly_words;
        uint64_t sum[VN];
        uint32_t digit[VN];
#pragma unroll
        for (int v = 0; v < VN; ++v) sum[v] = 0;
        auto store_row = [&](W *dst) {
            if constexpr (COMPACT) {
                W val[VN];
#pragma unroll
                for (int v = 0; v < VN; ++v) val[v] = tab[digit[v]];
                *reinterpret_cast<VT *>(dst) = *reinterpret_cast<const VT *>(val);
                return;
            }
            for (uint32_t l = 0; l < g.Lm; ++l) {
                W val[VN];
                const bool below = l < g.off, above = l >= g.off + g.A;
                if (below || above || l == g.off + a) {
                    const W *tl = tab + static_cast<size_t>(below ? l : (above ? l - g.A + 1 : g.off)) * g.S;
#pragma unroll
                    for (int v = 0; v < VN; ++v) val[v] = tl[digit[v]];
                } else {
#pragma unroll
                    for (int v = 0; v < VN; ++v) val[v] = 0;
                }
                *reinterpret_cast<VT *>(dst + static_cast<size_t>(l) * N) = *reinterpret_cast<const VT *>(val);
            }
        };
        for (uint32_t j = 0; j < g.D; ++j) {
            const PMod pm = g.pm[j];
#pragma unroll
            for (int v = 0; v < VN; ++v) {
                const uint32_t x = pm.ofs + mod_p(r[v], pm);
                digit[v] = g.ytab[x];
                sum[v] += g.rtab[x];
            }
            store_row(o + j * row_step);
        }
#pragma unroll
        for (int v = 0; v < VN; ++v) {
            const uint64_t n = sum[v] + g.half;
            uint64_t w = __umul64hi(n, g.scale_m);  // at most one short
            if (n - w * g.scale >= g.scale) ++w;
            digit[v] = static_cast<uint32_t>(w);  // at most D
        }
        store_row(o + g.D * row_step);
    }
}

// The full window after the COMPACT kernel and the transform of its scratch: limb a of out[(row A + a) cw + d][col] is
// vector ((row cw + d) cols + col) A + a of `compact`, every other limb of that polynomial is zero.  One thread per
// (polynomial of out, vector of coefficients), which stores all L limbs.
template <typename W, int VN>
__global__ void __launch_bounds__(256) nrns_expand_kernel(W *__restrict__ out, const W *__restrict__ compact, size_t items, uint32_t cols,
                                                          uint32_t A, uint32_t cw, uint32_t logN, uint32_t log_cv) {
    typedef typename WordVec<W, VN>::type VT;
    const size_t t = item_index();
    if (t >= items) return;
    const uint32_t N = 1u << logN;
    const size_t poly = t >> log_cv;
    const uint32_t k0 = static_cast<uint32_t>(t - (poly << log_cv)) * VN;
    const size_t out_row = poly / cols, col = poly % cols;
    const size_t row = out_row / (static_cast<size_t>(A) * cw);
    const uint32_t rest = static_cast<uint32_t>(out_row % (static_cast<size_t>(A) * cw));
    const uint32_t a = rest / cw, d = rest % cw;
    W val[VN], zero[VN];
    *reinterpret_cast<VT *>(val) = *reinterpret_cast<const VT *>(compact + (((row * cw + d) * cols + col) * A + a) * N + k0);
#pragma unroll
    for (int v = 0; v < VN; ++v) zero[v] = 0;
    W *o = out + poly * A * N + k0;
    for (uint32_t l = 0; l < A; ++l) *reinterpret_cast<VT *>(o + static_cast<size_t>(l) * N) = *reinterpret_cast<const VT *>(l == a ? val : zero);
}

// out is [rows A D][cols][Lm][N]: row (row A + a) D + j holds r mod p_j in every limb.  One thread per (a, entry, vector).
struct ResidueMods {
    PMod pm[64];  // by value: this entry needs no table block
};

template <typename W, int VN>
__global__ void __launch_bounds__(256) nrns_residues_kernel(W *__restrict__ out, const W *__restrict__ src, MainArgs g, ResidueMods mods,
                                                            const LimbConst *__restrict__ limbs) {
    typedef typename WordVec<W, VN>::type VT;
    const uint32_t a = blockIdx.y;
    const uint32_t N = 1u << g.logN;
    const size_t poly_words = static_cast<size_t>(g.Lm) * N;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < g.items; t += stride) {
        const size_t entry = t >> g.log_cv;
        const uint32_t k0 = static_cast<uint32_t>(t - (entry << g.log_cv)) * VN;
        const size_t row = entry / g.cols, col = entry % g.cols;
        W r[VN];
        *reinterpret_cast<VT *>(r) = *reinterpret_cast<const VT *>(src + entry * poly_words + static_cast<size_t>(g.off + a) * N + k0);
        W *o = out + ((row * g.A + a) * g.D * g.cols + col) * poly_words + k0;
        const size_t row_step = static_cast<size_t>(g.cols) * poly_words;
        for (uint32_t j = 0; j < g.D; ++j) {
            const PMod pm = mods.pm[j];
            uint32_t x[VN];
#pragma unroll
            for (int v = 0; v < VN; ++v) x[v] = mod_p(r[v], pm);
            for (uint32_t l = 0; l < g.Lm; ++l) {
                const uint64_t q = limbs[l].q;
                W val[VN];
#pragma unroll
                for (int v = 0; v < VN; ++v) val[v] = static_cast<W>(x[v] >= q ? x[v] % q : x[v]);
                *reinterpret_cast<VT *>(o + j * row_step + static_cast<size_t>(l) * N) = *reinterpret_cast<const VT *>(val);
            }
        }
    }
}

// out is [A (D+1)][Lm][N]: every coefficient of vector v is gvals[v]
template <typename W>
__global__ void __launch_bounds__(256) nrns_gadget_kernel(W *__restrict__ out, const W *__restrict__ gvals, size_t words, uint32_t logN) {
    const size_t idx = item_index();
    if (idx >= words) return;
    out[idx] = gvals[idx >> logN];
}

// ---- host constants: 64/128-bit integers only ----
uint64_t h_mul(uint64_t a, uint64_t b, uint64_t m) { return static_cast<uint64_t>(static_cast<u128_t>(a) * b % m); }

uint64_t h_gcd(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// a^-1 mod m by the extended Euclidean algorithm (m need not be prime: p = 4 is a modulus); 0 when there is none
uint64_t h_inverse(uint64_t a, uint64_t m) {
    if (m == 1) return 0;
    __int128 r0 = m, r1 = a % m, t0 = 0, t1 = 1;
    while (r1 != 0) {
        const __int128 qu = r0 / r1;
        const __int128 r2 = r0 - qu * r1, t2 = t0 - qu * t1;
        r0 = r1;
        r1 = r2;
        t0 = t1;
        t1 = t2;
    }
    if (r0 != 1) return 0;
    if (t0 < 0) t0 += m;
    return static_cast<uint64_t>(t0);
}

PMod p_mod(uint64_t p, uint32_t ofs) {
    PMod m;
    m.m64 = static_cast<uint64_t>((static_cast<u128_t>(1) << 64) / p);
    m.m32 = static_cast<uint32_t>((1ull << 32) / p);
    m.p = static_cast<uint32_t>(p);
    m.ofs = ofs;
    m.pad = 0;
    return m;
}

struct Window {
    size_t D, Lm, off, A;
    uint64_t scale;
    const uint64_t *p;
};

// the host part of a table block: everything but T
template <typename W>
void fill_host_tables(const GpuContext *ctx, const Window &wn, const TableLayout &lay, std::vector<unsigned char> &host) {
    const size_t D = wn.D, Lm = wn.Lm, A = wn.A, off = wn.off;
    const uint64_t *p = wn.p, *q = ctx->moduli.data();
    PMod *pm = reinterpret_cast<PMod *>(host.data() + lay.pm);
    uint64_t *rtab = reinterpret_cast<uint64_t *>(host.data() + lay.rtab);
    uint16_t *ytab = reinterpret_cast<uint16_t *>(host.data() + lay.ytab);
    uint64_t *ph = reinterpret_cast<uint64_t *>(host.data() + lay.ph);
    uint64_t *pmq = reinterpret_cast<uint64_t *>(host.data() + lay.pmq);
    uint64_t *rc = reinterpret_cast<uint64_t *>(host.data() + lay.rc);
    W *gvals = reinterpret_cast<W *>(host.data() + lay.gvals);
    std::vector<uint64_t> inv(D);
    uint32_t ofs = 0;
    for (size_t j = 0; j < D; ++j) {
        uint64_t hat = 1 % p[j];  // (P / p_j) mod p_j
        for (size_t i = 0; i < D; ++i)
            if (i != j) hat = h_mul(hat, p[i] % p[j], p[j]);
        inv[j] = h_inverse(hat, p[j]);
        pm[j] = p_mod(p[j], ofs);
        for (uint64_t x = 0; x < p[j]; ++x) {
            const uint64_t y = x * inv[j] % p[j];
            ytab[ofs + x] = static_cast<uint16_t>(y);
            rtab[ofs + x] = (y * wn.scale + p[j] / 2) / p[j];  // below 2^64 by the entry's bounds
        }
        ofs += static_cast<uint32_t>(p[j]);
    }
    for (size_t l = 0; l < Lm; ++l) {
        uint64_t all = 1 % q[l];
        for (size_t j = 0; j < D; ++j) {
            uint64_t hat = 1 % q[l];
            for (size_t i = 0; i < D; ++i)
                if (i != j) hat = h_mul(hat, p[i] % q[l], q[l]);
            ph[j * Lm + l] = hat;
            all = h_mul(all, p[j] % q[l], q[l]);
        }
        pmq[l] = all;
    }
    for (size_t a = 0; a < A; ++a) {
        const uint64_t qa = q[off + a];
        uint64_t hat = 1 % qa;  // (Q_act / q_a) mod q_a
        for (size_t b = 0; b < A; ++b)
            if (b != a) hat = h_mul(hat, q[off + b] % qa, qa);
        const uint64_t hinv = h_inverse(hat, qa);
        for (size_t l = 0; l < Lm; ++l) {
            uint64_t v = hinv % q[l];
            for (size_t b = 0; b < A; ++b)
                if (b != a) v = h_mul(v, q[off + b] % q[l], q[l]);
            rc[a * Lm + l] = v;
        }
    }
    // the gadget vector: entry a (D+1) + d is slot(a, g mod p_0, ...), g = (P/p_d) mod q_a, and (q_a - P mod q_a) mod q_a for d = D
    for (size_t a = 0; a < A; ++a) {
        const uint64_t qa = q[off + a];
        for (size_t d = 0; d <= D; ++d) {
            const uint64_t gv = d < D ? ph[d * Lm + off + a] : (qa - pmq[off + a]) % qa;
            std::vector<uint64_t> y(D);
            uint64_t sum = 0;
            for (size_t j = 0; j < D; ++j) {
                const uint32_t x = pm[j].ofs + static_cast<uint32_t>(gv % p[j]);
                y[j] = ytab[x];
                sum += rtab[x];
            }
            const uint64_t w = (sum + wn.scale / 2) / wn.scale;
            for (size_t l = 0; l < Lm; ++l) {
                uint64_t acc = 0;
                for (size_t j = 0; j < D; ++j) acc = (acc + h_mul(y[j] % q[l], ph[j * Lm + l], q[l])) % q[l];
                const uint64_t wp = h_mul(w % q[l], pmq[l], q[l]);
                const uint64_t v = acc >= wp ? acc - wp : acc + q[l] - wp;
                gvals[(a * (D + 1) + d) * Lm + l] = static_cast<W>(h_mul(v, rc[a * Lm + l], q[l]));
            }
        }
    }
}

// the table block for these arguments: the context's where it keeps one, else built into `scratch` for this call
template <typename W>
int tables_for(GpuContext *ctx, const Window &wn, CtxBlock &scratch, Tables *out) {
    const TableLayout lay(wn.p, wn.D, wn.Lm, wn.A, sizeof(W));
    std::vector<uint64_t> key = {sizeof(W), wn.Lm, wn.off, wn.A, wn.scale};
    key.insert(key.end(), wn.p, wn.p + wn.D);
    std::lock_guard<std::mutex> lock(ctx->mutex);
    auto it = ctx->nested_rns_tables.find(key);
    if (it != ctx->nested_rns_tables.end()) {
        *out = tables_at(it->second, lay);
        return 0;
    }
    std::vector<unsigned char> host(lay.T, 0);
    fill_host_tables<W>(ctx, wn, lay, host);
    const bool keep = lay.bytes <= kTableBytesMax && ctx->nested_rns_tables.size() < kTablesMax;
    void *dev = nullptr;
    if (keep) {
        HIP_TRY(hipMalloc(&dev, lay.bytes));
        const hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return set_error(e, "nested-RNS table upload");
        }
    } else {
        if (scratch.alloc(lay.bytes)) return 1;
        dev = scratch.ptr;
        HIP_TRY(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // `host` goes out of scope
    }
    const Tables tb = tables_at(dev, lay);
    const size_t words = static_cast<size_t>(wn.A) * lay.NZ * lay.S;
    MXX_TRACE_BYTES(static_cast<double>(words) * sizeof(W));
    MXX_LAUNCH((nrns_table_kernel<W>), item_grid(words, 256), dim3(256), 0, ctx->stream, static_cast<W *>(tb.T), tb, words,
               static_cast<uint32_t>(wn.Lm), static_cast<uint32_t>(wn.off), static_cast<uint32_t>(wn.A), wn.scale, ctx->d_limbs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (keep) (void)hipFree(dev);
        return set_error(e, "nested-RNS table kernel");
    }
    if (keep) ctx->nested_rns_tables.emplace(std::move(key), dev);
    *out = tb;
    return 0;
}

uint32_t log2_of(size_t v) {
    uint32_t lg = 0;
    while ((static_cast<size_t>(1) << lg) < v) ++lg;
    return lg;
}

MainArgs main_args(const GpuContext *ctx, const Tables &tb, const Window &wn, size_t entries, size_t cols, int VN) {
    MainArgs g;
    g.pm = tb.pm;
    g.rtab = tb.rtab;
    g.ytab = tb.ytab;
    g.T = tb.T;
    g.D = tb.D;
    g.S = tb.S;
    g.NZ = tb.NZ;
    g.Lm = static_cast<uint32_t>(wn.Lm);
    g.off = static_cast<uint32_t>(wn.off);
    g.A = static_cast<uint32_t>(wn.A);
    g.cols = static_cast<uint32_t>(cols);
    g.logN = ctx->logN;
    g.log_cv = ctx->logN - log2_of(static_cast<size_t>(VN));
    g.items = entries << g.log_cv;
    g.scale = wn.scale;
    g.scale_m = wn.scale == 1 ? ~0ull : static_cast<uint64_t>((static_cast<u128_t>(1) << 64) / wn.scale);
    g.half = wn.scale / 2;
    return g;
}

// blocks along x: enough lanes for the items, few enough that a block's work outweighs its table load
unsigned blocks_x(size_t items, size_t A) {
    const size_t want = (items + 255) / 256, cap = std::max<size_t>(1, 4096 / A);
    return static_cast<unsigned>(std::max<size_t>(1, std::min(want, cap)));
}

// compact: `out` is the scratch of the COMPACT form (the full window, EVAL result)
template <typename W>
int decompose(GpuContext *ctx, W *out, const W *src, const Tables &tb, const Window &wn, size_t entries, size_t cols, bool compact) {
    constexpr int VNMAX = 16 / sizeof(W);
    const bool vec = static_cast<size_t>(ctx->N) % VNMAX == 0;
    const MainArgs g = main_args(ctx, tb, wn, entries, cols, vec ? VNMAX : 1);
    const size_t lds = static_cast<size_t>(tb.NZ) * tb.S * sizeof(W);
    const bool in_lds = lds <= kLdsBytes;
    const dim3 grid(blocks_x(g.items, wn.A), static_cast<unsigned>(wn.A));
    // one window limb of every entry read, (D + 1) L words (compact: D + 1) written per coefficient of every window index
    const double words = static_cast<double>(entries) * wn.A * ctx->N;
    MXX_TRACE_BYTES(words * sizeof(W) * (1.0 + (wn.D + 1.0) * (compact ? 1 : wn.Lm)));
    auto launch = [&](auto vn, auto in_lds_, auto compact_) {
        MXX_LAUNCH((nrns_decompose_kernel<W, decltype(vn)::value, decltype(in_lds_)::value, decltype(compact_)::value>), grid, dim3(256),
                   decltype(in_lds_)::value ? lds : 0, ctx->stream, out, src, g);
    };
    auto pick = [&](auto vn) {
        if (in_lds && compact) launch(vn, std::true_type(), std::true_type());
        else if (in_lds) launch(vn, std::true_type(), std::false_type());
        else if (compact) launch(vn, std::false_type(), std::true_type());
        else launch(vn, std::false_type(), std::false_type());
    };
    if (vec) pick(std::integral_constant<int, VNMAX>());
    else pick(std::integral_constant<int, 1>());
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int expand(GpuContext *ctx, W *out, const W *compact, size_t out_polys, size_t cols, const Window &wn) {
    constexpr int VNMAX = 16 / sizeof(W);
    const bool vec = static_cast<size_t>(ctx->N) % VNMAX == 0;
    const uint32_t log_cv = ctx->logN - log2_of(static_cast<size_t>(vec ? VNMAX : 1));
    const size_t items = out_polys << log_cv;
    const uint32_t A = static_cast<uint32_t>(wn.A), cw = static_cast<uint32_t>(wn.D + 1);
    // the compact limb read once, every word of out written once
    MXX_TRACE_BYTES(static_cast<double>(out_polys) * ctx->N * sizeof(W) * (1.0 + wn.A));
    if (vec) MXX_LAUNCH((nrns_expand_kernel<W, VNMAX>), item_grid(items, 256), dim3(256), 0, ctx->stream, out, compact, items,
                        static_cast<uint32_t>(cols), A, cw, ctx->logN, log_cv);
    else MXX_LAUNCH((nrns_expand_kernel<W, 1>), item_grid(items, 256), dim3(256), 0, ctx->stream, out, compact, items,
                    static_cast<uint32_t>(cols), A, cw, ctx->logN, log_cv);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int residues(GpuContext *ctx, W *out, const W *src, const Window &wn, size_t entries, size_t cols) {
    constexpr int VNMAX = 16 / sizeof(W);
    const bool vec = static_cast<size_t>(ctx->N) % VNMAX == 0;
    Tables tb = {};
    tb.D = static_cast<uint32_t>(wn.D);
    const MainArgs g = main_args(ctx, tb, wn, entries, cols, vec ? VNMAX : 1);
    ResidueMods mods = {};
    for (size_t j = 0; j < wn.D; ++j) mods.pm[j] = p_mod(wn.p[j], 0);
    const dim3 grid(blocks_x(g.items, 1), static_cast<unsigned>(wn.A));
    const double words = static_cast<double>(entries) * wn.A * ctx->N;
    MXX_TRACE_BYTES(words * sizeof(W) * (1.0 + static_cast<double>(wn.D) * wn.Lm));
    if (vec) MXX_LAUNCH((nrns_residues_kernel<W, VNMAX>), grid, dim3(256), 0, ctx->stream, out, src, g, mods, ctx->d_limbs);
    else MXX_LAUNCH((nrns_residues_kernel<W, 1>), grid, dim3(256), 0, ctx->stream, out, src, g, mods, ctx->d_limbs);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename W>
int gadget(GpuContext *ctx, W *out, const Tables &tb, size_t words) {
    MXX_TRACE_BYTES(static_cast<double>(words) * sizeof(W));
    MXX_LAUNCH((nrns_gadget_kernel<W>), item_grid(words, 256), dim3(256), 0, ctx->stream, out, static_cast<const W *>(tb.gvals), words, ctx->logN);
    HIP_TRY(hipGetLastError());
    return 0;
}

// "" when the p-moduli and the scale are within the entries' bounds, else what is unsupported about them
std::string unsupported_moduli(const uint64_t *p, size_t D, uint64_t scale, bool with_scale) {
    if (D < 1 || D > 64) return "unsupported p_count (1..64)";
    uint64_t pmax = 0;
    for (size_t j = 0; j < D; ++j) {
        if (p[j] < 2 || p[j] >= (1ull << 16)) return "unsupported p modulus (2 <= p < 2^16; p[" + std::to_string(j) + "])";
        pmax = std::max(pmax, p[j]);
    }
    for (size_t j = 0; j < D; ++j)
        for (size_t i = 0; i < j; ++i)
            if (h_gcd(p[i], p[j]) != 1) return "unsupported p moduli: not pairwise coprime (p[" + std::to_string(i) + "], p[" + std::to_string(j) + "])";
    if (!with_scale) return "";
    if (scale < 1) return "unsupported scale (at least 1)";
    const u128_t lim = static_cast<u128_t>(1) << 64;
    if (static_cast<u128_t>(pmax - 1) * scale + pmax / 2 >= lim || static_cast<u128_t>(D) * scale + scale / 2 >= lim)
        return "unsupported scale: the rounded sums leave 64 bits";
    return "";
}

}  // namespace

extern "C" int gpupoly_matrix_nested_rns_decompose(GpuMatrix *out, const GpuMatrix *src, const uint64_t *p_moduli, size_t p_count,
                                                   uint64_t scale, size_t level_offset, size_t active_levels, int out_format) {
    ABI_GUARD_BEGIN
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_nested_rns_decompose: " + what); };
    if (!out || !src || !p_moduli) return refuse("null argument");
    if (out_format != GPU_POLY_FORMAT_COEFF && out_format != GPU_POLY_FORMAT_EVAL) return refuse("unknown out_format");
    if (src->format != GPU_POLY_FORMAT_COEFF && src->format != GPU_POLY_FORMAT_EVAL) return refuse("unknown format");
    const std::string bad = unsupported_moduli(p_moduli, p_count, scale, true);
    if (!bad.empty()) return refuse(bad);
    GpuContext *ctx = src->ctx;
    if (out->ctx != ctx) return refuse("context mismatch");
    if (out->level != src->level) return refuse("level mismatch");
    const size_t Lm = matrix_limbs(src), D = p_count, A = active_levels;
    if (A == 0) return refuse("active_levels must be at least 1");
    if (level_offset > Lm || A > Lm - level_offset) return refuse("the window leaves the matrix's limbs");
    if (out->cols != src->cols || out->rows != src->rows * A * (D + 1))
        return refuse("shape mismatch (out must be rows * active_levels * (p_count + 1) x cols)");
    if (storage_overlaps(out, src)) return refuse("the output overlaps the source");
    if (matrix_polys(src) == 0) {
        out->format = out_format;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const Window wn = {D, Lm, level_offset, A, scale, p_moduli};
    CtxBlock table_scratch(ctx), coeff_scratch(ctx);
    Tables tb;
    int rcode = ctx->wide ? tables_for<uint64_t>(ctx, wn, table_scratch, &tb) : tables_for<uint32_t>(ctx, wn, table_scratch, &tb);
    if (rcode) return rcode;
    const void *s = nullptr;
    if ((rcode = coeff_domain_source(src, coeff_scratch, &s))) return rcode;  // an EVAL source is inverse-transformed in a copy
    void *o = words_ptr(out);
    const size_t entries = matrix_polys(src), out_polys = matrix_polys(out);
    // EVAL over the full window of several limbs: all but limb a of a's rows is zero, so only that limb is produced (in
    // scratch, in the launchers' vector order), transformed, and spread over `out` with the zeros - the transform then
    // runs over 1 / L of the words.  Other windows transform `out` whole.
    if (out_format == GPU_POLY_FORMAT_EVAL && level_offset == 0 && A == Lm && Lm > 1) {
        CtxBlock compact(ctx);
        if (compact.alloc(out_polys * static_cast<size_t>(ctx->N) * ctx->word_bytes)) return 1;
        void *c = compact.ptr;
        rcode = ctx->wide ? decompose<uint64_t>(ctx, static_cast<uint64_t *>(c), static_cast<const uint64_t *>(s), tb, wn, entries, src->cols, true)
                          : decompose<uint32_t>(ctx, static_cast<uint32_t *>(c), static_cast<const uint32_t *>(s), tb, wn, entries, src->cols, true);
        if (rcode) return rcode;
        if ((rcode = launch_ntt(ctx, c, out_polys, static_cast<int>(Lm), false))) return rcode;
        rcode = ctx->wide ? expand<uint64_t>(ctx, static_cast<uint64_t *>(o), static_cast<const uint64_t *>(c), out_polys, src->cols, wn)
                          : expand<uint32_t>(ctx, static_cast<uint32_t *>(o), static_cast<const uint32_t *>(c), out_polys, src->cols, wn);
        if (rcode) return rcode;
        out->format = GPU_POLY_FORMAT_EVAL;
        return 0;
    }
    rcode = ctx->wide ? decompose<uint64_t>(ctx, static_cast<uint64_t *>(o), static_cast<const uint64_t *>(s), tb, wn, entries, src->cols, false)
                      : decompose<uint32_t>(ctx, static_cast<uint32_t *>(o), static_cast<const uint32_t *>(s), tb, wn, entries, src->cols, false);
    if (rcode) return rcode;
    out->format = GPU_POLY_FORMAT_COEFF;
    if (out_format == GPU_POLY_FORMAT_EVAL) {
        if ((rcode = launch_ntt(ctx, o, out_polys * Lm, static_cast<int>(Lm), false))) return rcode;
        out->format = GPU_POLY_FORMAT_EVAL;
    }
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_fill_nested_rns_gadget(GpuMatrix *out, const uint64_t *p_moduli, size_t p_count, uint64_t scale,
                                                     size_t level_offset, size_t active_levels, int out_format) {
    ABI_GUARD_BEGIN
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_fill_nested_rns_gadget: " + what); };
    if (!out || !p_moduli) return refuse("null argument");
    if (out_format != GPU_POLY_FORMAT_COEFF && out_format != GPU_POLY_FORMAT_EVAL) return refuse("unknown out_format");
    const std::string bad = unsupported_moduli(p_moduli, p_count, scale, true);
    if (!bad.empty()) return refuse(bad);
    GpuContext *ctx = out->ctx;
    const size_t Lm = matrix_limbs(out), D = p_count, A = active_levels;
    if (A == 0) return refuse("active_levels must be at least 1");
    if (level_offset > Lm || A > Lm - level_offset) return refuse("the window leaves the matrix's limbs");
    if (out->rows != 1 || out->cols != A * (D + 1)) return refuse("shape mismatch (out must be 1 x active_levels * (p_count + 1))");
    if (ctx_activate(ctx)) return 1;
    const Window wn = {D, Lm, level_offset, A, scale, p_moduli};
    CtxBlock table_scratch(ctx);
    Tables tb;
    int rcode = ctx->wide ? tables_for<uint64_t>(ctx, wn, table_scratch, &tb) : tables_for<uint32_t>(ctx, wn, table_scratch, &tb);
    if (rcode) return rcode;
    // n equal coefficients (not a constant polynomial): filled in the coefficient domain, transformed for EVAL
    void *o = words_ptr(out);
    rcode = ctx->wide ? gadget<uint64_t>(ctx, static_cast<uint64_t *>(o), tb, matrix_words(out))
                      : gadget<uint32_t>(ctx, static_cast<uint32_t *>(o), tb, matrix_words(out));
    if (rcode) return rcode;
    out->format = GPU_POLY_FORMAT_COEFF;
    if (out_format == GPU_POLY_FORMAT_EVAL) {
        if ((rcode = launch_ntt(ctx, o, matrix_polys(out) * Lm, static_cast<int>(Lm), false))) return rcode;
        out->format = GPU_POLY_FORMAT_EVAL;
    }
    return 0;
    ABI_GUARD_END
}

extern "C" int gpupoly_matrix_nested_rns_residues(GpuMatrix *out, const GpuMatrix *src, const uint64_t *p_moduli, size_t p_count,
                                                  size_t level_offset, size_t active_levels) {
    ABI_GUARD_BEGIN
    auto refuse = [&](const std::string &what) { return set_error("gpupoly_matrix_nested_rns_residues: " + what); };
    if (!out || !src || !p_moduli) return refuse("null argument");
    if (src->format != GPU_POLY_FORMAT_COEFF && src->format != GPU_POLY_FORMAT_EVAL) return refuse("unknown format");
    const std::string bad = unsupported_moduli(p_moduli, p_count, 1, false);
    if (!bad.empty()) return refuse(bad);
    GpuContext *ctx = src->ctx;
    if (out->ctx != ctx) return refuse("context mismatch");
    if (out->level != src->level) return refuse("level mismatch");
    const size_t Lm = matrix_limbs(src), D = p_count, A = active_levels;
    if (A == 0) return refuse("active_levels must be at least 1");
    if (level_offset > Lm || A > Lm - level_offset) return refuse("the window leaves the matrix's limbs");
    if (out->cols != src->cols || out->rows != src->rows * A * D) return refuse("shape mismatch (out must be rows * active_levels * p_count x cols)");
    if (storage_overlaps(out, src)) return refuse("the output overlaps the source");
    if (matrix_polys(src) == 0) {
        out->format = GPU_POLY_FORMAT_COEFF;
        return 0;
    }
    if (ctx_activate(ctx)) return 1;
    const Window wn = {D, Lm, level_offset, A, 1, p_moduli};
    CtxBlock coeff_scratch(ctx);
    const void *s = nullptr;
    int rcode = coeff_domain_source(src, coeff_scratch, &s);
    if (rcode) return rcode;
    void *o = words_ptr(out);
    rcode = ctx->wide ? residues<uint64_t>(ctx, static_cast<uint64_t *>(o), static_cast<const uint64_t *>(s), wn, matrix_polys(src), src->cols)
                      : residues<uint32_t>(ctx, static_cast<uint32_t *>(o), static_cast<const uint32_t *>(s), wn, matrix_polys(src), src->cols);
    if (rcode) return rcode;
    out->format = GPU_POLY_FORMAT_COEFF;  // residues of coefficients: the coefficient domain
    return 0;
    ABI_GUARD_END
}
