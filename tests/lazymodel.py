"""Word-exact CPU model of the lazy (redundant-form) transform kernels, with the peak of every intermediate.

Each transform family keeps its values in redundant form between reductions, and its correctness rests on a bound
written next to the kernel.  This module restates the arithmetic and the fold schedule each kernel runs, word for
word, and reports two numbers per run:

- `value`: the largest intermediate the given input produces, as a fraction of the word limit (2^W for unsigned
  words, 2^31 for the signed 32-bit form, 2^53 for doubles), and where it occurred (stage, element);
- `bound`: the analytical worst case over the same schedule - every operation's proven output range propagated
  element by element, independent of the input - as a fraction of the same limit.

A value at or past 1.0 means a register would wrap (or a double round) on a real GPU; the model then keeps computing
what the kernel computes (wrapped words, rounded doubles), so its residues show the wrong answer the kernel would give.
Threshold-bearing quantities (word size, the gs_exp_after cap, TIGHT prefolds, ELIM) are arguments, so a schedule can
be evaluated at a shifted threshold.

Sources restated (mxx_amd/csrc, line numbers as of this model; a change there must be mirrored here):
- ntt_lds.h: csub :37, fold_2q :86, mont_mul_lazy :102-106 (MULW load :474), ct_network_lazy :111-128 (forward Shoup
  butterfly), kTightCap = 4 :135 and ct_prefold :137-145 (TIGHT), gs_exp_after :152-163, gs_stage_lazy :169-199 and
  gs_fold :218-225 (inverse, cap), smul_lazy :238-241, gs_network_signed :250-274 and gs_fold_signed :278-283 (signed
  inverse), NttLdsCfg :286-291 (three passes), ntt_fwd_lazy_body :311-369 and ntt_inv_lazy_kernel :441-531 (pass
  order, prefolds, folds at pass ends), ntt_fwd_head_kernel :540-558 and ntt_inv_tail_kernel :605-623 (beyond LDS).
- ntt14.h: fwd_body :68-192 (register pass of 5 stages :85, block passes of 3 with prefolds :104-138), inv_kernel
  :307-420 (SGN folds (0,2) :370, (2,3) :387, (3,1) :402; register pass with N^-1 :416-419).
- ntt_f64.h: kFolded = 2 :31, mulmod :33-38, fold :39, fwd_next / inv_next :42-43, CtStages :47-71, GsStages :75-102,
  to_residue :104-109, small_kernel :123-180, fwd_body :186-238, head_kernel :256-307, inv_kernel :328-391,
  tail_kernel :396-412.
- ntt_rings.h: visit_ring (the ring table: pass split per ring size and word size), launch_ntt14, launch_split,
  launch_ntt_lds.  ntt_lds_u32.hip: launch_mul_intt_u32.  ntt_lds_u64.hip: launch_ntt_lds_u64 (the small kernel below
  2^10 first, then the same table), by_elim (ELIM by the widest modulus, 40 / 49 bits).
- runtime.hip: Shoup companions floor(w 2^W / q) :414, centred signed twiddles :467-474, lazy_ok `+ 7` :620,
  tight_ok `+ 4` :621, signed_ok `<= 24` :622, the 2^32 of the MULW N^-1 constants :640-646.

The worst-case inputs (candidates) reach the proven bound only for the double-precision inverse and the TIGHT
inverse; the double-precision forward construction reaches 0.50 of 2^53 against a proven 0.875.  For the other
integer forms they reach no further than all q - 1 and the alternating patterns they include (the forward's growth
hides in Shoup remainders no residue condition controls).  Where the vectors fall short, the shifts are settled by
the propagated bound, not by the vectors.

Only numpy and the standard library; twiddle tables are rebuilt from tests/plainref.py's min_root.
"""
from functools import lru_cache

import numpy as np

import plainref as P

F64_LIMIT = 1 << 53
KFOLDED = 2  # ntt_f64.h kFolded: bound after a fold, units of q / 4
TIGHT_CAP = 4  # ntt_lds.h kTightCap
U = 2.0 ** -53  # unit roundoff of a double


# ---------------------------------------------------------------------------------------------- tables, schedules
@lru_cache(maxsize=256)
def min_root(q: int, n: int) -> int:
    return P.min_root(q, n)


@lru_cache(maxsize=64)
def tables(q: int, n: int):
    """Forward / inverse twiddles in the kernels' bit-reversed layout: fwd[bitrev(i)] = psi^i, inv[bitrev(i)] = psi^-i
    (runtime.hip, gpu_context_create)."""
    logn = n.bit_length() - 1
    psi = min_root(q, n)
    ipsi = pow(psi, -1, q)
    fwd, inv = [0] * n, [0] * n
    p = ip = 1
    for i in range(n):
        r = P.bitrev(i, logn)
        fwd[r], inv[r] = p, ip
        p, ip = p * psi % q, ip * ipsi % q
    return tuple(fwd), tuple(inv)


def _lds_split(logn, logr):
    clast = logn - 2 * logr  # NttLdsCfg: P = 3 passes
    assert 1 <= clast <= logr, (logn, logr)
    return logr, clast


def int_schedule(W: int, logn: int, ntt14: str = "grouped"):
    """Pass split of the integer lazy kernels (ntt_rings.h visit_ring / launch_ntt14 /
    launch_split).  Returns (name, forward passes [(stages, prefold)] from stage 0 up, inverse passes [stages] from
    stage logn - 1 down).  `ntt14`: "grouped" (ntt14.h) or "whole" (MXX_HIP_NTT14=whole, and every 64-bit 2^14)."""
    if logn == 14 and W == 32 and ntt14 != "whole":
        return "ntt14", [(5, False), (3, True), (3, True), (3, True)], [3, 3, 3, 5]
    split = {(32, 16): (12, 4, 4), (32, 17): (12, 4, 5), (64, 15): (11, 4, 4), (64, 16): (12, 4, 4), (64, 17): (12, 4, 5)}
    if (W, logn) in split:
        sub, logr, pre = split[(W, logn)]
        logr, clast = _lds_split(sub, logr)
        # head: PRE stages, no prefold; the sub-vector kernel's pass 0 prefolds (the head leaves (1 + 2 PRE) q)
        return "split", [(pre, False), (logr, True), (logr, True), (clast, True)], [clast, logr, logr, pre]
    logr = {10: 4, 11: 4, 12: 4, 13: 5, 14: 5, 15: 5}[logn]
    if W == 64 and logn == 15:
        raise ValueError("64-bit 2^15 is a split size")
    logr, clast = _lds_split(logn, logr)
    return "lds", [(logr, False), (logr, True), (clast, True)], [clast, logr, logr]


def f64_elim(bits: int) -> int:
    """ntt_lds_u64.hip by_elim: the fold schedule by the widest modulus."""
    return 4095 if bits <= 40 else 63 if bits <= 49 else 15


def f64_schedule(logn: int):
    """ntt_rings.h visit_ring, 64-bit column (ntt_lds_u64.hip launch_ntt_lds_u64): (name, sub-vector log size, LOGR,
    PRE); "small" below 2^10."""
    if logn < 10:
        return "small", logn, 0, 0
    if logn >= 15:
        sub, logr, pre = {15: (11, 4, 4), 16: (12, 4, 4), 17: (12, 4, 5)}[logn]
        return "split", sub, logr, pre
    return "lds", logn, {10: 4, 11: 4, 12: 4, 13: 5, 14: 5}[logn], 0


def fwd_next(e: int) -> int:  # ntt_f64.h
    return e + 2 + (e + 1) // 2


def inv_next(e: int) -> int:  # ntt_f64.h
    return 2 * e


# ---------------------------------------------------------------------------------------------- peak bookkeeping
class Peak:
    """Largest intermediate (value) and largest proven bound (bound) as fractions of `limit`."""

    def __init__(self, limit, q):
        self.limit, self.q = limit, q
        self.value, self.where = 0.0, None
        self.bound, self.bwhere = 0.0, None
        self.bound_units = 0.0  # the largest bound in units of q: bound_exact() compares it with the limit exactly

    def see(self, true, stage, idx, bound_units=None):
        """`true`: exact (unwrapped) values at element positions `idx` (same trailing shape); `bound_units`: their
        proven bound in units of q (absolute value)."""
        a = np.abs(np.asarray(true))
        if a.size:
            k = int(np.argmax(a.reshape(-1)))
            frac = float(a.reshape(-1)[k]) / self.limit
            if frac > self.value:
                ix = np.broadcast_to(idx, a.shape).reshape(-1)[k]
                self.value, self.where = frac, (stage, int(ix))
        if bound_units is not None:
            b = np.asarray(bound_units, dtype=np.float64)
            k = int(np.argmax(b.reshape(-1)))
            frac = float(b.reshape(-1)[k]) * self.q / self.limit
            self.bound_units = max(self.bound_units, float(b.reshape(-1)[k]))
            if frac > self.bound:
                self.bound, self.bwhere = frac, (stage, int(np.broadcast_to(idx, b.shape).reshape(-1)[k]))

    def bound_exact(self):
        """The proven bound over the limit as a Fraction that is never below the true one: bound_units is propagated
        in float64 (sums and products of positive terms, at most ~100 roundings along any chain, each within a factor
        1 + 2^-53), so it is scaled by 1 + 2^-45 before the exact product with q (a plain float product of the two
        rounds to 1.0 near the limit)."""
        from fractions import Fraction

        return Fraction(self.bound_units) * (1 + Fraction(1, 1 << 45)) * self.q / self.limit

    def __repr__(self):
        return f"Peak(value={self.value:.4f} at {self.where}, bound={self.bound:.4f} at {self.bwhere})"


def _pairs(n, s):
    """Element indices (lo, hi) of CT stage s (t = n >> (s+1)), shaped (2^s, t); twiddle index 2^s + i per row."""
    t = n >> (s + 1)
    base = np.arange(n).reshape(1 << s, 2, t)
    return base[:, 0, :], base[:, 1, :], (1 << s) + np.arange(1 << s).reshape(-1, 1)


# ---------------------------------------------------------------------------------------------- integer lazy forms
def _words(x, W):
    return np.asarray(x, dtype=np.uint64) if W == 32 else np.asarray(x, dtype=np.uint64).astype(object)


def _const(vals, W):
    return np.asarray(vals, dtype=np.uint64) if W == 32 else np.asarray(vals, dtype=object)


def _shoup(V, w, ws, q, W):
    """V w - hi(V ws) q: the Shoup remainder (the exact value behind every lazy product), in [0, 2q) for V < 2^W."""
    return V * w - ((V * ws) >> W) * q


def _fold_2q(x, q, W):  # ntt_lds.h fold_2q: x + mulhi(x, floor(2^W / q)) (-q)
    return x - ((x * ((1 << W) // q)) >> W) * q


def _csub(x, m, W):  # ntt_lds.h csub: min(x, x - m) in W-bit words
    mask = (1 << W) - 1
    return np.minimum(x, (x + ((1 << W) - m)) & mask) if W == 32 else np.where(x >= m, x - m, x)


def int_fwd(x, q, W, passes, tight=False, peak=None):
    """ct_network_lazy over `passes` (int_schedule), TIGHT prefolds where a pass asks for them, then
    csub(fold_2q(v), q).  nT = V (-w) + hi(V ws) q is -(Shoup remainder) modulo 2^W, so A = U - nT and
    B = U + 2q + nT are U + r and U + 2q - r: the true values are formed and wrapped to W bits."""
    x = _words(x, W)
    n = x.shape[-1]
    mask = (1 << W) - 1
    fwd, _ = tables(q, n)
    ws = [(w << W) // q for w in fwd]
    pk = peak or Peak(1 << W, q)
    v = x.copy()
    b = np.full(n, 1.0)  # canonical inputs: < q
    s = 0
    for c, prefold in passes:
        if tight and prefold:  # ct_prefold<W, C, TIGHT>: < 16 q -> < 8 q (-> < 4 q for 5-stage passes)
            assert (b <= 16).all(), "TIGHT prefold input past 16 q"
            v = _csub(v, 8 * q, W)
            b = np.minimum(b, 8.0)
            if c > 4:
                v = _csub(v, 4 * q, W)
                b = np.minimum(b, 4.0)
        for _ in range(c):
            lo, hi, ti = _pairs(n, s)
            w = _const([fwd[i] for i in ti[:, 0]], W).reshape(-1, 1)
            wsv = _const([ws[i] for i in ti[:, 0]], W).reshape(-1, 1)
            Uv, Vv = v[..., lo], v[..., hi]
            r = _shoup(Vv, w, wsv, q, W)
            A, B = Uv + r, Uv + 2 * q - r
            bA = b[lo] + 2.0
            pk.see(A, s, lo, bA)
            pk.see(B, s, hi, bA)
            v = v.copy()
            v[..., lo], v[..., hi] = A & mask, B & mask
            b = b.copy()
            b[lo], b[hi] = bA, bA
            s += 1
    out = _csub(_fold_2q(v, q, W), q, W)
    return np.asarray(out, dtype=np.uint64), pk


def int_inv(x, q, W, passes, cap=31, peak=None, stop=None):
    """gs_stage_lazy over `passes` (from stage logn - 1 down; int_schedule), gs_fold after every pass but the last,
    N^-1 folded into stage 0, csub(v, q) out.  The exponent e of each element (value < 2^e q) is tracked as the kernel's
    gs_exp_after computes it at compile time: 1 at a pass start, e + 1 on the A path, 1 after a product.
    `stop`: return the words after that many passes (and their gs_fold) instead."""
    x = _words(x, W)
    n = x.shape[-1]
    mask = (1 << W) - 1
    _, inv = tables(q, n)
    ws = [(w << W) // q for w in inv]
    n_inv = pow(n, -1, q)
    last_w = inv[1 % n] * n_inv % q
    pk = peak or Peak(1 << W, q)
    v = x.copy()
    b = np.full(n, 1.0)
    s = n.bit_length() - 1
    for pi, c in enumerate(passes):
        e = np.ones(n, dtype=np.int64)
        for _ in range(c):
            s -= 1
            lo, hi, ti = _pairs(n, s)
            assert np.array_equal(e[lo], e[hi]), "gs_exp_after: partners share an exponent"
            e_prev = e[lo]
            pre = e_prev + 1 > cap
            X, Y = v[..., lo], v[..., hi]
            bX, bY = b[lo], b[hi]
            if pre.any():  # fold both inputs back to [0, 2q) first
                X = np.where(pre, _fold_2q(X, q, W), X)
                Y = np.where(pre, _fold_2q(Y, q, W), Y)
                bX, bY = np.where(pre, 2.0, bX), np.where(pre, 2.0, bY)
            e_in = np.where(pre, 1, e_prev)
            assert (bX <= 2.0 ** e_in).all() and (bY <= 2.0 ** e_in).all(), "input past its exponent bound"
            M = _const([[q << int(k) for k in row] for row in e_in], W)
            A, D = X + Y, X + M - Y
            bA, bD = bX + bY, bX + 2.0 ** e_in
            pk.see(A, s, lo, bA)
            pk.see(D, s, hi, bD)
            if W == 64 and (D < 0).any():
                pk.value = max(pk.value, 2.0)  # Y past its exponent bound: the word wraps below zero
            Aw, Dw = A & mask, D & mask
            v = v.copy()
            b = b.copy()
            if s == 0 and pi == len(passes) - 1:
                ni, nis = _const(n_inv, W), _const((n_inv << W) // q, W)
                lw, lws = _const(last_w, W), _const((last_w << W) // q, W)
                v[..., lo], v[..., hi] = _shoup(Aw, ni, nis, q, W), _shoup(Dw, lw, lws, q, W)
                b[lo], b[hi] = 2.0, 2.0
            else:
                w = _const([inv[i] for i in ti[:, 0]], W).reshape(-1, 1)
                wsv = _const([ws[i] for i in ti[:, 0]], W).reshape(-1, 1)
                v[..., lo], v[..., hi] = Aw, _shoup(Dw, w, wsv, q, W)
                b[lo], b[hi] = bA, 2.0
                e = e.copy()
                e[lo], e[hi] = e_in + 1, 1
        if pi < len(passes) - 1:  # gs_fold
            assert (b <= 2.0 ** e).all()
            v = np.where(e == 2, _csub(v, 2 * q, W), np.where(e > 2, _fold_2q(v, q, W), v))
            b = np.where(e >= 2, 2.0, b)
        if stop is not None and pi + 1 == stop:
            return np.asarray(v, dtype=np.uint64), pk
    return np.asarray(_csub(v, q, W), dtype=np.uint64), pk


# ---------------------------------------------------------------------------------------------- signed inverse (ntt14)
def _i32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _mulhi_i32(a, b):  # __mulhi(int, int): floor(a b / 2^32), both int32 (|a b| < 2^62: exact in int64)
    return (a * b) >> 32


def signed_inv14(x, q, passes=((3, 0, 2), (3, 2, 3), (3, 3, 1)), peak=None):
    """ntt14::inv_kernel<W, SGN = true>: gs_network_signed on the three block passes, each followed by
    gs_fold_signed<3, E0, KEEP> (fold where gs_exp_from(E0, u, 2) > KEEP), then the 5-stage register pass with
    A + (q << 6), D + (q << 6) into the unsigned Shoup products by N^-1.  Values are int32; the model keeps the true
    integers, checks them against 2^31 (2^32 for the shifted unsigned pair) and wraps as the kernel would.
    Bounds are intervals in units of q: smul_lazy gives (-q |D| / 2^32, q + q |D| / 2^32)."""
    x = np.asarray(x, dtype=np.int64)
    n = x.shape[-1]
    assert n == 1 << 14
    _, inv = tables(q, n)
    mu32 = (1 << 32) // q
    n_inv = pow(n, -1, q)
    last_w = inv[1] * n_inv % q
    pk = peak or Peak(1 << 31, q)
    pk_u = Peak(1 << 32, q)  # Ap, Dp: unsigned words
    ctr = np.array([c if c <= q // 2 else c - q for c in inv], dtype=np.int64)
    cws = np.array([(int(c) << 32) // q for c in ctr], dtype=np.int64)  # floor, also for negatives
    v = x.copy()
    lo_b, hi_b = np.zeros(n), np.ones(n)  # canonical: [0, q)
    s = 14

    def smul(D, bD, w, wsv):
        T = D * w - _mulhi_i32(D, wsv) * q
        r = bD * q / 2.0 ** 32
        return T, -r, 1.0 + r

    def absb(lo, hi):
        return np.maximum(np.abs(lo), np.abs(hi))

    all_passes = list(passes) + [(5, None, None)]
    for pi, (c, e0, keep) in enumerate(all_passes):
        e = np.full(n, e0 if e0 is not None else 1, dtype=np.int64)
        for _ in range(c):
            s -= 1
            lo, hi, ti = _pairs(n, s)
            X, Y = v[..., lo], v[..., hi]
            A, D = X + Y, X - Y
            lA, hA = lo_b[lo] + lo_b[hi], hi_b[lo] + hi_b[hi]
            lD, hD = lo_b[lo] - hi_b[hi], hi_b[lo] - lo_b[hi]
            pk.see(A, s, lo, absb(lA, hA))
            pk.see(D, s, hi, absb(lD, hD))
            A, D = _i32(A), _i32(D)
            v = v.copy()
            lo_b, hi_b = lo_b.copy(), hi_b.copy()
            if s == 0:
                qs = q << 6
                Ap, Dp = (A + qs) & 0xFFFFFFFF, (D + qs) & 0xFFFFFFFF
                pk_u.see(A + qs, s, lo, np.maximum(np.abs(lA + 64), np.abs(hA + 64)))
                pk_u.see(D + qs, s, hi, np.maximum(np.abs(lD + 64), np.abs(hD + 64)))
                if ((A + qs) < 0).any() or ((D + qs) < 0).any():
                    pk_u.value = max(pk_u.value, 2.0)  # a negative shifted word: the unsigned product is wrong
                if (lA + 64 < 0).any() or (lD + 64 < 0).any():
                    pk_u.bound = max(pk_u.bound, 2.0)
                v[..., lo] = _shoup(Ap.astype(object), n_inv, (n_inv << 32) // q, q, 32).astype(np.int64)
                v[..., hi] = _shoup(Dp.astype(object), last_w, (last_w << 32) // q, q, 32).astype(np.int64)
                lo_b[lo], hi_b[lo], lo_b[hi], hi_b[hi] = 0.0, 2.0, 0.0, 2.0
            else:
                w = ctr[ti[:, 0]].reshape(-1, 1)
                wsv = cws[ti[:, 0]].reshape(-1, 1)
                T, lT, hT = smul(D, absb(lD, hD), w, wsv)
                pk.see(T, s, hi, np.maximum(np.abs(lT), hT))
                v[..., lo], v[..., hi] = A, _i32(T)
                lo_b[lo], hi_b[lo] = lA, hA
                lo_b[hi], hi_b[hi] = lT, hT
                e = e.copy()
                e[lo], e[hi] = e[lo] + 1, 1
        if keep is not None:  # gs_fold_signed<3, E0, KEEP>
            f = e > keep
            F = v - _mulhi_i32(v, mu32) * q
            r = absb(lo_b, hi_b) * q / 2.0 ** 32
            pk.see(np.where(f, F, 0), s, np.arange(n), np.where(f, np.maximum(r, 1 + r), 0))
            v = np.where(f, _i32(F), v)
            lo_b, hi_b = np.where(f, -r, lo_b), np.where(f, 1 + r, hi_b)
    out = np.where(v >= q, v - q, v)  # csub(h, q)
    pk.value, pk.bound = max(pk.value, pk_u.value), max(pk.bound, pk_u.bound)
    pk.bound_units = max(pk.bound_units, pk_u.bound_units / 2)  # in terms of the 2^31 limit
    if pk_u.value >= pk.value:
        pk.where = pk_u.where
    return out.astype(np.uint64), pk


# ---------------------------------------------------------------------------------------------- double precision
_M62 = (1 << 62) - 1


def _smod62(x):  # int64 x (possibly wrapped) -> the representative in [-2^61, 2^61) of x mod 2^62
    return ((x + (1 << 61)) & _M62) - (1 << 61)


class _F64:
    """Doubles that hold integers, kept as exact int64.  mulmod is fma(-c, q, h) + l with c = rint(V wi), h = fl(V w),
    l = V w - h (ntt_f64.h): the integer V w - c q whenever it and h - c q stay below 2^53, rounded as a double
    would round otherwise (the model computes h - c q exactly modulo 2^62 and rounds it once)."""

    def __init__(self, q, peak):
        self.q, self.qd, self.qinv, self.pk = q, float(q), 1.0 / float(q), peak

    def mulmod(self, V, w, wi, bV, stage, idx):
        q = self.q
        Vd = V.astype(np.float64)
        c = np.rint(Vd * wi)
        h = Vd * w
        hm = np.fmod(h, 2.0 ** 62).astype(np.int64)
        ci = c.astype(np.int64)
        wint = np.asarray(w, dtype=np.float64).astype(np.int64)
        hc = _smod62(hm - ci * q)  # h - c q, exact (|.| < 2^61)
        l = _smod62(V * wint - hm)  # product rounding error, exact
        T = (hc.astype(np.float64) + l.astype(np.float64)).astype(np.int64)
        # |T| <= q (1/2 + |V w / q| (2u + u^2)): the quotient estimate rounds twice (wi, V wi) before rint
        bT = 0.5 + bV * q * (2 * U + U * U) * (1.0 - 1.0 / q)
        # h - c q = T - l with |l| <= ulp(|V| w) / 2: the fma is exact while that stays below 2^53
        vmax = bV * q * q
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(vmax, 1.0))) - 52)
        self.pk.see(hc, stage, idx, bT + ulp / 2.0 / q)
        self.pk.see(T, stage, idx, bT)
        return T, bT

    def add(self, a, b):
        return (a.astype(np.float64) + b.astype(np.float64)).astype(np.int64)

    def sub(self, a, b):
        return (a.astype(np.float64) - b.astype(np.float64)).astype(np.int64)

    def fold(self, x, bx):  # fma(-rint(x qinv), q, x): |.| <= q/2 + |x| (2u + u^2) / ... (units of q)
        r = np.rint(x.astype(np.float64) * self.qinv).astype(np.int64)
        f = (x - r * self.q).astype(np.float64).astype(np.int64)
        return f, 0.5 + bx * (2 * U + U * U) + U

    def residue(self, x, bx):  # to_residue
        f, _ = self.fold(x, bx)
        f = np.where(f < 0, f + self.q, f)
        f = np.where(f >= self.q, f - self.q, f)
        return f


def _ct_stage(fm, v, b, n, s, fwd, fwi):
    lo, hi, ti = _pairs(n, s)
    w = np.asarray([fwd[i] for i in ti[:, 0]], dtype=np.float64).reshape(-1, 1)
    wi = np.asarray([fwi[i] for i in ti[:, 0]], dtype=np.float64).reshape(-1, 1)
    T, bT = fm.mulmod(v[..., hi], w, wi, b[hi], s, hi)
    Uv = v[..., lo]
    A, B = fm.add(Uv, T), fm.sub(Uv, T)
    bA = b[lo] + bT
    fm.pk.see(A, s, lo, bA)
    fm.pk.see(B, s, hi, bA)
    v = v.copy()
    b = b.copy()
    v[..., lo], v[..., hi] = A, B
    b[lo], b[hi] = bA, bA
    return v, b


def _gs_stage(fm, v, b, n, s, inv, ivi, last, n_inv, last_w):
    lo, hi, ti = _pairs(n, s)
    X, Y = v[..., lo], v[..., hi]
    A, D = fm.add(X, Y), fm.sub(X, Y)
    bA = b[lo] + b[hi]
    fm.pk.see(A, s, lo, bA)
    fm.pk.see(D, s, hi, bA)
    v = v.copy()
    b = b.copy()
    if last:
        v[..., lo], b[lo] = fm.mulmod(A, np.float64(n_inv[0]), np.float64(n_inv[1]), bA, s, lo)
        v[..., hi], b[hi] = fm.mulmod(D, np.float64(last_w[0]), np.float64(last_w[1]), bA, s, hi)
    else:
        w = np.asarray([inv[i] for i in ti[:, 0]], dtype=np.float64).reshape(-1, 1)
        wi = np.asarray([ivi[i] for i in ti[:, 0]], dtype=np.float64).reshape(-1, 1)
        v[..., lo], b[lo] = A, bA
        v[..., hi], b[hi] = fm.mulmod(D, w, wi, bA, s, hi)
    return v, b


def _f64_consts(q, n):
    fwd, inv = tables(q, n)
    qd = float(q)
    fwi = [w / qd for w in fwd]
    ivi = [w / qd for w in inv]
    n_inv = pow(n, -1, q)
    lw = inv[1 % n] * n_inv % q
    return fwd, fwi, inv, ivi, (float(n_inv), n_inv / qd), (float(lw), lw / qd)


def f64_fwd(x, q, logn=None, elim=None, peak=None):
    """The double-precision forward transform the dispatcher runs for this ring (ntt_f64.h): small_kernel below 2^10
    (fold before every even stage from 2 on), otherwise head_kernel (split sizes) + fwd_body's three passes with
    CtStages folding wherever fwd_next would pass ELIM, a fold at every pass end, to_residue out."""
    x = np.asarray(x, dtype=np.int64)
    n = x.shape[-1]
    logn = n.bit_length() - 1
    elim = f64_elim(q.bit_length()) if elim is None else elim
    fwd, fwi, *_ = _f64_consts(q, n)
    pk = peak or Peak(F64_LIMIT, q)
    fm = _F64(q, pk)
    v, b = x.copy(), np.full(n, 1.0)
    name, sub, logr, pre = f64_schedule(logn)
    if name == "small":
        for s in range(logn):
            if s >= 2 and s % 2 == 0:
                v, b = fm.fold(v, b)
            v, b = _ct_stage(fm, v, b, n, s, fwd, fwi)
        return fm.residue(v, b).astype(np.uint64), pk
    clast = sub - 2 * logr
    passes = ([(pre, 4)] if pre else []) + [(logr, KFOLDED if pre else 4), (logr, KFOLDED), (clast, KFOLDED)]
    s = 0
    for pi, (c, e) in enumerate(passes):
        for _ in range(c):  # CtStages<C, K, E, ELIM>
            if fwd_next(e) > elim:
                v, b = fm.fold(v, b)
                e = KFOLDED
            assert fwd_next(e) <= elim
            v, b = _ct_stage(fm, v, b, n, s, fwd, fwi)
            e = fwd_next(e)
            s += 1
        if pi < len(passes) - 1:
            v, b = fm.fold(v, b)
    return fm.residue(v, b).astype(np.uint64), pk


def f64_inv(x, q, elim=None, peak=None):
    """Double-precision inverse (ntt_f64.h): small_kernel below 2^10 (fold before every odd stage); otherwise
    inv_kernel's contiguous pass from canonical inputs (E = 4), middle and strided passes from folded ones, a fold at
    every pass end, GsStages folding wherever inv_next would pass ELIM; tail_kernel's PRE stages at split sizes;
    N^-1 folded into stage 0's two products, to_residue out."""
    x = np.asarray(x, dtype=np.int64)
    n = x.shape[-1]
    logn = n.bit_length() - 1
    elim = f64_elim(q.bit_length()) if elim is None else elim
    _, _, inv, ivi, n_inv, last_w = _f64_consts(q, n)
    pk = peak or Peak(F64_LIMIT, q)
    fm = _F64(q, pk)
    v, b = x.copy(), np.full(n, 1.0)
    name, sub, logr, pre = f64_schedule(logn)
    if name == "small":
        for i, s in enumerate(range(logn - 1, -1, -1)):
            if i % 2 == 1:
                v, b = fm.fold(v, b)
            v, b = _gs_stage(fm, v, b, n, s, inv, ivi, s == 0, n_inv, last_w)
        return fm.residue(v, b).astype(np.uint64), pk
    clast = sub - 2 * logr
    passes = [(clast, 4), (logr, KFOLDED), (logr, KFOLDED)] + ([(pre, KFOLDED)] if pre else [])
    s = logn
    for pi, (c, e) in enumerate(passes):
        for _ in range(c):  # GsStages<C, K, E, ELIM, LAST>
            if inv_next(e) > elim:
                v, b = fm.fold(v, b)
                e = KFOLDED
            s -= 1
            v, b = _gs_stage(fm, v, b, n, s, inv, ivi, s == 0, n_inv, last_w)
            e = inv_next(e)
        if pi < len(passes) - 1:
            v, b = fm.fold(v, b)
    return fm.residue(v, b).astype(np.uint64), pk


# ---------------------------------------------------------------------------------------------- fused product load
def mont_load(a, w, q: int) -> np.ndarray:
    """What the MULW load of the fused product + inverse hands to the butterflies (ntt_lds.h:102-106 mont_mul_lazy,
    :474 and ntt14.h:362): csub(REDC(a w), q) = a w 2^-32 mod q, word for word (p = a w < q 2^32, m = p (-q^-1) mod
    2^32, (p + m q) >> 32 in [0, 2q))."""
    a = np.asarray(a, dtype=np.uint64).astype(object)
    w = np.asarray(w, dtype=np.uint64).astype(object)
    qninv = (-pow(q, -1, 1 << 32)) % (1 << 32)
    p = a * w
    m = (p & 0xFFFFFFFF) * qninv & 0xFFFFFFFF
    r = (p + m * q) >> 32
    return np.where(r >= q, r - q, r).astype(np.uint64)


def mulw_operand(c, w, q: int) -> np.ndarray:
    """The EVAL operand a with mont_load(a, w) = c: a = c 2^32 w^-1 mod q.  (The 2^32 the Montgomery product removes
    is restored only in the N^-1 constants of the last stage, runtime.hip:640-646, so a = c w^-1 would hand the
    butterflies c 2^-32 instead of c.)"""
    c = np.asarray(c, dtype=np.uint64)
    r = (1 << 32) % q
    winv = np.array([pow(int(v), -1, q) for v in np.asarray(w).reshape(-1)], dtype=object).reshape(np.shape(w))
    return ((c.astype(object) * r % q) * winv % q).astype(np.uint64)


# ---------------------------------------------------------------------------------------------- dispatch by class
def word_size(bits: int) -> int:
    return 32 if bits <= 30 else 64


def forms(bits: int, lazy_margin: int = 7, tight_margin: int = 4, signed_max: int = 24):
    """runtime.hip gpu_context_create: (lazy_ok, tight_ok, signed_ok) for a widest modulus of `bits` bits; the margins
    are arguments so that a shifted threshold can be modelled."""
    W = word_size(bits)
    lazy = bits + lazy_margin <= W
    tight = W == 32 and not lazy and bits + tight_margin <= 32
    return lazy, tight, W == 32 and bits <= signed_max


def transform(x, q, inverse, *, W=None, path="default", **shift):
    """The model of whichever lazy kernel family the library runs for one modulus (widest = q): path "default",
    "whole" / "unsigned" (MXX_HIP_NTT14) or "int" (MXX_HIP_NTT64).  Returns (residues, Peak, family name).
    `shift`: lazy_margin / tight_margin / signed_max / elim overrides (forms, f64_elim)."""
    bits = q.bit_length()
    W = W or word_size(bits)
    n = np.asarray(x).shape[-1]
    logn = n.bit_length() - 1
    elim = shift.pop("elim", None)
    lazy, tight, sgn = forms(bits, **shift)
    if W == 64 and bits <= 51 and path != "int":
        fam = "f64:" + f64_schedule(logn)[0]
        return (f64_inv(x, q, elim) if inverse else f64_fwd(x, q, elim=elim)) + (fam,)
    if not (lazy or tight) or logn < 10:
        raise ValueError("no lazy form for this modulus / ring")
    name, fp, ip = int_schedule(W, logn, "whole" if path == "whole" else "grouped")
    if inverse and name == "ntt14" and sgn and path != "unsigned" and not tight:
        return signed_inv14(x, q) + ("ntt14:signed",)
    fam = f"u{W}:{name}" + (":tight" if tight else "")
    if inverse:
        return int_inv(x, q, W, ip, TIGHT_CAP if tight else 31) + (fam,)
    return int_fwd(x, q, W, fp, tight) + (fam,)


# ---------------------------------------------------------------------------------------------- worst-case inputs
def worst_forward(q: int, n: int, f64: bool) -> np.ndarray:
    """Drives element 0 along its whole path: element 0 is the U operand of every forward stage s, and its partner
    there is element t = n >> (s+1), untouched by the earlier stages apart from multiples of q (every other input in
    its residue class mod 2t is zero).  Choosing x[t] = target * w_s^-1 (w_s = fwd[2^s]) fixes the partner product's
    residue: q - 1 for the integer forms (Shoup remainder q - 1 or 2q - 1, A grows by it), (q - 1) / 2 for doubles
    (|T| = (q-1)/2, the largest a rounded quotient leaves, and with the sign of U).  x[0] = q - 1."""
    psi = min_root(q, n)
    x = np.zeros(n, dtype=np.uint64)
    x[0] = q - 1
    target = (q - 1) // 2 if f64 else q - 1
    s = 0
    while (n >> (s + 1)) >= 1:
        w_s = pow(psi, n >> (s + 1), q)  # fwd[2^s] = psi^bitrev(2^s) = psi^(n / 2^(s+1))
        x[n >> (s + 1)] = target * pow(w_s, -1, q) % q
        s += 1
    return x


def worst_inverse(q: int, n: int, W: int, passes, cap: int = 31, seed: int = 0, tries: int = 24) -> np.ndarray:
    """The inverse's A path is pure addition, so the first pass is driven by all q - 1; the second pass's element 0
    sums, from every first-pass group, the output at one in-group index.  Groups are independent: every candidate
    vector gives each group one candidate, and each group keeps its best (a seeded search over `tries` vectors;
    the candidates mix q - 1, small values and uniform ones)."""
    rng = np.random.default_rng(seed)
    c0 = passes[0]
    g = 1 << c0
    cands = [np.full(n, q - 1, dtype=np.uint64)]
    for k in range(tries - 1):
        r = rng.integers(0, q, n, dtype=np.uint64)
        if k % 3 == 1:
            r = np.where(rng.random(n) < 0.5, np.uint64(q - 1), r).astype(np.uint64)
        cands.append(r)
    X = np.stack(cands)
    out = _first_pass_out(X, q, W, c0, cap)
    score = out.reshape(len(cands), n // g, g)[:, :, 0].astype(np.float64)  # first element of every group
    best = np.argmax(score, axis=0)
    x = X.reshape(len(cands), n // g, g)[best, np.arange(n // g)].reshape(n)
    return x.astype(np.uint64)


def _first_pass_out(X, q, W, c, cap):
    """Values the first inverse pass (its stages and its gs_fold) leaves, for a batch of inputs."""
    n = X.shape[-1]
    return int_inv(X, q, W, [c, n.bit_length() - 1 - c], cap, stop=1)[0]


def candidates(q: int, n: int, W: int, inv_passes=None, cap: int = 31, seed: int = 0, randoms: int = 2,
               tries: int = 24) -> np.ndarray:
    """The inputs the tests drive every transform with, (k, n): all q - 1, q - 1 alternating with 0 in runs of 1, 32 and
    n / 2 (the old patterns: they load one side of the inverse's butterflies and leave D = X + M - Y at its largest), the forward path constructions for both product forms, the inverse group search (integer schedules),
    and seeded uniform vectors."""
    rng = np.random.default_rng(seed)
    top = np.full(n, q - 1, dtype=np.uint64)
    rows = [top]  # all q - 1 first: the tests compare the constructions with it
    for run in sorted({1, min(32, n // 2), n // 2}):
        rows.append(np.where((np.arange(n) // run) % 2 == 1, np.uint64(0), top).astype(np.uint64))
    rows += [worst_forward(q, n, False), worst_forward(q, n, True)]
    if inv_passes is not None:
        rows.append(worst_inverse(q, n, W, inv_passes, cap, seed=seed, tries=tries))
    rows += [rng.integers(0, q, n, dtype=np.uint64) for _ in range(randoms)]
    return np.stack(rows)
