"""The LargeScalarMul gate, lhs * G^-1(G_d o c), from its structure, in exact Python integers.

Entry (j, (j, t, e)) of G_d o c is c * B^e in limb t (B = 2^base_bits) and 0 in every other limb, and digits are taken per
tower, so G^-1(G_d o c) = I_d (x) blockdiag_t(D_t): D_t[e'][e] is the polynomial whose coefficient i is digit e' of
(c_t[i] * B^e mod q_t), the same small integer in every limb, and

    out[i, (j, t, e)] = sum_{e' < dpt} lhs[i, (j, t, e')] * D_t[e'][e]        (every limb, every slot).

Nothing here shares code with the kernels or with oracle/: the digits are cut with Python's own shifts, the transform of a
digit polynomial is plainref's Horner evaluation.  Layouts are the library's: (rows, cols, L, n) residues."""
import numpy as np

import plainref as PR


_roots = {}  # (q, n) -> plainref.min_root


def digit(v: int, ep: int, base: int, width: int) -> int:
    """digit ep of v in base 2^base, cut at `width` bits (the last digit of a tower keeps width - (dpt - 1) base bits)"""
    lo = ep * base
    hi = min(lo + base, width)
    return 0 if hi <= lo else (int(v) >> lo) & ((1 << (hi - lo)) - 1)


def const_digits(C: int, moduli, base: int, dpt: int) -> list:
    """delta[t][e'][e] = digit e' of (C B^e mod q_t): the constant D_t[e'][e] of a constant polynomial C"""
    out = []
    for q in moduli:
        q = int(q)
        out.append([[digit(C * (1 << (base * e)) % q, ep, base, q.bit_length()) for e in range(dpt)] for ep in range(dpt)])
    return out


def digit_polys(c_coeff, moduli, base: int, dpt: int) -> list:
    """D[t][e'][e] = the n integer coefficients of D_t[e'][e] for c given by its COEFF residues (L, n)"""
    out = []
    for t, q in enumerate(moduli):
        q = int(q)
        ct = [int(v) for v in c_coeff[t]]
        out.append([[[digit(v * (1 << (base * e)) % q, ep, base, q.bit_length()) for v in ct] for e in range(dpt)] for ep in range(dpt)])
    return out


def mul_const(lhs, C: int, moduli, base: int, dpt: int) -> np.ndarray:
    """lhs * G^-1(G o C) for the constant C, every word: lhs is (rows, d k, L, n) EVAL residues"""
    rows, cols, L, n = lhs.shape
    k = dpt * L
    assert cols % k == 0 and L == len(moduli)
    delta = const_digits(C, moduli, base, dpt)
    x = lhs.astype(object)
    out = np.zeros(lhs.shape, dtype=object)
    for col in range(cols):
        j, loc = divmod(col, k)
        t, e = divmod(loc, dpt)
        for l in range(L):
            acc = 0
            for ep in range(dpt):
                acc = acc + x[:, j * k + t * dpt + ep, l, :] * delta[t][ep][e]
            out[:, col, l, :] = acc % int(moduli[l])
    return out.astype(np.uint64)


def mul_scalar_entries(lhs, c_coeff, moduli, base: int, dpt: int, entries, slots) -> dict:
    """{(i, col, l): [slot values]} of lhs * G^-1(G o c) for the chosen entries (i, col) and slots, c by its COEFF residues"""
    rows, cols, L, n = lhs.shape
    k = dpt * L
    D = digit_polys(c_coeff, moduli, base, dpt)
    out = {}
    for (i, col) in entries:
        j, loc = divmod(col, k)
        t, e = divmod(loc, dpt)
        for l in range(L):
            q = int(moduli[l])
            acc = [0] * len(slots)
            for ep in range(dpt):
                poly = np.array([[v % q for v in D[t][ep][e]]], dtype=np.uint64)
                if (q, n) not in _roots:
                    _roots[(q, n)] = PR.min_root(q, n)
                ev = PR.ntt_slots(poly, [q], slots, roots=[_roots[(q, n)]])[0]
                for a, s in enumerate(slots):
                    acc[a] += int(lhs[i, j * k + t * dpt + ep, l, s]) * int(ev[a])
            out[(i, col, l)] = [v % q for v in acc]
    return out


def restatement(oracle, lhs, c_eval, moduli, base: int):
    """oracle.matmul(lhs, matrix_ntt(decompose(matrix_ntt(G o c, inverse)))) and the decomposition (EVAL) it multiplied by:
    the reference's own sequence on the CPU.  c_eval: (1, 1, L, n) EVAL residues."""
    rows, cols, L, n = lhs.shape
    k = oracle.digits_per_tower(moduli, base) * L
    d = cols // k
    g = oracle.gadget_matrix(d, moduli, n, base)
    gc = oracle.pointwise("mul", g, c_eval, moduli)
    dec = oracle.matrix_ntt(oracle.decompose(oracle.matrix_ntt(gc, moduli, inverse=True), moduli, base), moduli)
    return oracle.matmul(lhs, dec, moduli), dec


def const_eval(C: int, moduli, n: int) -> np.ndarray:
    """the constant polynomial C in EVAL form: C mod q_l in every slot"""
    out = np.zeros((1, 1, len(moduli), n), dtype=np.uint64)
    for l, q in enumerate(moduli):
        out[0, 0, l, :] = int(C) % int(q)
    return out
