"""Plain big-integer reference of the ring operations, written from their definitions.

Shares no code with the kernels (mxx_amd/csrc) or the CPU oracle (oracle/): it imports only the standard library
and numpy, and every function restates the mathematical definition of its operation - no butterflies, no
Barrett or Shoup forms, no lazy bounds.  It is slow on purpose; callers sample slots and coefficients at large n.

Layout conventions match the library's: a ring element of L towers is an (L, n) array of residues.
"""
from __future__ import annotations

import numpy as np

_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)  # deterministic for every n < 3.3e24


def is_prime(q: int) -> bool:
    """Miller-Rabin with the first twelve prime bases: exact below 2^64."""
    if q < 2:
        return False
    for b in _MR_BASES:
        if q % b == 0:
            return q == b
    d, s = q - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for b in _MR_BASES:
        x = pow(b, d, q)
        if x in (1, q - 1):
            continue
        for _ in range(s - 1):
            x = x * x % q
            if x == q - 1:
                break
        else:
            return False
    return True


# ---------------------------------------------------------------------------------------------- primes and roots
def primes(n: int, bits: int, count: int, low: bool = False) -> list:
    """`count` primes q = 1 (mod 2n) of exactly `bits` bits: the largest ones (descending), or with `low` the
    smallest ones above 2^(bits-1) (ascending)."""
    m = 2 * n
    lo, hi = 1 << (bits - 1), 1 << bits
    out = []
    if low:
        q = lo + 1 + (-lo) % m  # smallest q > 2^(bits-1) with q = 1 (mod m)
        step = m
    else:
        q = hi - 1 - (hi - 2) % m  # largest q < 2^bits with q = 1 (mod m)
        step = -m
    while lo < q < hi and len(out) < count:
        if is_prime(q):
            out.append(q)
        q += step
    if len(out) < count:
        raise ValueError(f"only {len(out)} primes = 1 mod {m} of {bits} bits")
    return out


def min_root(q: int, n: int) -> int:
    """Smallest primitive 2n-th root of unity mod q (n a power of two, 2n | q - 1).

    x is a primitive 2n-th root iff x^n = -1.  One such root r is found by raising successive candidates to
    (q - 1) / 2n; every primitive 2n-th root is an odd power of r, so the minimum is searched over those."""
    assert n & (n - 1) == 0 and (q - 1) % (2 * n) == 0
    e = (q - 1) // (2 * n)
    for g in range(2, q):
        r = pow(g, e, q)
        if pow(r, n, q) == q - 1:
            break
    else:
        raise ValueError("no primitive root")
    best, cur, r2 = r, r, r * r % q
    for _ in range(n - 1):
        cur = cur * r2 % q
        best = min(best, cur)
    assert pow(best, n, q) == q - 1
    return best


def bitrev(k: int, logn: int) -> int:
    return int(format(k, f"0{logn}b")[::-1], 2) if logn else 0


# ---------------------------------------------------------------------------------------------- transform
def ntt_slots(a, moduli, slots, roots=None) -> np.ndarray:
    """Slots of the forward transform of the (L, n) coefficient array `a`: slot k of tower l is
    a_l(psi_l^(2 bitrev(k) + 1)) mod q_l, psi_l = min_root(q_l, n).  Horner's rule, one pass over the n
    coefficients for all chosen slots at once.  Returns an (L, len(slots)) uint64 array."""
    a = np.asarray(a)
    L, n = a.shape
    logn = n.bit_length() - 1
    roots = roots or [min_root(int(q), n) for q in moduli]
    slots = [int(k) for k in slots]
    xs = [[pow(roots[l], 2 * bitrev(k, logn) + 1, int(moduli[l])) for k in slots] for l in range(L)]
    if max(int(q) for q in moduli) < 1 << 32:
        # every intermediate acc * x + a < q^2 <= 2^64: exact in uint64
        q = np.asarray([int(v) for v in moduli], dtype=np.uint64).reshape(L, 1)
        x = np.asarray(xs, dtype=np.uint64)
        acc = np.zeros((L, len(slots)), dtype=np.uint64)
        coef = a.astype(np.uint64)
        for i in range(n - 1, -1, -1):
            acc = (acc * x + coef[:, i : i + 1]) % q
        return acc
    q = np.asarray([int(v) for v in moduli], dtype=object).reshape(L, 1)
    x = np.asarray(xs, dtype=object)
    acc = np.zeros((L, len(slots)), dtype=object)
    coef = np.asarray([[int(v) for v in row] for row in a], dtype=object)
    for i in range(n - 1, -1, -1):
        acc = (acc * x + coef[:, i : i + 1]) % q
    return np.asarray([[int(v) for v in row] for row in acc], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------- ring product
def negacyclic_coeffs(a, b, q: int, idx) -> list:
    """Coefficients `idx` of a * b in Z_q[x] / (x^n + 1), each from its defining sum
    c_k = sum_{i <= k} a_i b_(k-i) - sum_{i > k} a_i b_(n+k-i)."""
    n = len(a)
    out = []
    if q < 1 << 32:
        # vectorised over i: each product < 2^64 is reduced before the n-term sum (< n q < 2^64)
        av = np.asarray(a, dtype=np.uint64) % np.uint64(q)
        bv = np.asarray(b, dtype=np.uint64) % np.uint64(q)
        i = np.arange(n)
        for k in idx:
            k = int(k)
            terms = av * bv[(k - i) % n] % np.uint64(q)
            pos, neg = int(terms[: k + 1].sum()), int(terms[k + 1 :].sum())
            out.append((pos - neg) % q)
        return out
    ai = [int(v) for v in a]
    bi = [int(v) for v in b]
    for k in idx:
        k = int(k)
        pos = sum(ai[i] * bi[k - i] for i in range(k + 1))
        neg = sum(ai[i] * bi[n + k - i] for i in range(k + 1, n))
        out.append((pos - neg) % q)
    return out


def ring_matmul_coeffs(A, B, moduli, entries, idx) -> dict:
    """Chosen coefficients of the ring-matrix product A B, (rows, inner, L, n) x (inner, cols, L, n) coefficient
    arrays: {(r, c, l): [coefficient k for k in idx]} for every (r, c) in `entries` and every tower l."""
    inner, L = A.shape[1], A.shape[2]
    out = {}
    for r, c in entries:
        for l in range(L):
            q = int(moduli[l])
            acc = [0] * len(idx)
            for t in range(inner):
                for j, v in enumerate(negacyclic_coeffs(A[r, t, l], B[t, c, l], q, idx)):
                    acc[j] += v
            out[(r, c, l)] = [v % q for v in acc]
    return out


# ---------------------------------------------------------------------------------------------- decomposition
def digits_per_tower(moduli, base_bits: int) -> int:
    """ceil(k / b) for k = the bit width of the widest modulus."""
    k = max(int(q).bit_length() for q in moduli)
    return -(-k // base_bits)


def digits(x, moduli, base_bits: int, dpt: int) -> np.ndarray:
    """Base-2^b digits of each tower's residue.  x: (L, n) residues; returns (L * dpt, L, n): row t*dpt + d holds
    digit d of tower t's residue (the integer floor(x_t / 2^(d b)) mod 2^b, cut at bits(q_t)), reduced into every
    tower l (a digit of a wide tower can exceed a narrow modulus)."""
    x = np.asarray(x, dtype=np.uint64)
    L, n = x.shape
    out = np.zeros((L * dpt, L, n), dtype=np.uint64)
    for t in range(L):
        width = int(moduli[t]).bit_length()
        for d in range(dpt):
            lo = d * base_bits
            hi = min(lo + base_bits, width)
            if hi <= lo:
                continue  # past the tower's own width: digit 0
            dig = (x[t] >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)
            for l in range(L):
                out[t * dpt + d, l] = dig % np.uint64(int(moduli[l]))
    return out


def gadget(size: int, moduli, base_bits: int, n: int) -> np.ndarray:
    """Gadget matrix I_size (x) g in coefficient form, (size, size * L * dpt, L, n): entry (r, r*k + t*dpt + d) is
    the constant 2^(d b) in tower t and 0 in the other towers (g's CRT form: the digit of tower t only counts
    there)."""
    L = len(moduli)
    dpt = digits_per_tower(moduli, base_bits)
    k = L * dpt
    out = np.zeros((size, size * k, L, n), dtype=np.uint64)
    for r in range(size):
        for t in range(L):
            for d in range(dpt):
                out[r, r * k + t * dpt + d, t, 0] = pow(2, d * base_bits, int(moduli[t]))
    return out


def gadget_small(size: int, moduli, base_bits: int, n: int) -> np.ndarray:
    """The `small` gadget matrix I_size (x) (1, 2^b, ..., 2^((dpt-1) b)) in coefficient form, (size, size * dpt, L, n):
    entry (r, r*dpt + e) is the constant 2^(e b) mod q_l in every tower l."""
    L = len(moduli)
    dpt = digits_per_tower(moduli, base_bits)
    out = np.zeros((size, size * dpt, L, n), dtype=np.uint64)
    for r in range(size):
        for e in range(dpt):
            for l in range(L):
                out[r, r * dpt + e, l, 0] = pow(2, e * base_bits, int(moduli[l]))
    return out


def gadget_scalar_digits(c, moduli, base_bits: int, dpt: int) -> np.ndarray:
    """G^-1(g o c) for a ring element c given as (L, n) coefficient residues: the k x k block (k = L * dpt, returned as
    (k, k, L, n) coefficient residues) whose column (t, e) holds the digits of the element that is c_t * 2^(e b) mod q_t
    in tower t and 0 in every other tower - entry t*dpt + e of g o c."""
    L, n = np.asarray(c).shape
    k = L * dpt
    out = np.zeros((k, k, L, n), dtype=np.uint64)
    for t in range(L):
        q = int(moduli[t])
        for e in range(dpt):
            elem = np.zeros((L, n), dtype=np.uint64)
            elem[t] = [int(v) * pow(2, e * base_bits, q) % q for v in c[t]]
            out[:, t * dpt + e] = digits(elem, moduli, base_bits, dpt)
    return out


# ---------------------------------------------------------------------------------------------- fused products
def slot_mul_sum(addend, lhss, rhss, moduli, negate: bool, slots=None) -> np.ndarray:
    """addend +- sum_t lhss[t] rhss[t] in the evaluation domain, slot by slot:
    out[i, c, l, s] = addend[i, c, l, s] +- sum_t sum_k lhss[t][i, k, l, s] * rhss[t][k, c, l, s] mod q_l for s in `slots`
    (None: every index of the last axis).  lhss[t] is (rows, k_t, L, n), rhss[t] (k_t, cols, L, n), addend (rows, cols, L, n)
    or None (zero).  Python integers throughout; returns (rows, cols, L, len(slots)) uint64."""
    pick = (lambda a: np.asarray(a)) if slots is None else (lambda a: np.asarray(a)[..., [int(s) for s in slots]])
    q = np.asarray([int(v) for v in moduli], dtype=object).reshape(1, 1, -1, 1)
    total = None
    for lhs, rhs in zip(lhss, rhss):
        a, b = pick(lhs).astype(object), pick(rhs).astype(object)
        assert a.shape[1] == b.shape[0]
        for k in range(a.shape[1]):
            term = a[:, k, None] * b[None, k]
            total = term if total is None else total + term
    if addend is None:
        assert total is not None, "no operand to take the shape from"
        base = np.zeros(total.shape, dtype=object)
    else:
        base = pick(addend).astype(object)
    if total is None:
        total = np.zeros(base.shape, dtype=object)
    out = (base - total) % q if negate else (base + total) % q
    return out.astype(np.uint64)


def monomial_mul(a, shift: int, q) -> np.ndarray:
    """a * x^shift in Z_q[x] / (x^n + 1) for shift in [0, 2n), on coefficient residues (..., n): coefficient i goes to
    position i + shift, and every pass over x^n changes its sign.  q: an integer, or an array that broadcasts against
    a (one modulus per tower as an (L, 1) column)."""
    a = np.asarray(a, dtype=np.uint64)
    n = a.shape[-1]
    assert 0 <= shift < 2 * n
    qv = np.asarray(q, dtype=np.uint64)  # residues and moduli are below 2^62: q - a stays in uint64
    dst = np.arange(n) + int(shift)
    signed = np.where((dst // n) % 2 == 1, (qv - a) % qv, a)
    out = np.empty_like(a)
    out[..., dst % n] = signed
    return out


# ---------------------------------------------------------------------------------------------- wire format
def centred_crt(residues, moduli) -> int:
    """The integer x in (-Q/2, Q/2] with x = residues[l] (mod moduli[l]) for every l, Q = prod(moduli)."""
    Q = 1
    for q in moduli:
        Q *= int(q)
    x = 0
    for r, q in zip(residues, moduli):
        q = int(q)
        Qi = Q // q
        x += int(r) * Qi * pow(Qi, -1, q)
    x %= Q
    return x - Q if x > Q // 2 else x


def compact_width(values) -> int:
    """max_coeff_bits: 1 + the largest bit length of |x| (a sign bit), 0 when every value is 0."""
    w = max((abs(int(v)).bit_length() for v in values), default=0)
    return w + 1 if w else 0


def compact_pack(values, w: int) -> bytes:
    """Little-endian bit stream: value j occupies bits [j w, (j+1) w), |x| in its low w - 1 bits and the sign
    (1 = negative) in bit w - 1; ceil(len * w / 8) bytes."""
    if w == 0:
        return b""
    bits = []  # fields written most significant bit first, value 0 last: one int() over the whole stream
    for v in reversed(values):
        v = int(v)
        field = abs(v) | ((1 << (w - 1)) if v < 0 else 0)
        assert field >> w == 0
        bits.append(format(field, f"0{w}b"))
    return int("".join(bits), 2).to_bytes((len(values) * w + 7) // 8, "little")


def modulus_switch(c: int, Q: int, new_modulus: int) -> int:
    """floor(c * new_modulus / Q) mod new_modulus for c in [0, Q)."""
    return (c * new_modulus // Q) % new_modulus
