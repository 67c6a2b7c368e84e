"""CPU-only: the plain big-integer reference (tests/plainref.py) and the CPU oracle (oracle/) agree on every
modulus width class the library dispatches on, including widths and prime positions the oracle had never seen.

The two are independent restatements: plainref evaluates each definition directly (Horner per slot, the defining
sum per coefficient, Python-int CRT), the oracle runs butterflies and packed reductions.  Agreement here is what
lets tests/test_gpu_modulus_classes.py hold the kernels to plainref alone.
"""
import numpy as np
import pytest

import plainref as P
from oracle import oracle as O
from test_oracle import SURVEY_A1

# every width class boundary of the kernels' dispatch (mxx_amd/csrc/runtime.hip, ntt_lds_u64.hip, modarith.h)
WIDTHS = [10, 12, 15, 24, 25, 26, 28, 29, 31, 32, 33, 40, 41, 51, 52, 57, 58, 61, 62]


def _patterns(moduli, n, seed):
    """(P, L, n) inputs: random, all q - 1, alternating 0 / q - 1, a spike at n - 1."""
    rng = np.random.default_rng(seed)
    top = np.asarray(moduli, dtype=np.uint64).reshape(-1, 1) - np.uint64(1)
    rand = np.stack([rng.integers(0, int(q), n, dtype=np.uint64) for q in moduli])
    full = np.broadcast_to(top, (len(moduli), n)).copy()
    alt = full.copy()
    alt[:, 1::2] = 0
    spike = np.zeros_like(full)
    spike[:, n - 1] = top[:, 0]
    return np.stack([rand, full, alt, spike])


@pytest.mark.parametrize("key", list(SURVEY_A1))
def test_primes_reproduce_the_survey_bases(key):
    n, depth, bits = key
    assert P.primes(n, bits, depth) == SURVEY_A1[key]


def test_primes_reference_held_datum():
    assert P.primes(4, 17, 2) == [131041, 131009]


@pytest.mark.parametrize("bits", WIDTHS)
def test_primes_both_ends_of_the_class(bits):
    n = 4 if bits <= 12 else 256
    hi = P.primes(n, bits, 2)
    lo = P.primes(n, bits, 2, low=True)
    assert hi == O.gen_crt_basis(n, 2, bits)
    for q in hi + lo:
        assert q.bit_length() == bits and (q - 1) % (2 * n) == 0 and O.lib().orc_is_prime(q)
    # nothing skipped: no prime of the progression lies between 2^(bits-1) and the smallest one found
    assert all(not P.is_prime(q) for q in range((1 << (bits - 1)) + 1, lo[0], 2 * n))
    assert lo[0] < lo[1] and hi[0] > hi[1]


@pytest.mark.parametrize("low", [False, True])
@pytest.mark.parametrize("bits", WIDTHS)
def test_transform_matches_oracle_all_slots(bits, low):
    """Every slot of n = 4 and n = 32 (n = 2 and 4 at 10 bits, where 2n must divide q - 1 below 2^10)."""
    for n in ((2, 4) if bits <= 10 else (4, 32)):
        moduli = P.primes(n, bits, 2, low=low)
        for q in moduli:
            assert P.min_root(q, n) == O.min_primitive_root(q, 2 * n)
        pats = _patterns(moduli, n, bits * 7 + n)
        for x in pats:
            got = P.ntt_slots(x, moduli, range(n))
            for l, q in enumerate(moduli):
                assert np.array_equal(got[l], O.ntt_vec(x[l], q)), (bits, low, n, l)
                # the inverse: the oracle's inverse lands on a vector whose forward definition is x again
                inv = O.ntt_vec(x[l], q, inverse=True)
                assert np.array_equal(P.ntt_slots(inv[None], [q], range(n))[0], x[l])


@pytest.mark.parametrize("bits,low", [(24, True), (15, False), (51, False), (61, True)])
def test_transform_matches_oracle_sampled_slots_n16384(bits, low):
    n = 1 << 9 if bits == 15 else 1 << 14  # 2n | q - 1 leaves two 15-bit primes up to n = 512
    moduli = P.primes(n, bits, 2, low=low)
    x = _patterns(moduli, n, 99 + bits)[0]
    slots = sorted({0, 1, n - 1} | set(np.random.default_rng(bits).integers(0, n, 9).tolist()))
    got = P.ntt_slots(x, moduli, slots)
    for l, q in enumerate(moduli):
        assert np.array_equal(got[l], O.ntt_vec(x[l], q)[slots])


@pytest.mark.parametrize("bits", [12, 15, 26, 31, 32, 41, 58, 61])
def test_negacyclic_product_matches_oracle_schoolbook(bits):
    n = 16
    for low in (False, True):
        moduli = P.primes(n, bits, 2, low=low)
        pats = _patterns(moduli, n, bits)
        for l, q in enumerate(moduli):
            for a, b in ((pats[0, l], pats[1, l]), (pats[1, l], pats[1, l]), (pats[2, l], pats[3, l])):
                want = O.negacyclic_schoolbook(a, b, q)
                assert P.negacyclic_coeffs(a, b, q, range(n)) == [int(v) for v in want]


@pytest.mark.parametrize("moduli_spec,base", [
    (("hi", 24, 2), 12), (("lo", 24, 2), 12), (("hi", 17, 2), 15), (("hi", 15, 2), 13), (("hi", 12, 2), 12),
    (("hi", 28, 2), 14), (("hi", 32, 2), 16), (("lo", 33, 2), 11), (("hi", 61, 2), 20), (("hi", 10, 2), 5),
    (("mixed", (24, 12)), 12), (("mixed", (51, 33)), 17),
])
def test_decompose_and_gadget_match_oracle(moduli_spec, base):
    """Digits per tower, the short last digit (17 / 15, 15 / 13), one digit per tower (12 / 12) and mixed widths
    (the narrow tower's digits end at its own width; a wide tower's digit can exceed the narrow modulus)."""
    n = 4
    if moduli_spec[0] == "mixed":
        moduli = [P.primes(n, moduli_spec[1][0], 1)[0], P.primes(n, moduli_spec[1][1], 1)[0]]
    else:
        moduli = P.primes(n, moduli_spec[1], moduli_spec[2], low=moduli_spec[0] == "lo")
    dpt = P.digits_per_tower(moduli, base)
    assert dpt == O.digits_per_tower(moduli, base)
    M = _patterns(moduli, n, base)  # (4, L, n): a 4 x 1 matrix
    want = O.decompose(M[:, None], moduli, base)
    for r in range(M.shape[0]):
        got = P.digits(M[r], moduli, base, dpt)
        assert np.array_equal(got, want[r * len(moduli) * dpt : (r + 1) * len(moduli) * dpt, 0]), r
    assert np.array_equal(P.gadget(2, moduli, base, n), O.gadget_matrix(2, moduli, n, base, eval_format=False))


@pytest.mark.parametrize("spec", [(4, 10, 2), (8, 12, 3), (16, 24, 3), (16, 31, 2), (16, 32, 3), (8, 51, 2), (8, 61, 3)])
def test_compact_payload_matches_oracle(spec):
    n, bits, depth = spec
    moduli = P.primes(n, bits, depth)
    Q = int(np.prod([q for q in moduli], dtype=object))
    # every fast-path boundary of the device store: +-floor(q0/2), +-(floor(q0/2)+1), the same for q0 q1, +-floor(Q/2)
    h0, h01 = moduli[0] // 2, moduli[0] * moduli[1] // 2
    vals = [0, 1, -1, h0, -h0, h0 + 1, -(h0 + 1), h01, -h01, h01 + 1, -(h01 + 1), Q // 2, -(Q // 2)]  # Q is odd
    vals = [v for v in vals if abs(v) <= Q // 2]  # at depth 2, q0 q1 = Q
    vals += [0] * (-len(vals) % n)
    res = np.asarray([[[[v % q for v in vals[i * n:(i + 1) * n]] for q in moduli] for i in range(len(vals) // n)]],
                     dtype=np.uint64)
    for v in vals:
        assert P.centred_crt([v % q for q in moduli], moduli) == v
    payload, w, bpc = O.compact_payload(res, moduli)
    assert w == P.compact_width(vals) and bpc == (w + 7) // 8
    assert P.compact_pack(vals, w) == payload
    c = Q // 3
    assert P.modulus_switch(c, Q, 1 << 20) == (c << 20) // Q


# ---------------------------------------------------------------------------------------------- fused operations
# plainref's definitions of the fused products (slot_mul_sum, monomial_mul, gadget_small, gadget_scalar_digits) against
# the oracle's restatement of the same operation, composed there from O.matmul, O.pointwise, O.ntt_vec, O.matrix_ntt,
# O.gadget_matrix and O.decompose where the oracle has no entry of its own.  tests/test_gpu_fused_width_classes.py holds
# the kernels to plainref alone.
def _fused_rings(bits, low):
    """(n, moduli) of one class: n = 4 and 32 (2 and 4 at 10 bits); bits = "mixed": a 51-bit and a low 12-bit limb."""
    if bits == "mixed":
        return [(n, [P.primes(n, 51, 1)[0], P.primes(n, 12, 1, low=True)[0]]) for n in (4, 32)]
    return [(n, P.primes(n, bits, 2, low=low)) for n in ((2, 4) if bits <= 10 else (4, 32))]


def _rand(rng, shape, moduli):
    """(shape[0], shape[1], L, n) residues"""
    return np.stack([rng.integers(0, int(q), shape, dtype=np.uint64) for q in moduli], axis=2)


FUSED_CLASSES = [(b, low) for b in WIDTHS for low in (False, True)] + [("mixed", False)]


@pytest.mark.parametrize("bits,low", FUSED_CLASSES)
def test_slot_mul_sum_matches_oracle(bits, low):
    for n, moduli in _fused_rings(bits, low):
        rng = np.random.default_rng(n + 31 * len(moduli) + (bits if bits != "mixed" else 99))
        top = np.asarray(moduli, dtype=np.uint64).reshape(-1, 1) - np.uint64(1)
        lhss = [_rand(rng, (2, k, n), moduli) for k in (1, 4, 2)]
        rhss = [_rand(rng, (k, 3, n), moduli) for k in (1, 4, 2)]
        lhss[1][:, 1:3] = top  # (q - 1)^2 products, two in a row
        rhss[1][1:3] = top
        addend = _rand(rng, (2, 3, n), moduli)
        addend[0, 0] = top
        prod = np.zeros_like(addend)
        for a, b in zip(lhss, rhss):
            prod = O.pointwise("add", prod, O.matmul(a, b, moduli), moduli)
        for negate in (False, True):
            want = O.pointwise("sub" if negate else "add", addend, prod, moduli)
            assert np.array_equal(P.slot_mul_sum(addend, lhss, rhss, moduli, negate), want)
            zero = np.zeros_like(addend)
            assert np.array_equal(P.slot_mul_sum(None, lhss, rhss, moduli, negate), O.pointwise("sub" if negate else "add", zero, prod, moduli))
        slots = [0, n - 1]
        assert np.array_equal(P.slot_mul_sum(addend, lhss, rhss, moduli, True, slots), O.pointwise("sub", addend, prod, moduli)[..., slots])
        assert np.array_equal(P.slot_mul_sum(addend, [], [], moduli, True), addend)


@pytest.mark.parametrize("bits,low", FUSED_CLASSES)
def test_monomial_mul_matches_oracle(bits, low):
    """a * x^s is the negacyclic product with the one-hot +-x^(s mod n), and slot by slot the product with its transform."""
    for n, moduli in _fused_rings(bits, low):
        pats = _patterns(moduli, n, 5 * n + len(moduli))
        for l, q in enumerate(moduli):
            for s in sorted({0, 1, n - 1, n, n + 1, 2 * n - 1, (3 * n) // 2}):
                mono = np.zeros(n, dtype=np.uint64)
                mono[s % n] = 1 if s < n else q - 1
                assert np.array_equal(P.monomial_mul(np.asarray([1] + [0] * (n - 1)), s, q), mono)
                for a in pats[:, l]:
                    got = P.monomial_mul(a, s, q)
                    assert np.array_equal(got, O.negacyclic_schoolbook(a, mono, q)), (bits, low, n, l, s)
                    slotwise = [int(x) * int(f) % q for x, f in zip(O.ntt_vec(a, q), O.ntt_vec(mono, q))]
                    assert [int(v) for v in O.ntt_vec(got, q)] == slotwise
        # every tower at once, one modulus per row
        col = np.asarray(moduli, dtype=np.uint64).reshape(-1, 1)
        assert np.array_equal(P.monomial_mul(pats[0], n + 1, col), np.stack([P.monomial_mul(pats[0, l], n + 1, q) for l, q in enumerate(moduli)]))


def _fused_bases(moduli):
    """two digits per tower, and a smaller base whose last digit is short where the width allows one"""
    width = max(int(q).bit_length() for q in moduli)
    return sorted({(width + 1) // 2, width // 3 + 1, max(width // 5, 1) + 1})


@pytest.mark.parametrize("bits,low", FUSED_CLASSES)
def test_gadget_small_and_scalar_digits_match_oracle(bits, low):
    for n, moduli in _fused_rings(bits, low):
        L = len(moduli)
        pats = _patterns(moduli, n, 3 * n + L)
        for base in _fused_bases(moduli):
            dpt = P.digits_per_tower(moduli, base)
            k = L * dpt
            assert np.array_equal(P.gadget_small(2, moduli, base, n), O.gadget_matrix(2, moduli, n, base, small=True, eval_format=False))
            g_eval = O.gadget_matrix(1, moduli, n, base)  # 1 x k, evaluation domain
            for c in pats:
                c_eval = O.matrix_ntt(c[None, None], moduli)
                gc = O.matrix_ntt(O.pointwise("mul", g_eval, c_eval, moduli), moduli, inverse=True)  # g o c, coefficients
                want = O.decompose(gc, moduli, base)
                assert want.shape == (k, k, L, n)
                assert np.array_equal(P.gadget_scalar_digits(c, moduli, base, dpt), want), (bits, low, n, base)
