"""CPU-only: the structured formula of the LargeScalarMul gate (tests/gadget_scalar_model.py, exact Python integers) against
the reference's own sequence on the CPU restatement - oracle.matmul(lhs, matrix_ntt(decompose(matrix_ntt(G o c, inverse)))) -
on every ring the GPU tests use.  The decomposition itself is held to its claimed structure: all off-diagonal blocks zero,
I_d (x) the d = 1 decomposition; for a constant, the same value in every slot and below 2^base_bits."""
import numpy as np
import pytest

import gadget_scalar_model as GM

# (n, limbs, limb bits, base bits)
RINGS = {"n2_18bit": (2, 2, 18, 6), "n16_18bit": (16, 3, 18, 6), "n16_18bit_base7": (16, 3, 18, 7), "n16_18bit_base4": (16, 3, 18, 4),
         "n256_51bit": (256, 3, 51, 17), "n256_61bit": (256, 2, 61, 20), "n256_31bit": (256, 2, 31, 8), "n16384_24bit": (16384, 2, 24, 12)}


def setup(oracle, ring):
    n, depth, bits, base = RINGS[ring]
    moduli = oracle.gen_crt_basis(n, depth, bits)
    return n, moduli, base, oracle.digits_per_tower(moduli, base)


def constants(moduli):
    Q = 1
    for q in moduli:
        Q *= int(q)
    return [0, 1, Q - 1, (Q << 70) + 0x1234567]  # the last one: three words and more, above Q


@pytest.mark.parametrize("ring", list(RINGS))
def test_constant_scalar(oracle, ring):
    n, moduli, base, dpt = setup(oracle, ring)
    L = len(moduli)
    k = dpt * L
    d, rows = (1, 1) if n > 256 else (2, 2)
    lhs = oracle.random_matrix(900, rows, d * k, moduli, n)
    for C in constants(moduli):
        want, dec = GM.restatement(oracle, lhs, GM.const_eval(C, moduli, n), moduli, base)
        assert np.array_equal(GM.mul_const(lhs, C, moduli, base, dpt), want), C
        # the structure: I_d (x) blockdiag_t(D_t), D_t constant and below 2^base_bits
        delta = GM.const_digits(C, moduli, base, dpt)
        for r in range(d * k):
            for c in range(d * k):
                (jr, tr, ep), (jc, tc, e) = (r // k, r % k // dpt, r % dpt), (c // k, c % k // dpt, c % dpt)
                if jr != jc or tr != tc:
                    assert not dec[r, c].any(), (r, c)
                    continue
                v = delta[tr][ep][e]
                assert v < (1 << base)
                for l in range(L):
                    assert (dec[r, c, l] == v % int(moduli[l])).all(), (r, c, l)


@pytest.mark.parametrize("ring", list(RINGS))
def test_ring_element_scalar(oracle, ring):
    n, moduli, base, dpt = setup(oracle, ring)
    L = len(moduli)
    k = dpt * L
    d, rows = (1, 1) if n > 256 else (2, 2)
    lhs = oracle.random_matrix(901, rows, d * k, moduli, n)
    top = np.array([int(q) - 1 for q in moduli], dtype=np.uint64).reshape(1, 1, L, 1)
    for c_eval in (oracle.random_matrix(902, 1, 1, moduli, n), np.broadcast_to(top, (1, 1, L, n)).copy()):
        want, dec = GM.restatement(oracle, lhs, c_eval, moduli, base)
        c_coeff = oracle.matrix_ntt(c_eval, moduli, inverse=True)[0, 0]
        # off-diagonal blocks are zero and the diagonal blocks repeat the d = 1 decomposition
        for r in range(d * k):
            for c in range(d * k):
                if r // k != c // k or r % k // dpt != c % k // dpt:
                    assert not dec[r, c].any(), (r, c)
                else:
                    assert np.array_equal(dec[r, c], dec[r % k, c % k])
        entries = sorted({(0, 0), (rows - 1, d * k - 1), (rows // 2, (d * k) // 2)})
        slots = sorted({0, n - 1, n // 2})
        got = GM.mul_scalar_entries(lhs, c_coeff, moduli, base, dpt, entries, slots)
        for (i, col, l), vals in got.items():
            assert vals == [int(want[i, col, l, s]) for s in slots], (i, col, l)
