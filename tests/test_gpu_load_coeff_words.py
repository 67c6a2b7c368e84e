"""GPU: the exact coefficient load (`gpupoly_matrix_load_coeff_words`) against plain Python big integers, and the host
mirror that rides on it (`GpuDCRTPolyMatrix.from_coeff_words` / `from_coeffs` / `load_coeff_words`, `GpuDCRTPoly.from_biguints`
and everything built on it).

Expected values come from the definition alone: coefficient x, given as little-endian 64-bit words, becomes x % q_l for
every limb (src/poly/dcrt/gpu.rs:841-857), never from the library's own store.  Every width class, limb counts on both
sides of 8 / 16 / 64, rings from 2 to 2^16; per cell the values at every limb's and word's boundary, values above Q, and
the inputs that reach the kernel's lazy-accumulator bound (csrc/coeff_load.hip: residue q_l - 1 followed by S words of all
ones, S = 1, 2, 4 words per Horner step).
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261016

# (n, bits, limbs): the cells of test_gpu_scale_round.py, and 29- and 30-bit moduli: the widest that take 4 words per
# Horner step and the only width that takes 2 (csrc/coeff_load.hip)
CELLS = [
    (512, 29, 5),
    (64, 30, 3),
    (2, 10, 2),
    (16, 24, 1),
    (64, 20, 8),
    (256, 24, 9),
    (1024, 28, 16),
    (2048, 28, 17),
    (64, 31, 2),
    (128, 31, 53),
    (256, 51, 8),
    (64, 51, 9),
    (128, 57, 16),
    (32, 62, 17),
    (16, 60, 64),
    (65536, 28, 53),
]
SMALL_CELLS = [(512, 29, 5), (64, 30, 3), (2, 10, 2), (16, 24, 1), (256, 24, 9), (1024, 28, 16), (64, 31, 2), (128, 31, 53), (64, 51, 9), (32, 62, 17), (16, 60, 64)]

_PARAMS = {}


def _params(gpu, n, bits, L):
    key = (n, bits, L)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, L), 1)
    return _PARAMS[key]


def _words_of(Q):
    return -(-Q.bit_length() // 64)


def _to_words(vals, wpc, cols, k):
    """(1, cols, k, wpc) little-endian words of the values, coefficient j of entry c = vals[c * k + j]"""
    assert len(vals) == cols * k
    buf = b"".join(v.to_bytes(8 * wpc, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(1, cols, k, wpc)


def _expected(vals, moduli, cols, k, n):
    """(1, cols, L, n) residues x % q_l, coefficients at or above k zero"""
    out = np.zeros((1, cols, len(moduli), n), dtype=np.uint64)
    if k:
        arr = np.asarray(vals, dtype=object).reshape(cols, k)
        for l, q in enumerate(moduli):
            out[0, :, l, :k] = (arr % q).astype(np.uint64)
    return out


def _special_values(moduli, wpc):
    """the planted values that fit wpc words"""
    Q = math.prod(moduli)
    vals = [0, 1, Q - 1, Q, Q + 1, (1 << (64 * wpc)) - 1]
    for q in moduli:
        vals += [q - 1, q, q + 1]
    for j in range(1, wpc + 1):
        vals += [(1 << (64 * j)) - 1, 1 << (64 * j)]
    return list(dict.fromkeys(v for v in vals if v < 1 << (64 * wpc)))


def _lazy_maxima(moduli):
    """residue q - 1 after the top step, then S words of all ones (once and twice): the accumulator's maximum for S words
    per step (coeff_load.hip), for every limb.  9 words hold the largest: 62 + 2 * 256 bits."""
    vals = []
    for q in moduli:
        for S in (1, 2, 4):
            for reps in (1, 2):
                vals.append(((q - 1) << (64 * S * reps)) | ((1 << (64 * S * reps)) - 1))
    return vals


LAZY_WORDS = 9


def _fill(vals, count, bound, seed):
    rnd = random.Random(seed)
    return vals + [rnd.randrange(bound) for _ in range(count - len(vals))]


def _loads_for_cell(moduli, n, seed):
    """[(values, wpc, cols)]: (A) words(Q) words, planted values + random below Q; (B) words(Q) + 2 words, planted values +
    random over the full width; (C) the lazy maxima + random over 9 words"""
    Q = math.prod(moduli)
    wq = _words_of(Q)
    out = []
    for wpc, planted, bound in ((wq, _special_values(moduli, wq), Q),
                                (wq + 2, _special_values(moduli, wq + 2), 1 << (64 * (wq + 2))),
                                (LAZY_WORDS, _lazy_maxima(moduli), 1 << (64 * LAZY_WORDS))):
        cols = -(-(len(planted) + 8) // n)
        out.append((_fill(planted, cols * n, bound, seed + wpc), wpc, cols))
    return out


@pytest.mark.parametrize("n,bits,L", CELLS)
def test_load_matches_big_integers_coeff_and_eval(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    for vals, wpc, cols in _loads_for_cell(moduli, n, SEED + n + L):
        words = _to_words(vals, wpc, cols, n)
        want = _expected(vals, moduli, cols, n, n)
        got = M.from_coeff_words(p, words, eval_format=False)
        assert not got.is_ntt and got.level == L - 1 and got.size() == (1, cols)
        res = got.to_rns()
        bad = np.argwhere(res != want)
        assert bad.size == 0, (wpc, bad[:4], [hex(vals[int(b[1]) * n + int(b[3])]) for b in bad[:4]])
        ev = M.from_coeff_words(p, words, eval_format=True)
        ref = M.from_rns(p, want, False)
        ref.ntt_all_in_place()
        assert ev.is_ntt and np.array_equal(ev.to_rns(), ref.to_rns()), wpc


@pytest.mark.parametrize("n,bits,L", SMALL_CELLS)
def test_one_word_short_polys_and_lower_levels(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    rnd = random.Random(SEED + 3 * n + L)
    rng = np.random.default_rng(SEED + n)
    # one word per coefficient: no staging in the kernel
    vals = _fill([0, 1, (1 << 64) - 1, 1 << 63, (1 << 32) - 1, 1 << 32] + [q for q in moduli] + [q - 1 for q in moduli], 3 * n + 64, 1 << 64, SEED)[: 3 * n]
    got = M.from_coeff_words(p, _to_words(vals, 1, 3, n), eval_format=False)
    assert np.array_equal(got.to_rns(), _expected(vals, moduli, 3, n, n))
    # short polynomials over a matrix that held non-zero data: the tail comes back 0
    Q = math.prod(moduli)
    for wpc in (1, _words_of(Q) + 1):
        for k in sorted({0, 1, n - 1, n}):
            junk = np.stack([rng.integers(1, q, size=(2, n), dtype=np.uint64) for q in moduli], axis=1)[None]
            m = M.from_rns(p, junk, True)
            vals = [rnd.randrange(1 << (64 * wpc)) for _ in range(2 * k)]
            m.load_coeff_words(_to_words(vals, wpc, 2, k), eval_format=False)
            assert not m.is_ntt
            assert np.array_equal(m.to_rns(), _expected(vals, moduli, 2, k, n)), (wpc, k)
    # below full level: exactly level + 1 limbs
    if L >= 2:
        wpc = _words_of(Q)
        low = M._new_zero_with_state(p, 1, 2, L - 2, False)
        low.load_rns(np.ones((1, 2, L - 1, n), dtype=np.uint64), False)
        vals = _fill(_special_values(moduli, wpc), max(2 * n, 0), 1 << (64 * wpc), SEED + L)[: 2 * n]
        low.load_coeff_words(_to_words(vals, wpc, 2, n), eval_format=False)
        res = low.to_rns()
        assert res.shape == (1, 2, L - 1, n) and low.level == L - 2
        assert np.array_equal(res, _expected(vals, moduli[: L - 1], 2, n, n))
        low_e = M.from_coeff_words(p, _to_words(vals, wpc, 2, n), eval_format=True, level=L - 2)
        ref = M.from_rns(p, res, False)
        ref.ntt_all_in_place()
        assert low_e.level == L - 2 and np.array_equal(low_e.to_rns(), ref.to_rns())


def test_load_over_a_packed_uniform_sample(gpu):
    """a fresh uniform sample of a context with moduli below 2^24 may be stored in 3 bytes per residue: the load writes words"""
    n, bits, L = 256, 24, 9
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    m = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, 2, gpu.DistType.FinRingDist())
    assert m.layout in ("words", "packed24")
    wpc = _words_of(math.prod(moduli))
    vals = _fill([], 2 * n, 1 << (64 * wpc), SEED)
    m.load_coeff_words(_to_words(vals, wpc, 2, n), eval_format=False)
    assert m.layout == "words" and np.array_equal(m.to_rns(), _expected(vals, moduli, 2, n, n))


def _random_residues(moduli, rows, cols, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, q, size=(rows, cols, n), dtype=np.uint64) for q in moduli], axis=2)


@pytest.mark.parametrize("n,bits,L", SMALL_CELLS + [(65536, 28, 53)])
def test_store_and_load_are_inverses(gpu, n, bits, L):
    from mxx_amd import _ffi

    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    wq = _words_of(Q)
    M = gpu.GpuDCRTPolyMatrix
    lib = _ffi.lib()
    res = _random_residues(moduli, 1, 2, n, SEED + L)
    for eval_format in (False, True):
        m = M.from_rns(p, res, eval_format)
        for wpc in (wq, wq + 3):
            words = np.empty((1, 2, n, wpc), dtype=np.uint64)
            assert lib.gpupoly_matrix_store_coeff_words(m.raw, words.ctypes.data_as(C.POINTER(C.c_uint64)), wpc) == 0
            back = M.from_coeff_words(p, words, eval_format=eval_format)
            assert back.is_ntt == eval_format and np.array_equal(back.to_rns(), res), (eval_format, wpc)
    # store(load(x)) = x mod Q
    for vals, wpc, cols in _loads_for_cell(moduli, n, SEED + 5 * n):
        for eval_format in (False, True):
            m = M.from_coeff_words(p, _to_words(vals, wpc, cols, n), eval_format=eval_format)
            assert m.coeffs() == [[[v % Q for v in vals[c * n:(c + 1) * n]] for c in range(cols)]], (wpc, eval_format)


def _raw_load(mat_raw, words, wpc, k, fmt):
    from mxx_amd import _ffi

    ptr = words.ctypes.data_as(C.POINTER(C.c_uint64)) if words is not None else None
    return _ffi.lib().gpupoly_matrix_load_coeff_words(mat_raw, ptr, wpc, k, fmt)


def test_refusals_launch_nothing_and_leave_the_target_alone(gpu):
    from mxx_amd import _ffi

    n, bits, L = 64, 24, 3
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    res = _random_residues(moduli, 1, 2, n, SEED)
    target = gpu.GpuDCRTPolyMatrix.from_rns(p, res, True)  # EVAL-tagged: a COEFF load that went through would retag it
    words = np.full((1, 2, n, 2), 5, dtype=np.uint64)
    lib = _ffi.lib()
    COEFF, EVAL = 0, 1
    cases = [
        (None, words, 2, n, COEFF),                 # null matrix
        (target.raw, None, 2, n, COEFF),            # null words with coefficients to read
        (target.raw, None, 1, 1, EVAL),
        (target.raw, words, 0, n, COEFF),           # no words per coefficient
        (target.raw, words, 1 << 32, n, COEFF),     # above 2^32 - 1
        (target.raw, words, 2, n + 1, COEFF),       # more coefficients than the ring has
        (target.raw, words, 2, n, 2),               # neither COEFF nor EVAL
        (target.raw, words, 2, n, -1),
    ]
    for raw, w, wpc, k, fmt in cases:
        c0 = lib.gpupoly_launch_count()
        assert _raw_load(raw, w, wpc, k, fmt) != 0, (wpc, k, fmt)
        assert "gpupoly_matrix_load_coeff_words" in _ffi.last_error_string()
        assert lib.gpupoly_launch_count() == c0
        assert target.is_ntt and np.array_equal(target.to_rns(), res)  # to_rns() asks for EVAL: the tag still says so
    # and the accepted edges: no coefficients with null words is the zero matrix; an empty matrix launches nothing
    assert _raw_load(target.raw, None, 1, 0, COEFF) == 0
    target.is_ntt = False
    assert not target.to_rns().any()
    for rows, cols in ((0, 2), (2, 0), (0, 0)):
        empty = gpu.GpuDCRTPolyMatrix(p, rows, cols, L - 1, True)
        c0 = lib.gpupoly_launch_count()
        assert _raw_load(empty.raw, words, 2, n, COEFF) == 0 and _raw_load(empty.raw, words, 2, n, EVAL) == 0
        assert lib.gpupoly_launch_count() == c0


@pytest.mark.parametrize("n,bits,L", [(256, 24, 9), (1024, 28, 16), (64, 51, 9), (32, 62, 17), (16384, 24, 10), (65536, 28, 53)])
def test_launch_budget(gpu, n, bits, L):
    from mxx_amd import _ffi

    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    lib = _ffi.lib()
    res = _random_residues(moduli, 1, 2, n, SEED)
    M.from_rns(p, res, False).ntt_all_in_place()  # warm
    x = M.from_rns(p, res, False)
    c0 = lib.gpupoly_launch_count()
    x.ntt_all_in_place()
    ntt_launches = lib.gpupoly_launch_count() - c0
    assert ntt_launches >= 1
    for wpc in (1, _words_of(math.prod(moduli)) + 1):
        for k in (0, 1, n):
            words = _to_words(_fill([], 2 * k, 1 << (64 * wpc), SEED + k), wpc, 2, k)
            m = M(p, 1, 2, L - 1, True)
            c0 = lib.gpupoly_launch_count()
            m.load_coeff_words(words, eval_format=False)
            assert lib.gpupoly_launch_count() - c0 == 1, (wpc, k)
            c0 = lib.gpupoly_launch_count()
            m.load_coeff_words(words, eval_format=True)
            assert lib.gpupoly_launch_count() - c0 == 1 + ntt_launches, (wpc, k)


@pytest.mark.parametrize("n,bits,L", [(256, 28, 3), (64, 51, 9), (32, 62, 17), (64, 31, 2)])
def test_mirror_constructors_equal_the_host_loop(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    Q = p.modulus()
    Poly = gpu.GpuDCRTPoly
    rnd = random.Random(SEED + n)
    big = [rnd.randrange(Q) for _ in range(n)]
    over = [rnd.randrange(Q << 70) for _ in range(n - 1)]  # above Q, short
    u32s = [rnd.getrandbits(32) for _ in range(n)]
    bools = [rnd.random() < 0.5 for _ in range(n)]
    usize = rnd.getrandbits(min(n, 64))
    pairs = [
        (Poly.from_biguints(p, big), big),
        (Poly.from_biguints(p, over), over),
        (Poly.from_biguints(p, []), []),
        (Poly.from_coeffs(p, big[: n // 2]), big[: n // 2]),
        (Poly.from_biguints_eval(p, big), big),
        (Poly.from_u32s(p, np.asarray(u32s, dtype=np.uint32)), u32s),
        (Poly.from_bool_vec(p, bools), [1 if b else 0 for b in bools]),
        (Poly.from_biguint_to_constant(p, Q - 2), [Q - 2]),
        (Poly.from_biguint_to_constant(p, (1 << 64) - 1), [(1 << 64) - 1]),
        (Poly.from_usize_to_lsb(p, usize), [(usize >> i) & 1 for i in range(n)]),
        (Poly.const_max(p), [Q - 1] * n),
        (Poly.const_minus_one(p), [Q - 1]),
        (Poly.const_zero(p), [0]),
        (Poly.const_one(p), [1]),
    ]
    for i, (got, coeffs) in enumerate(pairs):
        host = Poly._from_biguints_host(p, coeffs)
        assert got.is_ntt() and host.is_ntt() and got.level() == host.level() == L - 1, i
        assert np.array_equal(got.inner.to_rns(), host.inner.to_rns()), i


def test_matrix_from_coeffs_inverts_coeffs_ragged_rows_and_negatives(gpu):
    n, bits, L = 64, 51, 9
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    assert _words_of(Q) > 1
    M = gpu.GpuDCRTPolyMatrix
    res = _random_residues(moduli, 3, 2, n, SEED + 1)
    for eval_format in (True, False):
        m = M.from_rns(p, res, eval_format)
        back = M.from_coeffs(p, m.coeffs(), eval_format)
        assert back.is_ntt == eval_format and back.size() == (3, 2) and back == m
        assert np.array_equal(back.to_rns(), res)
    # ragged: padded with zeros to the longest
    rnd = random.Random(SEED)
    rows = [[[rnd.randrange(Q) for _ in range(k)] for k in ks] for ks in ((0, 5), (n, 1), (7, 3))]
    flat = [v for row in rows for poly in row for v in poly + [0] * (n - len(poly))]
    got = M.from_coeffs(p, rows, eval_format=False)
    assert np.array_equal(got.to_rns(), _expected(flat, moduli, 6, n, n).reshape(3, 2, L, n))
    short = M.from_coeffs(p, [[[1, 2], [3]]], eval_format=False)  # the longest is below n
    assert np.array_equal(short.to_rns(), _expected([1, 2, 3, 0], moduli, 2, 2, n))
    assert M.from_coeffs(p, [], True).size() == (0, 0) and M.from_coeffs(p, [[], []], True).size() == (2, 0)
    for bad in ([[[1, -1]]], [[[-(1 << 70)], [5]]]):
        with pytest.raises(ValueError):
            M.from_coeffs(p, bad)
    with pytest.raises(ValueError):
        gpu.GpuDCRTPoly.from_biguints(p, [3, -4])
