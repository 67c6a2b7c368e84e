"""GPU: the exact centred infinity norm of every entry (`gpupoly_matrix_centered_max_abs`) and the mirror's
`centered_max_abs` against plain Python big integers.

Expected values come from the definition alone: max over an entry's coefficients v in [0, Q_l) of min(v, Q_l - v), Q_l the
product of the matrix's own limbs.  Every modulus width class in both word sizes, limb counts on both sides of the
kernel's 8 / 16 / 64 bounds, levels below full, rings from 2 to 2^16, COEFF and EVAL inputs; beyond random values,
0, 1, Q_l - 1, floor(Q_l/2), floor(Q_l/2) + 1, values that share their top words, the maximum in the first and in the
last coefficient, fast-path and Garner-path coefficients in one entry, all-zero entries, the shapes, the refusals and an
M3A-shape preimage.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261016

# (n, bits, limbs): 32-bit words to 31 bits (10-24-bit lazy, 28-bit tight, 31-bit generic), 64-bit words above
# (32 / 33-bit `%` limbs, 41 / 51-bit double-precision transforms, 57-62-bit integer forms)
CELLS = [
    (2, 10, 2),
    (16, 24, 1),
    (64, 20, 8),
    (256, 24, 9),
    (1024, 28, 16),
    (2048, 28, 17),
    (64, 31, 2),
    (128, 31, 53),
    (8192, 24, 3),
    (256, 32, 3),
    (64, 33, 2),
    (256, 41, 8),
    (256, 51, 9),
    (128, 57, 16),
    (32, 62, 17),
    (16, 60, 64),
    (4096, 31, 64),
]

_PARAMS = {}


def _params(gpu, n, bits, L):
    key = (n, bits, L)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, L), 1)
    return _PARAMS[key]


def _centred(v, Q):
    return min(v, Q - v)


def _signed(rnd, mag_limit, Q):
    """a value in [0, Q) whose centred representative is a random c with |c| <= mag_limit"""
    c = rnd.randint(0, mag_limit)
    return (Q - c) % Q if rnd.random() < 0.5 else c


def _entry(kind, n, moduli, rnd, j=0):
    """n values in [0, Q) of one entry"""
    Q = math.prod(moduli)
    h = Q // 2
    small = moduli[0] // 2
    two = moduli[0] * moduli[1] // 2 if len(moduli) > 1 else small
    if kind == "random":
        return [rnd.randrange(Q) for _ in range(n)]
    if kind == "zero":
        return [0] * n
    if kind == "small":  # the first fast path
        return [_signed(rnd, small, Q) for _ in range(n)]
    if kind == "two":  # the second fast path
        return [_signed(rnd, two, Q) for _ in range(n)]
    if kind == "mixed":  # fast-path and Garner-path coefficients in one entry
        vals = [_signed(rnd, small, Q) for _ in range(n)]
        for i in rnd.sample(range(n), max(1, n // 8)):
            vals[i] = _signed(rnd, two, Q)
        for i in rnd.sample(range(n), max(1, n // 16)):
            vals[i] = rnd.randrange(Q)
        return vals
    if kind == "planted":  # 0, 1, Q - 1, floor(Q/2), floor(Q/2) + 1, rotated by j so that n = 2 sees each of them
        planted = [0, 1, Q - 1, h, h + 1]
        vals = [_signed(rnd, small, Q) for _ in range(n)]
        for i in range(min(n, 5)):
            vals[i] = planted[(i + j) % 5]
        return vals
    if kind in ("first", "last"):  # the one largest value in the first / last coefficient, the rest strictly below
        top = max(2, min(two, h))
        vals = [_signed(rnd, top - 1, Q) for _ in range(n)]
        vals[0 if kind == "first" else n - 1] = top if rnd.random() < 0.5 else Q - top
        return vals
    if kind == "ties":  # every |x| shares the words above word 0 (and above word 1 for half of them): the max is settled below
        if h >> 64 == 0:
            hi, lo_bits = 0, max(1, h.bit_length() - 1)
        else:
            hi, lo_bits = rnd.randrange(h >> 64), 64
        mags = []
        for i in range(n):
            m = (hi << 64) | rnd.getrandbits(lo_bits)
            if i % 2 and h >> 128:
                m = (((h >> 128) - 1) << 128) | ((hi & ((1 << 64) - 1)) << 64) | rnd.getrandbits(64)
            mags.append(m)
        return [(Q - m) % Q if i % 3 == 1 else m for i, m in enumerate(mags)]
    raise ValueError(kind)


def _residues(entries, moduli, rows, cols, n):
    """(rows, cols, L, n) residues, entry (r, c) = entries[r * cols + c]"""
    arr = np.asarray(entries, dtype=object).reshape(rows, cols, n)
    return np.stack([(arr % q).astype(np.uint64) for q in moduli], axis=2)


def _expected(entries, Q, rows, cols):
    return [[max(_centred(v, Q) for v in entries[r * cols + c]) for c in range(cols)] for r in range(rows)]


def _device_words(m, wpv, sentinel=0xA5A5A5A5A5A5A5A5):
    from mxx_amd import _ffi

    buf = np.full((m.nrow, m.ncol, wpv), sentinel, dtype=np.uint64)
    st = _ffi.lib().gpupoly_matrix_centered_max_abs(m.raw, buf.ctypes.data_as(C.POINTER(C.c_uint64)), wpv)
    return st, buf


def _words_of(v, wpv):
    return [(v >> (64 * w)) & ((1 << 64) - 1) for w in range(wpv)]


KINDS = ["random", "zero", "small", "two", "mixed", "planted", "planted", "planted", "first", "last", "ties", "ties"]


def _check(gpu, p, moduli, entries, rows, cols, n, host=True):
    """COEFF and EVAL inputs against the big-integer values; residues and format left as they were"""
    M = gpu.GpuDCRTPolyMatrix
    Q = math.prod(moduli)
    want = _expected(entries, Q, rows, cols)
    res = _residues(entries, moduli, rows, cols, n)
    a = M.from_rns(p, res, False)
    assert a.level == len(moduli) - 1
    got = a.centered_max_abs(axis="entries")
    assert got == want
    assert not a.is_ntt and np.array_equal(a.to_rns(), res)
    if host:
        assert a._centered_max_abs_host(axis="entries") == want
    e = M.from_rns(p, res, False)
    e.ntt_all_in_place()
    e_rns = e.to_rns()
    assert e.centered_max_abs(axis="entries") == want
    assert e.is_ntt and np.array_equal(e.to_rns(), e_rns)  # still EVAL and unchanged
    # words above the value are zero-filled
    wpv = -(-Q.bit_length() // 64) + 2
    st, buf = _device_words(e, wpv)
    assert st == 0
    for r in range(rows):
        for c in range(cols):
            assert buf[r, c].tolist() == _words_of(want[r][c], wpv)


@pytest.mark.parametrize("n,bits,L", CELLS)
def test_matches_big_integers(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    rnd = random.Random(SEED + n + 7 * bits + L)
    levels = sorted({L - 1, (L - 1) // 2, 0} if L > 1 else {0}, reverse=True)
    for level in levels:
        lm = moduli[: level + 1]
        kinds = KINDS if n <= 4096 else ["mixed", "planted", "last", "ties"]
        entries = [_entry(k, n, lm, rnd, 2 * j) for j, k in enumerate(kinds)]  # planted offsets 0, 2, 4 (mod 5)
        rows = 2 if len(kinds) % 2 == 0 else 1
        _check(gpu, p, lm, entries, rows, len(kinds) // rows, n, host=n * len(kinds) * L <= 1 << 20)


def test_full_ring_53_limbs(gpu):
    """n = 2^16 with 53 x 28-bit limbs (the reference's parameter-search ring): 32 chunks per entry"""
    n, L = 1 << 16, 53
    p = _params(gpu, n, 28, L)
    moduli = p.moduli()
    rnd = random.Random(SEED + 53)
    entries = [_entry("mixed", n, moduli, rnd), _entry("ties", n, moduli, rnd)]
    _check(gpu, p, moduli, entries, 1, 2, n, host=False)


@pytest.mark.parametrize("logn", range(1, 17))
def test_every_ring(gpu, logn):
    n = 1 << logn
    p = _params(gpu, n, 28 if logn > 12 else 24, 3)
    moduli = p.moduli()
    rnd = random.Random(SEED + logn)
    kinds = ["mixed", "last", "planted"] if n >= 4 else ["planted", "last", "ties"]
    entries = [_entry(k, n, moduli, rnd, 2 * j) for j, k in enumerate(kinds)]
    _check(gpu, p, moduli, entries, 1, 3, n, host=n <= 1 << 12)


def test_axis_forms_and_shapes(gpu):
    n = 64
    p = _params(gpu, n, 41, 4)
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + 1)
    M = gpu.GpuDCRTPolyMatrix
    for rows, cols in ((1, 1), (3, 4), (9, 1), (1, 9)):
        kinds = [rnd.choice(["random", "zero", "small", "two", "mixed", "ties"]) for _ in range(rows * cols)]
        entries = [_entry(k, n, moduli, rnd) for k in kinds]
        m = M.from_rns(p, _residues(entries, moduli, rows, cols, n), False)
        if rnd.random() < 0.5:
            m.ntt_all_in_place()
        want = _expected(entries, Q, rows, cols)
        assert m.centered_max_abs(axis="entries") == want == m._centered_max_abs_host(axis="entries")
        assert m.centered_max_abs() == max(max(r) for r in want) == m._centered_max_abs_host()
        assert m.centered_max_abs(axis=1) == [max(r) for r in want] == m._centered_max_abs_host(axis=1)
        assert m.centered_max_abs(axis=0) == [max(want[r][c] for r in range(rows)) for c in range(cols)]
        assert m.centered_max_abs(axis=0) == m._centered_max_abs_host(axis=0)
    z = M.zero(p, 2, 3)
    assert z.centered_max_abs(axis="entries") == [[0, 0, 0], [0, 0, 0]] and z.centered_max_abs() == 0
    for rows, cols in ((0, 3), (3, 0), (0, 0)):
        e = M(p, rows, cols, len(moduli) - 1, True)
        for axis in (None, 0, 1, "entries"):
            assert e.centered_max_abs(axis=axis) == e._centered_max_abs_host(axis=axis)
        assert e.centered_max_abs(axis=1) == [0] * rows and e.centered_max_abs(axis=0) == [0] * cols
        st, buf = _device_words(e, 4)
        assert st == 0
    with pytest.raises(ValueError):
        z.centered_max_abs(axis="rows")
    poly = gpu.GpuDCRTPoly.from_biguints(p, [5, Q - 9, 3])
    assert poly.centered_max_abs() == 9


def test_more_workgroup_tasks_than_the_grid(gpu):
    """n = 2 and 1025 x 1025 entries: more tasks than the partial kernel's 2^20 workgroups, more entries than one grid
    dimension of 256-thread blocks holds at once"""
    n = 2
    p = _params(gpu, n, 24, 1)
    q = p.moduli()[0]
    rows = cols = 1025
    rng = np.random.default_rng(SEED)
    res = rng.integers(0, q, size=(rows, cols, 1, n), dtype=np.uint64)
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, res, False)
    want = np.minimum(res, np.uint64(q) - res).max(axis=(2, 3))
    assert m.centered_max_abs(axis="entries") == want.tolist()


def test_refusals_write_nothing(gpu):
    from mxx_amd import _ffi

    n = 16
    p = _params(gpu, n, 60, 5)
    moduli = p.moduli()
    rnd = random.Random(SEED + 2)
    entries = [_entry("random", n, moduli, rnd) for _ in range(2)]
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, _residues(entries, moduli, 1, 2, n), False)
    words = -(-math.prod(moduli).bit_length() // 64)
    assert words == 5
    lib = _ffi.lib()
    sentinel = 0x5A5A5A5A5A5A5A5A
    for wpv in (0, words - 1):
        st, buf = _device_words(m, wpv, sentinel)
        assert st != 0 and "gpupoly_matrix_centered_max_abs" in _ffi.last_error_string()
        assert "words" in _ffi.last_error_string()
        assert (buf == sentinel).all()
    buf = np.full((1, 2, words), sentinel, dtype=np.uint64)
    assert lib.gpupoly_matrix_centered_max_abs(None, buf.ctypes.data_as(C.POINTER(C.c_uint64)), words) != 0
    assert "gpupoly_matrix_centered_max_abs" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_centered_max_abs(m.raw, None, words) != 0
    assert "gpupoly_matrix_centered_max_abs" in _ffi.last_error_string()
    assert (buf == sentinel).all()
    # below full level the words of Q_level are what counts
    low = gpu.GpuDCRTPolyMatrix.from_rns(p, _residues(entries, moduli[:1], 1, 2, n), False)
    st, buf = _device_words(low, 1)
    assert st == 0 and buf[0].tolist() == [[max(_centred(v % moduli[0], moduli[0]) for v in e)] for e in entries]


def test_m3a_preimage_below_the_preimage_norm(gpu, oracle):
    """The M3A shape (n = 2^14, 10 x 24-bit limbs, base 2^12, d = 1, 50 target columns): a 22 x 50 preimage.  Its
    per-entry values equal the host form on a slice of columns, and the whole-matrix max lies below the bound."""
    from mxx_amd.trapdoor import compute_preimage_norm

    n, depth, bits, base, d, cols = 1 << 14, 10, 24, 12, 1, 50
    moduli = oracle.gen_crt_basis(n, depth, bits)
    p = gpu.GpuDCRTPolyParams(n, moduli, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, A = sampler.trapdoor(p, d)
    target = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, d, cols, gpu.DistType.FinRingDist())
    x = sampler.preimage(p, td, A, target)
    k = p.modulus_digits()
    assert x.size() == (k + 2, cols) and x.is_ntt
    per = x.centered_max_abs(axis="entries")
    part = x.slice_columns(0, 3)
    assert [row[:3] for row in per] == part._centered_max_abs_host(axis="entries")
    assert per == x.centered_max_abs(axis="entries")  # EVAL input left as it was: the same values again
    worst = x.centered_max_abs()
    assert worst == max(max(r) for r in per) and 0 < worst < compute_preimage_norm(math.sqrt(n), d * k, float(1 << base))
    assert A * x == target
