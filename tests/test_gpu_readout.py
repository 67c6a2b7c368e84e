"""GPU: bits and machine integers of the coefficients (`gpupoly_matrix_extract_bits`, `gpupoly_matrix_store_coeff_ints`)
and the mirror methods on top of them against plain Python integers.

Expected values come from the definitions alone: coefficient c in [0, Q_l), Q_l the product of the matrix's own limbs;
bit = c in [lo, hi) (or in [lo, Q_l) u [0, hi) for lo > hi); element = c mod 2^b, or x mod 2^b for the representative x of
c in (-Q_l/2, Q_l/2].  Inputs are uploaded as residues computed in Python.  Both word sizes, limb counts on both sides of
the kernels' 8 / 16 / 64 bounds, rings below one byte, of one byte, of one ballot word and of several blocks, levels
below full, COEFF and EVAL inputs; around every bound the values that differ from it in one mixed-radix digit only.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261018
U64 = (1 << 64) - 1

# (n, bits, limbs)
CELLS = [
    (2, 10, 2),
    (8, 24, 1),
    (16, 24, 3),
    (64, 24, 8),
    (64, 24, 9),
    (256, 28, 16),
    (64, 28, 17),
    (64, 31, 3),
    (256, 51, 2),
    (64, 51, 9),
    (32, 62, 17),
    (16, 60, 64),
    (16384, 24, 3),
]

_PARAMS = {}


def _params(gpu, n, bits, L):
    key = (n, bits, L)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, L), 1)
    return _PARAMS[key]


def _levels(L):
    return sorted({L - 1, (L - 1) // 2, 0}, reverse=True)


def _residues(values, moduli, rows, cols, n):
    """(rows, cols, L, n) residues of rows * cols * n values, entry (r, c) = values[(r * cols + c) * n :][:n]"""
    arr = np.asarray(values, dtype=object).reshape(rows, cols, n)
    return np.stack([(arr % q).astype(np.uint64) for q in moduli], axis=2)


def _shape(entries):
    return (2, entries // 2) if entries % 2 == 0 else (1, entries)


def _upload(gpu, p, moduli, values, n):
    """values (padded by the caller to whole entries) as a COEFF matrix and as its EVAL form, with their residues"""
    rows, cols = _shape(len(values) // n)
    res = _residues(values, moduli, rows, cols, n)
    M = gpu.GpuDCRTPolyMatrix
    a = M.from_rns(p, res, False)
    assert a.level == len(moduli) - 1 and not a.is_ntt
    e = M.from_rns(p, res, False)
    e.ntt_all_in_place()
    return a, e, res, e.to_rns()


def _fill(planted, n, rnd, extra):
    """the planted values followed by extra()-drawn ones up to whole entries (small rings: one entry more than needed)"""
    entries = -(-len(planted) // n) + (1 if n < 1024 else 0)
    return list(planted) + [extra() for _ in range(entries * n - len(planted))]


def _intervals(Q):
    quarter = (Q // 2) >> 1
    B = Q // 5
    return {
        "threshold": (quarter, 3 * quarter),
        "decode": (-(-(Q + 1) // 4), -(-(3 * Q + 1) // 4)),
        "full": (0, Q),
        "empty at 0": (0, 0),
        "empty at mid": (Q // 2, Q // 2),
        "empty at Q": (Q, Q),
        "first": (0, 1),
        "last": (Q - 1, Q),
        "wrap centred": (Q - B, B + 1),
        "wrap from Q": (Q, Q // 2),
    }


def _around(B, moduli):
    """B and the values that differ from it in one mixed-radix digit: the lowest, the second, the top one"""
    Q = math.prod(moduli)
    q0, top = moduli[0], Q // moduli[-1]
    base = B - B % q0
    cand = [B - 1, B, B + 1, 0, Q - 1, base, base + q0 - 1, B - q0, B + q0, B - top, B + top]
    return [v for v in cand if 0 <= v < Q]


def _member(c, lo, hi):
    return lo <= c < hi if lo <= hi else (c >= lo or c < hi)


def _want_bits(values, lo, hi, rows, cols, n):
    return np.array([_member(c, lo, hi) for c in values], dtype=bool).reshape(rows, cols, n)


def _words(v, count):
    return (C.c_uint64 * count)(*[(v >> (64 * w)) & U64 for w in range(count)])


def _raw_bits(m, lo, hi, bpp, wpb=None, sentinel=0xA5):
    from mxx_amd import _ffi

    Q = m._level_modulus()
    wpb = -(-Q.bit_length() // 64) if wpb is None else wpb
    buf = np.full((m.nrow, m.ncol, bpp), sentinel, dtype=np.uint8)
    st = _ffi.lib().gpupoly_matrix_extract_bits(m.raw, _words(lo, max(wpb, 1)), _words(hi, max(wpb, 1)), wpb,
                                                buf.ctypes.data_as(C.POINTER(C.c_uint8)), bpp)
    return st, buf


def _raw_ints(m, dtype, centred, cpp, elem_bytes=None, sentinel=0x5A):
    from mxx_amd import _ffi

    dt = np.dtype(dtype)
    buf = np.full((m.nrow, m.ncol, max(cpp, 1)), sentinel, dtype=np.uint8).repeat(dt.itemsize, axis=-1).view(dt)
    count, first = C.c_uint64(0xC0), C.c_uint64(0xF1)
    st = _ffi.lib().gpupoly_matrix_store_coeff_ints(m.raw, C.c_void_p(buf.ctypes.data), dt.itemsize if elem_bytes is None else elem_bytes,
                                                    centred, cpp, C.byref(count), C.byref(first))
    return st, buf, count.value, first.value


def _launches():
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_launch_count()


# ---- extract_bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits,L", CELLS)
def test_extract_bits_matches_python(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    rnd = random.Random(SEED + n + 7 * bits + L)
    for level in _levels(L):
        moduli = p.moduli()[: level + 1]
        Q = math.prod(moduli)
        intervals = _intervals(Q)
        planted = []
        for b in sorted({b for pair in intervals.values() for b in pair}):
            planted += _around(b, moduli)
        values = _fill(planted, n, rnd, lambda: rnd.randrange(Q))
        a, e, res, e_res = _upload(gpu, p, moduli, values, n)
        rows, cols = a.size()
        for name, (lo, hi) in intervals.items():
            want = _want_bits(values, lo, hi, rows, cols, n)
            if name.startswith("empty"):
                assert not want.any(), name
            elif name == "full":
                assert want.all(), name
            else:
                assert want.any() and not want.all(), name  # a kernel that returns a constant cannot pass
            for m in (a, e):
                got = m.extract_bits(lo, hi)
                assert got.dtype == bool and got.shape == (rows, cols, n)
                assert np.array_equal(got, want), (name, level, m.is_ntt, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(a.extract_bits_with_threshold(), _want_bits(values, *intervals["threshold"], rows, cols, n))
        assert np.array_equal(e.decode_bits(), _want_bits(values, *intervals["decode"], rows, cols, n))
        # padded slots over a sentinel: every byte written, the padding zero; bounds with zero words above Q's words
        lo, hi = intervals["threshold"]
        minb = -(-n // 8)
        packed = np.packbits(_want_bits(values, lo, hi, rows, cols, n), axis=-1, bitorder="little")
        for bpp, wpb in ((minb, None), (minb + 3, -(-Q.bit_length() // 64) + 2)):
            st, buf = _raw_bits(e, lo, hi, bpp, wpb)
            assert st == 0
            assert np.array_equal(buf[..., :minb], packed) and not buf[..., minb:].any(), (level, bpp)
        # the inputs are as they were
        assert not a.is_ntt and np.array_equal(a.to_rns(), res)
        assert e.is_ntt and np.array_equal(e.to_rns(), e_res)


# ---- coeffs_ints -------------------------------------------------------------------------------------------------------
def _centred(c, Q):
    return c if c <= Q // 2 else c - Q


def _want_ints(values, Q, dtype):
    """(elements as Python ints in the dtype's range, misfit flags)"""
    dt = np.dtype(dtype)
    b = 8 * dt.itemsize
    out, bad = [], []
    for c in values:
        if dt.kind == "u":
            out.append(c % (1 << b))
            bad.append(c >= 1 << b)
        else:
            x = _centred(c, Q)
            t = x % (1 << b)
            out.append(t - (1 << b) if t >> (b - 1) else t)
            bad.append(not -(1 << (b - 1)) <= x <= (1 << (b - 1)) - 1)
    return out, bad


def _ints_values(moduli, n, rnd):
    Q = math.prod(moduli)
    h = Q // 2
    planted = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 1 << 64, h, h + 1,
               Q - 1, Q - (1 << 31), Q - (1 << 31) - 1, Q - (1 << 63), Q - (1 << 63) - 1]
    planted = [v for v in planted if 0 <= v < Q]
    small = min(h, 1 << 20)

    def extra():  # half small centred values (so that a misfit is not the rule), half uniform
        if rnd.random() < 0.5:
            return rnd.randint(-small, small) % Q
        return rnd.randrange(Q)

    # two small values in front: the first misfit is not index 0 whenever something misfits at all
    return _fill([3 % Q, Q - 2] + planted, n, rnd, extra)


DTYPES = [np.uint32, np.uint64, np.int32, np.int64]


def _check_ints(m, values, Q, dtype, cpp, n):
    rows, cols = m.size()
    kept = [values[poly * n + k] for poly in range(rows * cols) for k in range(cpp)]
    want, bad = _want_ints(kept, Q, dtype)
    got, count, first = m.coeffs_ints_misfits(dtype, cpp)
    assert got.dtype == np.dtype(dtype) and got.shape == (rows, cols, cpp)
    assert got.reshape(-1).tolist() == want, (np.dtype(dtype).name, cpp)
    assert count == sum(bad)
    if count:
        idx = bad.index(True)
        assert first == (idx // cpp // cols, idx // cpp % cols, idx % cpp)
        with pytest.raises(OverflowError) as err:
            m.coeffs_ints(dtype, cpp)
        assert str(first) in str(err.value)
        assert np.array_equal(m.coeffs_ints(dtype, cpp, strict=False), got)
    else:
        assert first is None
        assert np.array_equal(m.coeffs_ints(dtype, cpp), got)
    return count


@pytest.mark.parametrize("n,bits,L", CELLS)
def test_coeffs_ints_match_python(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    rnd = random.Random(SEED + 3 * n + bits + 11 * L)
    for level in _levels(L):
        moduli = p.moduli()[: level + 1]
        Q = math.prod(moduli)
        values = _ints_values(moduli, n, rnd)
        a, e, res, e_res = _upload(gpu, p, moduli, values, n)
        for dtype in DTYPES:
            dt = np.dtype(dtype)
            ca = _check_ints(a, values, Q, dtype, n, n)
            ce = _check_ints(e, values, Q, dtype, n, n)
            assert ca == ce
            limit = 1 << (8 * dt.itemsize - (dt.kind == "i"))
            if (Q if dt.kind == "u" else Q // 2 + 1) <= limit:
                assert ca == 0  # Q < 2^b: nothing misfits unsigned; Q/2 < 2^(b-1): nothing misfits centred
            elif (Q if dt.kind == "u" else Q // 2) > limit:
                assert ca > 0  # the planted 2^b / 2^(b-1) lies below Q resp. Q/2
        assert not a.is_ntt and np.array_equal(a.to_rns(), res)
        assert e.is_ntt and np.array_equal(e.to_rns(), e_res)


@pytest.mark.parametrize("n,bits,L", [(8, 24, 1), (64, 31, 3), (64, 51, 9)])
def test_coeffs_per_poly_and_strict(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + n + L)
    values = _ints_values(moduli, n, rnd)
    a, e, _, _ = _upload(gpu, p, moduli, values, n)
    rows, cols = a.size()
    for cpp in (1, n - 1, n):
        for dtype in DTYPES:
            _check_ints(a, values, Q, dtype, cpp, n)
        _check_ints(e, values, Q, np.int32, cpp, n)
    c0 = _launches()
    for m in (a, e):
        got, count, first = m.coeffs_ints_misfits(np.int64, 0)
        assert got.shape == (rows, cols, 0) and count == 0 and first is None
        st, _, count, first = _raw_ints(m, np.uint64, 0, 0)
        assert st == 0 and count == 0 and first == U64
    assert _launches() == c0
    assert np.array_equal(a.const_coeffs_u64(strict=False), np.array([values[k * n] & U64 for k in range(rows * cols)],
                                                                     dtype=np.uint64).reshape(rows, cols))
    with pytest.raises(TypeError):
        a.coeffs_ints(np.int16)
    with pytest.raises(ValueError):
        a.coeffs_ints(np.int64, n + 1)


def test_small_moduli_never_misfit(gpu):
    """Q < 2^32 (so Q / 2 < 2^31): no dtype misfits; 2^32 <= Q < 2^63: the 64-bit dtypes never misfit, the 32-bit ones do"""
    rnd = random.Random(SEED + 5)
    for (n, bits, L), level in (((8, 24, 1), 0), ((2, 10, 2), 1), ((64, 31, 3), 0), ((64, 31, 3), 1)):
        p = _params(gpu, n, bits, L)
        moduli = p.moduli()[: level + 1]
        Q = math.prod(moduli)
        values = [rnd.randrange(Q) for _ in range(3 * n)]
        a, e, _, _ = _upload(gpu, p, moduli, values, n)
        for m in (a, e):
            counts = {np.dtype(dt).name: _check_ints(m, values, Q, dt, n, n) for dt in DTYPES}
            assert counts["uint64"] == 0 and counts["int64"] == 0
            if Q < 1 << 32:
                assert counts["uint32"] == 0 and counts["int32"] == 0
            else:
                assert 1 << 32 <= Q < 1 << 63 and counts["uint32"] > 0 and counts["int32"] > 0


# ---- agreement with the older device entries (independent kernels) -------------------------------------------------------
@pytest.mark.parametrize("n,bits,L", [(64, 24, 9), (256, 51, 2), (32, 62, 17)])
def test_agrees_with_older_device_entries(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + 17 * L)
    values = [rnd.randrange(Q) for _ in range(3 * n)] + [rnd.randrange(1 << 64) % Q for _ in range(n)]
    a, e, _, _ = _upload(gpu, p, moduli, values, n)
    rows, cols = a.size()
    # decode_bits = decode_centered(2), read through store_coeff_words
    decoded = np.array(e.decode_centered(2).coeffs(), dtype=object).astype(np.uint8).astype(bool)
    assert decoded.any() and not decoded.all()
    assert np.array_equal(e.decode_bits(), decoded) and np.array_equal(a.decode_bits(), decoded)
    # coeffs_ints(uint64) = word 0 of store_coeff_words where it fits
    words = np.array([[[c & U64 for c in poly] for poly in row] for row in a.coeffs()], dtype=np.uint64)
    fits = np.array([c <= U64 for c in values], dtype=bool).reshape(rows, cols, n)
    got, count, _ = a.coeffs_ints_misfits(np.uint64)
    assert count == (~fits).sum() and np.array_equal(got, words)  # truncated ones are word 0 too
    assert fits.any()
    # max |.| of coeffs_ints(int64) over a Gaussian sample = centered_max_abs()
    g = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 2, 3, gpu.DistType.GaussDist(4.578))
    ints = g.coeffs_ints(np.int64)
    assert int(np.abs(ints).max()) == g.centered_max_abs() > 0
    assert np.abs(ints).max(axis=2).tolist() == g.centered_max_abs(axis="entries")


def test_sampled_operands(gpu):
    """a uniform sample as the sampler leaves it (three-byte residues where the context allows them) and a Gaussian one"""
    p = _params(gpu, 256, 24, 3)
    Q = math.prod(p.moduli())
    u = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 2, 2, gpu.DistType.FinRingDist())
    quarter = (Q // 2) >> 1
    assert u.layout == "packed24"
    bits = u.extract_bits_with_threshold()
    v = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 2, 2, gpu.DistType.FinRingDist())
    assert v.layout == "packed24"
    assert np.array_equal(v.coeffs_ints(np.uint64, strict=False), (np.array(v.coeffs(), dtype=object) & U64).astype(np.uint64))
    ints, count, _ = u.coeffs_ints_misfits(np.uint64)
    coeffs = u.coeffs()
    want = np.array([[[quarter <= c < 3 * quarter for c in poly] for poly in row] for row in coeffs], dtype=bool)
    assert want.any() and not want.all() and np.array_equal(bits, want)
    assert np.array_equal(ints, np.array([[[c & U64 for c in poly] for poly in row] for row in coeffs], dtype=np.uint64))
    assert count == sum(c > U64 for row in coeffs for poly in row for c in poly)


# ---- the polynomial mirror -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits,L", [(64, 24, 3), (32, 62, 17)])
def test_poly_methods_match_their_host_forms(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    Q = p.modulus()
    rnd = random.Random(SEED + 23 * L)
    Poly = gpu.GpuDCRTPoly
    quarter = (Q // 2) >> 1
    vals = [rnd.randrange(Q) for _ in range(n - 6)] + [quarter - 1, quarter, 3 * quarter - 1, 3 * quarter, 0, Q - 1]
    poly = Poly.from_biguints(p, vals)
    got = poly.extract_bits_with_threshold()
    assert isinstance(got, list) and got == poly._extract_bits_with_threshold_host() == [quarter <= c < 3 * quarter for c in vals]
    assert True in got and False in got
    low = Poly.from_u64_vecs(p, [[v % p.moduli()[0]] for v in vals])  # level 0: the caps at the level's modulus
    assert low.level() == 0 and low.extract_bits_with_threshold() == low._extract_bits_with_threshold_host()

    bools = [rnd.random() < 0.5 for _ in range(n)]
    bp = Poly.from_bool_vec(p, bools)
    assert bp.to_bool_vec() == bools == bp._to_bool_vec_host()
    for bad in (2, Q - 1, 1 << 33):
        planted = [int(b) for b in bools]
        planted[n // 2] = bad
        pp = Poly.from_biguints(p, planted)
        with pytest.raises(ValueError) as new:
            pp.to_bool_vec()
        with pytest.raises(ValueError) as old:
            pp._to_bool_vec_host()
        assert str(new.value) == str(old.value) == f"Coefficient is not 0 or 1: {bad}"

    for c0 in (0, 5, (1 << 64) - 1, rnd.randrange(1 << 64)):
        cp = Poly.from_biguints(p, [c0] + vals[1:])
        assert cp.const_coeff_u64() == c0 == cp._const_coeff_u64_host()
        assert isinstance(cp.const_coeff_u64(), int)
    if Q > 1 << 64:
        for c0 in (1 << 64, Q - 1):
            cp = Poly.from_biguints(p, [c0, 1, 2])
            with pytest.raises(OverflowError) as new:
                cp.const_coeff_u64()
            with pytest.raises(OverflowError) as old:
                cp._const_coeff_u64_host()
            assert str(new.value) == str(old.value) == f"constant coefficient does not fit in u64: {c0}"

    digits = [rnd.randrange(1 << 32) for _ in range(n - 2)] + [0, (1 << 32) - 1]
    digits = [d % Q for d in digits]
    dp = Poly.from_biguints(p, digits)
    assert dp.coeffs_digits() == digits == dp.coeffs()
    if Q > 1 << 32:
        with pytest.raises(OverflowError):
            Poly.from_biguints(p, [1, 1 << 32]).coeffs_digits()


# ---- shapes, launches, refusals ------------------------------------------------------------------------------------------
def test_shapes_and_launch_budget(gpu):
    from mxx_amd import _ffi

    n = 64
    p = _params(gpu, n, 51, 4)
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + 1)
    M = gpu.GpuDCRTPolyMatrix
    lo, hi = Q // 3, Q - Q // 7
    wpc = -(-Q.bit_length() // 64)
    for rows, cols in ((1, 1), (3, 4), (9, 1)):
        values = [rnd.randrange(Q) if rnd.random() < 0.7 else rnd.randrange(1 << 30) for _ in range(rows * cols * n)]
        res = _residues(values, moduli, rows, cols, n)
        a = M.from_rns(p, res, False)
        e = M.from_rns(p, res, False)
        e.ntt_all_in_place()
        want_bits = _want_bits(values, lo, hi, rows, cols, n)
        want_ints, bad = _want_ints(values, Q, np.int64)
        words = np.empty((rows, cols, n, wpc), dtype=np.uint64)
        for m in (a, e):
            c0 = _launches()
            assert _ffi.lib().gpupoly_matrix_store_coeff_words(m.raw, words.ctypes.data_as(C.POINTER(C.c_uint64)), wpc) == 0
            older = _launches() - c0  # one kernel, and for an EVAL input the scratch inverse transform in front of it
            assert older == 1 if not m.is_ntt else older >= 2
            c0 = _launches()
            assert np.array_equal(m.extract_bits(lo, hi), want_bits)
            assert _launches() - c0 == older
            c0 = _launches()
            got, count, _ = m.coeffs_ints_misfits(np.int64)
            assert _launches() - c0 == older
            assert got.reshape(-1).tolist() == want_ints and count == sum(bad)
    for rows, cols in ((0, 3), (3, 0), (0, 0)):
        z = M(p, rows, cols, len(moduli) - 1, True)
        c0 = _launches()
        assert z.extract_bits(lo, hi).shape == (rows, cols, n)
        assert z.coeffs_ints(np.uint32).shape == (rows, cols, n)
        st, buf = _raw_bits(z, lo, hi, n // 8)
        assert st == 0
        st, _, count, first = _raw_ints(z, np.int32, 1, n)
        assert st == 0 and count == 0 and first == U64
        assert _launches() == c0


def test_more_tasks_than_a_grid_dimension(gpu):
    """n = 2 with one limb and 1025 x 1025 entries: sub-byte slots, thousands of blocks, an entry count that is no multiple
    of the 32 entries a wave holds"""
    n = 2
    p = _params(gpu, n, 24, 1)
    q = p.moduli()[0]
    rows = cols = 1025
    rng = np.random.default_rng(SEED)
    res = rng.integers(0, q, size=(rows, cols, 1, n), dtype=np.uint64)
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, res, False)
    lo, hi = q // 4, q // 2 + 5
    want = (res[:, :, 0, :] >= lo) & (res[:, :, 0, :] < hi)
    assert np.array_equal(m.extract_bits(lo, hi), want)
    st, buf = _raw_bits(m, lo, hi, 2)
    assert st == 0 and not buf[..., 1].any()
    assert np.array_equal(buf[..., 0], want[..., 0].astype(np.uint8) | (want[..., 1].astype(np.uint8) << 1))
    centred = np.where(res[:, :, 0, :] > q // 2, res[:, :, 0, :].astype(np.int64) - q, res[:, :, 0, :].astype(np.int64))
    got, count, first = m.coeffs_ints_misfits(np.int32)
    assert count == 0 and first is None and np.array_equal(got, centred.astype(np.int32))


def test_refusals_write_nothing(gpu):
    from mxx_amd import _ffi

    n = 16
    p = _params(gpu, n, 60, 5)
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + 2)
    values = [rnd.randrange(Q) for _ in range(2 * n)]
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, _residues(values, moduli, 1, 2, n), False)
    res = m.to_rns()
    lib = _ffi.lib()
    wq = -(-Q.bit_length() // 64)
    assert wq == 5
    c0 = _launches()

    def refused_bits(st, buf, what):
        assert st != 0, what
        assert "gpupoly_matrix_extract_bits" in _ffi.last_error_string(), what
        assert (buf == 0xA5).all(), what

    refused_bits(*_raw_bits(m, 1, 2, 2, wpb=0), "words_per_bound = 0")
    refused_bits(*_raw_bits(m, Q + 1, 2, 2), "lo above Q")
    refused_bits(*_raw_bits(m, 1, Q + 1, 2), "hi above Q")
    refused_bits(*_raw_bits(m, 1, 1 << (64 * wq), 2, wpb=wq + 1), "non-zero word above Q's words")
    refused_bits(*_raw_bits(m, 1 << (64 * (wq + 1)), 2, 2, wpb=wq + 2), "non-zero word above Q's words")
    refused_bits(*_raw_bits(m, 1, 2, 1), "bytes_per_poly below ceil(N / 8)")
    buf = np.full((1, 2, 2), 0xA5, dtype=np.uint8)
    u8 = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    one, two = _words(1, wq), _words(2, wq)
    for args in ((None, one, two, wq, u8, 2), (m.raw, None, two, wq, u8, 2), (m.raw, one, None, wq, u8, 2),
                 (m.raw, one, two, wq, None, 2)):
        refused_bits(lib.gpupoly_matrix_extract_bits(*args), buf, "null argument")
    # a one-word bound is fine where it says what is meant: Q's own word count is not required
    st, buf = _raw_bits(m, 1, 2, 2, wpb=1)
    assert st == 0 and np.array_equal(np.unpackbits(buf, axis=-1, bitorder="little").astype(bool), _want_bits(values, 1, 2, 1, 2, n))
    assert _launches() == c0 + 1

    c0 = _launches()

    def refused_ints(ret, what):
        st, buf, count, first = ret
        assert st != 0, what
        assert "gpupoly_matrix_store_coeff_ints" in _ffi.last_error_string(), what
        assert (buf.view(np.uint8) == 0x5A).all() and count == 0xC0 and first == 0xF1, what

    for eb in (0, 1, 2, 3, 5, 16, -4):
        refused_ints(_raw_ints(m, np.uint64, 0, n, elem_bytes=eb), f"elem_bytes = {eb}")
    refused_ints(_raw_ints(m, np.int64, 1, n + 1), "coeffs_per_poly above N")
    ints = np.full((1, 2, n), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    count, first = C.c_uint64(0xC0), C.c_uint64(0xF1)
    vp = C.c_void_p(ints.ctypes.data)
    for args in ((None, vp, 8, 0, n, C.byref(count), C.byref(first)), (m.raw, None, 8, 0, n, C.byref(count), C.byref(first)),
                 (m.raw, vp, 8, 0, n, None, C.byref(first)), (m.raw, vp, 8, 0, n, C.byref(count), None)):
        refused_ints((lib.gpupoly_matrix_store_coeff_ints(*args), ints, count.value, first.value), "null argument")
    assert _launches() == c0
    assert not m.is_ntt and np.array_equal(m.to_rns(), res)
    with pytest.raises(ValueError):
        m.extract_bits(0, Q + 1)
