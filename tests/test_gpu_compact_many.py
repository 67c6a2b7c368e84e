"""GPU: the compact wire format for many matrices per call (`gpupoly_matrix_store_compact_bytes_many`,
`gpupoly_matrix_load_compact_bytes_many`, the `*_compact_bytes_many` mirror and mxx_amd/storage.py).

Every comparison is exact (bytes and integers).  Expected values come from the one-matrix entries - whose code the batched
entries do not share on the fast path - AND from the CPU packing `oracle.compact_payload`.
"""
import ctypes as C

import numpy as np
import pytest

import ran
from conftest import make_params, rand_matrix

pytestmark = pytest.mark.gpu

FILL = 0xAB


def _lib():
    from mxx_amd import _ffi

    return _ffi.lib()


def _err():
    from mxx_amd import _ffi

    return _ffi.last_error_string()


def _signed(rng, shape, n, moduli, magnitude):
    """residues (rows, cols, L, n) of integers drawn from [-magnitude, magnitude]"""
    v = rng.integers(-magnitude, magnitude + 1, size=tuple(shape) + (n,), dtype=np.int64)
    return np.stack([np.mod(v, q).astype(np.uint64) for q in moduli], axis=-2)


def _cap_of(m):
    bits_upper = sum(q.bit_length() for q in m.params.moduli()[: m.level + 1]) + 1
    return (m.nrow * m.ncol * m.params.ring_dimension() * bits_upper + 7) // 8 + 16


def store_one(m):
    """the one-matrix entry on `m` itself -> (max_coeff_bits, bytes_per_coeff, payload)"""
    cap = _cap_of(m)
    buf = (C.c_uint8 * cap)()
    bits, bpc, plen = C.c_uint16(0), C.c_uint16(0), C.c_size_t(0)
    st = _lib().gpu_matrix_store_compact_bytes(m.raw, buf, cap, C.byref(bits), C.byref(bpc), C.byref(plen))
    assert st == 0, _err()
    m.is_ntt = False
    return bits.value, bpc.value, bytes(buf[: plen.value])


def store_many_raw(ms, capacity=None, raws=None):
    """the batched entry on `ms` themselves -> (status, widths, bpcs, offsets, lens, total, the whole buffer)"""
    n = len(ms)
    cap = sum(_cap_of(m) + 8 for m in ms) if capacity is None else capacity
    buf = (C.c_uint8 * max(cap, 1))()
    C.memset(buf, FILL, max(cap, 1))
    arr = (C.c_void_p * max(n, 1))(*(raws if raws is not None else [m.raw for m in ms]))
    bits, bpcs = (C.c_uint16 * max(n, 1))(), (C.c_uint16 * max(n, 1))()
    offs, lens, total = (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))(), C.c_size_t(12345)
    st = _lib().gpupoly_matrix_store_compact_bytes_many(arr, n, buf, cap, bits, bpcs, offs, lens, C.byref(total))
    return st, list(bits)[:n], list(bpcs)[:n], list(offs)[:n], list(lens)[:n], total.value, bytes(buf)


def store_many(ms):
    """-> [(width, bpc, payload)] after checking the layout of the buffer: offsets, zero padding, total"""
    st, bits, bpcs, offs, lens, total, buf = store_many_raw(ms)
    assert st == 0, _err()
    for m in ms:
        m.is_ntt = False
    at = 0
    for j in range(len(ms)):
        assert offs[j] % 8 == 0 and offs[j] == (at + 7) // 8 * 8, (j, offs, lens)
        assert buf[at : offs[j]] == bytes(offs[j] - at), f"padding before payload {j} is not zero"
        at = offs[j] + lens[j]
    assert total == at and (not ms or offs[0] == 0)
    assert all(b == FILL for b in buf[total:]), "bytes past out_total_len were written"
    return [(bits[j], bpcs[j], buf[offs[j] : offs[j] + lens[j]]) for j in range(len(ms))]


def load_many_raw(ms, payloads, widths, lens=None):
    n = len(ms)
    arr = (C.c_void_p * max(n, 1))(*[m.raw for m in ms])
    keep = [bytes(p) if len(p) else b"\0" for p in payloads]
    ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(k), C.c_void_p) for k in keep])
    ls = (C.c_size_t * max(n, 1))(*(lens if lens is not None else [len(p) for p in payloads]))
    ws = (C.c_uint16 * max(n, 1))(*widths)
    return _lib().gpupoly_matrix_load_compact_bytes_many(arr, n, ptrs, ls, ws)


def _matrix(gpu, p, coeff, eval_format):
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, coeff, False)
    if eval_format:
        m.ntt_all_in_place()
    return m


def _mixed_batch(gpu, oracle, p, big_shape, seed):
    """16 matrices: shapes 1x1, 3x5, big_shape, an empty 0x4, a zero matrix; magnitudes from 0 through width 2, ~20, ~47 to
    uniform; COEFF and EVAL alternating.  -> (coefficient residues, matrices)"""
    moduli, n = p.moduli(), p.ring_dimension()
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (3, 5), big_shape, (0, 4), (2, 2)]
    mags = [1, 2 ** 19, 2 ** 46, None, 0, 1, 2 ** 46, None]  # None: uniform residues; 0: the zero matrix
    coeffs, ms = [], []
    for j in range(16):
        shape, mag = shapes[j % len(shapes)], mags[j % len(mags)]
        if mag is None:
            c = rand_matrix(oracle, seed + j, shape[0], shape[1], moduli, n) if shape[0] else np.zeros(shape + (len(moduli), n), np.uint64)
        else:
            c = _signed(rng, shape, n, moduli, mag)
            if mag == 1 and c.size:
                c[0, 0, :, 0] = 1  # a tiny ring may draw only zeros: the width is 2 for certain
        coeffs.append(c)
        ms.append(_matrix(gpu, p, c, j % 2 == 1))
    return coeffs, ms


def _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got, use_oracle=True):
    for j, (c, m, (bits, bpc, payload)) in enumerate(zip(coeffs, ms, got)):
        moduli = m.params.moduli()[: m.level + 1]
        ref = _matrix_like(m, c)
        assert (bits, bpc, payload) == store_one(ref), f"matrix {j} differs from the one-matrix entry"
        if c.size and use_oracle:
            wp, wb, wc = oracle.compact_payload(c, moduli)
            assert (bits, bpc) == (wb, wc) and payload == wp, f"matrix {j} differs from the oracle"
        else:
            assert (bits, bpc, payload) == (0, 0, b"") or not use_oracle
        # the input is now in the coefficient domain (the device refuses to_rns in a format the matrix is not tagged with)
        assert not m.is_ntt and np.array_equal(m.to_rns(), c), f"matrix {j} is not INTT of what it was"


def _matrix_like(m, coeff):
    return type(m).from_rns(m.params, coeff, False)


@pytest.mark.parametrize("n,depth,bits,big_shape", [
    (4, 2, 17, (76, 4)), (16, 3, 24, (76, 4)), (64, 3, 51, (76, 4)), (256, 5, 24, (76, 4)), (256, 12, 51, (76, 4)),
    (4096, 3, 24, (7, 3)), (4096, 2, 51, (7, 3)), (16384, 2, 24, (2, 3)),
])
def test_sixteen_mixed_matrices_in_one_call(gpu, oracle, n, depth, bits, big_shape):
    p = make_params(gpu, oracle, n, depth, bits, 12 if bits == 24 else 1 if bits == 17 else 17)
    coeffs, ms = _mixed_batch(gpu, oracle, p, big_shape, 1000 + n + bits)
    got = store_many(ms)
    widths = [g[0] for g in got]
    print(f"n={n} bits={bits}: widths {widths}")
    assert 0 in widths and 2 in widths and max(widths) > 30  # really mixed
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)
    # and back: the batched load of what the batched store wrote
    back = [gpu.GpuDCRTPolyMatrix(p, m.nrow, m.ncol, m.level, True) for m in ms]
    assert load_many_raw(back, [g[2] for g in got], widths) == 0, _err()
    for j, (b, m) in enumerate(zip(back, ms)):
        b.is_ntt = False
        assert b == m, f"matrix {j} did not come back"


def test_a_packed24_uniform_sample_among_the_inputs(gpu, oracle):
    n = 1024
    p = make_params(gpu, oracle, n, 3, 24, 12)
    moduli = p.moduli()
    seed = gpu.GpuRngSeed.from_bytes(bytes((7 * i + 3) & 0xFF for i in range(32)))
    uni = gpu.GpuDCRTPolyMatrix.sample_distribution(p, 2, 3, gpu.DistType.FinRingDist().as_ffi(), 0.0, seed)
    assert uni.layout == "packed24" and uni.is_ntt
    want = uni.clone()
    rng = np.random.default_rng(5)
    c0, c2 = _signed(rng, (1, 2), n, moduli, 3), _signed(rng, (2, 1), n, moduli, 2 ** 30)
    ms = [_matrix(gpu, p, c0, False), uni, _matrix(gpu, p, c2, True)]
    got = store_many(ms)
    want_coeff = want.to_coeff_rns()
    assert got[1] == store_one(want)
    assert got[1][2] == oracle.compact_payload(want_coeff, moduli)[0]
    assert np.array_equal(uni.to_rns(), want_coeff)
    assert got[0] == store_one(_matrix(gpu, p, c0, False)) and got[2] == store_one(_matrix(gpu, p, c2, False))


def test_widths_are_per_matrix_and_neighbours_stay_intact(gpu, oracle):
    """a width-2 matrix between two wide ones keeps width 2; its last workgroup assembles more words than the matrix owns
    (n * polys is not a multiple of 256) and must not write them: the next payload starts there"""
    n = 64
    p = make_params(gpu, oracle, n, 3, 51, 17)
    moduli = p.moduli()
    rng = np.random.default_rng(11)
    coeffs = [rand_matrix(oracle, 71, 3, 1, moduli, n), _signed(rng, (1, 3), n, moduli, 1), rand_matrix(oracle, 72, 1, 5, moduli, n)]
    ms = [_matrix(gpu, p, c, False) for c in coeffs]
    got = store_many(ms)
    assert got[1][0] == 2 and got[0][0] > 100 and got[2][0] > 100
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)


@pytest.mark.parametrize("n,depth,bits,mag_one,mag_two", [(256, 10, 24, 2 ** 22, 2 ** 45), (128, 12, 51, 2 ** 49, 2 ** 62)])
def test_both_fast_forms_and_the_general_path_in_one_batch(gpu, oracle, hip_env, n, depth, bits, mag_one, mag_two):
    p = make_params(gpu, oracle, n, depth, bits, 12)
    moduli = p.moduli()
    rng = np.random.default_rng(depth * 1000 + bits)
    planted = _signed(rng, (1, 2), n, moduli, 5)
    planted[0, 1, :, 7] = rand_matrix(oracle, 7, 1, 1, moduli, n)[0, 0, :, 7]  # one uniform residue vector: beyond both fast forms
    coeffs = [_signed(rng, (3, 4), n, moduli, mag_one), planted, _signed(rng, (3, 4), n, moduli, mag_two)]
    ms = [_matrix(gpu, p, c, False) for c in coeffs]
    c0 = _lib().gpupoly_launch_count()
    with ran.launches() as launched:
        got = store_many(ms)
    launches = _lib().gpupoly_launch_count() - c0
    if FORCED["test_both_fast_forms_and_the_general_path_in_one_batch"]["pairs"][("MXX_HIP_SERDE", None)](dict(depth=depth)):
        launched.assert_ran("MXX_HIP_SERDE", None, moduli)
    # one batched width launch + the general width kernel for the flagged matrix, one batched pack launch + its general pack
    assert launches == 2 + 2, f"{launches} launches: the flagged matrix must not take its neighbours off the batched kernels"
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)
    hip_env.set("MXX_HIP_SERDE", "general")
    ms2 = [_matrix(gpu, p, c, False) for c in coeffs]
    c0 = _lib().gpupoly_launch_count()
    with ran.launches() as launched:
        general = store_many(ms2)
    assert _lib().gpupoly_launch_count() - c0 == 2 * 3
    if FORCED["test_both_fast_forms_and_the_general_path_in_one_batch"]["pairs"][("MXX_HIP_SERDE", "general")](dict(depth=depth)):
        launched.assert_ran("MXX_HIP_SERDE", "general", moduli)
    hip_env.unset("MXX_HIP_SERDE")
    assert general == got


def test_a_context_with_more_than_sixteen_limbs(gpu, oracle):
    n = 64
    p = make_params(gpu, oracle, n, 18, 24, 12)
    moduli = p.moduli()
    rng = np.random.default_rng(18)
    coeffs = [_signed(rng, (2, 2), n, moduli, 9), rand_matrix(oracle, 81, 1, 3, moduli, n), np.zeros((1, 1, 18, n), np.uint64)]
    ms = [_matrix(gpu, p, c, j == 1) for j, c in enumerate(coeffs)]
    got = store_many(ms)
    assert [g[0] for g in got][2] == 0 and got[0][0] == 5
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)
    back = [gpu.GpuDCRTPolyMatrix(p, m.nrow, m.ncol, m.level, False) for m in ms]
    assert load_many_raw(back, [g[2] for g in got], [g[0] for g in got]) == 0, _err()
    assert all(b == m for b, m in zip(back, ms))


def test_mixed_levels_in_one_call(gpu, oracle):
    n = 256
    p = make_params(gpu, oracle, n, 5, 24, 12)
    moduli = p.moduli()
    rng = np.random.default_rng(21)
    levels = [5, 2, 5, 1, 3, 2, 5]
    coeffs = [_signed(rng, (2, 3), n, moduli[:L], 2 ** (7 * j + 1)) for j, L in enumerate(levels)]
    ms = [_matrix(gpu, p, c, j % 2 == 0) for j, c in enumerate(coeffs)]
    assert [m.level + 1 for m in ms] == levels
    got = store_many(ms)
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)
    back = [gpu.GpuDCRTPolyMatrix(p, 2, 3, m.level, False) for m in ms]
    c0 = _lib().gpupoly_launch_count()
    assert load_many_raw(back, [g[2] for g in got], [g[0] for g in got]) == 0, _err()
    assert _lib().gpupoly_launch_count() - c0 == len(set(levels))  # one launch per level
    assert all(b == m for b, m in zip(back, ms))


def test_sixty_seven_matrices_and_one(gpu, oracle):
    n = 16
    p = make_params(gpu, oracle, n, 3, 24, 12)
    moduli = p.moduli()
    rng = np.random.default_rng(67)
    coeffs = [_signed(rng, (1 + j % 3, 1 + j % 5), n, moduli, 2 ** (j % 60)) for j in range(67)]
    ms = [_matrix(gpu, p, c, j % 3 == 0) for j, c in enumerate(coeffs)]
    got = store_many(ms)
    _check_against_one_matrix_entry_and_oracle(oracle, coeffs, ms, got)
    back = [gpu.GpuDCRTPolyMatrix(p, m.nrow, m.ncol, m.level, False) for m in ms]
    assert load_many_raw(back, [g[2] for g in got], [g[0] for g in got]) == 0, _err()
    assert all(b == m for b, m in zip(back, ms))
    # n = 1 is the one-matrix entry
    one = _matrix(gpu, p, coeffs[5], True)
    assert store_many([one]) == [store_one(_matrix(gpu, p, coeffs[5], True))]
    # n = 0 does nothing
    c0 = _lib().gpupoly_launch_count()
    st, *_rest, total, _buf = store_many_raw([])
    assert st == 0 and total == 0 and load_many_raw([], [], []) == 0
    assert _lib().gpupoly_launch_count() == c0


def test_capacity_too_small_reports_everything_and_the_retry_succeeds(gpu, oracle):
    n = 256
    p = make_params(gpu, oracle, n, 5, 24, 12)
    moduli = p.moduli()
    rng = np.random.default_rng(31)
    coeffs = [_signed(rng, (2, 2), n, moduli, 2 ** 9), _signed(rng, (1, 3), n, moduli, 2 ** 33), np.zeros((1, 1, 5, n), np.uint64)]
    ms = [_matrix(gpu, p, c, j == 0) for j, c in enumerate(coeffs)]
    want = [store_one(_matrix(gpu, p, c, False)) for c in coeffs]
    want_total = 0
    for w in want:  # every payload at the next multiple of 8; the total is the last offset + the last length
        want_total = (want_total + 7) // 8 * 8 + len(w[2])
    st, bits, bpcs, offs, lens, total, buf = store_many_raw(ms, capacity=want_total - 1)
    assert st != 0 and "payload buffer too small in gpupoly_matrix_store_compact_bytes_many" in _err()
    assert bits == [w[0] for w in want] and bpcs == [w[1] for w in want] and lens == [len(w[2]) for w in want]
    assert total == want_total and offs[0] == 0 and offs[1] == (lens[0] + 7) // 8 * 8 and offs[2] == total
    assert all(b == FILL for b in buf), "payload_out was written by a refused call"
    st, bits2, bpcs2, offs2, lens2, total2, buf = store_many_raw(ms, capacity=total)
    assert st == 0, _err()
    assert (bits2, bpcs2, offs2, lens2, total2) == (bits, bpcs, offs, lens, total)
    assert [buf[o : o + ln] for o, ln in zip(offs, lens)] == [w[2] for w in want]


def test_load_many_and_the_one_matrix_entries_read_each_others_bytes(gpu, oracle):
    n = 256
    p = make_params(gpu, oracle, n, 12, 51, 17)
    moduli = p.moduli()
    rng = np.random.default_rng(41)
    coeffs = [_signed(rng, (76, 4), n, moduli, 2 ** 20), _signed(rng, (1, 1), n, moduli, 1), rand_matrix(oracle, 91, 2, 2, moduli, n),
              np.zeros((2, 1, 12, n), np.uint64), _signed(rng, (3, 5), n, moduli, 2 ** 60)]
    ms = [_matrix(gpu, p, c, False) for c in coeffs]
    many = store_many([m.clone() for m in ms])
    ones = [store_one(m.clone()) for m in ms]
    assert many == ones
    fresh = lambda: [gpu.GpuDCRTPolyMatrix(p, m.nrow, m.ncol, m.level, True) for m in ms]  # noqa: E731
    # load_many(store_many(ms)) == ms, and of payloads the one-matrix store produced
    for source in (many, ones):
        back = fresh()
        assert load_many_raw(back, [g[2] for g in source], [g[0] for g in source]) == 0, _err()
        for b, m in zip(back, ms):
            b.is_ntt = False  # the device tag is COEFF now: == reads both through their own format
            assert b == m and np.array_equal(b.to_rns(), m.to_rns())
    # the one-matrix load of payloads produced by store_many
    for (bits, _, payload), m in zip(many, ms):
        b = gpu.GpuDCRTPolyMatrix(p, m.nrow, m.ncol, m.level, False)
        buf = C.cast(C.c_char_p(payload if payload else b"\0"), C.POINTER(C.c_uint8))
        assert _lib().gpu_matrix_load_compact_bytes(b.raw, buf, len(payload), bits) == 0, _err()
        assert b == m


def test_refused_loads_leave_every_matrix_as_it_was(gpu, oracle):
    n = 64
    p = make_params(gpu, oracle, n, 3, 51, 17)
    moduli = p.moduli()
    rng = np.random.default_rng(51)
    c_first, c_last = rand_matrix(oracle, 95, 1, 2, moduli, n), _signed(rng, (2, 2), n, moduli, 100)
    first = gpu.GpuDCRTPolyMatrix.from_rns(p, c_first, True)  # tagged EVAL, contents c_first
    last = _matrix(gpu, p, c_last, False)
    bits, _, payload = store_one(last.clone())
    src_bits, _, src_payload = store_one(_matrix(gpu, p, _signed(rng, (1, 2), n, moduli, 3), False))
    c0 = _lib().gpupoly_launch_count()
    for lens, widths, payloads, text in [
        ([len(src_payload), len(payload) - 1], [src_bits, bits], [src_payload, payload], "payload length mismatch"),
        ([len(src_payload), 3], [src_bits, 0], [src_payload, payload], "must be zero"),
    ]:
        assert load_many_raw([first, last], payloads, widths, lens=lens) != 0
        assert text in _err() and "gpupoly_matrix_load_compact_bytes_many" in _err()
    # a null payload for the last matrix
    arr = (C.c_void_p * 2)(first.raw, last.raw)
    ptrs = (C.c_void_p * 2)(C.cast(C.c_char_p(src_payload), C.c_void_p), None)
    assert _lib().gpupoly_matrix_load_compact_bytes_many(arr, 2, ptrs, (C.c_size_t * 2)(len(src_payload), len(payload)),
                                                          (C.c_uint16 * 2)(src_bits, bits)) != 0
    assert "null payload" in _err()
    assert _lib().gpupoly_launch_count() == c0
    assert first.is_ntt and np.array_equal(first.to_rns(), c_first)  # to_rns in EVAL: the device tag is still EVAL
    assert np.array_equal(last.to_rns(), c_last)


def test_refused_stores_launch_nothing_and_write_nothing(gpu, oracle):
    n = 64
    p, other = make_params(gpu, oracle, n, 3, 51, 17), make_params(gpu, oracle, n, 2, 51, 17)
    rng = np.random.default_rng(61)
    c = rand_matrix(oracle, 97, 1, 2, p.moduli(), n)
    a = gpu.GpuDCRTPolyMatrix.from_rns(p, c, True)
    b = _matrix(gpu, p, _signed(rng, (1, 1), n, p.moduli(), 9), False)
    foreign = _matrix(gpu, other, _signed(rng, (1, 1), n, other.moduli(), 9), False)
    c0 = _lib().gpupoly_launch_count()
    for ms, raws, text in [([a, foreign], None, "different contexts"), ([a, b, a], None, "twice"), ([a, b], [a.raw, None], "null matrix")]:
        st, bits, bpcs, offs, lens, total, buf = store_many_raw(ms, raws=raws)
        assert st != 0 and text in _err() and "gpupoly_matrix_store_compact_bytes_many" in _err()
        assert total == 12345 and not any(bits) and not any(lens) and all(x == FILL for x in buf)
        if raws is None:  # the load refuses the same lists
            assert load_many_raw(ms, [b"\0"] * len(ms), [0] * len(ms), lens=[0] * len(ms)) != 0 and text in _err()
    assert _lib().gpupoly_launch_count() == c0
    assert a.is_ntt and np.array_equal(a.to_rns(), c)  # still tagged EVAL, contents as they were


def test_launch_budget(gpu, oracle):
    """derived, not measured: 16 COEFF matrices of one level on the fast path are one width launch and one pack launch, one
    unpack launch; in EVAL form the inverse transforms stay per matrix, so the batched call saves 16 * 2 - 2 launches"""
    n = 256
    p = make_params(gpu, oracle, n, 12, 51, 17)
    moduli = p.moduli()
    rng = np.random.default_rng(71)
    coeffs = [_signed(rng, (76, 4), n, moduli, 2 ** 27) for _ in range(16)]
    ms = [_matrix(gpu, p, c, False) for c in coeffs]
    lib = _lib()
    c0 = lib.gpupoly_launch_count()
    got = store_many(ms)
    assert lib.gpupoly_launch_count() - c0 == 2
    back = [gpu.GpuDCRTPolyMatrix(p, 76, 4, 11, False) for _ in ms]
    c0 = lib.gpupoly_launch_count()
    assert load_many_raw(back, [g[2] for g in got], [g[0] for g in got]) == 0, _err()
    assert lib.gpupoly_launch_count() - c0 == 1
    assert all(b == m for b, m in zip(back, ms))
    ev_loop, ev_many = [_matrix(gpu, p, c, True) for c in coeffs], [_matrix(gpu, p, c, True) for c in coeffs]
    c0 = lib.gpupoly_launch_count()
    loop = [store_one(m) for m in ev_loop]
    c1 = lib.gpupoly_launch_count()
    many = store_many(ev_many)
    c2 = lib.gpupoly_launch_count()
    assert many == loop == got
    assert (c2 - c1) == (c1 - c0) - 30, f"loop {c1 - c0} launches, batched {c2 - c1}"


def test_mirror_equals_the_one_matrix_methods(gpu, oracle):
    n = 256
    p, other = make_params(gpu, oracle, n, 5, 24, 12), make_params(gpu, oracle, 64, 3, 51, 17)
    rng = np.random.default_rng(81)
    ms = [_matrix(gpu, p, _signed(rng, (2, 3), n, p.moduli(), 2 ** 25), True),
          _matrix(gpu, other, _signed(rng, (1, 2), 64, other.moduli(), 7), False),  # a second context: grouped, order kept
          _matrix(gpu, p, rand_matrix(oracle, 99, 1, 2, p.moduli(), n), False),
          gpu.GpuDCRTPolyMatrix.zero(p, 2, 2),
          gpu.GpuDCRTPolyMatrix(p, 0, 4, 4, True)]
    want = [m.clone().into_compact_bytes() for m in ms]
    tags = [m.is_ntt for m in ms]
    assert gpu.GpuDCRTPolyMatrix.to_compact_bytes_many(ms) == want
    assert [m.is_ntt for m in ms] == tags  # operands untouched
    clones = [m.clone() for m in ms]
    assert gpu.GpuDCRTPolyMatrix.into_compact_bytes_many(clones) == want
    assert not any(c.is_ntt for c in clones)
    assert gpu.GpuDCRTPolyMatrix.into_compact_bytes_many([]) == []
    # frames with slot padding behind them; the one-matrix from_compact_bytes keeps its assertion
    same_ctx = [0, 2, 3, 4]
    padded = [want[j] + bytes(5 + 3 * j) for j in same_ctx]
    back = gpu.GpuDCRTPolyMatrix.from_compact_bytes_many(p, padded)
    for b, j in zip(back, same_ctx):
        assert (b.size(), b.level, b.is_ntt) == (ms[j].size(), ms[j].level, tags[j]), j
        # a matrix without entries has no contents to compare (and the device tags of two such need not agree: the mirror's
        # transforms skip them); every other one equals the operand and what the one-matrix method reads from the frame
        if b.nrow * b.ncol:
            assert b == ms[j] and b == gpu.GpuDCRTPolyMatrix.from_compact_bytes(p, want[j]), j
    with pytest.raises(AssertionError):
        gpu.GpuDCRTPolyMatrix.from_compact_bytes(p, padded[0])
    assert gpu.GpuDCRTPolyMatrix.from_compact_bytes_many(p, []) == []


def test_lookup_buffer_round_trip_of_a_batched_preimage(gpu, oracle):
    """the outputs of one gpupoly_trapdoor_preimage_many call at the M4 ring go through get_lookup_buffer and come back"""
    from mxx_amd import storage
    from mxx_amd.sampler import seed_source

    n, depth, bits, base, d = 256, 12, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    with seed_source([bytes((31 * t + 5 * i + 11) & 0xFF for i in range(32)) for t in range(3)]):
        td, A = sampler.trapdoor(p, d)
    targets = [gpu.GpuDCRTPolyMatrix.from_rns(p, rand_matrix(oracle, 7000 + j, d, 4, moduli, n), True) for j in range(5)]
    seeds = [tuple(gpu.GpuRngSeed.from_bytes(bytes((t * 17 + i) & 0xFF for i in range(32))) for t in (3 * j, 3 * j + 1, 3 * j + 2)) for j in range(5)]
    xs = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    indices = [12, 3, 40, 0, 7]
    data = storage.get_lookup_buffer(list(zip(indices, xs)))
    assert all(x.is_ntt for x in xs)  # serialised on clones
    got = storage.matrices_from_lookup_buffer(p, data)
    assert [k for k, _ in got] == sorted(indices)
    by_index = dict(zip(indices, xs))
    for k, m in got:
        assert m == by_index[k] and m.is_ntt
    # the buffer is the layout of the blobs the one-matrix method gives
    order = sorted(range(5), key=lambda j: indices[j])
    assert data == storage.lookup_buffer_from_blobs(sorted(indices), [xs[j].to_compact_bytes() for j in order])


# forced kernel paths (tests/ran.py): a matrix rides the batched kernels up to 16 limbs unless the switch says general
# (serde.hip: ManyItem::batched); evaluated over the parameter lists by tests/test_ran_table_host.py
FORCED = {
    "test_both_fast_forms_and_the_general_path_in_one_batch": {"pairs": {
        ("MXX_HIP_SERDE", None): lambda c: c["depth"] <= 16,
        ("MXX_HIP_SERDE", "general"): lambda c: c["depth"] <= 16}},
}
