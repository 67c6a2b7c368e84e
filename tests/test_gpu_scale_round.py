"""GPU: exact scale-and-round (`gpupoly_matrix_scale_round`) and the coefficient-word store
(`gpupoly_matrix_store_coeff_words`) against plain Python big integers, and the host mirror's `modulus_switch`,
`decode_centered` and `coeffs()` that ride on them.

Expected values come from the definitions alone: floor((t c + h) / Q) mod t with h = 0 (modulus_switch,
src/element/finite_ring.rs:22-26) or h = floor(Q/2) (decode_centered_masked_integer_coeff,
src/decoder/masked_high_bit.rs:21-29), Q the full modulus, the result stored mod every limb.  Every width class,
limb counts on both sides of the kernel's 8 / 16 / 64 bounds, COEFF and EVAL inputs and out == in; beyond random
coefficients, 0, Q - 1, floor(Q/2), floor(Q/2) + 1 and the exact boundaries where the floor changes.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261016
AUX_M = (1 << 64) - 59  # the kernel's auxiliary prime: t must lie below it
MAX_T = AUX_M - 1

# (n, bits, limbs): 10-24-bit lazy, 28-bit tight, 31-bit, 51-bit (f64 transforms), 52-62-bit integer u64
CELLS = [
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

_PARAMS = {}


def _params(gpu, n, bits, L):
    key = (n, bits, L)
    if key not in _PARAMS:
        moduli = P.primes(n, bits, L)
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, moduli, 1)
    return _PARAMS[key]


def _boundaries(Q, t, h, ks):
    """c = ceil((k Q - h) / t) and c - 1 for each k: the floor of (t c + h) / Q steps from k - 1 to k between them."""
    out = []
    for k in ks:
        c = -(-(k * Q - h) // t)
        out.extend(x for x in (c, c - 1) if 0 <= x < Q)
    return out


def _values(Q, t, h, count, seed):
    ks = sorted({k for k in (1, 2, 3, t // 2, t - 1, t) if k >= 1})
    vals = list(dict.fromkeys([0, Q - 1, Q // 2, Q // 2 + 1] + _boundaries(Q, t, h, ks)))
    rnd = random.Random(seed)
    return vals + [rnd.randrange(Q) for _ in range(count - len(vals))]


def _residues(vals, moduli, cols, n):
    """(1, cols, L, n) residues of the values, coefficient j of entry c = vals[c * n + j]"""
    arr = np.asarray(vals, dtype=object).reshape(cols, n)
    return np.stack([(arr % q).astype(np.uint64) for q in moduli], axis=1)[None]


def _expected(vals, Q, t, h, moduli, cols, n):
    w = np.asarray([((t * c + h) // Q) % t for c in vals], dtype=np.uint64).reshape(cols, n)  # < t < 2^64
    return np.stack([w % np.uint64(q) for q in moduli], axis=1)[None]


def _call(out, inp, t, round_half):
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_matrix_scale_round(out.raw, inp.raw, t, round_half)


@pytest.mark.parametrize("n,bits,L", CELLS)
def test_scale_round_matches_big_integers(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    assert Q == p.modulus()
    M = gpu.GpuDCRTPolyMatrix
    ts = [1, 2, 3, 1 << 7, moduli[0], (1 << 62) + 1, MAX_T]
    if Q < 1 << 40:
        ts.append(Q + 12345)  # above Q: the switched value wraps mod Q
    for it, t in enumerate(ts):
        for round_half in (0, 1):
            h = Q // 2 if round_half else 0
            need = 4 + 12 * 2
            cols = max(2, -(-need // n)) if n < 1 << 12 else 1
            vals = _values(Q, t, h, cols * n, SEED + 7 * it + round_half + n)
            res = _residues(vals, moduli, cols, n)
            want = _expected(vals, Q, t, h, moduli, cols, n)
            # COEFF input, separate output: the input is left as it was
            a = M.from_rns(p, res, False)
            out = M(p, 1, cols, L - 1, True)
            assert _call(out, a, t, round_half) == 0
            out.is_ntt = False  # the entry tags its output COEFF: to_rns() in COEFF format reads it only then
            assert np.array_equal(out.to_rns(), want), (t, round_half)
            assert not a.is_ntt and np.array_equal(a.to_rns(), res)
            # EVAL input, separate output: the scratch inverse transform does not touch the input
            e = M.from_rns(p, res, False)
            e.ntt_all_in_place()
            e_rns = e.to_rns()
            out2 = M(p, 1, cols, L - 1, False)
            assert _call(out2, e, t, round_half) == 0
            assert np.array_equal(out2.to_rns(), want), (t, round_half, "eval")
            assert np.array_equal(e.to_rns(), e_rns)  # still EVAL-tagged and unchanged
            # out == in, from either format
            src = e if round_half else a
            assert _call(src, src, t, round_half) == 0
            src.is_ntt = False
            assert np.array_equal(src.to_rns(), want), (t, round_half, "in place")


@pytest.mark.parametrize("n,bits,L", [(16, 24, 1), (64, 31, 2), (256, 24, 9), (128, 57, 16), (32, 62, 17), (16, 60, 64)])
def test_store_coeff_words_matches_crt_and_refuses_short_words(gpu, n, bits, L):
    from mxx_amd import _ffi

    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    vals = _values(Q, 3, 0, 3 * n, SEED + L)
    res = _residues(vals, moduli, 3, n)
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, res, False)
    e = m.ensure_eval()
    e_rns = e.to_rns()

    def old_formula(rns, mods):  # coeffs() before the device store: sum of residue * CRT weight, mod Q
        QQ = math.prod(mods)
        weights = [(QQ // q) * pow(QQ // q, -1, q) for q in mods]
        return [[[sum(int(rns[r, c, l, i]) * w for l, w in enumerate(weights)) % QQ for i in range(rns.shape[-1])]
                 for c in range(rns.shape[1])] for r in range(rns.shape[0])]

    want = old_formula(res, moduli)
    assert want == [[vals[c * n:(c + 1) * n] for c in range(3)]]
    assert m.coeffs() == want
    assert e.coeffs() == want and e.is_ntt and np.array_equal(e.to_rns(), e_rns)  # input untouched
    if L > 1:  # below full level: the value mod Q_level
        low = gpu.GpuDCRTPolyMatrix.from_rns(p, res[:, :, : L - 1], False)
        assert low.coeffs() == old_formula(res[:, :, : L - 1], moduli[: L - 1])
    # the raw entry: extra words are zero, fewer than the modulus needs are refused
    wpc = -(-Q.bit_length() // 64)
    lib = _ffi.lib()
    buf = np.full((1, 3, n, wpc + 2), 7, dtype=np.uint64)
    assert lib.gpupoly_matrix_store_coeff_words(m.raw, buf.ctypes.data_as(C.POINTER(C.c_uint64)), wpc + 2) == 0
    assert not buf[..., wpc:].any()
    got = [sum(int(buf[0, c, i, w]) << (64 * w) for w in range(wpc)) for c in range(3) for i in range(n)]
    assert got == vals
    short = np.full((1, 3, n, wpc), 7, dtype=np.uint64)
    c0 = lib.gpupoly_launch_count()
    assert lib.gpupoly_matrix_store_coeff_words(m.raw, short.ctypes.data_as(C.POINTER(C.c_uint64)), wpc - 1) != 0
    assert "words_per_coeff" in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and (short == 7).all()


def _decode_coeff(c, Q, t):
    """decode_centered_masked_integer_coeff (src/decoder/masked_high_bit.rs:21-29)"""
    assert t > 1
    return ((t * c + Q // 2) // Q) % t


@pytest.mark.parametrize("n,bits,L", [(256, 28, 3), (64, 51, 9), (32, 62, 17)])
def test_mirror_uses_the_device_and_matches_the_host_paths(gpu, monkeypatch, n, bits, L):
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    M = gpu.GpuDCRTPolyMatrix
    vals = _values(Q, 1 << 20, 0, 2 * 2 * n, SEED + n)
    res = np.concatenate([_residues(vals[: 2 * n], moduli, 2, n), _residues(vals[2 * n:], moduli, 2, n)])
    m = M.from_rns(p, res, True)  # EVAL, as matrices usually are
    before = m.to_rns()
    hosts = {t: (m._modulus_switch_host(t), m._decode_centered_host(t)) for t in (2, 3, 1 << 20, moduli[0], MAX_T)}

    def boom(*a, **k):
        raise AssertionError("host path taken")

    monkeypatch.setattr(M, "_modulus_switch_host", boom)
    monkeypatch.setattr(M, "_decode_centered_host", boom)
    flat_c = [c for row in m.coeffs() for poly in row for c in poly]
    for t, (h_sw, h_dc) in hosts.items():
        sw, dc = m.modulus_switch(t), m.decode_centered(t)
        for got, host in ((sw, h_sw), (dc, h_dc)):
            assert got.is_ntt and host.is_ntt and got.level == host.level == L - 1
            assert (got.nrow, got.ncol) == (2, 2)
            assert np.array_equal(got.to_rns(), host.to_rns()), t
        assert [c for row in sw.coeffs() for poly in row for c in poly] == [P.modulus_switch(c, Q, t) % Q for c in flat_c]
        assert [c for row in dc.coeffs() for poly in row for c in poly] == [_decode_coeff(c, Q, t) % Q for c in flat_c]
    assert m.is_ntt and np.array_equal(m.to_rns(), before)
    # the poly form rides on the same coeffs()
    assert m.entry(1, 0).coeffs() == flat_c[2 * n: 3 * n]
    assert M.from_rns(p, res, False).entry(1, 0).coeffs() == vals[2 * n: 3 * n]


def test_unsupported_inputs_fall_back_to_the_host_path(gpu, monkeypatch):
    from mxx_amd import _ffi

    n, bits, L = 64, 28, 4
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    Q = math.prod(moduli)
    M = gpu.GpuDCRTPolyMatrix
    vals = _values(Q, 5, 0, 2 * n, SEED)
    res = _residues(vals, moduli, 2, n)
    m = M.from_rns(p, res, False)
    calls = []
    real_sw, real_dc = M._modulus_switch_host, M._decode_centered_host
    monkeypatch.setattr(M, "_modulus_switch_host", lambda self, t: calls.append(("sw", t)) or real_sw(self, t))
    monkeypatch.setattr(M, "_decode_centered_host", lambda self, t: calls.append(("dc", t)) or real_dc(self, t))
    lib = _ffi.lib()
    # t at or above the auxiliary prime: the entry says "unsupported" and launches nothing
    for t in (AUX_M, (1 << 64) - 1):
        out = M.from_rns(p, res, True)
        c0 = lib.gpupoly_launch_count()
        assert _call(out, m, t, 0) != 0 and "unsupported" in _ffi.last_error_string()
        assert lib.gpupoly_launch_count() == c0 and out.is_ntt and np.array_equal(out.to_rns(), res)
    for t in (AUX_M, (1 << 64) + 7, 1 << 80):
        calls.clear()
        sw, dc = m.modulus_switch(t), m.decode_centered(t)
        assert calls == [("sw", t), ("dc", t)]
        assert sw.is_ntt and sw.level == L - 1
        assert [c for row in sw.coeffs() for poly in row for c in poly] == [P.modulus_switch(c, Q, t) % Q for c in vals]
        assert [c for row in dc.coeffs() for poly in row for c in poly] == [_decode_coeff(c, Q, t) % Q for c in vals]
    # an input below full level: "unsupported" from the entry, the host path (coeffs mod Q_level, full Q) in the mirror
    low = M.from_rns(p, res[:, :, : L - 1], False)
    Ql = math.prod(moduli[: L - 1])
    out = M.from_rns(p, res, True)
    c0 = lib.gpupoly_launch_count()
    assert _call(out, low, 7, 0) != 0 and "unsupported" in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and out.is_ntt and np.array_equal(out.to_rns(), res)
    calls.clear()
    sw = low.modulus_switch(7)
    assert calls == [("sw", 7)] and sw.is_ntt and sw.level == L - 1
    assert [c for row in sw.coeffs() for poly in row for c in poly] == [P.modulus_switch(c % Ql, Q, 7) for c in vals]


def test_refusals_launch_nothing_and_leave_the_output_alone(gpu):
    from mxx_amd import _ffi

    n, bits, L = 64, 24, 3
    p = _params(gpu, n, bits, L)
    other = _params(gpu, n, 24, L + 1)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    res = _residues(_values(math.prod(moduli), 3, 0, 2 * n, SEED), moduli, 2, n)
    inp = M.from_rns(p, res, False)
    sentinel = np.flip(res, axis=-1).copy()
    narrow = M.from_rns(p, res[:, :1], False)
    foreign = M.from_rns(other, _residues([1] * 2 * n, other.moduli(), 2, n), False)
    low_out = M.from_rns(p, sentinel[:, :, : L - 1], True)
    lib = _ffi.lib()
    cases = {
        "null output": lambda out: lib.gpupoly_matrix_scale_round(None, inp.raw, 5, 0),
        "null input": lambda out: lib.gpupoly_matrix_scale_round(out.raw, None, 5, 1),
        "t = 0": lambda out: _call(out, inp, 0, 0),
        "shape": lambda out: _call(out, narrow, 5, 0),
        "context": lambda out: _call(out, foreign, 5, 0),
        "level": lambda out: _call(low_out, inp, 5, 0),
    }
    for name, fn in cases.items():
        out = M.from_rns(p, sentinel, True)  # EVAL-tagged: a tag flipped to COEFF would make to_rns() fail
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        assert "gpupoly_matrix_scale_round" in _ffi.last_error_string(), name
        assert lib.gpupoly_launch_count() == c0, name
        assert out.is_ntt and np.array_equal(out.to_rns(), sentinel), name
    # the output below full level is the one refused there: it is left alone too
    assert _call(low_out, inp, 5, 0) != 0 and "level" in _ffi.last_error_string()
    assert low_out.is_ntt and np.array_equal(low_out.to_rns(), sentinel[:, :, : L - 1])
    with pytest.raises(AssertionError):
        inp.decode_centered(1)
