"""GPU: rounded CRT recomposition in one call (`gpupoly_matrix_crt_recompose_rounded`) and the host
mirror's `crt_recompose_rows` / `crt_recompose_rows_terms` that ride on it.

Expected values come from plain Python big integers: limb i of row `slot` is floor((q_i c + floor(Q/2)) / Q) mod q_i for
c the coefficient of level (slot, i) (decode_centered_masked_integer_coeff, src/decoder/masked_high_bit.rs:21-29, with
t = q_i; the reconstruction coefficient of src/poly/mod.rs:45-60 is 1 mod q_i and 0 mod the other limbs).  Every width
class and limb counts on both sides of the rounding kernel's 8 / 16 / 64 bounds; beyond random coefficients, 0, Q - 1
(the v = q_i wrap), floor(Q/2), floor(Q/2) + 1 and the exact boundaries where the floor steps.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261019
ENTRY = "gpupoly_matrix_crt_recompose_rounded"

# (n, bits, limbs): 10-24-bit lazy, 28-bit tight, 31-bit, 51-bit (f64 transforms), 57-62-bit integer u64
CELLS = [
    (2, 10, 2), (16, 24, 1), (64, 20, 8), (256, 24, 9), (128, 28, 16), (64, 28, 17),
    (64, 31, 2), (64, 51, 8), (64, 51, 9), (32, 57, 16), (32, 62, 17), (16, 60, 64),
]

_PARAMS = {}


def _params(gpu, n, bits, L):
    key = (n, bits, L)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, L), 1)
    return _PARAMS[key]


def _decode(c, Q, q):
    return ((q * c + Q // 2) // Q) % q


def _specials(Q, q):
    """0, Q - 1, floor(Q/2), floor(Q/2) + 1 and, for k in {1, 2, q//2, q-1, q}, ceil((k Q - h) / q) and that minus 1:
    floor((q c + h) / Q) steps from k - 1 to k between the two."""
    h = Q // 2
    vals = [0, Q - 1, Q // 2, Q // 2 + 1]
    for k in (1, 2, q // 2, q - 1, q):
        c = -(-(k * Q - h) // q)
        vals.extend(x for x in (c, c - 1) if 0 <= x < Q)
    return list(dict.fromkeys(vals))


def _level_values(Q, q, count, slot, rnd):
    """count coefficients of one level: the specials (rotated by the slot, so that short levels cover them between the
    slots), then random ones"""
    sp = _specials(Q, q)
    off = (slot * count) % len(sp)
    sp = sp[off:] + sp[:off]
    return (sp + [rnd.randrange(Q) for _ in range(max(0, count - len(sp)))])[:count]


def _residues(vals, moduli, cols, n):
    """(1, cols, L, n) residues of the values, coefficient k of entry c = vals[c * n + k]"""
    arr = np.asarray(vals, dtype=object).reshape(cols, n)
    return np.stack([(arr % q).astype(np.uint64) for q in moduli], axis=1)[None]


def _expected(levels, moduli, num_slots, cols, n):
    """(num_slots, cols, L, n) COEFF residues of the recomposition of the integer levels[slot * L + i] (cols * n values)"""
    Q, L = math.prod(moduli), len(moduli)
    out = np.zeros((num_slots, cols, L, n), dtype=np.uint64)
    for s in range(num_slots):
        for i, q in enumerate(moduli):
            out[s, :, i, :] = np.asarray([_decode(c, Q, q) for c in levels[s * L + i]], dtype=np.uint64).reshape(cols, n)
    return out


def _matrix(gpu, p, vals, cols, eval_format):
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, _residues(vals, p.moduli(), cols, p.ring_dimension()), False)
    if eval_format:
        m.ntt_all_in_place()
    return m


def _random_levels(p, num_slots, cols, seed):
    moduli, n = p.moduli(), p.ring_dimension()
    Q, L = math.prod(moduli), len(moduli)
    rnd = random.Random(seed)
    return [_level_values(Q, moduli[j % L], cols * n, j // L, rnd) for j in range(num_slots * L)]


def _check_cell(gpu, p, num_slots, cols, seed):
    M = gpu.GpuDCRTPolyMatrix
    moduli, n = p.moduli(), p.ring_dimension()
    L = len(moduli)
    levels = _random_levels(p, num_slots, cols, seed)
    want = _expected(levels, moduli, num_slots, cols, n)
    for eval_format in (False, True):
        terms = [_matrix(gpu, p, v, cols, eval_format) for v in levels]
        before = [t.to_rns() for t in terms]
        out = M.crt_recompose_rows(p, terms, num_slots)
        assert out.is_ntt and out.level == L - 1 and (out.nrow, out.ncol) == (num_slots, cols)
        assert out.to_rns().shape == want.shape  # the entry tagged it EVAL: an EVAL read-out of a COEFF tag is refused
        assert np.array_equal(out.to_coeff_rns(), want), ("eval" if eval_format else "coeff")
        for t, b in zip(terms, before):
            assert t.is_ntt == eval_format and np.array_equal(t.to_rns(), b)


@pytest.mark.parametrize("n,bits,L", CELLS)
def test_recomposition_matches_big_integers(gpu, monkeypatch, n, bits, L):
    p = _params(gpu, n, bits, L)
    assert math.prod(p.moduli()) == p.modulus()

    def boom(*a, **k):
        raise AssertionError("the per-level loop was taken")

    monkeypatch.setattr(gpu.GpuDCRTPolyMatrix, "_crt_recompose_rows_loop", boom)
    _check_cell(gpu, p, 2, 2, SEED + n + L)
    if 2 * n < 16:  # two columns do not hold every special value of a level: once more with room for all of them
        _check_cell(gpu, p, 2, 16 // n, SEED + n + L + 1)


@pytest.mark.parametrize("n,bits,L", [(2, 10, 2), (64, 20, 8), (64, 51, 9)])
def test_equals_the_per_level_loop_bit_for_bit(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    moduli, Q = p.moduli(), p.modulus()
    es = p.reconst_coeffs()  # the loop's constants: 1 mod their own limb, 0 mod the others (src/poly/mod.rs:45-76)
    assert [[e % q for q in moduli] for e in es] == [[1 if j == i else 0 for j in range(L)] for i in range(L)]
    assert [p.to_crt_coeffs(i) for i in range(L)] == [(Q // q, e) for q, e in zip(moduli, es)]
    levels = _random_levels(p, 2, 2, SEED + 3 * n)
    terms = [_matrix(gpu, p, v, 2, True) for v in levels]
    fused, loop = M.crt_recompose_rows(p, terms, 2), M._crt_recompose_rows_loop(p, terms, 2)
    assert fused.is_ntt and loop.is_ntt and fused.size() == loop.size() == (2, 2)
    assert np.array_equal(fused.to_rns(), loop.to_rns())


@pytest.mark.parametrize("n,bits,L", [(64, 28, 3), (32, 57, 4)])
def test_signed_terms(gpu, n, bits, L):
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + n)
    num_slots, cols = 2, 2
    count = num_slots * L

    def rand_terms(T, eval_format):
        vals = [[[rnd.randrange(Q) for _ in range(cols * n)] for _ in range(T)] for _ in range(count)]
        return vals, [[_matrix(gpu, p, v, cols, eval_format) for v in level] for level in vals]

    # T = 4, (+, +, -, -): the levels formed with the existing + / -
    for eval_format in (True, False):
        _, mats = rand_terms(4, eval_format)
        fused = M.crt_recompose_rows_terms(p, mats, [1, 1, -1, -1], num_slots)
        formed = [a + b - c - d for a, b, c, d in mats]
        assert np.array_equal(fused.to_rns(), M.crt_recompose_rows(p, formed, num_slots).to_rns())
    # T = 8, mixed signs, against the big-integer sum; term 5 of every level is the very matrix that is term 1
    signs = [-1, 1, 1, -1, 1, -1, -1, 1]
    vals, mats = rand_terms(8, True)
    for v, m in zip(vals, mats):
        v[5], m[5] = v[1], m[1]
    fused = M.crt_recompose_rows_terms(p, mats, signs, num_slots)
    levels = [[sum(s * v[t][k] for t, s in enumerate(signs)) % Q for k in range(cols * n)] for v in vals]
    assert np.array_equal(fused.to_coeff_rns(), _expected(levels, moduli, num_slots, cols, n))
    # mixed domains: brought to EVAL on copies, the caller's matrices stay as they were
    mixed = [[m.ensure_coeff() if t % 2 else m for t, m in enumerate(level)] for level in mats]
    before = [[m.to_rns() for m in level] for level in mixed]
    again = M.crt_recompose_rows_terms(p, mixed, signs, num_slots)
    assert np.array_equal(again.to_rns(), fused.to_rns())
    for level, bs in zip(mixed, before):
        for t, (m, b) in enumerate(zip(level, bs)):
            assert m.is_ntt == (t % 2 == 0) and np.array_equal(m.to_rns(), b)


@pytest.mark.parametrize("n,bits,L", [(2, 10, 2), (256, 24, 3)])
def test_scaled_message_plus_small_error_recomposes_to_the_message(gpu, n, bits, L):
    """level (slot, i) = (Q / q_i) x + e mod Q with |e| < Q / (2 q_i) - 1 recomposes to x exactly: what the noise refresh
    relies on (the reference's own unit test runs n = 2 with two 10-bit limbs and two slots)"""
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + L)
    num_slots, cols = 2, 2
    xs = [[rnd.randrange(min(moduli)) for _ in range(cols * n)] for _ in range(num_slots)]
    xs[0][0], xs[0][1] = 0, min(moduli) - 1
    levels = []
    for s in range(num_slots):
        for q in moduli:
            Qi = Q // q
            emax = (Qi - 3) // 2  # the largest integer below Qi / 2 - 1 (Qi is odd)
            assert emax >= 1 and emax < Q / (2 * q) - 1
            es = [emax, -emax, 0, 1][: cols * n] + [rnd.randint(-emax, emax) for _ in range(max(0, cols * n - 4))]
            levels.append([(Qi * x + e) % Q for x, e in zip(xs[s], es)])
    for eval_format in (True, False):
        out = M.crt_recompose_rows(p, [_matrix(gpu, p, v, cols, eval_format) for v in levels], num_slots)
        got = out.to_coeff_rns()
        for s in range(num_slots):
            want = np.asarray(xs[s], dtype=np.uint64).reshape(cols, n)
            for i in range(L):
                assert np.array_equal(got[s, :, i, :], want), (s, i)
        assert out.coeffs() == [[xs[s][c * n:(c + 1) * n] for c in range(cols)] for s in range(num_slots)]


def test_chunks_of_whole_slots_give_the_same_bits(gpu, hip_env):
    n, bits, L, cols, num_slots = 64, 24, 3, 2, 7
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    levels = _random_levels(p, num_slots, cols, SEED + 5)
    terms = [_matrix(gpu, p, v, cols, True) for v in levels]
    want = _expected(levels, p.moduli(), num_slots, cols, n)
    whole = M.crt_recompose_rows(p, terms, num_slots)
    assert np.array_equal(whole.to_coeff_rns(), want)
    slot_bytes = L * cols * L * n * p.ctx().word_bytes()  # L levels of cols * L * n words
    for cap in (2 * slot_bytes, 3 * slot_bytes - 1, 1):  # 4 chunks of two slots (a last one of one), the same, 7 of one
        hip_env.set("MXX_HIP_CRT_RECOMPOSE_CHUNK_BYTES", str(cap))
        assert np.array_equal(M.crt_recompose_rows(p, terms, num_slots).to_rns(), whole.to_rns()), cap
    hip_env.restore()
    assert np.array_equal(M.crt_recompose_rows(p, terms, num_slots).to_rns(), whole.to_rns())


def test_launches_do_not_grow_with_the_slots(gpu):
    from mxx_amd import _ffi

    n, bits, L, cols, T = 256, 24, 3, 2, 4
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    Q = p.modulus()
    rnd = random.Random(SEED + 6)
    signs = [1, 1, -1, -1]
    lib = _ffi.lib()

    def terms_for(num_slots):
        return [[_matrix(gpu, p, [rnd.randrange(Q) for _ in range(cols * n)], cols, True) for _ in range(T)]
                for _ in range(num_slots * L)]

    rises = {}
    for num_slots in (1, 4):  # 12 and 48 term pointers: one pointer group either way
        mats = terms_for(num_slots)
        c0 = lib.gpupoly_launch_count()
        fused = M.crt_recompose_rows_terms(p, mats, signs, num_slots)
        rises[num_slots] = lib.gpupoly_launch_count() - c0
    assert rises[1] == rises[4] and 1 <= rises[4] <= 8, rises
    c0 = lib.gpupoly_launch_count()
    loop = M._crt_recompose_rows_loop(p, [a + b - c - d for a, b, c, d in mats], 4)
    loop_rise = lib.gpupoly_launch_count() - c0
    assert loop_rise >= 10 * rises[4], (loop_rise, rises)
    assert np.array_equal(fused.to_rns(), loop.to_rns())


def test_refusals_launch_nothing_and_leave_the_output_alone(gpu):
    from mxx_amd import _ffi

    n, bits, L, cols, num_slots = 64, 24, 3, 2, 2
    p = _params(gpu, n, bits, L)
    other = _params(gpu, n, 24, L + 1)
    M = gpu.GpuDCRTPolyMatrix
    moduli = p.moduli()
    Q = math.prod(moduli)
    rnd = random.Random(SEED + 7)
    count = num_slots * L
    lib = _ffi.lib()

    def rand_res(rows, c, limbs=L):
        return np.stack([np.asarray([[[rnd.randrange(q) for _ in range(n)] for _ in range(c)] for _ in range(rows)], dtype=np.uint64)
                         for q in moduli[:limbs]], axis=2)

    terms = [M.from_rns(p, rand_res(1, cols), False) for _ in range(count)]
    evals = [t.ensure_eval() for t in terms]
    sentinel = rand_res(num_slots, cols)
    wide = M.from_rns(p, rand_res(1, cols + 1), False)
    tall = M.from_rns(p, rand_res(2, cols), False)
    low = M.from_rns(p, rand_res(1, cols, L - 1), False)
    foreign = M.from_rns(other, np.ones((1, cols, L + 1, n), dtype=np.uint64), False)
    low_out = M.from_rns(p, sentinel[:, :, : L - 1], False)
    short_out = M.from_rns(p, sentinel[:1], False)

    def call(out, ts, signs=(1,), T=1, slots=num_slots, null_terms=False, null_signs=False):
        tarr = None if null_terms else (C.c_void_p * max(len(ts), 1))(*[None if t is None else t.raw.value for t in ts])
        sarr = None if null_signs else (C.c_int * max(len(signs), 1))(*signs)
        return lib.gpupoly_matrix_crt_recompose_rounded(None if out is None else out.raw, tarr, sarr, T, slots)

    def with_term(j, m):
        return terms[:j] + [m] + terms[j + 1:]

    cases = {
        "null out": (lambda out: call(None, terms), ""),
        "null terms": (lambda out: call(out, terms, null_terms=True), ""),
        "null signs": (lambda out: call(out, terms, null_signs=True), ""),
        "null term": (lambda out: call(out, with_term(count - 1, None)), ""),
        "no slots": (lambda out: call(out, terms, slots=0), ""),
        "T = 0": (lambda out: call(out, terms, signs=(1,), T=0), ""),
        "T = 9": (lambda out: call(out, terms * 9, signs=(1,) * 9, T=9), ""),
        "sign 0": (lambda out: call(out, terms, signs=(0,)), ""),
        "sign 2": (lambda out: call(out, terms * 2, signs=(1, 2), T=2), ""),
        "context": (lambda out: call(out, with_term(1, foreign)), ""),
        "term columns": (lambda out: call(out, with_term(2, wide)), ""),
        "term rows": (lambda out: call(out, with_term(3, tall)), ""),
        "out rows": (lambda out: call(short_out, terms), ""),
        "mixed formats": (lambda out: call(out, with_term(count - 1, evals[count - 1])), ""),
        "out below full level": (lambda out: call(low_out, terms), ""),
        "term below full level": (lambda out: call(out, with_term(count - 2, low)), "unsupported"),
        "out as a term": (lambda out: call(out, with_term(0, out.row_view(0, 1))), "overlap"),
    }
    for name, (fn, word) in cases.items():
        out = M.from_rns(p, sentinel, False)  # COEFF-tagged: a tag flipped to EVAL would make the COEFF read-out fail
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert ENTRY in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name
    for o, res in ((low_out, sentinel[:, :, : L - 1]), (short_out, sentinel[:1])):
        assert not o.is_ntt and np.array_equal(o.to_rns(), res)
    # `out` a view of its parent's first rows: a view of the parent's rows inside it is refused, one of the row after it is
    # an ordinary operand (rule 6)
    parent_res = rand_res(num_slots + 1, cols)
    parent = M.from_rns(p, parent_res, False)
    out = parent.row_view(0, num_slots)
    c0 = lib.gpupoly_launch_count()
    assert call(out, with_term(4, parent.row_view(1, 2))) != 0
    msg = _ffi.last_error_string()
    assert ENTRY in msg and "overlap" in msg
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), parent_res)
    last = parent.row_view(num_slots, num_slots + 1)
    assert call(out, with_term(4, last)) == 0
    levels = [parent_res[num_slots:] if j == 4 else t.to_rns() for j, t in enumerate(terms)]
    ints = [[[sum(int(lv[0, c, l, k]) * w for l, w in enumerate(p.reconst_coeffs())) % Q for k in range(n)] for c in range(cols)]
            for lv in levels]
    want = _expected([[x for poly in lv for x in poly] for lv in ints], moduli, num_slots, cols, n)
    out.is_ntt = True
    assert np.array_equal(out.to_coeff_rns(), want)
    assert np.array_equal(last.to_rns(), parent_res[num_slots:])  # the term row was not written
    # no columns: nothing launched, the tag set
    empty_terms = [M(p, 1, 0, L - 1, False) for _ in range(count)]
    empty = M(p, num_slots, 0, L - 1, False)
    c0 = lib.gpupoly_launch_count()
    assert call(empty, empty_terms) == 0 and lib.gpupoly_launch_count() == c0
    fmt_probe = M.crt_recompose_rows(p, empty_terms, num_slots)
    assert fmt_probe.is_ntt and fmt_probe.size() == (num_slots, 0)
    # the mirror keeps the reference's assertions
    with pytest.raises(AssertionError):
        M.crt_recompose_rows(p, terms[:-1], num_slots)
    with pytest.raises(AssertionError):
        M.crt_recompose_rows(p, with_term(2, wide), num_slots)


def test_levels_below_full_level_take_the_per_level_loop(gpu, monkeypatch):
    n, bits, L, cols, num_slots = 64, 28, 3, 1, 1
    p = _params(gpu, n, bits, L)
    M = gpu.GpuDCRTPolyMatrix
    moduli = p.moduli()
    Q, Ql = math.prod(moduli), math.prod(moduli[: L - 1])
    rnd = random.Random(SEED + 8)
    vals = [[rnd.randrange(Ql) for _ in range(cols * n)] for _ in range(num_slots * L)]
    lows = [M.from_rns(p, _residues(v, moduli[: L - 1], cols, n), False) for v in vals]
    calls = []
    real = M._crt_recompose_rows_loop
    monkeypatch.setattr(M, "_crt_recompose_rows_loop", staticmethod(lambda *a: calls.append(1) or real(*a)))
    out = M.crt_recompose_rows(p, lows, num_slots)
    assert calls == [1] and out.is_ntt and out.level == L - 1
    assert np.array_equal(out.to_coeff_rns(), _expected(vals, moduli, num_slots, cols, n))
