"""GPU: the fused products against the plain big-integer reference (tests/plainref.py) in every modulus width class.

tests/test_gpu_modulus_classes.py holds the transforms, the pointwise operations, `mul`, `decompose` and the wire format to
plainref at both edge primes of every width class.  The kernels behind mul_sum / mul_add_in_place / mul_sub_in_place,
mul_decompose_many, mul_gadget / add_scaled_gadget / gadget_block / gadget_mul, large_scalar_mul_many and monomial_sum /
mul_monomial / const_rotate_poly carry modular arithmetic of their own; their suites run them at the largest primes of
18, 24, 31, 51 and 61 bits and expect what the library's older entry points or the CPU oracle give.  Here every family
runs in every class - the two largest and the two smallest primes of the class in ONE context, so that the limbs of a
launch differ in their lazy window - and in four mixed-width contexts, and the expected value is plainref's alone:
nothing below is taken from oracle/ or from another entry point of the library.

How a result is checked.  Evaluation-domain operands are uploaded as residues (from_rns(..., True)): no transform sits
between the test's numbers and the kernel under test.  The result comes back with to_rns() and is compared bit for bit
in every (row, column, limb); in every slot up to n = 64 and in 8 slots (0, 1, n - 1 and five seeded ones) at n = 256,
where plainref's Horner evaluation of the digit polynomials is what costs.  Where an operation is defined through
coefficients (digits, rotations) plainref gives the coefficient-side value and P.ntt_slots takes it to the sampled slots;
the transforms themselves are held to plainref in all of these classes by test_gpu_modulus_classes.py.  Operations in the
coefficient domain are compared in every coefficient.

Two things the grid does not reach, stated so that nobody reads them into it:
  * gadget_scalar.hip sums up to 4 products of a residue with a table word without reducing ("below 2^64 for residues
    below 2^31").  That bound rests on arithmetic - 4 (q - 1)^2 <= 2^64 - 2^35 for the largest 31-bit prime - not on a
    test: the table words are transforms of digit polynomials, and a table whose words are all q - 1 cannot be
    constructed through the entry point.
  * The launch trace names a kernel by the text of its launch (`matmul_sum_kernel<W, TR, TC, SV, false>`), not by the
    instantiation, so the case for the large 64-bit register tile identifies the tile by the grid the trace reports -
    each tile shape gives a different number of workgroups - and by gpupoly_context_last_kernel, which carries
    `u64,4,4,2`, where the library sets it (the grouped product).
"""
import math

import numpy as np
import pytest

import plainref as P
import ran
from test_gpu_modulus_classes import MAX_INNER, SEED, _lazy_terms, _moduli, _params, _patterns, _root

pytestmark = pytest.mark.gpu

CLASSES = [10, 12, 15, 24, 28, 29, 31, 32, 33, 41, 51, 52, 57, 58, 61, 62]
# (n, ((bits, low), ...)): the specs of test_ring_matmul_mixed_widths
MIXED = [(64, ((51, False), (12, True))), (256, ((41, False), (31, True))), (256, ((51, False), (33, True))),
         (64, ((24, False), (12, True)))]
# base_bits per class; the first one also serves mul_decompose_many.  24 .. 61: the values of DECOMPOSE_CELLS (dpt 2, 2, 2,
# 2, 3, 3, 4).  31 and 62 bits: a second base of 6 bits (dpt 6 and 11) sends gadget_scalar_kernel and gadget_const_kernel
# through their any-dpt forms at the widest limb of either word width.  A short last digit: 15 / 13 (2 bits) for 32-bit
# words, 57 / 20 (17 bits) and 61 / 20 (1 bit) for 64-bit words.
BASES = {10: [5], 12: [6], 15: [13], 24: [12], 28: [14], 29: [15], 31: [16, 6], 32: [16], 33: [11], 41: [20], 51: [17], 52: [26],
         57: [20], 58: [20], 61: [20], 62: [31, 6]}
# mixed widths: a base wide enough for a digit of the wide tower to exceed the narrow modulus (and, at 31 and 34 bits, for
# 2^base itself to exceed it: the `% q` of the weight tables)
MIXED_BASES = [[17], [31], [34], [12]]
CELLS = [("class", b) for b in CLASSES] + [("mixed", i) for i in range(len(MIXED))]


def _cell_id(cell):
    if cell[0] == "class":
        return f"{cell[1]}bit"
    return "mixed_" + "_".join(str(b) for b, _ in MIXED[cell[1]][1])


_CELLS = {}


def _cell(cell):
    """(n, moduli, bases, slots) of a grid cell, made once"""
    if cell not in _CELLS:
        if cell[0] == "class":
            bits = cell[1]
            n = 64 if bits <= 12 else 256
            moduli, bases = _moduli(n, bits), BASES[bits]
            assert all(q.bit_length() == bits for q in moduli) and len(moduli) >= 2
        else:
            n, spec = MIXED[cell[1]]
            moduli, bases = [P.primes(n, bits, 1, low=low)[0] for bits, low in spec], MIXED_BASES[cell[1]]
        if n <= 64:
            slots = list(range(n))
        else:
            rng = np.random.default_rng(SEED + n)
            slots = sorted({0, 1, n - 1} | set(rng.choice(np.arange(2, n - 1), 5, replace=False).tolist()))
            assert len(slots) == 8
        _CELLS[cell] = (n, moduli, bases, slots)
    return _CELLS[cell]


def _seed(cell, salt):
    return SEED + 1000 * salt + (cell[1] if cell[0] == "class" else 100 + cell[1])


# ---------------------------------------------------------------------------------------------- host side
def _rand(rng, rows, cols, moduli, n):
    return np.stack([rng.integers(0, int(q), (rows, cols, n), dtype=np.uint64) for q in moduli], axis=2)


def _full(rows, cols, values, n):
    """every residue of limb l = values[l]"""
    col = np.asarray([int(v) for v in values], dtype=np.uint64).reshape(1, 1, -1, 1)
    return np.broadcast_to(col, (rows, cols, len(values), n)).copy()


def _top(rows, cols, moduli, n):
    return _full(rows, cols, [int(q) - 1 for q in moduli], n)


def _qobj(moduli):
    return np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, -1, 1)


def _eval_slots(coeff, moduli, slots):
    """P.ntt_slots of every polynomial of a (..., L, n) coefficient array: (..., L, len(slots)).  A constant polynomial (zero
    included) is its own value at every point and is not evaluated."""
    coeff = np.asarray(coeff, dtype=np.uint64)
    L, n = coeff.shape[-2:]
    flat = coeff.reshape(-1, n)
    out = np.zeros((flat.shape[0], len(slots)), dtype=np.uint64)
    const = ~flat[:, 1:].any(axis=1)
    out[const] = flat[const, :1]
    rows = np.flatnonzero(~const)
    if rows.size:
        ms = [int(moduli[i % L]) for i in rows]
        out[rows] = P.ntt_slots(flat[rows], ms, slots, [_root(q, n) for q in ms])
    return out.reshape(coeff.shape[:-1] + (len(slots),))


def _windows(moduli):
    """the lazy window of every limb: ((1 << acc) - q) // (q - 1)^2, capped at 2^20 as the library caps it"""
    wide = max(moduli) >> 31 != 0
    return [min(_lazy_terms(q, wide), 1 << 20) for q in moduli]


# the classes whose windows a term list can pass, (smallest, largest) window over the four primes of the context
STATED_WINDOWS = {29: (64, 255), 31: (4, 15), 58: (4096, 16383), 62: (16, 63)}
# inner sizes per term, all operands q - 1: no single term passes the larger window, their sum passes both.  58 bits: 4100
# products pass the largest prime's window of 4096; the smallest prime's 16383 would take operands past MAX_INNER.
STATED_TERMS = {29: [100, 100, 100], 31: [3, 3, 12], 58: [2000, 2100], 62: [40, 30]}


def _past_window_terms(cell, moduli):
    w = _windows(moduli)
    small, big = min(w), max(w)
    if cell[0] == "class" and cell[1] in STATED_TERMS:
        assert (small, big) == STATED_WINDOWS[cell[1]], (small, big)
        ks = STATED_TERMS[cell[1]]
        assert max(ks) <= big and sum(ks) > (big if sum(ks) < MAX_INNER else small)
        return ks
    if big + 1 <= MAX_INNER:
        half = big // 2 + 1
        assert half <= big < 2 * half
        return [half, half]
    # the window exceeds MAX_INNER products (24 bits: 2^16; 10 .. 15 bits: the cap of 2^20; 32 .. 57 bits and every mixed
    # context: 2^14 and more): 8 terms of one product each, the closed form without a fold inside the loop
    return [1] * 8


def _up(gpu, p, a, ev=True):
    return gpu.GpuDCRTPolyMatrix.from_rns(p, np.ascontiguousarray(a), ev)


def _sl(a, slots):
    return None if a is None else np.asarray(a)[..., slots]


# ---------------------------------------------------------------------------------------------- mul_sum
@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_mul_sum(gpu, hip_env, cell):
    """out = addend +- sum_t lhss[t] rhss[t]: the 1-, 2-, 4- and 8-row tiles of 32-bit words (rows 1, 2, 3, 5; 64-bit words
    choose theirs by occupancy), 9 rows through scratch + combine and through the term-table kernel, every addend form and
    sign, a block placed in a wider `out`, the in-place forms, and q - 1 operands whose terms pass the window together."""
    n, moduli, bases, slots = _cell(cell)
    p = _params(gpu, n, moduli, bases[0])
    M = gpu.GpuDCRTPolyMatrix
    rng = np.random.default_rng(_seed(cell, 1))
    ks, cols, wide_cols, dst = [1, 4, 2], 3, 7, 2
    A = [_rand(rng, 9, k, moduli, n) for k in ks]
    B = [_rand(rng, k, cols, moduli, n) for k in ks]
    A[1][:, 1:3] = _top(9, 2, moduli, n)  # two (q - 1)^2 products in a row in every output
    B[1][1:3] = _top(2, cols, moduli, n)
    AD, SENT = _rand(rng, 9, wide_cols, moduli, n), _rand(rng, 9, wide_cols, moduli, n)
    AD[:, dst] = _top(9, 1, moduli, n)[:, 0]
    dB = [_up(gpu, p, b) for b in B]

    def run(rows, addend, negate, placed):
        lh = [_up(gpu, p, a[:rows]) for a in A]
        d0, width = (dst, wide_cols) if placed else (0, cols)
        out_host = SENT[:rows, :width]
        add_host = None if addend == "none" else (out_host if addend == "out" else AD[:rows, :width])
        out = _up(gpu, p, out_host)
        add = None if addend == "none" else (out if addend == "out" else _up(gpu, p, add_host))
        got = M.mul_sum(lh, dB, addend=add, negate=negate, out=out, dst_col=d0)
        assert got is out and out.is_ntt
        want = out_host[..., slots].copy()
        want[:, d0:d0 + cols] = P.slot_mul_sum(None if add_host is None else _sl(add_host[:, d0:d0 + cols], slots),
                                               [_sl(a[:rows], slots) for a in A], [_sl(b, slots) for b in B], moduli, negate)
        assert np.array_equal(out.to_rns()[..., slots], want), (rows, addend, negate, placed, p.ctx().last_kernel())

    for rows in (1, 2, 3, 5):
        for addend in ("none", "separate", "out"):
            for negate in (False, True):
                run(rows, addend, negate, False)
    run(2, "separate", False, True)
    run(5, "out", True, True)
    run(9, "separate", True, True)  # above 8 rows: products into scratch, one combine pass per term
    run(9, "none", False, False)
    hip_env.set("MXX_HIP_MUL_SUM_PATH", "tile")  # two row tiles of the term-table kernel
    with ran.launches() as launched:
        run(9, "out", False, True)
    with ran.launches() as launched_again:
        run(9, "separate", True, False)
    if FORCED["test_mul_sum"]["pairs"][("MXX_HIP_MUL_SUM_PATH", "tile")](dict(cell=cell)):
        launched.assert_ran("MXX_HIP_MUL_SUM_PATH", "tile", moduli)
        launched_again.assert_ran("MXX_HIP_MUL_SUM_PATH", "tile", moduli)
    hip_env.unset("MXX_HIP_MUL_SUM_PATH")

    # the in-place forms
    for negate in (False, True):
        x = _up(gpu, p, AD[:3, :cols])
        (x.mul_sub_in_place if negate else x.mul_add_in_place)(_up(gpu, p, A[1][:3]), dB[1])
        want = P.slot_mul_sum(_sl(AD[:3, :cols], slots), [_sl(A[1][:3], slots)], [_sl(B[1], slots)], moduli, negate)
        assert np.array_equal(x.to_rns()[..., slots], want), ("in place", negate)

    # every operand q - 1: (q - 1)^2 = 1 (mod q), so the block is addend +- K for K products; every slot is compared
    kt = _past_window_terms(cell, moduli)
    K = sum(kt)
    lh = [_up(gpu, p, _top(2, k, moduli, n)) for k in kt]
    rh = [_up(gpu, p, _top(k, cols, moduli, n)) for k in kt]
    a = [q - 5 for q in moduli]
    addend = _up(gpu, p, _full(2, cols, a, n))
    for negate in (False, True):
        got = M.mul_sum(lh, rh, addend=addend, negate=negate).to_rns()
        want = _full(2, cols, [(x - K) % q if negate else (x + K) % q for x, q in zip(a, moduli)], n)
        assert np.array_equal(got, want), ("q - 1 operands", kt, negate)


# ---------------------------------------------------------------------------------------------- mul_decompose_many
@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_mul_decompose_many(gpu, cell):
    """outs[j] = lhss[j] G^-1(B) + addends[j] o scalars[j]: a 1-row and a 2-row operand against one B (2 x 3) whose
    coefficient residues are the worst-case patterns (all q - 1, alternating at every period, a spike, random).  Expected:
    the operand times the transformed P.digits of B, slot by slot."""
    n, moduli, bases, slots = _cell(cell)
    L, base = len(moduli), bases[0]
    p = _params(gpu, n, moduli, base)
    M = gpu.GpuDCRTPolyMatrix
    dpt = P.digits_per_tower(moduli, base)
    k, r, cols = L * dpt, 2, 3
    assert p.modulus_digits() == k
    pats = _patterns(moduli, n, _seed(cell, 2))[0]
    Bc = np.stack([pats[i % pats.shape[0]] for i in range(r * cols)]).reshape(r, cols, L, n)
    dig = np.zeros((r * k, cols, L, n), dtype=np.uint64)
    for i in range(r):
        for c in range(cols):
            dig[i * k:(i + 1) * k, c] = P.digits(Bc[i, c], moduli, base, dpt)
    D = _eval_slots(dig, moduli, slots)
    rng = np.random.default_rng(_seed(cell, 3))
    S = [_rand(rng, rows, r * k, moduli, n) for rows in (1, 2)]
    S[1][1, : 2 * dpt] = _top(1, 2 * dpt, moduli, n)[0]
    AD = [_rand(rng, rows, cols, moduli, n) for rows in (1, 2)]
    AD[1][0, 0] = _top(1, 1, moduli, n)[0, 0]
    SC = _rand(rng, 1, 1, moduli, n)
    SC[0, 0, :, slots[0]] = [q - 1 for q in moduli]  # (q - 1)(q - 1) in the epilogue's product
    q = _qobj(moduli)
    scaled = (_sl(AD[1], slots).astype(object) * _sl(SC, slots).astype(object)) % q
    dS = [_up(gpu, p, s) for s in S]
    dB = _up(gpu, p, Bc, False)
    # addend o scalar on the 2-row operand only; then a bare addend on the 1-row operand only
    for addends, scalars, wants in (
        ([None, _up(gpu, p, AD[1])], [None, _up(gpu, p, SC)], [None, scaled]),
        ([_up(gpu, p, AD[0]), None], [None, None], [_sl(AD[0], slots), None]),
    ):
        outs = M.mul_decompose_many(dS, dB, addends=addends, scalars=scalars)
        for j, out in enumerate(outs):
            want = P.slot_mul_sum(wants[j], [_sl(S[j], slots)], [D], moduli, False)
            assert out.is_ntt and np.array_equal(out.to_rns()[..., slots], want), (j, p.ctx().last_kernel())


# ---------------------------------------------------------------------------------------------- mul_gadget / gadget_mul
def _gadget_slots(moduli, base, n, d, small, count):
    """G = I_d (x) g at `count` slots: its entries are constants, so every slot holds the constant"""
    G = P.gadget_small(d, moduli, base, n) if small else P.gadget(d, moduli, base, n)
    assert not G[..., 1:].any()
    return np.broadcast_to(G[..., :1], G.shape[:3] + (count,)).copy()


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_gadget_products(gpu, cell):
    """addend +- (lhs G[:, window]) o scalar and addend +- G rhs without G: the window whole, starting inside a tower and as
    the last column alone; lhs absent (the identity: gadget_block, add_scaled_gadget); `small` on and off; every addend form
    and sign; a block placed in a wider `out`; gadget_mul of full-size residues, all q - 1 included, in both domains."""
    n, moduli, bases, slots = _cell(cell)
    L, S = len(moduli), len(slots)
    M = gpu.GpuDCRTPolyMatrix
    q = _qobj(moduli)
    for base in bases:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        rng = np.random.default_rng(_seed(cell, 4) + base)
        d, rows = 2, 3
        lhs = _rand(rng, rows, d, moduli, n)
        lhs[0, 1] = _top(1, 1, moduli, n)[0, 0]
        sc = _rand(rng, 1, 1, moduli, n)
        sc[0, 0, :, slots[-1]] = [m - 1 for m in moduli]
        d_lhs, d_sc = _up(gpu, p, lhs), _up(gpu, p, sc)
        eye = np.zeros((d, d, L, S), dtype=np.uint64)
        eye[np.arange(d), np.arange(d)] = 1
        for small in (False, True):
            kk = dpt if small else L * dpt
            G = _gadget_slots(moduli, base, n, d, small, S)
            assert G.shape[1] == d * kk
            inside = 1 if small else dpt + 1  # digit 1 of a tower
            assert dpt >= 2

            def want(lhs_slots, lo, hi, scalar, addend_block, negate):
                W = G[:, lo:hi].astype(object)
                if scalar is not None:
                    W = (W * _sl(scalar, slots).astype(object)) % q
                return P.slot_mul_sum(addend_block, [lhs_slots], [W], moduli, negate)

            for lo, hi, scalar, addend, negate in (
                (0, d * kk, sc, "none", False), (0, d * kk, sc, "separate", True), (inside, d * kk - 1, None, "out", False),
                (d * kk - 1, d * kk, sc, "out", True), (inside, inside + 2, None, "none", True), (d * kk - 1, d * kk, None, "separate", False),
            ):
                cols = hi - lo
                pad = 2 if addend == "out" else 0  # in place: the block sits at column 2 of a wider out
                out_host = _rand(rng, rows, cols + pad + (1 if pad else 0), moduli, n)
                add_host = None if addend == "none" else (out_host if addend == "out" else _rand(rng, rows, cols, moduli, n))
                out = _up(gpu, p, out_host)
                add = None if addend == "none" else (out if addend == "out" else _up(gpu, p, add_host))
                got = d_lhs.mul_gadget(scalar=None if scalar is None else d_sc, col_start=lo, col_end=hi, addend=add, negate=negate,
                                       out=out if addend == "out" else None, dst_col=pad, small=small)
                exp = out_host[..., slots].copy() if addend == "out" else None
                block = want(_sl(lhs, slots), lo, hi, scalar, None if add_host is None else _sl(add_host, slots)[:, pad:pad + cols], negate)
                if exp is None:
                    exp = block
                else:
                    exp[:, pad:pad + cols] = block
                assert got.is_ntt and np.array_equal(got.to_rns()[..., slots], exp), (base, small, lo, hi, addend, negate)

            # lhs absent: +-G[:, window] o scalar
            for lo, hi, scalar, negate in ((0, d * kk, sc, True), (inside, d * kk, None, False), (d * kk - 1, d * kk, sc, False)):
                got = M.gadget_block(p, d, lo, hi, scalar=None if scalar is None else d_sc, negate=negate, small=small)
                assert np.array_equal(got.to_rns()[..., slots], want(eye, lo, hi, scalar, None, negate)), (base, small, lo, hi, "block")
            for gcol, cols, scalar, negate in ((0, d * kk, sc, False), (inside, kk, None, True), (d * kk - 1, 1, sc, True)):
                host = _rand(rng, d, cols, moduli, n)
                x = _up(gpu, p, host)
                x.add_scaled_gadget(scalar=None if scalar is None else d_sc, negate=negate, gadget_col=gcol, small=small)
                exp = want(eye, gcol, gcol + cols, scalar, _sl(host, slots), negate)
                assert np.array_equal(x.to_rns()[..., slots], exp), (base, small, gcol, cols, "add_scaled_gadget")

            # G rhs: rhs holds residues of full size (a recomposition of anything, not only of digits)
            rhs = _rand(rng, d * kk, 2, moduli, n)
            rhs[:, 1] = _top(d * kk, 1, moduli, n)[:, 0]
            ad = _rand(rng, d, 2, moduli, n)
            for ev, addend, negate in ((True, False, False), (True, True, True), (False, True, False), (False, False, True)):
                got = M.gadget_mul(_up(gpu, p, rhs, ev), addend=_up(gpu, p, ad, ev) if addend else None, negate=negate, small=small)
                assert got.is_ntt == ev
                # G's entries are constants: the same sum coefficient by coefficient as slot by slot
                exp = P.slot_mul_sum(_sl(ad, slots) if addend else None, [G], [_sl(rhs, slots)], moduli, negate)
                assert np.array_equal(got.to_rns()[..., slots], exp), (base, small, ev, addend, negate, "gadget_mul")


# ---------------------------------------------------------------------------------------------- large_scalar_mul_many
def _raw_large_scalar(gpu, outs, lhss, addends, scalar, negate, base):
    """the two entries themselves: the mirror always makes fresh outputs, and an addend that IS the output needs the handles"""
    import ctypes as C

    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    n = len(lhss)
    arr = lambda ms: (C.c_void_p * n)(*[None if m is None else m.raw.value for m in ms])  # noqa: E731
    if isinstance(scalar, int):
        words = M._int_words(scalar)
        st = _ffi.lib().gpupoly_matrix_mul_decompose_gadget_const_many(arr(outs), arr(lhss), arr(addends), n, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                       len(words), 1 if negate else 0, base)
        _ffi.check_status(st, "gpupoly_matrix_mul_decompose_gadget_const_many")
    else:
        st = _ffi.lib().gpupoly_matrix_mul_decompose_gadget_scalar_many(arr(outs), arr(lhss), arr(addends), n, scalar.raw, 1 if negate else 0, base)
        _ffi.check_status(st, "gpupoly_matrix_mul_decompose_gadget_scalar_many")
    for o in outs:
        o._touch()
        o.is_ntt = True


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_large_scalar_mul_many(gpu, cell):
    """outs[j] = addends[j] +- lhss[j] G^-1(G_dj o c), d = 1 and 2 in one call.  c: a ring element of random coefficients, the
    element all of whose residues are q - 1, and the integer constants 1, 2^base - 1, Q - 1 and a random one below Q.
    Expected: P.gadget_scalar_digits of c, taken to the slots by P.ntt_slots, under P.slot_mul_sum per diagonal block."""
    n, moduli, bases, slots = _cell(cell)
    L = len(moduli)
    M = gpu.GpuDCRTPolyMatrix
    Q = math.prod(moduli)
    for base in bases:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        k = L * dpt
        rng = np.random.default_rng(_seed(cell, 5) + base)
        ds = (1, 2)
        lhs = [_rand(rng, d, d * k, moduli, n) for d in ds]
        lhs[1][0, :dpt] = _top(1, dpt, moduli, n)[0]
        ad = [_rand(rng, d, d * k, moduli, n) for d in ds]
        d_lhs = [_up(gpu, p, x) for x in lhs]

        ring = [_rand(rng, 1, 1, moduli, n)[0, 0], _top(1, 1, moduli, n)[0, 0]]
        consts = [1, (1 << base) - 1, Q - 1, int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % Q]
        if cell[0] == "mixed":
            # a value of the wide tower whose digit exceeds the narrow modulus: its low `base` bits all ones
            wide_q, narrow_q = moduli[0], moduli[1]
            c = _rand(rng, 1, 1, moduli, n)[0, 0]
            hi = rng.integers(0, (wide_q >> base) - 1, n, dtype=np.uint64)
            c[0] = (hi << np.uint64(base)) | np.uint64((1 << base) - 1)
            assert int(c[0].max()) < wide_q and int((c[0] & np.uint64((1 << base) - 1)).min()) >= narrow_q
            ring.append(c)
            assert (consts[1] % wide_q) & ((1 << base) - 1) >= narrow_q  # the constant path's host `%` runs too

        def check(scalar_host, scalar_dev, variants):
            D = _eval_slots(P.gadget_scalar_digits(scalar_host, moduli, base, dpt), moduli, slots)
            for addend, negate in variants:
                outs = [_up(gpu, p, x) for x in ad] if addend else [M(p, d, d * k, L - 1, True) for d in ds]
                _raw_large_scalar(gpu, outs, d_lhs, outs if addend else [None, None], scalar_dev, negate, base)
                for j, d in enumerate(ds):
                    got = outs[j].to_rns()[..., slots]
                    for b in range(d):
                        cs = slice(b * k, (b + 1) * k)
                        want = P.slot_mul_sum(_sl(ad[j][:, cs], slots) if addend else None, [_sl(lhs[j][:, cs], slots)], [D], moduli, negate)
                        assert np.array_equal(got[:, cs], want), (base, j, b, addend, negate, type(scalar_dev).__name__)
            return D

        every = [(False, False), (False, True), (True, False), (True, True)]
        D0 = None
        for i, c in enumerate(ring):
            D = check(c, _up(gpu, p, c[None, None], False), every if i == 0 else [(False, False), (True, True)])
            D0 = D if i == 0 else D0
        for i, value in enumerate(consts):
            c = np.zeros((L, n), dtype=np.uint64)
            c[:, 0] = [value % q for q in moduli]
            check(c, value, every if i == 3 else [(False, True), (True, False)])
        # the mirror, once: fresh outputs, separate addends
        outs = M.large_scalar_mul_many(d_lhs, _up(gpu, p, ring[0][None, None], False), addends=[None, _up(gpu, p, ad[1])], negate=True)
        for j, d in enumerate(ds):
            for b in range(d):
                cs = slice(b * k, (b + 1) * k)
                want = P.slot_mul_sum(_sl(ad[j][:, cs], slots) if j else None, [_sl(lhs[j][:, cs], slots)], [D0], moduli, True)
                assert np.array_equal(outs[j].to_rns()[..., slots][:, cs], want), (base, j, b, "mirror")


# ---------------------------------------------------------------------------------------------- monomials
@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_monomial_products(gpu, cell):
    """addend +- sum_j mats[j] x^shifts[j], mul_monomial and x^s itself (fill_monomial, const_rotate_poly) in both domains, for
    1 and 5 polynomials.  COEFF: P.monomial_mul in every coefficient.  EVAL: the product by x^s is, slot by slot, the
    product by the transform of x^s = P.monomial_mul(1, s), taken to the sampled slots by P.ntt_slots."""
    n, moduli, bases, slots = _cell(cell)
    L = len(moduli)
    p = _params(gpu, n, moduli, bases[0])
    M = gpu.GpuDCRTPolyMatrix
    rng = np.random.default_rng(_seed(cell, 6))
    qcol = np.asarray(moduli, dtype=np.uint64).reshape(-1, 1)
    one = np.zeros((L, n), dtype=np.uint64)
    one[:, 0] = 1
    edge = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    aligned = [4, n - 4, n + 8, 2 * n - 4]  # multiples of 4 only: the 16-byte COEFF form
    mono = {s: P.monomial_mul(one, s, qcol) for s in edge + aligned}
    F = {s: _eval_slots(m, moduli, slots)[None, None] for s, m in mono.items()}  # (1, 1, L, S)

    def coeff_sum(mats, shifts, addend, negate):
        acc = np.zeros_like(mats[0]) if addend is None else addend.copy()
        for a, s in zip(mats, shifts):
            r = P.monomial_mul(a, s, qcol)
            acc = (acc + (qcol - r) % qcol) % qcol if negate else (acc + r) % qcol  # both below q < 2^62
        return acc

    for polys in (1, 5):
        X = [_rand(rng, 1, polys, moduli, n) for _ in range(3)]
        X[1][0, 0] = _top(1, 1, moduli, n)[0, 0]
        A = _rand(rng, 1, polys, moduli, n)
        for ev in (False, True):
            dX = [_up(gpu, p, x, ev) for x in X]
            for shifts, addend, negate in ((edge, "none", False), (edge, "separate", True), (aligned, "out", False), (aligned, "none", True),
                                           (edge + aligned, "out", True)):
                mats = [X[j % 3] for j in range(len(shifts))]
                dm = [dX[j % 3] for j in range(len(shifts))]
                add = None if addend == "none" else _up(gpu, p, A, ev)
                got = M.monomial_sum(dm, shifts, addend=add, negate=negate, out=add if addend == "out" else None)
                assert got.is_ntt == ev
                a_host = None if addend == "none" else A
                if ev:
                    want = P.slot_mul_sum(_sl(a_host, slots), [F[s] for s in shifts], [_sl(m, slots) for m in mats], moduli, negate)
                    assert np.array_equal(got.to_rns()[..., slots], want), (polys, shifts, addend, negate, "eval")
                else:
                    assert np.array_equal(got.to_rns(), coeff_sum(mats, shifts, a_host, negate)), (polys, shifts, addend, negate, "coeff")
            for s in edge + aligned[:1]:
                got = dX[1].mul_monomial(s)
                assert got.is_ntt == ev
                if ev:
                    assert np.array_equal(got.to_rns()[..., slots], P.slot_mul_sum(None, [F[s]], [_sl(X[1], slots)], moduli, False)), (polys, s)
                else:
                    assert np.array_equal(got.to_rns(), P.monomial_mul(X[1], s, qcol)), (polys, s)
    for s in edge:
        assert np.array_equal(M.monomial(p, 1, 1, s, False).to_rns()[0, 0], mono[s]), s
        assert np.array_equal(M.monomial(p, 1, 2, s, True).to_rns()[0, 1][:, slots], F[s][0, 0]), s
        rot = gpu.GpuDCRTPoly.const_rotate_poly(p, s).inner
        assert rot.is_ntt and np.array_equal(rot.to_rns()[0, 0][:, slots], F[s][0, 0]), s

    # every residue q - 1 and every shift n: x^n = -1, every product is (q - 1)^2 = 1 (mod q), in either domain.  A call is
    # cut into launches of 64 terms, so only windows below 64 are passed inside a launch (31 and 62 bits: 16 and 64 terms
    # pass both limbs' windows of 15 and 63); 29 and 58 bits run past their windows of 255 and 4096 across launches, the
    # other classes 8 terms.
    w = _windows(moduli)
    count = min(max(w) + 1, MAX_INNER) if cell[0] == "class" and cell[1] in STATED_WINDOWS else 8
    if cell == ("class", 58):
        assert count == MAX_INNER > min(w)
    top = _top(1, 5, moduli, n)
    assert np.array_equal(P.monomial_mul(top, n, qcol), np.ones_like(top))
    for ev in (False, True):
        m, add = _up(gpu, p, top, ev), _up(gpu, p, top, ev)
        got = M.monomial_sum([m] * count, [n] * count, addend=add)
        assert np.array_equal(got.to_rns(), _full(1, 5, [(q - 1 + count) % q for q in moduli], n)), (ev, count)
        got = M.monomial_sum([m] * count, [n] * count, addend=add, negate=True, out=add)
        assert np.array_equal(got.to_rns(), _full(1, 5, [(q - 1 - count) % q for q in moduli], n)), (ev, count, "negated in place")


# ---------------------------------------------------------------------------------------------- the large 64-bit tiles
# The 64-bit register tiles are chosen by occupancy (matmul_tile.h: stacked_tile), so the shapes above never reach the
# 4 x 4 x 2 tile.  n = 2^14, one 62-bit limb, closed forms: no host reference cost.
BIG_N, BIG_ROWS, BIG_COLS = 1 << 14, 8, 32


def _big_grid_442(L=1):
    """workgroups of the 4 x 4 x 2 tile: 2 slots per lane, 256 lanes; 2 x 2 x 1 gives 8 times and 1 x 1 x 1 32 times as many"""
    return (BIG_N // 2 // 256) * ((BIG_ROWS + 3) // 4) * ((BIG_COLS + 3) // 4) * L


def _traced(gpu, fn):
    from mxx_amd import _ffi

    gpu.gpu_device_sync()
    _ffi.trace_begin()
    out = fn()
    gpu.gpu_device_sync()
    return out, _ffi.trace_end()


def test_mul_sum_large_u64_tile(gpu):
    """8 rows x 32 columns, terms of 9 and 8 products of q - 1 operands: two row tiles and eight column tiles of the
    4 x 4 x 2 tile, 17 products against the window of 16."""
    q = P.primes(BIG_N, 62, 1)[0]
    assert _windows([q]) == [16]
    p = gpu.GpuDCRTPolyParams(BIG_N, [q], 31)
    M = gpu.GpuDCRTPolyMatrix
    ks = [9, 8]
    lh = [_up(gpu, p, _top(BIG_ROWS, k, [q], BIG_N)) for k in ks]
    rh = [_up(gpu, p, _top(k, BIG_COLS, [q], BIG_N)) for k in ks]
    addend = _up(gpu, p, _full(BIG_ROWS, BIG_COLS, [q - 5], BIG_N))
    out, recs = _traced(gpu, lambda: M.mul_sum(lh, rh, addend=addend, negate=True))
    ran = [r for r in recs if "matmul_sum_kernel" in r["kernel"]]
    assert len(ran) == 1 and (ran[0]["blocks"], ran[0]["threads"]) == (_big_grid_442(), 256), recs
    got = out.to_rns()
    assert got.shape == (BIG_ROWS, BIG_COLS, 1, BIG_N) and (got == np.uint64((q - 5 - sum(ks)) % q)).all()


def test_mul_decompose_many_large_u64_tile(gpu):
    """two operands of 4 rows (8 stacked rows) against G^-1(B), B 8 x 32 constants q - 1 at base 2^31: 16 digit rows whose
    transforms are the digits themselves, so every output is (q - 1) r (d0 + d1) + addend o scalar."""
    q = P.primes(BIG_N, 62, 1)[0]
    base, r = 31, 8
    p = gpu.GpuDCRTPolyParams(BIG_N, [q], base)
    M = gpu.GpuDCRTPolyMatrix
    dpt = P.digits_per_tower([q], base)
    assert dpt == 2 and p.modulus_digits() == 2
    const = np.zeros((r, BIG_COLS, 1, BIG_N), dtype=np.uint64)
    const[..., 0] = q - 1
    d = P.digits(const[0, 0], [q], base, dpt)[:, 0, 0]  # the two digits of q - 1
    assert int(d[0]) + (int(d[1]) << base) == q - 1
    lh = [_up(gpu, p, _top(BIG_ROWS // 2, r * dpt, [q], BIG_N)) for _ in range(2)]
    addend = _up(gpu, p, _full(BIG_ROWS // 2, BIG_COLS, [q - 3], BIG_N))
    scalar = _up(gpu, p, _full(1, 1, [q - 1], BIG_N))
    outs, recs = _traced(gpu, lambda: M.mul_decompose_many(lh, _up(gpu, p, const, False), addends=[addend, None], scalars=[scalar, None]))
    assert "u64,4,4,2" in p.ctx().last_kernel(), p.ctx().last_kernel()
    ran = [x for x in recs if "matmul_group_kernel" in x["kernel"]]
    assert len(ran) == 1 and (ran[0]["blocks"], ran[0]["threads"]) == (_big_grid_442(), 256), recs
    prod = (q - 1) * r * (int(d[0]) + int(d[1])) % q
    for out, extra in zip(outs, ((q - 3) * (q - 1) % q, 0)):
        got = out.to_rns()
        assert got.shape == (BIG_ROWS // 2, BIG_COLS, 1, BIG_N) and (got == np.uint64((prod + extra) % q)).all()


# forced kernel paths (tests/ran.py): gpupoly_matrix_mul_sum keeps the term-table kernel at every height under the
# switch, with no condition of its own; evaluated over the parameter lists by tests/test_ran_table_host.py
FORCED = {
    "test_mul_sum": {"cls": lambda c: ran.Launched.word_class(_cell(c["cell"])[1]), "pairs": {
        ("MXX_HIP_MUL_SUM_PATH", "tile"): lambda c: True}},
}
