"""GPU: the nested-RNS gadget vector, its decomposition and the p-residues on the device
(`gpupoly_matrix_fill_nested_rns_gadget`, `gpupoly_matrix_nested_rns_decompose`, `gpupoly_matrix_nested_rns_residues`,
DESIGN.md section 5z) and `NestedRnsContext` on top of them.

The expected words come from `Plain` below, a big-integer restatement of nested_rns_gadget_vector /
nested_rns_gadget_decomposed (src/gadgets/arith/nested_rns/encoding.rs:196-338): it works mod Q on Python ints with
P/p_j, P and the reconstruction coefficient as whole integers and only takes residues of the finished value, so it
shares neither tables nor limb-wise arithmetic with the kernels.  Every output word is compared bit for bit.

Cells: the reference's own test context (n = 4, 6 x 18 bits, p bits 6, scale 2^8, the 2 x 2 matrix and the window of
tests.rs:1135-1217, and the full window); n = 64 and 256 at 24, 28, 31, 51 and 60-bit limbs with 1, 3 and 9 limbs, p
bits 5, 7 and 10, scales 1, 3, 2^7, 2^8, windows at both ends, in the middle, of one limb and whole; an explicit p list
with p_max just below 2^16, whose table slice does not fit LDS (the kernel's global-read form); a source below full
level.  Inputs: 0, Q - 1, 1, 2, the q0 + 3 style values of tests.rs:1151-1197, residues that reach a tie of the inner
and of the outer rounded division (found through `Plain`), random values (64-bit residues above 2^32 in the wide
cells).  COEFF and EVAL sources, both output formats."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261020
DECOMPOSE = "gpupoly_matrix_nested_rns_decompose"
GADGET = "gpupoly_matrix_fill_nested_rns_gadget"
RESIDUES = "gpupoly_matrix_nested_rns_residues"


def rdiv(a, b):
    return (a + b // 2) // b


def is_tie(a, b):
    """a / b lies exactly between two integers"""
    return b % 2 == 0 and a % b == b // 2


class Plain:
    """The section's definitions on whole integers, for the window [off, off + A) of the limbs q_all."""

    def __init__(self, q_all, ps, scale, off, A):
        self.q_all, self.ps, self.scale, self.off, self.A = list(q_all), list(ps), scale, off, A
        self.Q = math.prod(q_all)
        self.Pfull = math.prod(ps)
        self.qs = self.q_all[off:off + A]
        q_act = math.prod(self.qs)
        self.inv = [pow((self.Pfull // p) % p, -1, p) for p in ps]
        self.rc = [(q_act // q) * pow((q_act // q) % q, -1, q) for q in self.qs]
        self.inner_ties = self.outer_ties = 0
        self._slots = {}

    def terms(self, xs, count=False):
        ys = [(x % p) * inv % p for x, p, inv in zip(xs, self.ps, self.inv)]
        total = sum(rdiv(y * self.scale, p) for y, p in zip(ys, self.ps))
        if count:
            self.inner_ties += sum(is_tie(y * self.scale, p) for y, p in zip(ys, self.ps))
            self.outer_ties += is_tie(total, self.scale)
        return ys, rdiv(total, self.scale)

    def slot(self, a, s):
        """slot(a, s) as an integer mod Q"""
        ys, w = self.terms([s % p for p in self.ps])
        return ((sum(y * (self.Pfull // p) for y, p in zip(ys, self.ps)) - w * self.Pfull) * self.rc[a]) % self.Q

    def slot_residues(self, a, s):
        key = (a, s)
        if key not in self._slots:
            v = self.slot(a, s)
            self._slots[key] = [v % q for q in self.q_all]
        return self._slots[key]

    def gadget_values(self):
        """A (D+1) integers mod Q"""
        out = []
        for a, q in enumerate(self.qs):
            gs = [(self.Pfull // p) % q for p in self.ps] + [(q - self.Pfull % q) % q]
            out.extend(self.slot(a, g) for g in gs)
        return out

    def digits(self, r):
        ys, w = self.terms([r % p for p in self.ps], count=True)
        return ys + [w]

    def decomposed(self, coeffs, rows, cols, n):
        """coeffs[row][col][k] integers -> (rows A (D+1), cols, L, n) residues"""
        cw = len(self.ps) + 1
        out = np.zeros((rows * self.A * cw, cols, len(self.q_all), n), dtype=np.uint64)
        for row in range(rows):
            for col in range(cols):
                for k, c in enumerate(coeffs[row][col]):
                    for a, q in enumerate(self.qs):
                        for d, s in enumerate(self.digits(c % q)):
                            out[(row * self.A + a) * cw + d, col, :, k] = self.slot_residues(a, s)
        return out

    def residues(self, coeffs, rows, cols, n):
        D = len(self.ps)
        out = np.zeros((rows * self.A * D, cols, len(self.q_all), n), dtype=np.uint64)
        for row in range(rows):
            for col in range(cols):
                for k, c in enumerate(coeffs[row][col]):
                    for a, q in enumerate(self.qs):
                        for j, p in enumerate(self.ps):
                            out[(row * self.A + a) * D + j, col, :, k] = [(c % q % p) % ql for ql in self.q_all]
        return out

    def tie_residues(self, limit=20000, want=2):
        """small residues r whose digits reach a tie of the inner division (some even p whose y * scale can lie half way)
        and of the outer one (an even scale)"""
        need_inner = any(is_tie(y * self.scale, p) for p in self.ps for y in range(p))
        need_outer = self.scale % 2 == 0
        inner, outer = [], []
        for r in range(limit):
            if (len(inner) >= want or not need_inner) and (len(outer) >= want or not need_outer):
                break
            ys = [(r % p) * inv % p for p, inv in zip(self.ps, self.inv)]
            if need_inner and len(inner) < want and any(is_tie(y * self.scale, p) for y, p in zip(ys, self.ps)):
                inner.append(r)
            if need_outer and len(outer) < want and is_tie(sum(rdiv(y * self.scale, p) for y, p in zip(ys, self.ps)), self.scale):
                outer.append(r)
        return inner, outer


def _rns(coeffs, moduli, rows, cols, n):
    arr = np.asarray(coeffs, dtype=object).reshape(rows, cols, n)
    return np.stack([(arr % q).astype(np.uint64) for q in moduli], axis=2)


def _inputs(plain, rows, cols, n, rnd, extra=()):
    """rows x cols x n integers below Q: the special values first, spread over the entries, then random ones"""
    Q, qs = plain.Q, plain.qs
    inner, outer = plain.tie_residues()
    sp = [0, Q - 1, 1, 2, qs[0] + 3, qs[-1] + 5, qs[0] + qs[-1] + 7, qs[0] - 1, Q // 2] + inner + outer + list(extra)
    sp = [v % Q for v in sp]
    total = rows * cols * n
    flat = (sp + [rnd.randrange(Q) for _ in range(max(0, total - len(sp)))])[:total]
    rnd.shuffle(flat)
    return [[flat[(r * cols + c) * n:(r * cols + c + 1) * n] for c in range(cols)] for r in range(rows)]


_PARAMS = {}


def _params(gpu, n, moduli):
    key = (n, tuple(moduli))
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, list(moduli), 1)
    return _PARAMS[key]


def _check(gpu, p, ps, scale, off, A, rows, cols, seed, level=None, coeffs=None, want_ties=()):
    """decomposition (both source domains, both output formats), gadget vector and residues against Plain"""
    M = gpu.GpuDCRTPolyMatrix
    n = p.ring_dimension()
    moduli = p.moduli() if level is None else p.moduli()[:level + 1]
    plain = Plain(moduli, ps, scale, off, A)
    rnd = random.Random(seed)
    if coeffs is None:
        coeffs = _inputs(plain, rows, cols, n, rnd)
    src_res = _rns(coeffs, moduli, rows, cols, n)
    want = plain.decomposed(coeffs, rows, cols, n)
    for kind in want_ties:
        assert getattr(plain, kind + "_ties") > 0, f"the inputs reach no {kind} tie"
    src_coeff = M.from_rns(p, src_res, False)
    src_eval = M.from_rns(p, src_res, False)
    src_eval.ntt_all_in_place()
    eval_res = src_eval.to_rns()
    for src, res in ((src_coeff, src_res), (src_eval, eval_res)):
        for eval_format in (False, True):
            got = src.nested_rns_decompose(ps, scale, off, A, eval_format)
            assert got.is_ntt == eval_format and got.size() == (want.shape[0], cols) and got.level == len(moduli) - 1
            assert np.array_equal(got.to_coeff_rns(), want), (src.is_ntt, eval_format)
            assert np.array_equal(src.to_rns(), res)  # the source is unchanged
    D = len(ps)
    gvals = plain.gadget_values()
    gwant = np.stack([np.full(n, v % q, dtype=np.uint64) for v in gvals for q in moduli]).reshape(1, A * (D + 1), len(moduli), n)
    for eval_format in (False, True):
        g = M.nested_rns_gadget_vector(p, ps, scale, off, A, eval_format, level)
        assert g.is_ntt == eval_format
        assert np.array_equal(g.to_coeff_rns(), gwant)  # all n coefficients of an entry equal, and the right ones
    rwant = plain.residues(coeffs, rows, cols, n)
    for src in (src_coeff, src_eval):
        r = src.nested_rns_residues(ps, off, A)
        assert not r.is_ntt and np.array_equal(r.to_rns(), rwant)
    return plain, coeffs, want, gwant


def test_the_reference_test_context(gpu):
    """n = 4, 6 x 18 bits, p bits 6, scale 2^8, the 2 x 2 matrix of tests.rs:1151-1197 under the window (1, 2) and the
    full window; in limb off + a the gadget entries times the digit rows sum to the source residue, where Plain says so."""
    cpu = gpu.DCRTPolyParams(4, 6, 18, 6)
    p = gpu.GpuDCRTPolyParams.from_cpu_params(cpu)
    ctx = gpu.NestedRnsContext(p, 6, 2, 1 << 8)
    assert ctx.p_moduli[:6] == [3, 4, 5, 7, 11, 13]
    moduli = p.moduli()
    for off, A, levels_arg, off_arg in ((1, 2, 2, 1), (0, 6, None, None)):
        q0, q1 = moduli[off], moduli[off + 1]
        coeffs = [[[1, q0 + 3, q1 + 5, q0 + q1 + 7], [q0 + 11, 13, q1 + 17, q0 + q1 + 19]],
                  [[q1 + 23, q0 + q1 + 29, 31, q0 + 37], [q0 + q1 + 41, q1 + 43, q0 + 47, 53]]]
        plain, _, want, gwant = _check(gpu, p, ctx.p_moduli, ctx.scale, off, A, 2, 2, SEED, coeffs=coeffs)
        src = gpu.GpuDCRTPolyMatrix.from_coeffs(p, coeffs)
        dec = ctx.gadget_decomposed(src, levels_arg, off_arg)
        gv = ctx.gadget_vector(levels_arg, off_arg)
        assert np.array_equal(dec.to_coeff_rns(), want) and np.array_equal(gv.to_coeff_rns(), gwant)
        res = ctx.residues(src, levels_arg, off_arg).to_rns()
        enc = ctx.encode_poly(coeffs[1][0][3], levels_arg, off_arg)
        assert len(enc) == A * len(ctx.p_moduli)
        for j, poly in enumerate(enc):  # the constant polynomial of coefficient 3 of entry (1, 0), slot by slot
            assert int(poly.inner.to_coeff_rns()[0, 0, 0, 0]) == int(res[A * len(ctx.p_moduli) + j, 0, 0, 3])
        # sum_d gadget[a (D+1) + d] * digit row d = r in limb off + a: confirmed on integers for every input, then on the device's words
        cw = len(ctx.p_moduli) + 1
        gints = plain.gadget_values()
        got, gdev = dec.to_coeff_rns(), gv.to_coeff_rns()
        for row in range(2):
            for col in range(2):
                for k, c in enumerate(coeffs[row][col]):
                    for a in range(A):
                        q = moduli[off + a]
                        digs = plain.digits(c % q)
                        assert sum(gints[a * cw + d] * plain.slot(a, s) for d, s in enumerate(digs)) % q == c % q
                        dev = sum(int(gdev[0, a * cw + d, off + a, k]) * int(got[(row * A + a) * cw + d, col, off + a, k]) for d in range(cw))
                        assert dev % q == c % q


# (n, bits, limbs, p bits, muls, scale, (off, A), rows, cols)
CELLS = [
    (64, 24, 1, 5, 1, 1, (0, 1), 2, 2),
    (256, 24, 3, 7, 2, 1 << 8, (1, 2), 1, 2),
    (64, 24, 9, 10, 4, 3, (2, 4), 1, 1),
    (256, 28, 1, 7, 2, 3, (0, 1), 1, 1),
    (64, 28, 3, 5, 1, 1 << 7, (0, 3), 2, 1),
    (64, 28, 9, 7, 2, 1 << 8, (8, 1), 1, 2),
    (64, 31, 1, 10, 4, 1 << 7, (0, 1), 1, 2),
    (256, 31, 3, 5, 1, 3, (0, 2), 1, 1),
    (64, 31, 9, 7, 2, 1, (4, 5), 1, 1),
    (64, 51, 1, 7, 2, 1 << 8, (0, 1), 2, 2),
    (64, 51, 3, 10, 4, 1, (2, 1), 1, 2),
    (256, 51, 9, 7, 2, 3, (0, 9), 1, 1),
    (256, 60, 1, 10, 4, 1 << 8, (0, 1), 1, 1),
    (64, 60, 3, 7, 2, 1 << 7, (1, 1), 2, 2),
    (64, 60, 9, 10, 4, 1 << 8, (0, 5), 1, 1),
]


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "n%d-%dbit-L%d-p%d-m%d-s%d-w%d_%d-%dx%d" % (c[:6] + c[6] + c[7:]))
def test_cells_are_bit_identical_to_the_plain_reference(gpu, cell):
    n, bits, L, pbits, muls, scale, (off, A), rows, cols = cell
    p = _params(gpu, n, P.primes(n, bits, L))
    ctx = gpu.NestedRnsContext(p, pbits, muls, scale)
    assert max(ctx.p_moduli) < 1 << pbits and 4 in ctx.p_moduli
    # sum_j y_j / p_j is an integer plus r / P with r < q far below P here, so the outer division is never near a tie
    # in these contexts; the explicit p lists below reach that one
    ties = ("inner",) if scale % 2 else ()
    _check(gpu, p, ctx.p_moduli, scale, off, A, rows, cols, SEED + n + bits + L, want_ties=ties)


def test_both_kinds_of_tie_in_one_call(gpu):
    """scale 6 with p = 4: y = 2 gives 12 / 4 (no tie) but y = 1 gives 6 / 4, an inner tie; the even scale has outer ties"""
    n = 64
    p = _params(gpu, n, P.primes(n, 28, 3))
    _check(gpu, p, [3, 4, 5, 7, 11, 13, 17], 6, 0, 3, 1, 2, SEED + 1, want_ties=("inner", "outer"))


def test_table_slice_beyond_lds_and_source_below_full_level(gpu):
    """p_max = 65521: the slice of one window index (3 limbs x 65521 words) does not fit LDS, the kernel reads the table
    from memory; then a two-limb matrix of a three-limb context"""
    n = 64
    for bits in (24, 51):
        p = _params(gpu, n, P.primes(n, bits, 3))
        _check(gpu, p, [3, 4, 5, 7, 65521], 1 << 8, 1, 1, 1, 2, SEED + bits)
        _check(gpu, p, [3, 4, 5, 7, 11, 13, 17, 19, 23], 3, 0, 2, 2, 1, SEED + bits + 1, level=1, want_ties=("inner",))


def test_refusals_launch_nothing_and_leave_the_output_alone(gpu):
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    n, L = 64, 3
    moduli = P.primes(n, 28, L)
    p = _params(gpu, n, moduli)
    other = _params(gpu, n, P.primes(n, 28, L + 1))
    rnd = random.Random(SEED + 9)
    ps = [3, 4, 5, 7, 11]
    D, off, A, rows, cols = len(ps), 1, 2, 2, 2
    lib = _ffi.lib()

    def rand_res(r, c, limbs=L):
        return np.stack([np.asarray([[[rnd.randrange(q) for _ in range(n)] for _ in range(c)] for _ in range(r)], dtype=np.uint64)
                         for q in moduli[:limbs]], axis=2)

    src_res = rand_res(rows, cols)
    src = M.from_rns(p, src_res, False)
    out_rows = rows * A * (D + 1)
    sentinel = rand_res(out_rows, cols)
    foreign = M.from_rns(other, np.ones((rows, cols, L + 1, n), dtype=np.uint64), False)
    low = M.from_rns(p, src_res[:, :, :L - 1], False)

    def call(out, s=src, moduli_=ps, scale=1 << 8, off_=off, A_=A, fmt=0, count=None, null_p=False):
        arr = None if null_p else (C.c_uint64 * max(1, len(moduli_)))(*moduli_)
        return lib.gpupoly_matrix_nested_rns_decompose(None if out is None else out.raw, None if s is None else s.raw, arr,
                                                       len(moduli_) if count is None else count, scale, off_, A_, fmt)

    cases = {
        "null out": (lambda out: call(None), ""),
        "null src": (lambda out: call(out, s=None), ""),
        "null moduli": (lambda out: call(out, null_p=True), ""),
        "format": (lambda out: call(out, fmt=7), ""),
        "no moduli": (lambda out: call(out, count=0), "unsupported"),
        "65 moduli": (lambda out: call(out, moduli_=[3] * 65), "unsupported"),
        "not coprime": (lambda out: call(out, moduli_=[3, 4, 5, 7, 6]), "unsupported"),
        "p = 1": (lambda out: call(out, moduli_=[3, 4, 5, 7, 1]), "unsupported"),
        "p = 2^16": (lambda out: call(out, moduli_=[3, 4, 5, 7, 1 << 16]), "unsupported"),
        "p = 2^16 + 1": (lambda out: call(out, moduli_=[3, 4, 5, 7, (1 << 16) + 1]), "unsupported"),
        "scale 0": (lambda out: call(out, scale=0), "unsupported"),
        "scale 2^62": (lambda out: call(out, scale=1 << 62), "unsupported"),
        "context": (lambda out: call(out, s=foreign), ""),
        "level": (lambda out: call(out, s=low), ""),
        "no levels": (lambda out: call(out, A_=0), ""),
        "window past the end": (lambda out: call(out, off_=2), ""),
        "offset past the end": (lambda out: call(out, off_=L + 1, A_=1), ""),
        "offset wraps": (lambda out: call(out, off_=(1 << 64) - 1, A_=2), ""),
        "shape": (lambda out: call(out, A_=1), ""),
        "out is src": (lambda out: call(out, s=out), ""),  # never the right shape
        "src a view of out": (lambda out: call(out, s=out.row_view(0, rows)), "overlap"),
        "src a view of out's last rows": (lambda out: call(out, s=out.row_view(out_rows - rows, out_rows)), "overlap"),
    }
    for name, (fn, word) in cases.items():
        out = M.from_rns(p, sentinel, False)
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert DECOMPOSE in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name
    # rows of one parent: `out` over the source's rows is refused, `out` beside them is an ordinary call
    parent_res = rand_res(out_rows + rows + 1, cols)
    parent = M.from_rns(p, parent_res, False)
    c0 = lib.gpupoly_launch_count()
    assert call(parent.row_view(0, out_rows), s=parent.row_view(out_rows - 1, out_rows + 1)) != 0
    msg = _ffi.last_error_string()
    assert DECOMPOSE in msg and "overlap" in msg
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), parent_res)
    view_src = parent.row_view(out_rows, out_rows + rows)
    assert call(parent.row_view(0, out_rows), s=view_src) == 0
    plain = Plain(moduli, ps, 1 << 8, off, A)
    ints = [[[sum(int(parent_res[out_rows + r, c, l, k]) * w for l, w in enumerate(p.reconst_coeffs())) % plain.Q for k in range(n)]
             for c in range(cols)] for r in range(rows)]
    got = parent.to_rns()
    assert np.array_equal(got[:out_rows], plain.decomposed(ints, rows, cols, n))
    assert np.array_equal(got[out_rows:], parent_res[out_rows:])  # the source rows and the row after them were not written

    # the other two entries share the checks
    gout = M.from_rns(p, sentinel[:1, :1].repeat(A * (D + 1), axis=1), False)
    gsent = gout.to_rns()
    parr = (C.c_uint64 * 5)(3, 4, 5, 7, 6)
    good = (C.c_uint64 * 5)(*ps)
    for args, word in (((gout.raw, parr, 5, 1 << 8, off, A, 0), "unsupported"), ((gout.raw, good, 5, 1 << 8, 2, A, 0), ""),
                       ((gout.raw, good, 5, 1 << 8, off, 1, 0), ""), ((None, good, 5, 1 << 8, off, A, 0), "")):
        c0 = lib.gpupoly_launch_count()
        assert lib.gpupoly_matrix_fill_nested_rns_gadget(*args) != 0
        msg = _ffi.last_error_string()
        assert GADGET in msg and word in msg and lib.gpupoly_launch_count() == c0
        assert np.array_equal(gout.to_rns(), gsent)
    rout = M.from_rns(p, sentinel[:rows * A * D], False)
    big = (C.c_uint64 * 5)(3, 4, 5, 7, 1 << 16)
    for args, word in (((rout.raw, src.raw, parr, 5, off, A), "unsupported"), ((rout.raw, src.raw, big, 5, off, A), "unsupported"),
                       ((rout.raw, src.raw, good, 5, 2, A), ""), ((rout.raw, rout.raw, good, 5, off, A), ""),
                       ((rout.raw, None, good, 5, off, A), "")):
        c0 = lib.gpupoly_launch_count()
        assert lib.gpupoly_matrix_nested_rns_residues(*args) != 0
        msg = _ffi.last_error_string()
        assert RESIDUES in msg and word in msg and lib.gpupoly_launch_count() == c0
        assert np.array_equal(rout.to_rns(), sentinel[:rows * A * D])
