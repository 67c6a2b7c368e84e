"""GPU: which operands may share memory - the one overlap rule of include/gpupoly.h on every entry point.

Overlap means byte ranges: a row view (`gpupoly_matrix_row_view`) is another object over its parent's bytes.
  1. the point-wise entries run in place on the very same block (same object, or a view with the same start and length)
     and give the out-of-place result, value for value;
  2. any other overlap of their output with an operand is refused;
  3. every other entry that reads matrices and writes one refuses any overlap of what it writes with what it reads;
  4. several outputs: no two writers, no output over another gate's operand;
  5. copy_block / add_block read the source block in full before the first write whenever storage is shared;
  6. disjoint views of one parent are ordinary operands.
A refused call launches nothing and leaves residues and format tags of every matrix as they were.

Expected values come from the CPU restatement (oracle.pointwise / matmul / matrix_ntt / decompose), plain Python big
integers (scale_round) or numpy slicing of a host copy taken before the call (moves) - never from a second device call.
Three contexts, the smallest that reach each word width and both code shapes: n = 256 with two 24-bit limbs (32-bit
words, 16 bytes per lane), n = 64 with two 51-bit limbs (64-bit words), n = 2 with one 17-bit limb (a polynomial is 8
bytes: a view at an odd row is only 8-byte aligned, and transpose / concat / split take their copy_block fall-back).
Rows 0 and 1 of the random matrices are all q - 1 and all 0, so that a stale read does not hide behind chance.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import make_params, rand_matrix

pytestmark = pytest.mark.gpu

# (n, limbs, bits per limb, base_bits): digits per tower 2 / 3 / 1, so k = digits * limbs = 4 / 6 / 1
CTXS = [(256, 2, 24, 12), (64, 2, 51, 17), (2, 1, 17, 17)]
CTX_IDS = ["n256_u32", "n64_u64", "n2_8byte_polys"]
T_SCALE = 65537  # scale_round's t


class _Shape:
    """what the case tables need of a context before any device exists"""

    def __init__(self, cell):
        self.n, self.L, self.bits, self.base = cell
        self.dpt = -(-self.bits // self.base)
        self.k = self.dpt * self.L
        self.segments = self.n % 64 == 0  # the segmented samplers' rings (include/gpupoly.h)
        self.c = (float(1 << self.base) + 1.0) * 4.578  # the G-sampler's width for this base


class _Cx(_Shape):
    def __init__(self, gpu, oracle, cell):
        super().__init__(cell)
        self.gpu, self.oracle = gpu, oracle
        self.p = make_params(gpu, oracle, self.n, self.L, self.bits, self.base)
        self.moduli = self.p.moduli()
        self.M = gpu.GpuDCRTPolyMatrix
        assert self.p.modulus_digits() == self.k
        self._cache = None

    def data(self, seed, rows, cols):
        """uniform residues with row 0 = q - 1 and row 1 = 0 everywhere"""
        a = rand_matrix(self.oracle, seed, rows, cols, self.moduli, self.n)
        for l, q in enumerate(self.moduli):
            a[0, :, l, :] = q - 1
        if rows > 1:
            a[1] = 0
        return a

    def up(self, a, eval_format=True):
        return self.M.from_rns(self.p, a, eval_format)

    def ntt(self, a, inverse=False):
        return self.oracle.matrix_ntt(a, self.moduli, inverse=inverse)

    def pw(self, op, a, b):
        return self.oracle.pointwise(op, np.ascontiguousarray(a), np.ascontiguousarray(b), self.moduli)

    def neg(self, a):
        return self.pw("sub", np.zeros_like(a), a)

    def by_scalar(self, a, s):
        return self.pw("mul", a, np.broadcast_to(s, a.shape).copy())

    def p1_cache(self):
        """the covariance cache of A = B = D = 0 (d = 1: tp2 and the output have two rows)"""
        if self._cache is None:
            z = self.up(np.zeros((1, 1, self.L, self.n), dtype=np.uint64), False)
            self._cache = self.M.create_p1_covariance_cache(z, z, z, 10.0, 30.0, 4.578)
        return self._cache


_CX = {}


@pytest.fixture(params=range(len(CTXS)), ids=CTX_IDS)
def cx(request, gpu, oracle):
    if request.param not in _CX:
        _CX[request.param] = _Cx(gpu, oracle, CTXS[request.param])
    return _CX[request.param]


def _lib():
    from mxx_amd import _ffi

    return _ffi.lib()


def _call(fn, *args):
    """status, message and the kernel launches the call issued"""
    from mxx_amd import _ffi

    before = _lib().gpupoly_launch_count()
    rc = fn(*args)
    launched = _lib().gpupoly_launch_count() - before
    return rc, (_ffi.last_error_string() if rc else ""), launched


def _ok(fn, *args):
    rc, msg, _ = _call(fn, *args)
    assert rc == 0, msg


def _arr(ms):
    return (C.c_void_p * len(ms))(*[m.raw.value for m in ms])


def _ops(gates):
    from mxx_amd import _ffi

    kinds = {"mul": _ffi.GPUPOLY_OP_MUL, "add": _ffi.GPUPOLY_OP_ADD, "sub": _ffi.GPUPOLY_OP_SUB, "mul_scalar": _ffi.GPUPOLY_OP_MUL_SCALAR,
             "neg": _ffi.GPUPOLY_OP_NEG, "decompose": _ffi.GPUPOLY_OP_DECOMPOSE, "mul_decompose": _ffi.GPUPOLY_OP_MUL_DECOMPOSE}
    ops = (_ffi.GpuBatchOp * len(gates))()
    for i, (kind, out, lhs, rhs) in enumerate(gates):
        ops[i].kind, ops[i].out, ops[i].lhs, ops[i].rhs = kinds[kind], out.raw, lhs.raw, (rhs.raw if rhs is not None else None)
    return ops


def _same(m, variant):
    """the very block of m: the object itself, or another object over the same bytes"""
    return m if variant == "object" else m.row_view(0, m.nrow)


VARIANTS = ["object", "view"]


# ---- 1. the allowed in-place forms, value for value -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("eval_format", [True, False], ids=["eval", "coeff"])
@pytest.mark.parametrize("form", ["out_is_lhs", "out_is_rhs", "out_is_lhs_is_rhs"])
@pytest.mark.parametrize("op", ["add", "sub"])
def test_add_sub_in_place(cx, op, form, eval_format, variant):
    """gpu_matrix_add / gpu_matrix_sub with the output as the left operand (what the reference's wrapper calls,
    src/matrix/gpu_dcrt_poly.rs:406,449), the right one, and both."""
    fn = _lib().gpu_matrix_add if op == "add" else _lib().gpu_matrix_sub
    a, b = cx.data(11, 8, 3), cx.data(12, 8, 3)[::-1].copy()  # q - 1 meets 0 and a random row
    ga, gb = cx.up(a, eval_format), cx.up(b, eval_format)
    va, va2, vb = _same(ga, variant), _same(ga, variant), _same(gb, variant)  # alive until the calls have returned
    if form == "out_is_lhs":
        _ok(fn, ga.raw, va.raw, gb.raw)
        assert np.array_equal(ga.to_rns(), cx.pw(op, a, b)) and np.array_equal(gb.to_rns(), b)
    elif form == "out_is_rhs":
        _ok(fn, gb.raw, ga.raw, vb.raw)
        assert np.array_equal(gb.to_rns(), cx.pw(op, a, b)) and np.array_equal(ga.to_rns(), a)
    else:
        _ok(fn, ga.raw, va.raw, va2.raw)
        assert np.array_equal(ga.to_rns(), cx.pw(op, a, a))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("eval_format", [True, False], ids=["eval", "coeff"])
def test_neg_in_place(cx, eval_format, variant):
    a = cx.data(13, 8, 3)
    ga = cx.up(a, eval_format)
    va = _same(ga, variant)
    _ok(_lib().gpupoly_matrix_neg, ga.raw, va.raw)
    assert np.array_equal(ga.to_rns(), cx.neg(a))


@pytest.mark.parametrize("variant", VARIANTS)
def test_mul_scalar_in_place(cx, variant):
    """out == lhs, and the 1x1 out == lhs == scalar (the square of a ring element)"""
    a, s = cx.data(14, 8, 3), cx.data(15, 3, 1)[2:]
    ga, gs = cx.up(a), cx.up(s)
    va = _same(ga, variant)
    _ok(_lib().gpu_matrix_mul_scalar, ga.raw, va.raw, gs.raw)
    assert np.array_equal(ga.to_rns(), cx.by_scalar(a, s)) and np.array_equal(gs.to_rns(), s)
    for one in (s, cx.data(16, 1, 1)):  # a random element and q - 1
        g1 = cx.up(one)
        v1, v2 = _same(g1, variant), _same(g1, variant)
        _ok(_lib().gpu_matrix_mul_scalar, g1.raw, v1.raw, v2.raw)
        assert np.array_equal(g1.to_rns(), cx.pw("mul", one, one))


def _scale_round_want(cx, coeff, round_half):
    """floor((t c + h) / Q) mod t of every coefficient, by Python integers, as residues of every limb"""
    Q = math.prod(cx.moduli)
    h = Q // 2 if round_half else 0
    x = np.zeros(coeff.shape[:2] + coeff.shape[3:], dtype=object)
    for l, q in enumerate(cx.moduli):
        x += coeff[:, :, l, :].astype(object) * ((Q // q) * pow(Q // q, -1, q))
    w = ((T_SCALE * (x % Q) + h) // Q) % T_SCALE
    return np.stack([(w % q).astype(np.uint64) for q in cx.moduli], axis=2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("round_half", [0, 1])
@pytest.mark.parametrize("eval_format", [True, False], ids=["eval", "coeff"])
def test_scale_round_in_place(cx, eval_format, round_half, variant):
    """out == in: a COEFF input is rescaled where it lies, an EVAL input is inverse-transformed there first"""
    coeff = cx.data(17, 4, 3)
    g = cx.up(cx.ntt(coeff) if eval_format else coeff, eval_format)
    vg = _same(g, variant)
    _ok(_lib().gpupoly_matrix_scale_round, g.raw, vg.raw, T_SCALE, round_half)
    g.is_ntt = False  # the entry tags its output COEFF: to_rns() in COEFF format reads it only then
    assert np.array_equal(g.to_rns(), _scale_round_want(cx, coeff, round_half))


@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_pointwise_gates_in_place(cx, variant):
    """the ADD / SUB / NEG / MUL_SCALAR gates of gpupoly_batch on the very block of their output, all in one call"""
    d = [cx.data(20 + i, 8, 3) for i in range(7)]
    s, one = cx.data(30, 3, 1)[2:], cx.data(31, 1, 1)
    g = [cx.up(x) for x in d]
    gs, g1 = cx.up(s), cx.up(one)
    v = lambda m: _same(m, variant)
    keep = [v(g[0]), v(g[3]), v(g[4]), v(g[4]), v(g[5]), v(g[6]), v(g1), v(g1)]  # the views live until the call returns
    gates = [("add", g[0], keep[0], g[1]), ("sub", g[3], g[2], keep[1]), ("add", g[4], keep[2], keep[3]), ("neg", g[5], keep[4], None),
             ("mul_scalar", g[6], keep[5], gs), ("mul_scalar", g1, keep[6], keep[7])]
    _ok(_lib().gpupoly_batch, _ops(gates), len(gates), cx.base)
    assert np.array_equal(g[0].to_rns(), cx.pw("add", d[0], d[1]))
    assert np.array_equal(g[3].to_rns(), cx.pw("sub", d[2], d[3]))
    assert np.array_equal(g[4].to_rns(), cx.pw("add", d[4], d[4]))
    assert np.array_equal(g[5].to_rns(), cx.neg(d[5]))
    assert np.array_equal(g[6].to_rns(), cx.by_scalar(d[6], s))
    assert np.array_equal(g1.to_rns(), cx.pw("mul", one, one))
    for m, x in ((g[1], d[1]), (g[2], d[2]), (gs, s)):
        assert np.array_equal(m.to_rns(), x)  # the operands that were only read


# ---- 2. disjoint views of one parent are ordinary operands ----------------------------------------------------------------
def _rows(cx, total, lens):
    """consecutive row blocks of the given lengths inside `total` rows, and the rows left over as guards: from row 0
    where polynomials are 16-byte multiples, from row 1 - odd starts, 8-byte alignment - on the n = 2 context"""
    at = 1 if cx.n == 2 else 0
    blocks = []
    for ln in lens:
        blocks.append((at, at + ln))
        at += ln
    assert at <= total and total - sum(lens) >= 1, "one guard row at least"
    return blocks


def _check_untouched(parent, host, written):
    """every row outside `written` - the guard row among them - bit for bit as before"""
    now = parent.to_rns()
    keep = [r for r in range(host.shape[0]) if not (written[0] <= r < written[1])]
    assert np.array_equal(now[keep], host[keep])
    return now[written[0] : written[1]]


@pytest.mark.parametrize("entry", ["mul", "add", "add_rows", "transpose", "decompose_base", "mul_scalar_intt"])
def test_disjoint_views_of_one_parent(cx, entry):
    lib = _lib()
    if entry in ("mul", "add", "add_rows"):
        host = cx.data(40, 8, 3)
        P = cx.up(host)
        (o, l, r) = _rows(cx, 8, [2, 2, 3])
        out, lhs, rhs = P.row_view(*o), P.row_view(*l), P.row_view(*r)
        if entry == "mul":
            _ok(lib.gpu_matrix_mul, out.raw, lhs.raw, rhs.raw)
            want = cx.oracle.matmul(host[l[0] : l[1]], host[r[0] : r[1]], cx.moduli)
        else:
            rhs2 = P.row_view(r[0] + 1, r[1])
            if entry == "add":
                _ok(lib.gpu_matrix_add, out.raw, lhs.raw, rhs2.raw)
            else:  # the sum lands in rows `o` of the parent itself: the operands are views of its other rows
                _ok(lib.gpupoly_matrix_add_rows, P.raw, o[0], lhs.raw, rhs2.raw)
            want = cx.pw("add", host[l[0] : l[1]], host[r[0] + 1 : r[1]])
        assert np.array_equal(_check_untouched(P, host, o), want)
        assert np.array_equal(out.to_rns(), want)
    elif entry == "transpose":
        host = cx.data(41, 8, 3)
        P = cx.up(host)
        (o, s) = _rows(cx, 8, [3, 3]) if cx.n == 2 else [(0, 3), (4, 7)]
        out, src = P.row_view(*o), P.row_view(*s)
        _ok(lib.gpupoly_matrix_transpose, out.raw, src.raw)
        want = np.ascontiguousarray(host[s[0] : s[1]].transpose(1, 0, 2, 3))
        assert np.array_equal(_check_untouched(P, host, o), want)
    elif entry == "decompose_base":
        total = 2 * cx.k + 2 + 2
        host = cx.data(42, total, 3)
        P = cx.up(host, False)
        (o, s) = _rows(cx, total, [2 * cx.k, 2])
        out = P.row_view(*o)  # tagged COEFF like its parent: the digits stay coefficients
        src = P.row_view(*s)
        _ok(lib.gpu_matrix_decompose_base, src.raw, cx.base, out.raw)
        want = cx.oracle.decompose(np.ascontiguousarray(host[s[0] : s[1]]), cx.moduli, cx.base)
        assert np.array_equal(_check_untouched(P, host, o), want)
    else:
        host = cx.data(43, 8, 1)
        P = cx.up(host)
        (o, l, sc) = _rows(cx, 8, [2, 2, 1])
        out = P.row_view(*o)
        lhs, scalar = P.row_view(*l), P.row_view(*sc)
        _ok(lib.gpupoly_matrix_mul_scalar_intt, out.raw, lhs.raw, scalar.raw)
        want = cx.ntt(cx.by_scalar(np.ascontiguousarray(host[l[0] : l[1]]), host[sc[0] : sc[1]]), inverse=True)
        out.is_ntt = False  # tagged COEFF by the entry
        assert np.array_equal(out.to_rns(), want)
        # the parent's own tag is still EVAL: its bytes are read as they lie
        assert np.array_equal(_check_untouched(P, host, o), want)


# ---- 3. the refusal matrix -------------------------------------------------------------------------------------------------
# One entry: (name, token the message must contain, rule, output shape, operands [(rows, cols, eval_format)], operand
# positions to alias, call(lib, cx, out, ops)).  Rule 2 entries refuse a partial overlap ("shifted"); rule 3 / 4 entries
# refuse the very same block through another object as well ("exact"), wherever an operand can have the output's shape.
def _seed():
    from mxx_amd import _ffi

    return _ffi.GpuRngSeed()


def _segs(cols):
    from mxx_amd import _ffi

    return (_ffi.GpuRngSeed * 1)(), (C.c_size_t * 1)(cols), 1


def _batch1(kind):
    def call(lib, cx, out, ops):
        return lib.gpupoly_batch(_ops([(kind, out, ops[0], ops[1] if len(ops) > 1 else None)]), 1, cx.base)

    return call


def _entries(s):
    E, Cf = True, False
    k, dpt = s.k, s.dpt
    sq = (3, 3, E)
    out = []
    add = lambda *e: out.append(e)
    # rule 2: the point-wise entries
    add("add", "gpu_matrix_add", 2, (3, 3), [sq, sq], [0, 1], lambda lib, cx, o, p: lib.gpu_matrix_add(o.raw, p[0].raw, p[1].raw))
    add("sub", "gpu_matrix_sub", 2, (3, 3), [sq, sq], [0, 1], lambda lib, cx, o, p: lib.gpu_matrix_sub(o.raw, p[0].raw, p[1].raw))
    add("neg", "gpupoly_matrix_neg", 2, (3, 3), [sq], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_neg(o.raw, p[0].raw))
    add("mul_scalar", "gpu_matrix_mul_scalar", 2, (3, 1), [(3, 1, E), (1, 1, E)], [0, 1],
        lambda lib, cx, o, p: lib.gpu_matrix_mul_scalar(o.raw, p[0].raw, p[1].raw))
    add("mul_scalar_intt", "gpupoly_matrix_mul_scalar_intt", 2, (3, 1), [(3, 1, E), (1, 1, E)], [0, 1],
        lambda lib, cx, o, p: lib.gpupoly_matrix_mul_scalar_intt(o.raw, p[0].raw, p[1].raw))
    add("scale_round", "gpupoly_matrix_scale_round", 2, (3, 3), [(3, 3, Cf)], [0],
        lambda lib, cx, o, p: lib.gpupoly_matrix_scale_round(o.raw, p[0].raw, T_SCALE, 1))
    add("scale_round_eval", "gpupoly_matrix_scale_round", 2, (3, 3), [sq], [0],
        lambda lib, cx, o, p: lib.gpupoly_matrix_scale_round(o.raw, p[0].raw, T_SCALE, 0))
    add("copy", "gpu_matrix_copy", 2, (3, 3), [sq], [0], lambda lib, cx, o, p: lib.gpu_matrix_copy(o.raw, p[0].raw))
    add("batch_add", "gpupoly_batch", 2, (3, 3), [sq, sq], [0, 1], _batch1("add"))
    add("batch_sub", "gpupoly_batch", 2, (3, 3), [sq, sq], [0, 1], _batch1("sub"))
    add("batch_neg", "gpupoly_batch", 2, (3, 3), [sq], [0], _batch1("neg"))
    add("batch_mul_scalar", "gpupoly_batch", 2, (3, 1), [(3, 1, E), (1, 1, E)], [0, 1], _batch1("mul_scalar"))
    # rule 3: everything else that reads matrices and writes one
    add("mul", "gpu_matrix_mul", 3, (3, 3), [sq, sq], [0, 1], lambda lib, cx, o, p: lib.gpu_matrix_mul(o.raw, p[0].raw, p[1].raw))
    add("tensor_lhs", "gpupoly_matrix_tensor", 3, (3, 3), [sq, (1, 1, E)], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_tensor(o.raw, p[0].raw, p[1].raw))
    add("tensor_rhs", "gpupoly_matrix_tensor", 3, (3, 3), [(1, 1, E), sq], [1], lambda lib, cx, o, p: lib.gpupoly_matrix_tensor(o.raw, p[0].raw, p[1].raw))
    add("mul_tensor_identity", "gpupoly_matrix_mul_tensor_identity", 3, (3, 3), [sq, sq], [0, 1],
        lambda lib, cx, o, p: lib.gpupoly_matrix_mul_tensor_identity(o.raw, p[0].raw, p[1].raw, 1))
    for name, kk, fn in (("mul_decompose", k, lambda lib, cx, o, p: lib.gpupoly_matrix_mul_decompose(o.raw, p[0].raw, p[1].raw, cx.base)),
                         ("mul_decompose_small", dpt, lambda lib, cx, o, p: lib.gpupoly_matrix_mul_decompose_small(o.raw, p[0].raw, p[1].raw, cx.base)),
                         ("mul_tensor_identity_decompose", k,
                          lambda lib, cx, o, p: lib.gpupoly_matrix_mul_tensor_identity_decompose(o.raw, p[0].raw, p[1].raw, 1, cx.base))):
        add(name + "_rhs", "gpupoly_matrix_" + name, 3, (3, 3), [(3, 3 * kk, E), sq], [1], fn)
        add(name + "_lhs", "gpupoly_matrix_" + name, 3, (3, kk), [(3, kk, E), (1, kk, E)], [0], fn)
    add("add_rows", "gpupoly_matrix_add_rows", 3, (2, 3), [(2, 3, E), (2, 3, E)], [0, 1],
        lambda lib, cx, o, p: lib.gpupoly_matrix_add_rows(o.raw, 0, p[0].raw, p[1].raw))
    add("ntt_add_rows", "gpupoly_matrix_ntt_add_rows", 3, (2, 3), [(2, 3, Cf), (2, 3, E)], [0, 1],
        lambda lib, cx, o, p: lib.gpupoly_matrix_ntt_add_rows(o.raw, 0, p[0].raw, p[1].raw, 0))
    add("transpose", "gpupoly_matrix_transpose", 3, (3, 3), [sq], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_transpose(o.raw, p[0].raw))
    add("fill_identity", "gpupoly_matrix_fill_identity", 3, (1, 1), [(1, 1, E)], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_fill_identity(o.raw, p[0].raw))
    add("identity_chunk", "gpu_matrix_fill_small_decomposed_identity_chunk", 3, (3, 3), [(1, 3, E)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_fill_small_decomposed_identity_chunk(o.raw, p[0].raw, 1))
    add("decompose_base", "gpu_matrix_decompose_base", 3, (2 * k, 3), [(2, 3, Cf)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_decompose_base(p[0].raw, cx.base, o.raw))
    add("decompose_base_eval_src", "gpu_matrix_decompose_base", 3, (2 * k, 3), [(2, 3, E)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_decompose_base(p[0].raw, cx.base, o.raw))
    add("decompose_base_small", "gpu_matrix_decompose_base", 3, (2 * dpt, 3), [(2, 3, Cf)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_decompose_base_small(p[0].raw, cx.base, o.raw))
    # the source is EVAL: a refusal comes before it is taken to the coefficient domain
    add("gauss_samp", "gauss_samp_gq_arb_base", 3, (2 * k, 3), [(2, 3, E)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_gauss_samp_gq_arb_base(p[0].raw, cx.base, cx.c, 4.578, _seed(), o.raw))
    add("p1_cached", "sample_p1_full_cached", 3, (2, 3), [(2, 3, Cf)], [0],
        lambda lib, cx, o, p: lib.gpu_matrix_sample_p1_full_cached(cx.p1_cache().raw, p[0].raw, _seed(), o.raw))
    p1_full = lambda lib, cx, o, p: lib.gpu_matrix_sample_p1_full(p[0].raw, p[1].raw, p[2].raw, p[3].raw, 10.0, 30.0, 4.578, _seed(), o.raw)
    add("p1_full_tp2", "gpu_matrix_sample_p1_full", 3, (2, 3), [(1, 1, Cf)] * 3 + [(2, 3, Cf)], [3], p1_full)
    add("p1_full_abd", "gpu_matrix_sample_p1_full", 3, (2, 1), [(1, 1, Cf)] * 3 + [(2, 1, Cf)], [0, 1, 2], p1_full)
    if s.segments:
        add("gauss_samp_segments", "gauss_samp_gq_arb_base", 3, (2 * k, 3), [(2, 3, E)], [0],
            lambda lib, cx, o, p: lib.gpupoly_matrix_gauss_samp_gq_arb_base_segments(p[0].raw, cx.base, cx.c, 4.578, *_segs(3), o.raw))
        add("p1_cached_segments", "sample_p1_full_cached", 3, (2, 3), [(2, 3, Cf)], [0],
            lambda lib, cx, o, p: lib.gpupoly_matrix_sample_p1_full_cached_segments(cx.p1_cache().raw, p[0].raw, *_segs(3), o.raw))
    # rule 4: several outputs (one product / gate whose output meets its own operand, then two whose storage meets)
    add("mul_batch", "gpupoly_matrix_mul_batch", 3, (3, 3), [sq, sq], [0, 1],
        lambda lib, cx, o, p: lib.gpupoly_matrix_mul_batch(_arr([o]), _arr([p[0]]), _arr([p[1]]), 1))
    add("mul_batch_other_product", "gpupoly_matrix_mul_batch", 3, (3, 3), [sq] * 5, [3, 4],  # p[2] is the second product's output
        lambda lib, cx, o, p: lib.gpupoly_matrix_mul_batch(_arr([o, p[2]]), _arr([p[0], p[3]]), _arr([p[1], p[4]]), 2))
    add("mul_batch_two_writers", "gpupoly_matrix_mul_batch", 3, (3, 3), [sq] * 5, [4],  # p[4] is the second product's output
        lambda lib, cx, o, p: lib.gpupoly_matrix_mul_batch(_arr([o, p[4]]), _arr([p[0], p[2]]), _arr([p[1], p[3]]), 2))
    add("batch_mul", "gpupoly_batch", 3, (3, 3), [sq, sq], [0, 1], _batch1("mul"))
    add("batch_decompose", "gpupoly_batch", 3, (2 * k, 3), [(2, 3, Cf)], [0], _batch1("decompose"))
    add("batch_mul_decompose_rhs", "gpupoly_batch", 3, (3, 3), [(3, 3 * k, E), sq], [1], _batch1("mul_decompose"))
    add("batch_mul_decompose_lhs", "gpupoly_batch", 3, (3, k), [(3, k, E), (1, k, E)], [0], _batch1("mul_decompose"))
    add("batch_other_gate", "gpupoly_batch", 3, (3, 3), [sq] * 4, [3],  # gate 1 negates p[3] into p[2]
        lambda lib, cx, o, p: lib.gpupoly_batch(_ops([("add", o, p[0], p[1]), ("neg", p[2], p[3], None)]), 2, cx.base))
    add("batch_two_writers", "gpupoly_batch", 3, (3, 3), [sq] * 4, [3],  # gate 1 writes p[3]
        lambda lib, cx, o, p: lib.gpupoly_batch(_ops([("add", o, p[0], p[1]), ("neg", p[3], p[2], None)]), 2, cx.base))
    add("concat_columns", "gpupoly_matrix_concat_columns", 3, (3, 3), [sq], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_concat_columns(o.raw, _arr([p[0]]), 1))
    add("split_columns", "gpupoly_matrix_split_columns", 3, (3, 3), [sq], [0], lambda lib, cx, o, p: lib.gpupoly_matrix_split_columns(p[0].raw, _arr([o]), 1))
    return out


def _ways(entry):
    """(position, way) pairs an entry is refused in"""
    name, _tok, rule, oshape, operands, positions, _call_ = entry
    pairs = []
    for pos in positions:
        rows, cols, _fmt = operands[pos]
        assert cols == oshape[1], (name, "an aliasing operand has the output's column count")
        if rows >= 2 or oshape[0] >= 2:
            pairs.append((pos, "shifted"))
        if rule == 3 and (rows, cols) == tuple(oshape):
            pairs.append((pos, "exact"))
    return pairs


REFUSALS = [(ci, e[0], pos, way) for ci, cell in enumerate(CTXS) for e in _entries(_Shape(cell)) for pos, way in _ways(e)]


@pytest.mark.parametrize("ci,name,pos,way", REFUSALS, ids=[f"{CTX_IDS[c]}-{nm}-operand{ps}-{w}" for c, nm, ps, w in REFUSALS])
def test_overlap_is_refused_with_nothing_launched_and_nothing_changed(gpu, oracle, ci, name, pos, way):
    """Operand `pos` overlaps the output - both are row views of one parent, shifted by one row against each other, or two
    objects over exactly the same rows.  The call is refused, names its entry point and the reason, launches no kernel,
    and every matrix passed in keeps its residues and its format tag (to_rns() asks for the format the matrix had, and
    the store refuses another)."""
    if ci not in _CX:
        _CX[ci] = _Cx(gpu, oracle, CTXS[ci])
    cx = _CX[ci]
    entry = next(e for e in _entries(cx) if e[0] == name)
    _n, token, _rule, (orows, ocols), operands, _positions, call = entry
    rows, cols, fmt = operands[pos]
    parent_host = cx.data(50 + pos, max(orows, rows) + 2, ocols)
    if name == "p1_full_abd":
        parent_host[:] = 0  # the covariance operand is a view of it: A = B = D = 0 is a valid covariance whatever the call does
    parent = cx.up(parent_host, fmt)  # views start with their parent's tag: the one the aliasing operand needs
    out = parent.row_view(1, 1 + orows)
    if way == "exact":
        at = (1, 1 + orows)
    else:
        at = (0, rows) if rows >= 2 else (1, 2)  # one row: the first row of a taller output
    alias = parent.row_view(*at)
    assert (at != (1, 1 + orows)) == (way == "shifted") and at[0] < 1 + orows and 1 < at[1], "the case is what it says"
    host = [None if j == pos else cx.data(60 + j, r, c) for j, (r, c, _f) in enumerate(operands)]
    if name.startswith("p1_full"):
        for j in range(3):
            if host[j] is not None:
                host[j][:] = 0
    mats = [alias if j == pos else cx.up(host[j], f) for j, (_r, _c, f) in enumerate(operands)]
    if name.startswith("p1_cached"):
        cx.p1_cache()  # built outside the counted call
    rc, msg, launched = _call(call, _lib(), cx, out, mats)
    assert rc != 0, f"{name}: operand {pos} overlapping the output ({way}) was accepted"
    assert token in msg and ("alias" in msg or "overlap" in msg), msg
    assert launched == 0, f"{name}: {launched} kernel launches in a refused call"
    assert np.array_equal(parent.to_rns(), parent_host)
    assert np.array_equal(out.to_rns(), parent_host[1 : 1 + orows])
    assert np.array_equal(alias.to_rns(), parent_host[at[0] : at[1]])
    for j, m in enumerate(mats):
        if j != pos:
            assert np.array_equal(m.to_rns(), host[j]), f"operand {j} changed"


@pytest.mark.parametrize("entry", ["add_rows", "ntt_add_rows"])
def test_row_block_writers_are_judged_on_the_destination_rows(cx, entry):
    """out[2:4] = f(operands): an operand that is a view of other rows of `out` is legal and gives the right sum; one
    that reaches into rows 2..3 is refused with nothing launched and nothing changed."""
    lib = _lib()
    host = cx.data(70, 6, 3)
    addend_host = cx.data(71, 2, 3)
    P = cx.up(host, entry == "add_rows")
    first, last, reaching = P.row_view(0, 2), P.row_view(4, 6), P.row_view(1, 3)
    addend = cx.up(addend_host, True)
    if entry == "add_rows":
        refused = lambda: lib.gpupoly_matrix_add_rows(P.raw, 2, reaching.raw, last.raw)
        refused2 = lambda: lib.gpupoly_matrix_add_rows(P.raw, 2, first.raw, reaching.raw)
        legal = lambda: lib.gpupoly_matrix_add_rows(P.raw, 2, first.raw, last.raw)
        want = cx.pw("add", host[0:2], host[4:6])
    else:
        refused = lambda: lib.gpupoly_matrix_ntt_add_rows(P.raw, 2, reaching.raw, addend.raw, 0)
        refused2 = lambda: lib.gpupoly_matrix_ntt_add_rows(P.raw, 2, reaching.raw, addend.raw, 1)
        legal = lambda: lib.gpupoly_matrix_ntt_add_rows(P.raw, 2, first.raw, addend.raw, 0)
        want = cx.pw("add", cx.ntt(np.ascontiguousarray(host[0:2])), addend_host)
    for fn in (refused, refused2):
        rc, msg, launched = _call(fn)
        assert rc != 0 and "gpupoly_matrix_" + entry in msg and "alias" in msg and launched == 0, (rc, msg, launched)
        assert np.array_equal(P.to_rns(), host) and np.array_equal(reaching.to_rns(), host[1:3]) and np.array_equal(addend.to_rns(), addend_host)
    _ok(legal)
    P.is_ntt = True if entry == "ntt_add_rows" else P.is_ntt  # the whole destination is tagged EVAL
    assert np.array_equal(_check_untouched(P, host, (2, 4)), want)
    assert np.array_equal(first.to_rns(), host[0:2])  # the view keeps its own tag (COEFF for ntt_add_rows: not consumed)


def test_all_gather_columns_refuses_a_block_inside_its_output(gpu, oracle, monkeypatch):
    """full[r] must be disjoint from local_blocks[r] by bytes: a one-context communicator (event-ordered peer copies)
    whose block is a view of the output's parent, shifted and exact"""
    monkeypatch.setenv("MXX_HIP_COMM", "peer")
    if 0 not in _CX:
        _CX[0] = _Cx(gpu, oracle, CTXS[0])
    cx = _CX[0]
    lib = _lib()
    comm = C.c_void_p()
    _ok(lib.gpupoly_comm_create, (C.c_void_p * 1)(cx.p.ctx_raw()), 1, C.byref(comm))
    try:
        host = cx.data(80, 5, 3)
        P = cx.up(host)
        full = P.row_view(1, 4)
        for at in ((0, 3), (1, 4)):
            block = P.row_view(*at)
            rc, msg, launched = _call(lib.gpupoly_matrix_all_gather_columns, comm, _arr([block]), _arr([full]))
            assert rc != 0 and "gpupoly_matrix_all_gather_columns" in msg and "alias" in msg and launched == 0, (rc, msg, launched)
            assert np.array_equal(P.to_rns(), host) and np.array_equal(full.to_rns(), host[1:4]) and np.array_equal(block.to_rns(), host[at[0] : at[1]])
    finally:
        lib.gpupoly_comm_destroy(comm)


# ---- 4. block copies with shared storage ------------------------------------------------------------------------------------
# (source corner, destination corner, rows, cols) in the parent's coordinates, a 6 x 3 matrix
RECTS = {
    "shifted_down_and_right": ((1, 0), (2, 1), 3, 2),  # overlapping: the destination is the source moved by (1, 1)
    "disjoint": ((1, 0), (3, 2), 2, 1),
    "identical": ((1, 1), (1, 1), 3, 2),  # add_block doubles in place
}


@pytest.mark.parametrize("shared", ["same_object", "src_is_a_view", "both_are_views"])
@pytest.mark.parametrize("rect", list(RECTS))
@pytest.mark.parametrize("op", ["copy_block", "add_block"])
def test_block_copies_read_the_source_block_before_they_write(cx, op, rect, shared):
    """out and src share storage: the result is that of reading the whole source block first (numpy on a host copy
    taken before the call)."""
    (sr, sc), (dr, dc), rows, cols = RECTS[rect]
    host = cx.data(90, 6, 3)
    P = cx.up(host)
    if shared == "same_object":
        out, src, so, do = P, P, 0, 0
    elif shared == "src_is_a_view":
        out, src, so, do = P, P.row_view(1, 6), 1, 0
    else:
        out, src, so, do = P.row_view(0, 5), P.row_view(1, 6), 1, 0
    fn = _lib().gpu_matrix_copy_block if op == "copy_block" else _lib().gpu_matrix_add_block
    _ok(fn, out.raw, src.raw, dr - do, dc, sr - so, sc, rows, cols)
    want = host.copy()
    block = host[sr : sr + rows, sc : sc + cols].copy()
    if op == "copy_block":
        want[dr : dr + rows, dc : dc + cols] = block
    else:
        want[dr : dr + rows, dc : dc + cols] = cx.pw("add", host[dr : dr + rows, dc : dc + cols], block)
    assert np.array_equal(P.to_rns(), want)


def test_matrix_copy_onto_itself(cx):
    """gpu_matrix_copy: the same block (object or view) is a no-op; a shifted view is refused"""
    lib = _lib()
    host = cx.data(91, 5, 3)
    P = cx.up(host)
    a, same, shifted = P.row_view(1, 4), P.row_view(1, 4), P.row_view(0, 3)
    for dst, src in ((P, P), (a, same)):
        rc, msg, launched = _call(lib.gpu_matrix_copy, dst.raw, src.raw)
        assert rc == 0 and launched == 0, msg
        assert np.array_equal(P.to_rns(), host)
    rc, msg, launched = _call(lib.gpu_matrix_copy, a.raw, shifted.raw)
    assert rc != 0 and "gpu_matrix_copy" in msg and "overlap" in msg and launched == 0, (rc, msg, launched)
    assert np.array_equal(P.to_rns(), host)


# ---- 5. split_columns: every block is written ---------------------------------------------------------------------------------
def test_split_columns_blocks_must_be_disjoint(cx):
    lib = _lib()
    src_host = cx.data(92, 3, 4)
    src = cx.up(src_host)
    # the same block twice: two writers
    blk_host = cx.data(93, 3, 2)
    blk = cx.up(blk_host)
    rc, msg, launched = _call(lib.gpupoly_matrix_split_columns, src.raw, _arr([blk, blk]), 2)
    assert rc != 0, "a split into the same block twice was accepted"
    assert "gpupoly_matrix_split_columns" in msg and ("alias" in msg or "overlap" in msg) and launched == 0, (msg, launched)
    assert np.array_equal(blk.to_rns(), blk_host) and np.array_equal(src.to_rns(), src_host)
    # two views of one parent that meet in one row
    P_host = cx.data(94, 7, 2)
    P = cx.up(P_host)
    top, meeting = P.row_view(0, 3), P.row_view(2, 5)
    rc, msg, launched = _call(lib.gpupoly_matrix_split_columns, src.raw, _arr([top, meeting]), 2)
    assert rc != 0 and ("alias" in msg or "overlap" in msg) and launched == 0, (rc, msg, launched)
    assert np.array_equal(P.to_rns(), P_host)
    # two disjoint views of one parent: an ordinary split (odd start rows: 8-byte alignment on the n = 2 context)
    lo, hi = P.row_view(1, 4), P.row_view(4, 7)
    _ok(lib.gpupoly_matrix_split_columns, src.raw, _arr([lo, hi]), 2)
    want = P_host.copy()
    want[1:4], want[4:7] = src_host[:, 0:2], src_host[:, 2:4]
    assert np.array_equal(P.to_rns(), want) and np.array_equal(src.to_rns(), src_host)
    # a concat may read one block twice
    wide = cx.up(cx.data(95, 3, 4))
    _ok(lib.gpupoly_matrix_concat_columns, wide.raw, _arr([blk, blk]), 2)
    assert np.array_equal(wide.to_rns(), np.concatenate([blk_host, blk_host], axis=1))
