"""GPU: the whole text of what the six target-builder entries refuse with (`gpupoly_matrix_lut_targets`, `_lwe_targets`,
`_wee25_targets` and their `_combine` / `_product` instruments; mxx_amd/csrc/row_targets.h).

The entries' own refusal tests look for a keyword; the checks behind them are shared helpers that each entry calls in its
own order, with its own shape sentences and its own position suffix, so this one pins every message letter by letter, the
order of the checks through calls with two faults at once, and that a refused call launches nothing.  EXPECTED was recorded
by running these very calls against the library as it was before the helpers were shared; one text differs from that
record on purpose: the LUT combine entry's "too many target polynomials" names the entry that was called, which no
test-sized call reaches."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params
from test_gpu_lut_targets import CONTEXTS

pytestmark = pytest.mark.gpu

KEY = bytes((7 * i + 1) & 0xFF for i in range(32))
LUT, LUT_COMBINE = "gpupoly_matrix_lut_targets", "gpupoly_matrix_lut_targets_combine"
LWE, LWE_COMBINE = "gpupoly_matrix_lwe_targets", "gpupoly_matrix_lwe_targets_combine"
WEE25, WEE25_PRODUCT = "gpupoly_matrix_wee25_targets", "gpupoly_matrix_wee25_targets_product"

_CHUNK = {  # the cases of the four chunk entries whose text does not depend on the entry
    "null output in the middle": "null output (row 1)",
    "output of another level, last": "level mismatch (row 2)",
    "output of another width": "the outputs differ in width (row 1)",
    "output rows": "shape mismatch: an output is d x chunk columns (row 2)",
    "base_bits 63": "base_bits must be in 1..62",
    "chunk past the end": "column chunk past the operands' columns",
    "the same output twice": "overlap: an output is given twice",
    "two overlapping row views": "overlap: an output overlaps another output",
    "two faults: null y_words, base_bits 0": "null array",
    "two faults: words_per_y 0, null output": "null output (row 1)",
    "two faults: chunk past the end, another width": "column chunk past the operands' columns",
}
_WEE25 = {
    "null output in the middle": "null output (block 0, part 1)",
    "output of another level, last": "level mismatch (block 1, part 1)",
    "output of another width": "shape mismatch: an output is secret_size x m_b (block 1, part 0)",
    "T_bottom shape": "shape mismatch: T_bottom is m_b x (a multiple of m_b)",
    "COEFF T_bottom": "requires Eval format",
    "base_bits 63": "base_bits must be in 1..62",
    "part past the end": "column parts past T_bottom's columns",
    "output overlaps T_bottom": "overlap: an output overlaps T_bottom (row 3)",
    "the same output twice": "overlap: an output is given twice",
    "two overlapping row views": "overlap: an output overlaps another output",
    "two faults: null idx, base_bits 0": "null array",
    "two faults: secret_size 0, null output": "null output (block 0, part 1)",
    "two faults: part past the end, COEFF T_bottom": "requires Eval format",
}
EXPECTED = {
    LUT: dict(_CHUNK, **{
        "W operand shape": "shape mismatch: the W operands are d x (d * digits per tower * limbs)",
        "COEFF operand": "requires Eval format",
        "output overlaps w_identity": "overlap: an output overlaps an operand (row 1)",
        "output overlaps w_gy": "overlap: an output overlaps an operand (row 2)",
        "output overlaps w_v": "overlap: an output overlaps an operand (row 1)",
        "output overlaps w_vx": "overlap: an output overlaps an operand (row 2)",
    }),
    LUT_COMBINE: dict(_CHUNK, **{
        "W operand shape": "shape mismatch: the W operands are d x (d * digits per tower * limbs)",
        "product shape": "shape mismatch: the product is 2d x (rows * chunk columns)",
        "COEFF operand": "requires Eval format",
        "output overlaps w_identity": "overlap: an output overlaps an operand (row 1)",
        "output overlaps w_gy": "overlap: an output overlaps an operand (row 2)",
        "output overlaps the product": "overlap: an output overlaps the product (row 1)",
    }),
    LWE: dict(_CHUNK, **{
        "A_z shape": "shape mismatch: A_z is d x (d * digits per tower * limbs)",
        "A_lt shape": "shape mismatch: A_lt is d x (d * digits per tower * limbs)",
        "COEFF operand": "requires Eval format",
        "output overlaps a_z": "overlap: an output overlaps an operand (row 1)",
        "output overlaps a_lt": "overlap: an output overlaps an operand (row 2)",
    }),
    LWE_COMBINE: dict(_CHUNK, **{
        "digits shape": "shape mismatch: the digits are m x (rows * chunk columns)",
        "A_lt shape": "shape mismatch: A_lt is d x (d * digits per tower * limbs)",
        "product shape": "shape mismatch: the product is d x (rows * chunk columns)",
        "COEFF operand": "requires Eval format",
        "output overlaps the digits": "overlap: an output overlaps an operand (row 1)",
        "output overlaps a_lt": "overlap: an output overlaps an operand (row 2)",
        "output overlaps the product": "overlap: an output overlaps the product (row 1)",
    }),
    WEE25: dict(_WEE25),
    WEE25_PRODUCT: dict(_WEE25, **{
        "stacked W shape": "shape mismatch: the stacked W is (blocks * secret_size) x m_b",
        "COEFF stacked W": "requires Eval format",
        "output overlaps the stacked W": "overlap: an output overlaps the stacked W (row 2)",
    }),
}


def _raw(m):
    return None if m is None else m.raw


def _raw_outs(outs):
    return (C.c_void_p * len(outs))(*[None if o is None else o.raw.value for o in outs])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))


def _swap(outs, j, m):
    return outs[:j] + [m] + outs[j + 1:]


def chunk_cases(gpu, oracle):
    """{entry: {case: call}} for the LUT and LWE entries: n16_24, d = 2, c = 2, T = 3, the chunk from column 1"""
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    p = make_params(gpu, oracle, *CONTEXTS["n16_24"])
    M, lib, base = gpu.GpuDCRTPolyMatrix, _ffi.lib(), p.base_bits()
    top, d, c, T = p.crt_depth() - 1, 2, 2, 3
    m = d * p.modulus_digits()
    y_arr, i_arr = np.arange(1, 2 * T + 1, dtype=np.uint64), np.arange(T, dtype=np.uint64)
    tags, keep, _ = hash_tags_arg(KEY, [b"a", b"bb", b"ccc"])
    w = [M(p, d, m, top, True) for _ in range(4)]  # w_identity / a_lt, w_gy / a_z, w_v, w_vx
    lut_prod, lwe_digits, lwe_prod = M(p, 2 * d, T * c, top, True), M(p, m, T * c, top, True), M(p, d, T * c, top, True)
    narrow, coeff = M(p, d, m - 1, top, True), M(p, d, m, top, False)
    parent = M(p, 3 * d, c, top, True)

    def fresh():
        return [M(p, d, c, top, True) for _ in range(T)]

    def over(mat, j):  # a d x c output inside mat's storage, at rows [j d, (j + 1) d) of its d x c blocks
        return mat.reshape_view(mat.nrow * mat.ncol // c, c).row_view(j * d, (j + 1) * d)

    def lut(outs, ops=(), col_start=1, base_bits=base, y=y_arr, wpy=2):
        o = dict(zip(("w_identity", "w_gy", "w_v", "w_vx"), w), **dict(ops))
        return lib.gpupoly_matrix_lut_targets(_raw_outs(outs), T, *[_raw(o[k]) for k in ("w_identity", "w_gy", "w_v", "w_vx")], col_start,
                                              base_bits, _ptr(y), wpy, _ptr(i_arr), C.byref(tags))

    def lut_combine(outs, ops=(), col_start=1, base_bits=base, y=y_arr, wpy=2):
        o = dict(dict(w_identity=w[0], w_gy=w[1], product=lut_prod), **dict(ops))
        return lib.gpupoly_matrix_lut_targets_combine(_raw_outs(outs), T, *[_raw(o[k]) for k in ("w_identity", "w_gy", "product")], col_start,
                                                      base_bits, _ptr(y), wpy, _ptr(i_arr))

    def lwe(outs, ops=(), col_start=1, base_bits=base, y=y_arr, wpy=2):
        o = dict(dict(a_z=w[1], a_lt=w[0]), **dict(ops))
        return lib.gpupoly_matrix_lwe_targets(_raw_outs(outs), T, _raw(o["a_z"]), _raw(o["a_lt"]), col_start, base_bits, _ptr(y), wpy,
                                              _ptr(i_arr), C.byref(tags))

    def lwe_combine(outs, ops=(), col_start=1, base_bits=base, y=y_arr, wpy=2):
        o = dict(dict(a_lt=w[0], digits=lwe_digits, product=lwe_prod), **dict(ops))
        return lib.gpupoly_matrix_lwe_targets_combine(_raw_outs(outs), T, *[_raw(o[k]) for k in ("a_lt", "digits", "product")], col_start,
                                                      base_bits, _ptr(y), wpy, _ptr(i_arr))

    def common(f):
        return {
            "accepted": lambda: f(fresh()),
            "null output in the middle": lambda: f(_swap(fresh(), 1, None)),
            "output of another level, last": lambda: f(_swap(fresh(), 2, M(p, d, c, 0, True))),
            "output of another width": lambda: f(_swap(fresh(), 1, M(p, d, c + 1, top, True))),
            "output rows": lambda: f(_swap(fresh(), 2, M(p, d + 1, c, top, True))),
            "base_bits 63": lambda: f(fresh(), base_bits=63),
            "chunk past the end": lambda: f(fresh(), col_start=m - 1),
            "the same output twice": lambda: (lambda o: f([o[0], o[1], o[0]]))(fresh()),
            "two overlapping row views": lambda: f([parent.row_view(0, d), parent.row_view(d - 1, 2 * d - 1), parent.row_view(2 * d, 3 * d)]),
            "two faults: null y_words, base_bits 0": lambda: f(fresh(), y=None, base_bits=0),
            "two faults: words_per_y 0, null output": lambda: f(_swap(fresh(), 1, None), wpy=0),
            "two faults: chunk past the end, another width": lambda: f(_swap(fresh(), 1, M(p, d, c + 1, top, True)), col_start=m - 1),
        }

    cases = {
        LUT: dict(common(lut), **{
            "W operand shape": lambda: lut(fresh(), {"w_gy": narrow}),
            "COEFF operand": lambda: lut(fresh(), {"w_v": coeff}),
            "output overlaps w_identity": lambda: lut(_swap(fresh(), 1, over(w[0], 0))),
            "output overlaps w_gy": lambda: lut(_swap(fresh(), 2, over(w[1], 1))),
            "output overlaps w_v": lambda: lut(_swap(fresh(), 1, over(w[2], 2))),
            "output overlaps w_vx": lambda: lut(_swap(fresh(), 2, over(w[3], 3))),
        }),
        LUT_COMBINE: dict(common(lut_combine), **{
            "W operand shape": lambda: lut_combine(fresh(), {"w_gy": narrow}),
            "product shape": lambda: lut_combine(fresh(), {"product": lwe_prod}),
            "COEFF operand": lambda: lut_combine(fresh(), {"product": M(p, 2 * d, T * c, top, False)}),
            "output overlaps w_identity": lambda: lut_combine(_swap(fresh(), 1, over(w[0], 0))),
            "output overlaps w_gy": lambda: lut_combine(_swap(fresh(), 2, over(w[1], 1))),
            "output overlaps the product": lambda: lut_combine(_swap(fresh(), 1, over(lut_prod, 2))),
        }),
        LWE: dict(common(lwe), **{
            "A_z shape": lambda: lwe(fresh(), {"a_z": narrow}),
            "A_lt shape": lambda: lwe(fresh(), {"a_lt": M(p, d, m + 1, top, True)}),
            "COEFF operand": lambda: lwe(fresh(), {"a_z": coeff}),
            "output overlaps a_z": lambda: lwe(_swap(fresh(), 1, over(w[1], 0))),
            "output overlaps a_lt": lambda: lwe(_swap(fresh(), 2, over(w[0], 1))),
        }),
        LWE_COMBINE: dict(common(lwe_combine), **{
            "digits shape": lambda: lwe_combine(fresh(), {"digits": lwe_prod}),
            "A_lt shape": lambda: lwe_combine(fresh(), {"a_lt": narrow}),
            "product shape": lambda: lwe_combine(fresh(), {"product": lut_prod}),
            "COEFF operand": lambda: lwe_combine(fresh(), {"digits": M(p, m, T * c, top, False)}),
            "output overlaps the digits": lambda: lwe_combine(_swap(fresh(), 1, over(lwe_digits, 5))),
            "output overlaps a_lt": lambda: lwe_combine(_swap(fresh(), 2, over(w[0], 1))),
            "output overlaps the product": lambda: lwe_combine(_swap(fresh(), 1, over(lwe_prod, 2))),
        }),
    }
    return cases, keep


def wee25_cases(gpu, oracle):
    """{entry: {case: call}} for the Wee25 entries: n16_24, s = 2, T = 2, P = 2 of T_bottom's 4 parts of m_b = 3 columns, from part 1"""
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    p = make_params(gpu, oracle, *CONTEXTS["n16_24"])
    M, lib, base = gpu.GpuDCRTPolyMatrix, _ffi.lib(), p.base_bits()
    top, s, T, NP, m_b, parts = p.crt_depth() - 1, 2, 2, 2, 3, 4
    i_arr = np.array([4, 9], dtype=np.uint64)
    tags, keep, _ = hash_tags_arg(KEY, [b"a", b"bb"])
    t_bottom, w_stacked = M(p, m_b, parts * m_b, top, True), M(p, T * s, m_b, top, True)
    ragged, coeff_tb = M(p, m_b, parts * m_b - 1, top, True), M(p, m_b, parts * m_b, top, False)
    parent = M(p, T * NP * s, m_b, top, True)

    def fresh():
        return [M(p, s, m_b, top, True) for _ in range(T * NP)]

    def over(mat, j):  # an s x m_b output inside mat's storage
        return mat.reshape_view(mat.nrow * mat.ncol // m_b, m_b).row_view(j * s, (j + 1) * s)

    def full(outs, tb=t_bottom, ws=None, part_start=1, secret=s, base_bits=base, idx=i_arr):
        return lib.gpupoly_matrix_wee25_targets(_raw_outs(outs), T, NP, _raw(tb), part_start, secret, base_bits, _ptr(idx), C.byref(tags))

    def product(outs, tb=t_bottom, ws=w_stacked, part_start=1, secret=s, base_bits=base, idx=i_arr):
        return lib.gpupoly_matrix_wee25_targets_product(_raw_outs(outs), T, NP, _raw(ws), _raw(tb), part_start, secret, base_bits, _ptr(idx))

    def views():
        v = [parent.row_view(j * s, (j + 1) * s) for j in range(T * NP)]
        return _swap(v, 1, parent.row_view(s - 1, 2 * s - 1))

    def common(f):
        return {
            "accepted": lambda: f(fresh()),
            "null output in the middle": lambda: f(_swap(fresh(), 1, None)),
            "output of another level, last": lambda: f(_swap(fresh(), 3, M(p, s, m_b, 0, True))),
            "output of another width": lambda: f(_swap(fresh(), 2, M(p, s, m_b - 1, top, True))),
            "T_bottom shape": lambda: f(fresh(), tb=ragged),
            "COEFF T_bottom": lambda: f(fresh(), tb=coeff_tb),
            "base_bits 63": lambda: f(fresh(), base_bits=63),
            "part past the end": lambda: f(fresh(), part_start=parts - 1),
            "output overlaps T_bottom": lambda: f(_swap(fresh(), 3, over(t_bottom, 1))),
            "the same output twice": lambda: (lambda o: f(_swap(o, 3, o[0])))(fresh()),
            "two overlapping row views": lambda: f(views()),
            "two faults: null idx, base_bits 0": lambda: f(fresh(), idx=None, base_bits=0),
            "two faults: secret_size 0, null output": lambda: f(_swap(fresh(), 1, None), secret=0),
            "two faults: part past the end, COEFF T_bottom": lambda: f(fresh(), tb=coeff_tb, part_start=parts - 1),
        }

    cases = {
        WEE25: common(full),
        WEE25_PRODUCT: dict(common(product), **{
            "stacked W shape": lambda: product(fresh(), ws=M(p, T * s + 1, m_b, top, True)),
            "COEFF stacked W": lambda: product(fresh(), ws=M(p, T * s, m_b, top, False)),
            "output overlaps the stacked W": lambda: product(_swap(fresh(), 2, over(w_stacked, 1))),
        }),
    }
    return cases, keep


def collect(gpu, cases):
    """{entry: {case: what the call left in last_error_string()}}; every call but "accepted" is refused and launches nothing"""
    from mxx_amd import _ffi

    lib, got = _ffi.lib(), {}
    for entry, calls in cases.items():
        assert calls["accepted"]() == 0, (entry, _ffi.last_error_string())
        got[entry] = {}
        for name, fn in calls.items():
            if name == "accepted":
                continue
            gpu.gpu_device_sync()
            c0 = lib.gpupoly_launch_count()
            _ffi.trace_begin()
            rc = fn()
            msg = _ffi.last_error_string()
            trace = _ffi.trace_end()
            assert rc != 0, (entry, name)
            assert trace == [] and lib.gpupoly_launch_count() == c0, (entry, name, trace)
            got[entry][name] = msg
    return got


@pytest.mark.parametrize("family", ["chunk", "wee25"])
def test_every_refusal_has_its_whole_text(gpu, oracle, family):
    cases, keep = (chunk_cases if family == "chunk" else wee25_cases)(gpu, oracle)
    got = collect(gpu, cases)
    for entry, calls in got.items():
        assert set(calls) == set(EXPECTED[entry]), entry
        for name, msg in calls.items():
            assert msg == entry + ": " + EXPECTED[entry][name], (entry, name)
    del keep


def test_the_combine_kernels_keep_their_trace_labels(gpu, oracle):
    """A launch is traced under the text of its kernel argument, and a trace tells the digit-count instances of a combine
    kernel apart by the literal digit count in it (n16_24 at base 2^12: 2 digits per tower).  Recorded from the library
    as it was before the launcher was shared."""
    from mxx_amd import _ffi

    cases, keep = chunk_cases(gpu, oracle)
    for entry, label in ((LUT, "lut_combine_kernel<W, VN, 2>"), (LUT_COMBINE, "lut_combine_kernel<W, VN, 2>"),
                         (LWE, "lwe_combine_kernel<W, VN, 2>"), (LWE_COMBINE, "lwe_combine_kernel<W, VN, 2>")):
        gpu.gpu_device_sync()
        _ffi.trace_begin()
        assert cases[entry]["accepted"]() == 0, entry
        names = [e["kernel"] for e in _ffi.trace_end()]
        assert names.count(label) == 1 and names[-1] == label, (entry, names)
    del keep
