"""gpupoly_matrix_fill_monomial / _mul_monomial / _monomial_sum: out = addend +- sum_j mats[j] * x^shifts[j] on the device.

The CPU reference lives here: in COEFF the signed rotation rule in exact integers (coefficient i receives +a[m] when
m = (i - s) mod 2N < N, else -a[m - N]); in EVAL the oracle's transform of the rotated coefficients, and - independently of
the oracle - plainref.ntt_slots on a handful of slots.  Bit-exact; also against the existing entry points (fill, mul_scalar,
add per term), with inputs untouched, every refusal leaving the output and the launch counter alone, and ceil(n / 64)
launches per call."""
import ctypes as C

import numpy as np
import pytest

import plainref as P

pytestmark = pytest.mark.gpu

# (n, limbs, bits): the two smallest rings (no 16-byte vector of coefficients at n = 2; logN = 1 is the smallest
# bit-reversal), a small 3-limb ring, 64-bit words with the double-precision-transform context class, lazy_terms = 4
# (31 bits) and = 64 (61 bits), and the ring of the vector paths
RINGS = {
    "n2_18bit": (2, 2, 18),
    "n4_18bit": (4, 2, 18),
    "n16_18bit": (16, 3, 18),
    "n256_51bit": (256, 3, 51),
    "n256_31bit": (256, 2, 31),
    "n256_61bit": (256, 2, 61),
    "n16384_24bit": (16384, 2, 24),
}
POOL = 5  # distinct operand matrices of a pool; longer term lists cycle through them with their own shifts

_params, _pools = {}, {}


def params(gpu, ring):
    if ring not in _params:
        n, L, bits = RINGS[ring]
        _params[ring] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, L), 1)
    return _params[ring]


def shift_set(n):
    return [0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, (1 << 63) + 5]


def term_shifts(n, count):
    """`count` shifts: the edge set first, one of them repeated, then odd and even ones spread over [0, 2N) - at
    n = 16384 most are no multiple of 4"""
    base = shift_set(n) + [1]
    return [base[j] if j < len(base) else (j * 2654435761 + 3) % (2 * n) for j in range(count)]


# ---------------------------------------------------------------------------------------------- CPU reference
def qcol(moduli):
    return np.array([int(q) for q in moduli], dtype=np.uint64).reshape(-1, 1)


def rotate(a, s, moduli):
    """a * x^s on coefficient residues (..., L, n), by the signed rotation rule"""
    n = a.shape[-1]
    m = (np.arange(n) - (int(s) % (2 * n))) % (2 * n)
    r = a[..., m % n]
    q = qcol(moduli)
    return np.where(m >= n, (q - r) % q, r)


def sum_coeff(mats, shifts, addend, negate, moduli):
    """addend +- sum_j mats[j] x^shifts[j] on coefficient residues, reduced after every term (all values below q < 2^62)"""
    q = qcol(moduli)
    acc = np.zeros_like(mats[0]) if addend is None else addend.copy()
    for a, s in zip(mats, shifts):
        r = rotate(a, s, moduli)
        acc = (acc + (q - r) % q) % q if negate else (acc + r) % q
    return acc


def pool(gpu, oracle, ring, shape, level=None):
    """coefficient-domain operands of one (ring, shape): POOL matrices and an addend, with their transforms and device
    handles in both domains; computed once and never written"""
    key = (ring, shape, level)
    if key not in _pools:
        p = params(gpu, ring)
        n, L, _ = RINGS[ring]
        L = L if level is None else level + 1
        moduli = p.moduli()[:L]
        seed = 7000 + 13 * len(_pools)
        coeff = [oracle.random_matrix(seed + j, shape[0], shape[1], moduli, n) for j in range(POOL + 1)]
        evals = [oracle.matrix_ntt(c, moduli) for c in coeff]
        for a in coeff + evals:
            a.setflags(write=False)
        M = gpu.GpuDCRTPolyMatrix
        dev = {False: [M.from_rns(p, c, False) for c in coeff], True: [M.from_rns(p, e, True) for e in evals]}
        _pools[key] = dict(p=p, n=n, moduli=moduli, coeff=coeff, evals=evals, dev=dev)
    return _pools[key]


def expected(oracle, S, idx, shifts, addend, negate, ev):
    e = sum_coeff([S["coeff"][i] for i in idx], shifts, S["coeff"][POOL] if addend else None, negate, S["moduli"])
    return oracle.matrix_ntt(e, S["moduli"]) if ev else e


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value)


def launches():
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_launch_count()


def run(gpu, oracle, S, ev, count, addend_mode, negate, shifts=None):
    """one monomial_sum on pool operands against the reference; addend_mode: none / fresh / inplace"""
    M = gpu.GpuDCRTPolyMatrix
    idx = [j % POOL for j in range(count)]
    shifts = term_shifts(S["n"], count) if shifts is None else shifts
    mats = [S["dev"][ev][i] for i in idx]
    if addend_mode == "none":
        got = M.monomial_sum(mats, shifts, negate=negate)
    elif addend_mode == "fresh":
        got = M.monomial_sum(mats, shifts, addend=S["dev"][ev][POOL], negate=negate)
    else:
        acc = S["dev"][ev][POOL].clone()
        got = M.monomial_sum(mats, shifts, addend=acc, negate=negate, out=acc)
        assert got is acc
    want = expected(oracle, S, idx, shifts, addend_mode != "none", negate, ev)
    assert got.is_ntt == ev
    assert np.array_equal(got.to_rns(), want), f"count={count} addend={addend_mode} negate={negate} eval={ev}"


# ---------------------------------------------------------------------------------------------- results
@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_every_edge_shift_alone_and_summed(gpu, oracle, ring, ev):
    S = pool(gpu, oracle, ring, (3, 3))
    n, moduli = S["n"], S["moduli"]
    src = S["dev"][ev][0]
    for s in shift_set(n):
        want = rotate(S["coeff"][0], s, moduli)
        got = src.mul_monomial(s)
        assert got.is_ntt == ev
        assert np.array_equal(got.to_rns(), oracle.matrix_ntt(want, moduli) if ev else want), f"shift {s}"
    run(gpu, oracle, S, ev, 9, "fresh", False)  # the eight edge shifts and a repeated one in one call
    assert raw_same(src, gpu.GpuDCRTPolyMatrix.from_rns(S["p"], (S["evals"] if ev else S["coeff"])[0], ev)), "operand changed"


@pytest.mark.parametrize("count", [1, 2, 64, 65])
@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_term_counts_with_every_addend_form_and_sign(gpu, oracle, ring, ev, count):
    S = pool(gpu, oracle, ring, (3, 3))
    for negate in (False, True):
        for addend_mode in ("none", "fresh", "inplace"):
            run(gpu, oracle, S, ev, count, addend_mode, negate)


# polynomial-tile edges (1, 9 and 17 polynomials against tiles of 4), and the shapes large enough for the tiled EVAL
# kernels to be chosen: 65 polynomials at n = 16384 (16-byte loads), 37 x 37 at n = 256 with 64-bit words, and 131073
# polynomials at n = 2 (one slot per lane); each ends in a tile with a single live polynomial
@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
@pytest.mark.parametrize("ring,shape", [
    ("n16_18bit", (1, 1)), ("n16_18bit", (1, 17)), ("n256_51bit", (1, 1)), ("n256_51bit", (1, 17)),
    ("n16384_24bit", (1, 1)), ("n16384_24bit", (1, 17)), ("n16384_24bit", (1, 65)), ("n256_51bit", (37, 37)),
    ("n2_18bit", (1, 131073)),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_shapes_and_polynomial_tiles(gpu, oracle, ring, shape, ev):
    S = pool(gpu, oracle, ring, shape)
    run(gpu, oracle, S, ev, 3, "fresh", True)
    run(gpu, oracle, S, ev, 5, "none", False)


@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
def test_aligned_coeff_shifts_take_the_vector_path(gpu, oracle, ev):
    """every shift a multiple of 4 (both signs, a wrap across N); in EVAL the same call for comparison"""
    S = pool(gpu, oracle, "n16384_24bit", (3, 3))
    n = S["n"]
    run(gpu, oracle, S, ev, 6, "fresh", False, shifts=[0, 4, n - 4, n, n + 8, 2 * n - 4])
    S64 = pool(gpu, oracle, "n256_51bit", (3, 3))
    run(gpu, oracle, S64, ev, 5, "inplace", True, shifts=[2, 254, 256, 258, 510])


@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
def test_level_0_of_a_three_limb_context(gpu, oracle, ev):
    S = pool(gpu, oracle, "n16_18bit", (3, 3), level=0)
    assert S["dev"][ev][0].level == 0 and S["p"].crt_depth() == 3
    run(gpu, oracle, S, ev, 9, "fresh", False)
    run(gpu, oracle, S, ev, 2, "none", True)


def test_empty_operands_and_zero_terms(gpu, oracle):
    M = gpu.GpuDCRTPolyMatrix
    S = pool(gpu, oracle, "n16_18bit", (3, 3))
    p = S["p"]
    top = p.crt_depth() - 1
    gpu.gpu_device_sync()
    c0 = launches()
    empty = [M(p, 0, 3, top, True) for _ in range(2)]
    out = M.monomial_sum(empty, [1, 2], addend=M(p, 0, 3, top, True))
    assert out.size() == (0, 3) and out.is_ntt
    assert M(p, 0, 3, top, False).mul_monomial(3).size() == (0, 3)
    assert launches() == c0, "an empty operand launched a kernel"
    for ev in (False, True):
        # no terms, an addend: its residues and its tag
        out = M.from_rns(p, S["coeff" if ev else "evals"][1], not ev)
        got = M.monomial_sum([], [], addend=S["dev"][ev][POOL], out=out)
        assert got.is_ntt == ev and raw_same(got, S["dev"][ev][POOL])
        # no terms, no addend: zeros under the tag the output had
        out = M.from_rns(p, S["coeff"][1], ev)
        got = M.monomial_sum([], [], out=out)
        assert got.is_ntt == ev and not got.to_rns().any()
        assert raw_same(got, M._new_zero_with_state(p, 3, 3, top, ev))


@pytest.mark.parametrize("count", [5, 64, 65])
@pytest.mark.parametrize("ring", ["n256_31bit", "n256_61bit"])
def test_worst_case_for_the_lazy_accumulators(gpu, oracle, ring, count):
    """every residue q - 1 and every shift N: every EVAL factor is q - 1, every product (q - 1)^2 = 1 (mod q)"""
    M = gpu.GpuDCRTPolyMatrix
    p = params(gpu, ring)
    n, L, _ = RINGS[ring]
    moduli = p.moduli()
    top = np.empty((3, 3, L, n), dtype=np.uint64)
    top[:] = (qcol(moduli) - np.uint64(1))
    q = qcol(moduli)
    plus = (top + np.uint64(count % int(min(moduli)))) % q  # addend + J (mod q), addend = q - 1
    for ev in (False, True):
        m, add = M.from_rns(p, top, ev), M.from_rns(p, top, ev)
        got = M.monomial_sum([m] * count, [n] * count, addend=add)
        assert np.array_equal(got.to_rns(), plus), f"eval={ev}"
        if not ev:  # the rotation rule's value for the COEFF form
            assert np.array_equal(sum_coeff([top] * count, [n] * count, top, False, moduli), plus)
        got = M.monomial_sum([m] * count, [n] * count, addend=add, negate=True, out=add)
        assert np.array_equal(got.to_rns(), (top + q - np.uint64(count)) % q), f"eval={ev} negated in place"
        got = M.monomial_sum([m] * count, [n] * count)
        assert np.array_equal(got.to_rns(), np.broadcast_to(np.uint64(count), top.shape)), f"eval={ev} no addend"


@pytest.mark.parametrize("ring", ["n16_18bit", "n256_51bit", "n16384_24bit"])
def test_eval_slots_against_the_plain_reference(gpu, oracle, ring):
    S = pool(gpu, oracle, ring, (3, 3))
    n, moduli = S["n"], S["moduli"]
    slots = sorted({0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1} & set(range(n)))
    shifts = [1, n + 3, (1 << 63) + 5]
    got = gpu.GpuDCRTPolyMatrix.monomial_sum([S["dev"][True][j] for j in range(3)], shifts, addend=S["dev"][True][POOL]).to_rns()
    want = sum_coeff([S["coeff"][j] for j in range(3)], shifts, S["coeff"][POOL], False, moduli)
    roots = [P.min_root(int(q), n) for q in moduli]
    for r, c in ((0, 0), (2, 1)):
        assert np.array_equal(got[r, c][:, slots], P.ntt_slots(want[r, c], moduli, slots, roots)), f"entry ({r}, {c})"
    filled = gpu.GpuDCRTPolyMatrix.monomial(S["p"], 1, 1, n + 3, True).to_rns()[0, 0]
    one_hot = np.zeros((len(moduli), n), dtype=np.uint64)
    one_hot[:, 3] = [int(q) - 1 for q in moduli]
    assert np.array_equal(filled[:, slots], P.ntt_slots(one_hot, moduli, slots, roots))


# ---------------------------------------------------------------------------------------------- algebra, existing entries
@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
@pytest.mark.parametrize("ring", ["n2_18bit", "n16_18bit", "n256_61bit", "n16384_24bit"])
def test_algebraic_identities(gpu, oracle, ring, ev):
    M = gpu.GpuDCRTPolyMatrix
    S = pool(gpu, oracle, ring, (3, 3))
    n, src = S["n"], S["dev"][ev][2]
    for s in (1, n - 1, n + 5 if n > 5 else n + 1):
        zero = M.monomial_sum([src, src], [s, s + n])
        assert not zero.to_rns().any(), f"x^{s} + x^{s + n} != 0"
        assert raw_same(src.mul_monomial(s).mul_monomial(2 * n - s), src), f"round trip over shift {s}"


@pytest.mark.parametrize("ring", ["n4_18bit", "n256_51bit", "n256_31bit", "n16384_24bit"])
def test_agreement_with_the_existing_entry_points(gpu, oracle, ring):
    M = gpu.GpuDCRTPolyMatrix
    S = pool(gpu, oracle, ring, (3, 3))
    p, n = S["p"], S["n"]
    mats = S["dev"][True][:3]
    for s in shift_set(n):
        mono = M.monomial(p, 1, 1, s, True)
        assert raw_same(mats[0].mul_scalar(mono), mats[0].mul_monomial(s)), f"mul_scalar by fill_monomial({s})"
        coeff_form = M.monomial(p, 1, 1, s, False)
        assert not coeff_form.is_ntt
        coeff_form.ntt_all_in_place()
        assert raw_same(mono, coeff_form), f"fill_monomial({s}): EVAL against the transform of COEFF"
        assert raw_same(gpu.GpuDCRTPoly.const_rotate_poly(p, s).inner, mono)
    # what a caller runs today: per term a one-hot upload, mul_scalar and +
    shifts = [0, 1, n - 1]
    acc = S["dev"][True][POOL]
    for m, s in zip(mats, shifts):
        acc = acc + m.mul_scalar(gpu.GpuDCRTPoly.from_u32s(p, [0] * s + [1]))
    assert raw_same(acc, M.monomial_sum(mats, shifts, addend=S["dev"][True][POOL]))
    sub = S["dev"][True][POOL]
    for m, s in zip(mats, shifts):
        sub = sub - m.mul_scalar(M.monomial(p, 1, 1, s + n + 1, True))
    assert raw_same(sub, M.monomial_sum(mats, [s + n + 1 for s in shifts], addend=S["dev"][True][POOL], negate=True))


def test_inputs_stay_as_they_were_and_a_packed_sample_gives_the_words_result(gpu, oracle):
    M = gpu.GpuDCRTPolyMatrix
    S = pool(gpu, oracle, "n16384_24bit", (3, 3))
    p, moduli = S["p"], S["moduli"]
    for ev in (False, True):
        mats, add = S["dev"][ev][:3], S["dev"][ev][POOL]
        M.monomial_sum(mats, [3, 5, 16390], addend=add, negate=True)
        host = S["evals"] if ev else S["coeff"]
        for j, m in enumerate(mats + [add]):
            assert m.is_ntt == ev and np.array_equal(m.to_rns(), host[j if j < 3 else POOL])
    sample = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, 2, gpu.DistType.FinRingDist())
    assert sample.layout == "packed24"
    ev = sample.is_ntt
    got = M.monomial_sum([sample, sample], [7, 16384 + 2], negate=True)
    res = sample.to_rns()
    coeff_res = oracle.matrix_ntt(res, moduli, inverse=True) if ev else res
    want = sum_coeff([coeff_res, coeff_res], [7, 16384 + 2], None, True, moduli)
    assert got.is_ntt == ev and np.array_equal(got.to_rns(), oracle.matrix_ntt(want, moduli) if ev else want)
    assert sample.is_ntt == ev and np.array_equal(sample.to_rns(), res)


# ---------------------------------------------------------------------------------------------- refusals, launches
REFUSALS = ["null_out", "null_mats", "null_shifts", "null_mat_1", "second_context", "level_mismatch", "shape_mismatch",
            "mixed_formats_among_mats", "addend_of_the_other_format", "out_is_mat_1", "out_row_view_overlaps_mat_1",
            "addend_row_view_shifted_against_out", "mul_monomial_in_place", "fill_monomial_bad_format"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing_and_leave_the_output_as_it_was(gpu, oracle, case):
    from mxx_amd import _ffi

    lib = _ffi.lib()
    M = gpu.GpuDCRTPolyMatrix
    ring = "n16_18bit"
    S = pool(gpu, oracle, ring, (2, 3))
    p, n, moduli = S["p"], S["n"], S["moduli"]
    mats = [S["dev"][True][j] for j in range(3)]
    addend = S["dev"][True][POOL]
    out = M.from_rns(p, S["coeff"][4], False)  # known residues under the COEFF tag: a refused call leaves both
    who = "gpupoly_matrix_monomial_sum"
    keep = []
    if case == "second_context":
        p2 = gpu.GpuDCRTPolyParams(n, p.moduli(), 1, dnum=9)
        assert p2.ctx_raw().value != p.ctx_raw().value
        mats[2] = M.from_rns(p2, S["evals"][2], True)
    elif case == "level_mismatch":
        mats[1] = M.from_rns(p, S["evals"][1][:, :, :2], True)
    elif case == "shape_mismatch":
        mats[2] = M.from_rns(p, S["evals"][2][:1], True)
    elif case == "mixed_formats_among_mats":
        mats[2] = S["dev"][False][2]
    elif case == "addend_of_the_other_format":
        addend = S["dev"][False][POOL]
    elif case == "out_is_mat_1":
        out = M.from_rns(p, S["evals"][4], True)
        mats[1] = out
    elif case in ("out_row_view_overlaps_mat_1", "addend_row_view_shifted_against_out"):
        parent = M.from_rns(p, np.concatenate([S["evals"][3], S["evals"][4]]), True)  # 4 x 3
        keep.append(parent)
        out = parent.row_view(0, 2)
        if case == "out_row_view_overlaps_mat_1":
            mats[1] = parent.row_view(1, 3)
        else:
            addend = parent.row_view(1, 3)
    before = out.clone()
    arr = (C.c_void_p * 3)(*[m.raw.value for m in mats])
    shifts = (C.c_uint64 * 3)(1, n, 5)
    gpu.gpu_device_sync()
    c0 = launches()
    if case == "null_out":
        rc = lib.gpupoly_matrix_monomial_sum(None, addend.raw, arr, shifts, 3, 0)
    elif case == "null_mats":
        rc = lib.gpupoly_matrix_monomial_sum(out.raw, addend.raw, None, shifts, 3, 0)
    elif case == "null_shifts":
        rc = lib.gpupoly_matrix_monomial_sum(out.raw, addend.raw, arr, None, 3, 0)
    elif case == "null_mat_1":
        arr[1] = None
        rc = lib.gpupoly_matrix_monomial_sum(out.raw, addend.raw, arr, shifts, 3, 0)
    elif case == "mul_monomial_in_place":
        who = "gpupoly_matrix_mul_monomial"
        rc = lib.gpupoly_matrix_mul_monomial(out.raw, out.raw, 3)
    elif case == "fill_monomial_bad_format":
        who = "gpupoly_matrix_fill_monomial"
        rc = lib.gpupoly_matrix_fill_monomial(out.raw, 3, 2)
    else:
        rc = lib.gpupoly_matrix_monomial_sum(out.raw, addend.raw, arr, shifts, 3, 1)
    assert launches() == c0, "a refused call launched a kernel"
    assert rc != 0 and who in _ffi.last_error_string(), _ffi.last_error_string()
    assert raw_same(out, before), f"{case}: the output changed (residues or tag)"


@pytest.mark.parametrize("ev", [False, True], ids=["coeff", "eval"])
def test_a_call_issues_one_launch_per_64_terms(gpu, oracle, ev):
    M = gpu.GpuDCRTPolyMatrix
    S = pool(gpu, oracle, "n256_51bit", (3, 3))
    for count, want in ((2, 1), (64, 1), (65, 2)):
        mats = [S["dev"][ev][j % POOL] for j in range(count)]
        shifts = term_shifts(S["n"], count)
        out = M(S["p"], 3, 3, S["p"].crt_depth() - 1, ev)
        assert out.layout == "words" and all(m.layout == "words" for m in mats)
        c0 = launches()
        M.monomial_sum(mats, shifts, addend=S["dev"][ev][POOL], out=out)
        assert launches() - c0 == want, f"{count} terms"
