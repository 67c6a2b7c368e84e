"""gpupoly_matrix_mul_decompose_gadget_scalar_many / _const_many: the LargeScalarMul gate without G or its digit matrix.

    outs[j] = addends[j] +- lhss[j] * G^-1(G_dj o c)

Every case is held, bit for bit, to (1) the CPU restatement - oracle.matmul(lhs, matrix_ntt(decompose(matrix_ntt(G o c,
inverse)))), exact integer add / sub mod q on the host; (2) the existing device sequence - gpu_matrix_fill_gadget,
gpu_matrix_mul_scalar, gpupoly_matrix_mul_decompose, gpu_matrix_add / _sub / gpupoly_matrix_neg - through gpu_matrix_equal
(residues and tag); (3) the Python-integer model of tests/gadget_scalar_model.py (every word for a constant, a handful of
entries for a ring element).  Inputs are compared with their uploads afterwards.  Every axis is covered against one default
of the others (d = 2, rows 2, one operand, no addend)."""
import ctypes as C

import numpy as np
import pytest

import gadget_scalar_model as GM
from conftest import make_params

pytestmark = pytest.mark.gpu

SM, CM = "gpupoly_matrix_mul_decompose_gadget_scalar_many", "gpupoly_matrix_mul_decompose_gadget_const_many"
# (n, limbs, limb bits, base bits): the scalar-access path with dpt 3; the default small ring; a base that does not divide;
# dpt 5 (the loop path and its reduce-every-4 bound); 64-bit words; dpt 4 at the widest words of each class (the 4-product
# lazy bound); the 16-byte path with several chunks and 2^14 transforms of the table
RINGS = {"n2_18bit": (2, 2, 18, 6), "n16_18bit": (16, 3, 18, 6), "n16_18bit_base7": (16, 3, 18, 7), "n16_18bit_base4": (16, 3, 18, 4),
         "n256_51bit": (256, 3, 51, 17), "n256_61bit": (256, 2, 61, 20), "n256_31bit": (256, 2, 31, 8), "n16384_24bit": (16384, 2, 24, 12)}
AXES = ["n16_18bit", "n256_51bit", "n16384_24bit"]  # the rings every axis runs on: u32 small, u64, u32 16-byte path
DMAX, RMAX = 3, 5
D_D, D_R = 2, 2  # the defaults

_pool = {}


def pool(gpu, oracle, ring, limbs=None):
    """Host inputs of one ring, made once and never written."""
    key = (ring, limbs)
    if key not in _pool:
        n, depth, bits, base = RINGS[ring]
        p = make_params(gpu, oracle, n, depth, bits, base)
        moduli = p.moduli()[: limbs or depth]
        L = len(moduli)
        dpt = -(-p.crt_bits() // base)
        k = dpt * L
        Q = 1
        for m in moduli:
            Q *= int(m)
        P = dict(p=p, moduli=moduli, n=n, L=L, base=base, dpt=dpt, k=k, Q=Q, oracle=oracle, DEC={},
                 SL=oracle.random_matrix(910, RMAX, DMAX * k, moduli, n), SC=oracle.random_matrix(911, 1, 1, moduli, n),
                 AD=oracle.random_matrix(912, RMAX, DMAX * k, moduli, n), SENT=oracle.random_matrix(913, RMAX, DMAX * k, moduli, n))
        P["SC_COEFF"] = oracle.matrix_ntt(P["SC"], moduli, inverse=True)
        P["TOP"] = np.broadcast_to(qcol(P) - 1, (1, 1, L, n)).astype(np.uint64)
        for name in ("SL", "SC", "SC_COEFF", "TOP", "AD", "SENT"):
            P[name].setflags(write=False)
        _pool[key] = P
    return _pool[key]


def qcol(P):
    return np.array([int(m) for m in P["moduli"]], dtype=np.uint64).reshape(1, 1, -1, 1)


def constants(P):
    """0, 1, Q - 1 and a three-word value above Q"""
    big = (1 << 190) + 0x9E3779B97F4A7C15
    assert big > P["Q"]
    return {"zero": 0, "one": 1, "Q_minus_1": P["Q"] - 1, "three_words": big}


def dev(gpu, P, data, eval_format=True):
    """upload; shapes without entries come from the constructor"""
    M = gpu.GpuDCRTPolyMatrix
    if data.shape[0] == 0 or data.shape[1] == 0:
        return M(P["p"], data.shape[0], data.shape[1], P["L"] - 1, eval_format)
    return M.from_rns(P["p"], np.ascontiguousarray(data), eval_format)


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag (a tag mismatch is 'not equal' there)"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value) or a.nrow * a.ncol == 0


def launches():
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_launch_count()


def _arr(ms):
    if ms is None:
        return None
    return (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])


def int_words(value):
    wpc = max(1, -(-int(value).bit_length() // 64))
    return (C.c_uint64 * wpc)(*[(int(value) >> (64 * i)) & (2**64 - 1) for i in range(wpc)]), wpc


def raw_call(outs, lhss, addends, scalar, negate, base):
    """scalar: a device matrix (the ring-element entry) or an int (the constant entry); returns rc"""
    from mxx_amd import _ffi

    n = len(lhss)
    if isinstance(scalar, int):
        words, wpc = int_words(scalar)
        return _ffi.lib().gpupoly_matrix_mul_decompose_gadget_const_many(_arr(outs), _arr(lhss), _arr(addends), n, words, wpc, 1 if negate else 0, base)
    return _ffi.lib().gpupoly_matrix_mul_decompose_gadget_scalar_many(_arr(outs), _arr(lhss), _arr(addends), n, None if scalar is None else scalar.raw,
                                                                      1 if negate else 0, base)


def host_dec(P, c_key, c_eval, d):
    """NTT(G^-1(G_d o c)) on the CPU restatement, cached per (scalar, d)"""
    if (c_key, d) not in P["DEC"]:
        o, moduli = P["oracle"], P["moduli"]
        gc = o.pointwise("mul", o.gadget_matrix(d, moduli, P["n"], P["base"]), c_eval, moduli)
        dec = o.matrix_ntt(o.decompose(o.matrix_ntt(gc, moduli, inverse=True), moduli, P["base"]), moduli)
        dec.setflags(write=False)
        P["DEC"][(c_key, d)] = dec
    return P["DEC"][(c_key, d)]


def run(gpu, oracle, ring, scalar="eval", ops=((D_R, D_D),), addend="none", negate=False, limbs=None, lhs_worst=False, model=True):
    """One call against the CPU restatement, the device sequence and the integer model.  scalar: "eval", "coeff" (the same
    ring element tagged COEFF), "top" (all residues q - 1) or ("const", name).  ops: (rows, d) per operand.  addend: "none",
    "separate", "out" (the out block itself) or "mixed" (by operand: none, separate, out, ...).  Returns the launch count."""
    from mxx_amd import _ffi

    P = pool(gpu, oracle, ring, limbs)
    q, k, n, moduli = qcol(P), P["k"], P["n"], P["moduli"]
    if isinstance(scalar, tuple):
        Cst = constants(P)[scalar[1]]
        c_eval, sc = GM.const_eval(Cst, moduli, n), Cst
    else:
        Cst = None
        c_eval = P["TOP"] if scalar == "top" else P["SC"]
        sc = dev(gpu, P, P["SC_COEFF"], False) if scalar == "coeff" else dev(gpu, P, c_eval)
    c_key = scalar if scalar != "coeff" else "eval"
    sc_seq = dev(gpu, P, c_eval)  # the sequence's scalar: EVAL, as gpu_matrix_mul_scalar wants it
    lhss, outs, adds, wants, seqs, inputs, hosts = [], [], [], [], [], [], []
    for j, (rows, d) in enumerate(ops):
        cols = d * k
        take = lambda a: np.roll(a, j, axis=0)[:rows, :cols] if j else a[:rows, :cols]  # noqa: E731
        lhs_host = np.broadcast_to(q - 1, (rows, cols, P["L"], n)).astype(np.uint64) if lhs_worst else take(P["SL"])
        mode = ("none", "separate", "out")[j % 3] if addend == "mixed" else addend
        add_host = None if mode == "none" else take(P["AD"])
        # (1) the CPU restatement
        if rows and cols:
            prod = oracle.matmul(lhs_host, host_dec(P, c_key, c_eval, d), moduli)
            if add_host is None:
                want = (q - prod) % q if negate else prod
            else:
                want = (add_host + (q - prod)) % q if negate else (add_host + prod) % q
        else:
            want = np.zeros((rows, cols, P["L"], n), dtype=np.uint64)
        lhs = dev(gpu, P, lhs_host)
        if mode == "out":
            out = dev(gpu, P, add_host)
            add = out
        else:
            out = dev(gpu, P, take(P["SENT"]), False)  # known residues under the other tag: the call must write both
            add = None if add_host is None else dev(gpu, P, add_host)
        # (2) the existing device sequence
        seq = None
        if rows and cols:
            pd = lhs._large_scalar_mul_host(sc_seq)
            if add is None:
                seq = -pd if negate else pd
            else:
                seq = add - pd if negate else add + pd
        lhss.append(lhs), outs.append(out), adds.append(add), wants.append(want), seqs.append(seq), hosts.append((lhs_host, add_host))
        inputs += [lhs] + ([add] if mode == "separate" else [])
    if not isinstance(sc, int):
        inputs.append(sc)
    before = [m.clone() for m in inputs]
    assert all(m.layout == "words" for m in inputs + outs)

    gpu.gpu_device_sync()
    c0 = launches()
    rc = raw_call(outs, lhss, adds if any(a is not None for a in adds) else None, sc, negate, P["base"])
    count = launches() - c0
    assert rc == 0, _ffi.last_error_string()
    if isinstance(sc, int):
        nonempty = sum(1 for rows, d in ops if rows and d)
        assert count == -(-nonempty // 64), f"{count} launches for {nonempty} operands with entries"
    elif not any(rows and d for rows, d in ops):
        assert count == 0, f"{count} launches for empty shapes"
    modelled = False
    for j, (rows, d) in enumerate(ops):
        out = outs[j]
        out.is_ntt = True  # the mirror's tag follows the library's: raw_same below compares the library's
        assert out.size() == (rows, d * k)
        if not (rows and d):
            continue
        got = out.to_rns()
        assert np.array_equal(got, wants[j]), f"operand {j}: against the CPU restatement"
        assert raw_same(out, seqs[j]), f"operand {j}: against the sequence of existing entry points (residues and tag)"
        # (3) exact integers, independent of oracle/ and of the kernels: the first operand with entries
        if model and not modelled:
            modelled = True
            lhs_host, add_host = hosts[j]
            sign = -1 if negate else 1
            if Cst is not None:
                pm = GM.mul_const(lhs_host, Cst, moduli, P["base"], P["dpt"]).astype(object)
                a = 0 if add_host is None else add_host.astype(object)
                assert np.array_equal(((a + sign * pm) % q.astype(object)).astype(np.uint64), got), "against the integer model"
            else:
                c_coeff = oracle.matrix_ntt(c_eval, moduli, inverse=True)[0, 0]
                entries = sorted({(0, 0), (rows - 1, d * k - 1)} | ({(rows // 2, (d * k) // 2)} if n <= 256 else set()))
                slots = sorted({0, n - 1, n // 2})
                for (i, col, l), vals in GM.mul_scalar_entries(lhs_host, c_coeff, moduli, P["base"], P["dpt"], entries, slots).items():
                    ql = int(moduli[l])
                    for s, v in zip(slots, vals):
                        a = 0 if add_host is None else int(add_host[i, col, l, s])
                        assert int(got[i, col, l, s]) == (a + sign * v) % ql, (i, col, l, s)
    for j, (m, b) in enumerate(zip(inputs, before)):
        assert raw_same(m, b), f"input {j} changed"
    return count


SCALARS = ["eval", "coeff", "top", ("const", "zero"), ("const", "one"), ("const", "Q_minus_1"), ("const", "three_words")]
SCALAR_IDS = ["eval", "coeff", "top", "c0", "c1", "cQ-1", "c3words"]
BOTH = ["eval", ("const", "three_words")]
BOTH_IDS = ["ring", "const"]


@pytest.mark.parametrize("scalar", SCALARS, ids=SCALAR_IDS)
@pytest.mark.parametrize("ring", list(RINGS))
def test_every_scalar_on_every_ring(gpu, oracle, ring, scalar):
    run(gpu, oracle, ring, scalar=scalar, addend="separate", negate=True)


@pytest.mark.parametrize("scalar", BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize("ring", list(RINGS))
def test_lhs_all_q_minus_1(gpu, oracle, ring, scalar):
    """with the scalar at q - 1 too for the ring element: the lazy sums at their bound"""
    run(gpu, oracle, ring, scalar="top" if scalar == "eval" else ("const", "Q_minus_1"), lhs_worst=True)
    run(gpu, oracle, ring, scalar=scalar, lhs_worst=True, addend="out", negate=True)


@pytest.mark.parametrize("scalar", BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize("rows", [0, 1, 5])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("ring", AXES)
def test_shapes(gpu, oracle, ring, d, rows, scalar):
    run(gpu, oracle, ring, scalar=scalar, ops=((rows, d),), model=(d, rows) == (3, 5))


@pytest.mark.parametrize("scalar", BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize("negate", [False, True], ids=["plus", "minus"])
@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("ring", AXES)
def test_addend_and_sign(gpu, oracle, ring, addend, negate, scalar):
    run(gpu, oracle, ring, scalar=scalar, addend=addend, negate=negate)


MIXED = [(1, 1), (2, 2), (1, 3), (5, 1), (3, 2)]


@pytest.mark.parametrize("scalar", BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize("count", [0, 1, 2, 65])
@pytest.mark.parametrize("ring", ["n16_18bit", "n256_51bit"])
def test_operands_per_call(gpu, oracle, ring, count, scalar):
    """2: a 1 x dk vector and a d x dk matrix; 65: mixed rows_j and d_j, a second launch"""
    ops = {0: (), 1: ((D_R, D_D),), 2: ((1, D_D), (D_D, D_D))}[count] if count < 65 else tuple(MIXED[j % len(MIXED)] for j in range(65))
    run(gpu, oracle, ring, scalar=scalar, ops=ops, addend="mixed" if count else "none", negate=bool(count % 2))


def test_empty_operands_among_others(gpu, oracle):
    for scalar in BOTH:
        run(gpu, oracle, "n16_18bit", scalar=scalar, ops=((0, 2), (2, 2), (2, 0), (1, 1)), addend="mixed")
        run(gpu, oracle, "n16_18bit", scalar=scalar, ops=((0, 2), (3, 0)))


@pytest.mark.parametrize("scalar", SCALARS[:3] + BOTH[1:], ids=SCALAR_IDS[:3] + BOTH_IDS[1:])
def test_a_level_below_the_top(gpu, oracle, scalar):
    """k shrinks with the level: 2 of 3 limbs, 1 of 3 limbs"""
    run(gpu, oracle, "n16_18bit", scalar=scalar, limbs=2, ops=((2, 3), (1, 1)), addend="mixed", negate=True)
    run(gpu, oracle, "n256_51bit", scalar=scalar, limbs=1, addend="out")


@pytest.mark.parametrize("ring", ["n16_18bit", "n16_18bit_base4", "n256_61bit", "n16384_24bit"])
def test_every_tower_its_own_group(gpu, oracle, ring, hip_env):
    """the budget switch set below one tower's table: L groups, each with its own table kernel, transform and product"""
    whole = run(gpu, oracle, ring, scalar="eval", ops=((2, 2), (1, 1)), addend="mixed", model=False)
    hip_env.set("MXX_HIP_GADGET_SCALAR_BUDGET", "1")
    split = run(gpu, oracle, ring, scalar="eval", ops=((2, 2), (1, 1)), addend="mixed", negate=True)
    assert split > whole, (split, whole)
    hip_env.restore()
    assert run(gpu, oracle, ring, scalar="eval", ops=((2, 2), (1, 1)), addend="mixed", model=False) == whole


@pytest.mark.parametrize("ring", ["n16_18bit", "n256_51bit"])
def test_launch_counts_of_the_ring_element_entry(gpu, oracle, ring):
    """the table is built once per call: as many launches for 3 operands as for 1, one more for 65"""
    one = run(gpu, oracle, ring, scalar="eval", ops=((2, 2),), model=False)
    three = run(gpu, oracle, ring, scalar="eval", ops=((2, 2), (1, 1), (5, 3)), model=False)
    many = run(gpu, oracle, ring, scalar="eval", ops=tuple(MIXED[j % len(MIXED)] for j in range(65)), model=False)
    assert one >= 3 and three == one and many == one + 1, (one, three, many)
    # a COEFF scalar skips the inverse transform
    assert run(gpu, oracle, ring, scalar="coeff", ops=((2, 2),), model=False) < one


def test_a_packed24_lhs_gives_the_words_result(gpu, oracle):
    ring = "n16384_24bit"
    P = pool(gpu, oracle, ring)
    p, k = P["p"], P["k"]
    M = gpu.GpuDCRTPolyMatrix
    sc = dev(gpu, P, P["SC"])
    for scalar in (sc, constants(P)["three_words"]):
        sample = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 2, 2 * k, gpu.DistType.FinRingDist())
        assert sample.layout == "packed24" and sample.is_ntt
        got = sample.large_scalar_mul(scalar)
        res = sample.to_rns()
        words = M.from_rns(p, res, True)
        assert words.layout == "words"
        assert got == words.large_scalar_mul(scalar) and got == words._large_scalar_mul_host(scalar)
        c_eval = P["SC"] if scalar is sc else GM.const_eval(scalar, P["moduli"], P["n"])
        assert np.array_equal(got.to_rns(), oracle.matmul(res, host_dec(P, "eval" if scalar is sc else ("const", "three_words"), c_eval, 2), P["moduli"]))
        assert np.array_equal(sample.to_rns(), res)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
COMMON = ["null_outs", "null_lhss", "null_out_j", "null_lhs_j", "base_0", "base_63", "lhs_of_a_second_context", "addend_of_a_second_context",
          "out_of_a_second_context", "lhs_level", "addend_level", "out_level", "lhs_cols", "out_shape", "addend_shape", "coeff_lhs", "coeff_addend",
          "out_is_lhs", "out_is_a_row_view_of_lhs", "out_is_the_lhs_of_another_operand", "two_outs_share_a_block",
          "addend_is_a_shifted_view_of_out", "addend_is_another_operands_out"]
REFUSALS = ([("scalar", c) for c in COMMON + ["null_scalar", "scalar_level", "scalar_of_a_second_context", "scalar_not_1x1", "out_is_the_scalar"]] +
            [("const", c) for c in COMMON + ["null_const_words", "no_words"]])


@pytest.mark.parametrize("entry,case", REFUSALS, ids=[f"{e}-{c}" for e, c in REFUSALS])
def test_refusals_launch_nothing_and_leave_every_out_as_it_was(gpu, oracle, entry, case):
    """two operands, the fault in the second: everything is checked for every j before the first launch"""
    from mxx_amd import _ffi

    ring = "n256_51bit"
    P = pool(gpu, oracle, ring)
    p, base, k = P["p"], P["base"], P["k"]
    M = gpu.GpuDCRTPolyMatrix
    rows, d = 2, 2
    cols = d * k
    second = lambda: gpu.GpuDCRTPolyParams(RINGS[ring][0], P["moduli"], base, dnum=9)  # noqa: E731  same ring, its own context
    lower = lambda a: M.from_rns(p, np.ascontiguousarray(a[:, :, :2]), True)  # noqa: E731  2 of 3 limbs
    lhss = [dev(gpu, P, P["SL"][:rows, :cols]), dev(gpu, P, P["SL"][1:1 + rows, :cols])]
    outs = [dev(gpu, P, P["SENT"][:rows, :cols], False), dev(gpu, P, P["SENT"][1:1 + rows, :cols], False)]
    adds = [dev(gpu, P, P["AD"][:rows, :cols]), dev(gpu, P, P["AD"][1:1 + rows, :cols])]
    sc = dev(gpu, P, P["SC"]) if entry == "scalar" else 12345
    overlap, keep, n = False, [], 2
    null_outs = null_lhss = no_words = null_words = False
    if case == "null_outs":
        null_outs = True
    elif case == "null_lhss":
        null_lhss = True
    elif case == "null_out_j":
        outs[1] = None
    elif case == "null_lhs_j":
        lhss[1] = None
    elif case == "base_0":
        base = 0
    elif case == "base_63":
        base = 63
    elif case == "lhs_of_a_second_context":
        lhss[1] = M.from_rns(second(), np.ascontiguousarray(P["SL"][:rows, :cols]), True)
    elif case == "addend_of_a_second_context":
        adds[1] = M.from_rns(second(), np.ascontiguousarray(P["AD"][:rows, :cols]), True)
    elif case == "out_of_a_second_context":
        outs[1] = M.from_rns(second(), np.ascontiguousarray(P["SENT"][:rows, :cols]), False)
    elif case == "scalar_of_a_second_context":
        sc = M.from_rns(second(), np.ascontiguousarray(P["SC"]), True)
    elif case == "lhs_level":
        lhss[1] = lower(P["SL"][:rows, :cols])
    elif case == "addend_level":
        adds[1] = lower(P["AD"][:rows, :cols])
    elif case == "out_level":
        outs[1] = lower(P["SENT"][:rows, :cols])
    elif case == "scalar_level":
        sc = lower(P["SC"])
    elif case == "lhs_cols":
        lhss[1] = dev(gpu, P, P["SL"][:rows, :cols - 1])
        outs[1] = dev(gpu, P, P["SENT"][:rows, :cols - 1], False)
        adds[1] = None
    elif case == "out_shape":
        outs[1] = dev(gpu, P, P["SENT"][:rows + 1, :cols], False)
    elif case == "addend_shape":
        adds[1] = dev(gpu, P, P["AD"][:rows, :cols + k])
    elif case == "coeff_lhs":
        lhss[1] = dev(gpu, P, P["SL"][:rows, :cols], False)
    elif case == "coeff_addend":
        adds[1] = dev(gpu, P, P["AD"][:rows, :cols], False)
    elif case == "scalar_not_1x1":
        sc = dev(gpu, P, P["SL"][:1, :2])
    elif case == "null_scalar":
        sc = None
    elif case == "null_const_words":
        null_words = True
    elif case == "no_words":
        no_words = True
    elif case == "out_is_lhs":
        outs[1], overlap = lhss[1], True
    elif case == "out_is_a_row_view_of_lhs":
        parent = dev(gpu, P, P["SL"][:rows + 1, :cols])
        lhss[1], outs[1], overlap = parent.row_view(0, rows), parent.row_view(1, 1 + rows), True
        keep.append(parent)
    elif case == "out_is_the_lhs_of_another_operand":
        outs[1], overlap = lhss[0], True
    elif case == "two_outs_share_a_block":
        parent = dev(gpu, P, P["SENT"][:rows + 1, :cols])
        outs[0], outs[1], overlap = parent.row_view(0, rows), parent.row_view(1, 1 + rows), True
        keep.append(parent)
    elif case == "addend_is_a_shifted_view_of_out":
        parent = dev(gpu, P, P["SENT"][:rows + 1, :cols])
        outs[1], adds[1], overlap = parent.row_view(1, 1 + rows), parent.row_view(0, rows), True
        keep.append(parent)
    elif case == "addend_is_another_operands_out":
        outs[0] = dev(gpu, P, P["SENT"][:rows, :cols])
        adds[1], overlap = outs[0], True
    elif case == "out_is_the_scalar":
        # the overlap must be the only fault: a ring whose k is 1, so that a 1 x 1 output has a valid shape
        p1 = make_params(gpu, oracle, 16, 1, 18, 18)
        m1 = p1.moduli()
        assert p1.crt_bits() <= 18
        sc = M.from_rns(p1, oracle.random_matrix(920, 1, 1, m1, 16), True)
        lhss, outs, adds, overlap, n, base = [M.from_rns(p1, oracle.random_matrix(921, 1, 1, m1, 16), True)], [sc], [None], True, 1, 18
    else:
        raise AssertionError(case)
    live = [m for m in outs if m is not None]
    before = [m.clone() for m in live]
    tags = [m.is_ntt for m in live]
    gpu.gpu_device_sync()
    c0 = launches()
    lib = _ffi.lib()
    o_arr, l_arr, a_arr = (None if null_outs else _arr(outs)), (None if null_lhss else _arr(lhss)), _arr(adds)
    if entry == "scalar":
        rc = lib.gpupoly_matrix_mul_decompose_gadget_scalar_many(o_arr, l_arr, a_arr, n, None if sc is None else sc.raw, 0, base)
    else:
        words, wpc = int_words(sc)
        rc = lib.gpupoly_matrix_mul_decompose_gadget_const_many(o_arr, l_arr, a_arr, n, None if null_words else words, 0 if no_words else wpc, 0, base)
    msg = _ffi.last_error_string()
    assert launches() == c0, "a refused call launched a kernel"
    assert rc != 0 and (SM if entry == "scalar" else CM) in msg, msg
    if overlap:
        assert "overlaps" in msg, msg
    for m, b, tag in zip(live, before, tags):
        assert m.is_ntt == tag and raw_same(m, b), f"{case}: an output changed (residues or tag)"


# ---- the host mirror ------------------------------------------------------------------------------------------------------
def test_mirror(gpu, oracle, monkeypatch):
    n, depth, bits, base = RINGS["n16_18bit"]
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    d, k = 2, p.modulus_digits()
    g = M.gadget_matrix(p, d)
    s = M.from_rns(p, oracle.random_matrix(930, 1, d * k, moduli, n), True)
    key = M.from_rns(p, oracle.random_matrix(931, d, d * k, moduli, n), True)
    a = M.from_rns(p, oracle.random_matrix(932, d, d * k, moduli, n), True)
    x = M.from_rns(p, oracle.random_matrix(933, 1, 1, moduli, n), True)
    x_poly = gpu.GpuDCRTPoly(x)  # scalars may be polynomials or 1 x 1 matrices, in either domain
    want = s.mul_decompose(g.mul_scalar(x))
    assert s.large_scalar_mul(x_poly) == want and s.large_scalar_mul(x) == want and s._large_scalar_mul_host(x) == want
    assert s.large_scalar_mul(x.clone().into_coeff_domain()) == want
    big = (1 << 130) + 77
    c_poly = gpu.GpuDCRTPoly.from_biguints(p, [big])
    want_c = s.mul_decompose(g.mul_scalar(c_poly))
    assert s.large_scalar_mul(big) == want_c and s.large_scalar_mul([big]) == want_c and s._large_scalar_mul_host(big) == want_c
    coeffs = [3, big, 0, 5]
    assert s.large_scalar_mul(coeffs) == s.mul_decompose(g.mul_scalar(gpu.GpuDCRTPoly.from_biguints(p, coeffs)))
    # the vector and the key matrix of an encoding in one call, with addends and a sign
    got = M.large_scalar_mul_many([s, key], big, addends=[None, a], negate=True)
    assert got[0] == -want_c and got[1] == a - key.mul_decompose(g.mul_scalar(c_poly))
    assert M.large_scalar_mul_many([], 5) == []
    # the reference's sequence runs when its chunk switch is set
    from mxx_amd import matrix as mat

    monkeypatch.setattr(mat, "mul_decompose_column_chunk_width_is_set", lambda: True)
    monkeypatch.setattr(mat, "mul_decompose_column_chunk_width", lambda: 1)
    c0 = launches()
    got = M.large_scalar_mul_many([s, key], x_poly, addends=[None, a], negate=True)
    assert got[0] == -want and got[1] == a - key.mul_decompose(g.mul_scalar(x))
    assert launches() - c0 > 8
