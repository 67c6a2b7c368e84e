"""gpupoly_matrix_mul_gadget / gpupoly_matrix_gadget_mul: products with G_d = I_d (x) g that never build G.

    mul_gadget:  out[:, dst_col .. dst_col + cols) = addend block +- (lhs * G_d[:, gadget_col .. gadget_col + cols)) o scalar
    gadget_mul:  out = addend +- G_d * rhs

Every case is held, bit for bit, to (1) the CPU restatement - oracle.gadget_matrix, a window of it, oracle.matmul /
oracle.pointwise, exact integer add / sub mod q on the host; (2) the sequence of the existing entry points - fill_gadget,
copy_block for the window, mul / mul_scalar, add / sub / neg, copy_block into place - through gpu_matrix_equal (residues and
tag); (3) for a handful of entries exact Python integers on plainref.gadget.  Every call also has its launch count checked
(exactly one on words-layout operands, none for empty shapes) and its inputs compared with their uploads afterwards.  Every
axis is covered against one default of the others."""
import ctypes as C

import numpy as np
import pytest

import plainref as PR
from conftest import make_params

pytestmark = pytest.mark.gpu

# (n, limbs, limb bits, base bits): the scalar path (a limb vector of 8 bytes); dpt 3, k 9; a base that does not divide;
# 64-bit words; dpt 4 at the widest words of each class; the 16-byte path with several chunks per limb vector
RINGS = {"n2_18bit": (2, 2, 18, 6), "n16_18bit": (16, 3, 18, 6), "n16_18bit_base7": (16, 3, 18, 7), "n256_51bit": (256, 3, 51, 17),
         "n256_61bit": (256, 2, 61, 20), "n256_31bit": (256, 2, 31, 8), "n16384_24bit": (16384, 2, 24, 12)}
AXES = ["n16_18bit", "n256_51bit", "n16384_24bit"]  # the rings every axis runs on: u32 scalar-sized, u64, u32 16-byte path
DMAX, RMAX, CMAX, WIDE_PAD = 3, 5, 3, 3  # pool sizes: block rows of G, rows of lhs, columns of rhs; columns around a placed block
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
        kmax = dpt * L
        width = DMAX * kmax + WIDE_PAD
        P = dict(p=p, moduli=moduli, n=n, L=L, base=base, dpt=dpt, oracle=oracle, G={},
                 SL=oracle.random_matrix(810, RMAX, DMAX, moduli, n), SC=oracle.random_matrix(811, 1, 1, moduli, n),
                 AD=oracle.random_matrix(812, RMAX, width, moduli, n), SENT=oracle.random_matrix(813, RMAX, width, moduli, n),
                 RH=oracle.random_matrix(814, DMAX * kmax, CMAX, moduli, n))
        for name in ("SL", "SC", "AD", "SENT", "RH"):
            P[name].setflags(write=False)
        _pool[key] = P
    return _pool[key]


def digits_of(P, small):
    return P["dpt"] if small else P["dpt"] * P["L"]


def host_gadget(P, d, small):
    """oracle.gadget_matrix (EVAL), cached per (d, small)"""
    if (d, small) not in P["G"]:
        g = P["oracle"].gadget_matrix(d, P["moduli"], P["n"], P["base"], small=small)
        g.setflags(write=False)
        P["G"][(d, small)] = g
    return P["G"][(d, small)]


def qcol(P):
    return np.array([int(m) for m in P["moduli"]], dtype=np.uint64).reshape(1, 1, -1, 1)


def add_mod(x, y, q):
    return (x + y) % q  # both below q < 2^62


def sub_mod(x, y, q):
    return (x + (q - y)) % q


def dev(gpu, P, data, eval_format=True):
    """upload; shapes without entries come from the constructor"""
    M = gpu.GpuDCRTPolyMatrix
    if data.shape[0] == 0 or data.shape[1] == 0:
        return M(P["p"], data.shape[0], data.shape[1], P["L"] - 1, eval_format)
    return M.from_rns(P["p"], np.ascontiguousarray(data), eval_format)


def dev_gadget(gpu, P, d, small):
    """gpu_matrix_fill_gadget / _small_gadget at the pool's level (GpuDCRTPolyMatrix.gadget_matrix is top level only)"""
    from mxx_amd import _ffi

    g = gpu.GpuDCRTPolyMatrix(P["p"], d, d * digits_of(P, small), P["L"] - 1, True)
    fn = _ffi.lib().gpu_matrix_fill_small_gadget if small else _ffi.lib().gpu_matrix_fill_gadget
    _ffi.check_status(fn(g.raw, P["base"]), "gpu_matrix_fill_gadget")
    return g


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag (a tag mismatch is 'not equal' there)"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value) or a.nrow * a.ncol == 0


def launches():
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_launch_count()


def _raw(m):
    return None if m is None else m.raw


def raw_mul_gadget(out, dst_col, lhs, scalar, gadget_col, cols, addend, negate, base, small):
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_matrix_mul_gadget(_raw(out), dst_col, _raw(lhs), _raw(scalar), gadget_col, cols, _raw(addend),
                                                1 if negate else 0, base, 1 if small else 0)


def raw_gadget_mul(out, rhs, addend, negate, base, small):
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_matrix_gadget_mul(_raw(out), _raw(rhs), _raw(addend), 1 if negate else 0, base, 1 if small else 0)


def weight(P, l, t, e, small):
    """w(l, t, e) in exact Python integers"""
    q = int(P["moduli"][l])
    return pow(pow(2, P["base"], q), e, q) if (small or t == l) else 0


def windows(P, d, small):
    k = digits_of(P, small)
    return {"whole": (0, d * k), "one_column": (1 if d * k > 1 else 0, 1), "crossing": (k - 1, min(3, d * k - (k - 1))),
            "last_column": (d * k - 1, 1), "empty": (d * k // 2, 0)}


# ---- mul_gadget ---------------------------------------------------------------------------------------------------------
def run_mul_gadget(gpu, oracle, ring, d=D_D, rows=D_R, with_lhs=True, with_scalar=True, addend="separate", negate=False, small=False,
                   window="whole", placed=False, limbs=None, worst=False):
    """One call against the CPU restatement, the device sequence and (a few entries) exact integers.  addend: "none",
    "separate" or "out".  placed: the block goes to columns [2, 2 + cols) of a wider sentinel.  worst: every operand q - 1."""
    P = pool(gpu, oracle, ring, limbs)
    M = gpu.GpuDCRTPolyMatrix
    q = qcol(P)
    L, n = P["L"], P["n"]
    if not with_lhs:
        rows = d
    gc, cols = windows(P, d, small)[window]
    dst = 2 if placed else 0
    width = cols + WIDE_PAD if placed else cols
    top = lambda a: np.broadcast_to(q - 1, a.shape).astype(np.uint64) if worst else a  # noqa: E731
    lhs_host = top(P["SL"][:rows, :d]) if with_lhs else None
    sc_host = top(P["SC"]) if with_scalar else None
    out_host = top(P["SENT"][:rows, :width])
    add_host = None if addend == "none" else (out_host if addend == "out" else top(P["AD"][:rows, :width]))
    # (1) the CPU restatement
    want = out_host.copy()
    prod = None
    if rows and cols:
        gw = np.ascontiguousarray(host_gadget(P, d, small)[:, gc:gc + cols])
        prod = oracle.matmul(lhs_host, gw, P["moduli"]) if with_lhs else gw
        if with_scalar:
            prod = oracle.pointwise("mul", prod, sc_host, P["moduli"])
        if add_host is None:
            block = sub_mod(np.zeros_like(prod), prod, q) if negate else prod
        else:
            block = (sub_mod if negate else add_mod)(add_host[:, dst:dst + cols], prod, q)
        want[:, dst:dst + cols] = block
    # device operands
    lhs = dev(gpu, P, lhs_host) if with_lhs else None
    sc = dev(gpu, P, sc_host) if with_scalar else None
    out = dev(gpu, P, out_host)
    add = None if addend == "none" else (out if addend == "out" else dev(gpu, P, add_host))
    # (2) the sequence of existing entry points, placed with copy_block
    seq_out = out.clone()
    if rows and cols:
        gwd = dev_gadget(gpu, P, d, small).slice_columns(gc, gc + cols)
        pd = lhs * gwd if with_lhs else gwd
        if with_scalar:
            pd = pd.mul_scalar(sc)
        if add is None:
            blk = -pd if negate else pd
        else:
            ab = add.slice_columns(dst, dst + cols)
            blk = ab - pd if negate else ab + pd
        seq_out.copy_block_from(blk, 0, dst, 0, 0, rows, cols)
    inputs = [m for m in (lhs, sc, add if addend == "separate" else None) if m is not None]
    before = [m.clone() for m in inputs]
    assert all(m.layout == "words" for m in inputs + [out])

    gpu.gpu_device_sync()
    c0 = launches()
    rc = raw_mul_gadget(out, dst, lhs, sc, gc, cols, add, negate, P["base"], small)
    count = launches() - c0
    from mxx_amd import _ffi
    assert rc == 0, _ffi.last_error_string()
    assert count == (1 if rows and cols else 0), f"{count} launches"
    if rows and width:
        got = out.to_rns()
        assert np.array_equal(got, want), "against the CPU restatement (columns outside the block included)"
        # (3) exact integers for a handful of entries, independent of oracle/
        if cols:
            k = digits_of(P, small)
            plain = None if small else PR.gadget(d, P["moduli"], P["base"], n)
            for (i, c) in {(0, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)}:
                j, loc = divmod(gc + c, k)
                t, e = (0, loc) if small else divmod(loc, P["dpt"])
                for l in range(L):
                    ql = int(P["moduli"][l])
                    w = weight(P, l, t, e, small)
                    if plain is not None:
                        assert w == int(plain[j, gc + c, l, 0])
                    for s in {0, n - 1, n // 2}:
                        x = int(lhs_host[i, j, l, s]) if with_lhs else int(i == j)
                        v = x * w * (int(sc_host[0, 0, l, s]) if with_scalar else 1)
                        a = 0 if add_host is None else int(add_host[i, dst + c, l, s])
                        assert int(got[i, dst + c, l, s]) == ((a - v) % ql if negate else (a + v) % ql), (i, c, l, s)
    assert out.size() == (rows, width)
    assert raw_same(out, seq_out), "against the sequence of existing entry points (residues and tag)"
    for j, (m, b) in enumerate(zip(inputs, before)):
        assert raw_same(m, b), f"input {j} changed"


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_mul_gadget_on_every_ring(gpu, oracle, ring, small):
    run_mul_gadget(gpu, oracle, ring, negate=True, small=small)
    run_mul_gadget(gpu, oracle, ring, with_lhs=False, addend="out", negate=True, small=small)  # A -= G x


@pytest.mark.parametrize("rows", [1, 2, 5, 0])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("ring", AXES)
def test_mul_gadget_shapes(gpu, oracle, ring, d, rows):
    run_mul_gadget(gpu, oracle, ring, d=d, rows=rows)


@pytest.mark.parametrize("with_lhs", [True, False], ids=["lhs", "identity"])
@pytest.mark.parametrize("window", ["whole", "one_column", "crossing", "last_column", "empty"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("ring", AXES)
def test_mul_gadget_windows(gpu, oracle, ring, d, window, with_lhs):
    run_mul_gadget(gpu, oracle, ring, d=d, window=window, with_lhs=with_lhs, with_scalar=False, addend="none")
    run_mul_gadget(gpu, oracle, ring, d=d, window=window, with_lhs=with_lhs, addend="out", negate=True)


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("negate", [False, True], ids=["plus", "minus"])
@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("with_scalar", [False, True], ids=["noscalar", "scalar"])
@pytest.mark.parametrize("with_lhs", [True, False], ids=["lhs", "identity"])
@pytest.mark.parametrize("ring", ["n256_51bit", "n16384_24bit"])
def test_mul_gadget_options(gpu, oracle, ring, with_lhs, with_scalar, addend, negate, small):
    run_mul_gadget(gpu, oracle, ring, with_lhs=with_lhs, with_scalar=with_scalar, addend=addend, negate=negate, small=small)


@pytest.mark.parametrize("with_lhs", [True, False], ids=["lhs", "identity"])
@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("ring", AXES)
def test_mul_gadget_placement_leaves_the_other_columns(gpu, oracle, ring, addend, with_lhs):
    run_mul_gadget(gpu, oracle, ring, placed=True, window="crossing", addend=addend, with_lhs=with_lhs, negate=addend != "separate")
    run_mul_gadget(gpu, oracle, ring, placed=True, window="empty", addend=addend, with_lhs=with_lhs)


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_mul_gadget_at_a_level_below_the_top(gpu, oracle, small):
    """k shrinks with the level: 2 of 3 limbs"""
    for with_lhs in (True, False):
        for addend in ("separate", "out"):
            run_mul_gadget(gpu, oracle, "n16_18bit", limbs=2, d=3, with_lhs=with_lhs, addend=addend, negate=True, small=small)
    run_mul_gadget(gpu, oracle, "n256_51bit", limbs=1, window="crossing", placed=True, small=small)


@pytest.mark.parametrize("ring", ["n256_31bit", "n256_51bit", "n256_61bit"])
def test_mul_gadget_worst_case_inputs(gpu, oracle, ring):
    """lhs, scalar and addend all q - 1"""
    for negate in (False, True):
        run_mul_gadget(gpu, oracle, ring, worst=True, negate=negate)
        run_mul_gadget(gpu, oracle, ring, worst=True, negate=negate, addend="out", small=True)


# ---- gadget_mul ---------------------------------------------------------------------------------------------------------
def run_gadget_mul(gpu, oracle, ring, d=D_D, c=CMAX, eval_format=True, addend="separate", negate=False, small=False, limbs=None, worst=False):
    P = pool(gpu, oracle, ring, limbs)
    q = qcol(P)
    L, n, dpt = P["L"], P["n"], P["dpt"]
    k = digits_of(P, small)
    top = lambda a: np.broadcast_to(q - 1, a.shape).astype(np.uint64) if worst else a  # noqa: E731
    rhs_host = top(P["RH"][:d * k, :c])
    out_host = top(P["SENT"][:d, :c])
    add_host = None if addend == "none" else (out_host if addend == "out" else top(P["AD"][:d, :c]))
    # (1) the CPU restatement: the constants of G scale whole limb vectors, so the same numbers serve COEFF and EVAL
    want = out_host.copy()
    if d and c:
        prod = oracle.matmul(host_gadget(P, d, small), rhs_host, P["moduli"])
        if add_host is None:
            want = sub_mod(np.zeros_like(prod), prod, q) if negate else prod
        else:
            want = (sub_mod if negate else add_mod)(add_host, prod, q)
    rhs = dev(gpu, P, rhs_host, eval_format)
    out = dev(gpu, P, out_host, not eval_format if addend != "out" else eval_format)  # the tag must come from rhs
    add = None if addend == "none" else (out if addend == "out" else dev(gpu, P, add_host, eval_format))
    # (2) the existing sequence (EVAL only: gpu_matrix_mul wants EVAL operands)
    seq = None
    if eval_format and d and c:
        pd = dev_gadget(gpu, P, d, small) * rhs
        if add is None:
            seq = -pd if negate else pd
        else:
            seq = add - pd if negate else add + pd
    inputs = [rhs] + ([add] if addend == "separate" else [])
    before = [m.clone() for m in inputs]
    assert all(m.layout == "words" for m in inputs + [out])

    gpu.gpu_device_sync()
    c0 = launches()
    rc = raw_gadget_mul(out, rhs, add, negate, P["base"], small)
    count = launches() - c0
    from mxx_amd import _ffi
    assert rc == 0, _ffi.last_error_string()
    assert count == (1 if d and c else 0), f"{count} launches"
    out.is_ntt = eval_format  # the mirror's tag follows the library's: raw_same below compares the library's
    if d and c:
        got = out.to_rns()
        assert np.array_equal(got, want), "against the CPU restatement"
        # (3) exact integers
        for (j, col) in {(0, 0), (d - 1, c - 1)}:
            for l in range(L):
                ql = int(P["moduli"][l])
                for s in {0, n - 1, n // 2}:
                    v = sum(weight(P, l, l, e, small) * int(rhs_host[j * k + (0 if small else l * dpt) + e, col, l, s]) for e in range(dpt))
                    a = 0 if add_host is None else int(add_host[j, col, l, s])
                    assert int(got[j, col, l, s]) == ((a - v) % ql if negate else (a + v) % ql), (j, col, l, s)
    if seq is not None:
        assert raw_same(out, seq), "against the sequence of existing entry points (residues and tag)"
    else:
        ref = dev(gpu, P, want, eval_format)
        assert raw_same(out, ref), "residues and tag (rhs's format)"
    for j, (m, b) in enumerate(zip(inputs, before)):
        assert raw_same(m, b), f"input {j} changed"


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_gadget_mul_on_every_ring(gpu, oracle, ring, small):
    run_gadget_mul(gpu, oracle, ring, negate=True, small=small)


@pytest.mark.parametrize("eval_format", [True, False], ids=["eval", "coeff"])
@pytest.mark.parametrize("c", [1, 3, 0])
@pytest.mark.parametrize("d", [1, 2, 3, 0])
@pytest.mark.parametrize("ring", AXES)
def test_gadget_mul_shapes_and_formats(gpu, oracle, ring, d, c, eval_format):
    run_gadget_mul(gpu, oracle, ring, d=d, c=c, eval_format=eval_format)


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("negate", [False, True], ids=["plus", "minus"])
@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("eval_format", [True, False], ids=["eval", "coeff"])
@pytest.mark.parametrize("ring", ["n256_51bit", "n16384_24bit"])
def test_gadget_mul_options(gpu, oracle, ring, eval_format, addend, negate, small):
    run_gadget_mul(gpu, oracle, ring, eval_format=eval_format, addend=addend, negate=negate, small=small)


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_gadget_mul_at_a_level_below_the_top(gpu, oracle, small):
    run_gadget_mul(gpu, oracle, "n16_18bit", limbs=2, d=3, negate=True, small=small)
    run_gadget_mul(gpu, oracle, "n256_51bit", limbs=1, addend="out", eval_format=False, small=small)


@pytest.mark.parametrize("ring", ["n256_31bit", "n256_51bit", "n256_61bit"])
def test_gadget_mul_worst_case_inputs(gpu, oracle, ring):
    """rhs and addend all q - 1 (not digit-sized: the entry takes any rhs)"""
    for negate in (False, True):
        run_gadget_mul(gpu, oracle, ring, worst=True, negate=negate)
        run_gadget_mul(gpu, oracle, ring, worst=True, negate=negate, addend="out", small=True)


# ---- the identities the reference's own tests state ---------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["n16_18bit_base7", "n256_61bit", "n16384_24bit"])
def test_gadget_mul_of_a_decomposition_gives_the_matrix_back(gpu, oracle, ring):
    n, depth, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M = gpu.GpuDCRTPolyMatrix
    moduli = p.moduli()
    m = M.from_rns(p, oracle.random_matrix(820, 2, 3, moduli, n), True)
    assert M.gadget_mul(m.decompose()) == m
    assert M.gadget_matrix(p, 2) * m.decompose() == m
    # small: values that fit limb 0, the same integer in every limb
    vals = oracle.random_matrix(821, 2, 3, moduli[:1], n)  # below q_0
    res = np.concatenate([vals % np.uint64(int(ql)) for ql in moduli], axis=2)
    ms = M.from_rns(p, res, False)
    digits = ms.small_decompose()
    ms.ntt_all_in_place()
    assert M.gadget_mul(digits, small=True) == ms
    assert M.small_gadget_matrix(p, 2) * digits == ms


@pytest.mark.parametrize("ring", list(RINGS))
def test_mul_gadget_with_everything_defaulted_is_the_gadget_matrix(gpu, oracle, ring):
    n, depth, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M = gpu.GpuDCRTPolyMatrix
    for d in (1, 3):
        g = M.gadget_matrix(p, d)
        k = p.modulus_digits()
        assert M.gadget_block(p, d, 0, d * k) == g
        assert M.identity(p, d).mul_gadget() == g
        assert M.gadget_block(p, d, k - 1, min(d * k, k + 2)) == g.slice(0, d, k - 1, min(d * k, k + 2))
        gs = M.small_gadget_matrix(p, d)
        ks = gs.ncol // d
        assert M.gadget_block(p, d, 0, d * ks, small=True) == gs
        assert M.gadget_block(p, d, d * ks - 1, d * ks, small=True) == gs.slice(0, d, d * ks - 1, d * ks)
    assert np.array_equal(M.gadget_block(p, 2, 0, 2 * p.modulus_digits()).to_rns(), oracle.matrix_ntt(PR.gadget(2, p.moduli(), base, n), p.moduli()))


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------
def test_a_packed24_lhs_gives_the_words_result(gpu, oracle):
    n, depth, bits, base = RINGS["n16384_24bit"]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M = gpu.GpuDCRTPolyMatrix
    sample = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 2, 2, gpu.DistType.FinRingDist())
    assert sample.layout == "packed24" and sample.is_ntt
    got = sample.mul_gadget(negate=True)
    res = sample.to_rns()
    words = M.from_rns(p, res, True)
    assert words.layout == "words"
    assert got == words.mul_gadget(negate=True) and got == -(words * M.gadget_matrix(p, 2))
    assert np.array_equal(sample.to_rns(), res)
    # and as the digit rows of gadget_mul
    rows = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, p.modulus_digits(), 2, gpu.DistType.FinRingDist())
    assert rows.layout == "packed24"
    got = M.gadget_mul(rows)
    assert got == M.gadget_matrix(p, 1) * M.from_rns(p, rows.to_rns(), True)


def test_the_trace_states_the_algorithmic_bytes(gpu, oracle):
    """in place: the hit vectors read and written plus the scalar; one pass: every vector written, the addend read, the scalar;
    gadget_mul: dpt reads and one write per output vector"""
    from mxx_amd import _ffi

    P = pool(gpu, oracle, "n16384_24bit")
    d, c, k, L, dpt, base = 2, 3, digits_of(P, False), P["L"], P["dpt"], P["base"]
    vec = P["n"] * 4  # bytes of a limb vector
    a, x = dev(gpu, P, P["AD"][:d, :d * k]), dev(gpu, P, P["SC"])
    out, rhs, out2 = dev(gpu, P, P["SENT"][:d, :d * k]), dev(gpu, P, P["RH"][:d * k, :c]), dev(gpu, P, P["SENT"][:d, :c])
    acc = a.clone()
    gpu.gpu_device_sync()
    _ffi.trace_begin()
    assert raw_mul_gadget(acc, 0, None, x, 0, d * k, acc, True, base, False) == 0
    assert raw_mul_gadget(out, 0, None, x, 0, d * k, a, True, base, False) == 0
    assert raw_gadget_mul(out2, rhs, None, False, base, False) == 0
    recs = _ffi.trace_end()
    assert [("mul_gadget_kernel" in r["kernel"], "gadget_mul_kernel" in r["kernel"]) for r in recs] == [(True, False), (True, False), (False, True)], recs
    assert recs[0]["bytes"] == vec * (2 * d * k + L) and recs[0]["blocks"] < recs[1]["blocks"]
    assert recs[1]["bytes"] == vec * (2 * d * d * k * L + L)
    assert recs[2]["bytes"] == vec * d * c * L * (dpt + 1)
    assert out == acc


# ---- refusals ---------------------------------------------------------------------------------------------------------------
MG, GM = "gpupoly_matrix_mul_gadget", "gpupoly_matrix_gadget_mul"
REFUSALS = ["mg_null_out", "mg_base_0", "mg_base_63", "mg_lhs_of_a_second_context", "mg_scalar_of_a_second_context",
            "mg_addend_of_a_second_context", "mg_level_mismatch", "mg_lhs_rows", "mg_block_out_of_range", "mg_window_out_of_range",
            "mg_window_out_of_range_identity", "mg_addend_shape", "mg_coeff_lhs", "mg_coeff_scalar", "mg_coeff_addend", "mg_scalar_not_1x1",
            "mg_partial_block_into_coeff_out", "mg_addend_is_a_shifted_view_of_out", "mg_out_is_a_row_view_of_lhs", "mg_out_is_the_scalar",
            "gm_null_out", "gm_null_rhs", "gm_base_0", "gm_base_63", "gm_rhs_of_a_second_context", "gm_addend_of_a_second_context",
            "gm_level_mismatch", "gm_rhs_rows", "gm_rhs_cols", "gm_addend_shape", "gm_mixed_formats", "gm_out_is_a_row_view_of_rhs",
            "gm_addend_is_a_shifted_view_of_out"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing_and_leave_out_as_it_was(gpu, oracle, case):
    from mxx_amd import _ffi

    ring = "n256_51bit"
    P = pool(gpu, oracle, ring)
    p, base = P["p"], P["base"]
    M = gpu.GpuDCRTPolyMatrix
    d, rows, c = 2, 2, 3
    k = digits_of(P, False)
    cols = d * k
    lhs, sc = dev(gpu, P, P["SL"][:rows, :d]), dev(gpu, P, P["SC"])
    addend = dev(gpu, P, P["AD"][:rows, :cols])
    rhs = dev(gpu, P, P["RH"][:d * k, :c])
    # `out` holds known residues under the COEFF tag wherever the rule allows it: a refused call must leave both
    is_mg = case.startswith("mg_")
    out = dev(gpu, P, P["SENT"][:rows, :cols], False) if is_mg else dev(gpu, P, P["SENT"][:d, :c], False)
    if not is_mg:
        addend = dev(gpu, P, P["AD"][:d, :c])
    dst, gc, overlap, keep = 0, 0, False, []
    second = lambda: gpu.GpuDCRTPolyParams(RINGS[ring][0], P["moduli"], base, dnum=9)  # noqa: E731  same ring, its own context
    what = case[3:]
    if what == "null_out":
        out = None
    elif what == "null_rhs":
        rhs = None
    elif what == "base_0":
        base = 0
    elif what == "base_63":
        base = 63
    elif what == "lhs_of_a_second_context":
        lhs = M.from_rns(second(), np.ascontiguousarray(P["SL"][:rows, :d]), True)
    elif what == "scalar_of_a_second_context":
        sc = M.from_rns(second(), np.ascontiguousarray(P["SC"]), True)
    elif what == "rhs_of_a_second_context":
        rhs = M.from_rns(second(), np.ascontiguousarray(P["RH"][:d * k, :c]), True)
    elif what == "addend_of_a_second_context":
        addend = M.from_rns(second(), np.ascontiguousarray(P["AD"][:out.nrow, :out.ncol]), True)
    elif what == "level_mismatch":
        if is_mg:
            lhs = M.from_rns(p, np.ascontiguousarray(P["SL"][:rows, :d, :2]), True)
        else:
            rhs = M.from_rns(p, np.ascontiguousarray(P["RH"][:d * k, :c, :2]), True)
    elif what == "lhs_rows":
        lhs = dev(gpu, P, P["SL"][:rows + 1, :d])
    elif what == "block_out_of_range":
        addend, dst = None, 1  # dst_col + cols > out->cols
        out = dev(gpu, P, P["SENT"][:rows, :cols])
    elif what == "window_out_of_range":
        gc = 1  # gadget_col + cols > d * k
    elif what == "window_out_of_range_identity":
        lhs, gc = None, 1
    elif what == "addend_shape":
        addend = dev(gpu, P, P["AD"][:out.nrow, :out.ncol + 1])
    elif what == "coeff_lhs":
        lhs = dev(gpu, P, P["SL"][:rows, :d], False)
    elif what == "coeff_scalar":
        sc = dev(gpu, P, P["SC"], False)
    elif what == "coeff_addend":
        addend = dev(gpu, P, P["AD"][:rows, :cols], False)
    elif what == "scalar_not_1x1":
        sc = dev(gpu, P, P["SL"][:1, :2])
    elif what == "partial_block_into_coeff_out":
        out = dev(gpu, P, P["SENT"][:rows, :cols + WIDE_PAD], False)
        addend, dst = None, 2
    elif what == "addend_is_a_shifted_view_of_out":
        r_, c_ = (rows, cols) if is_mg else (d, c)
        parent = dev(gpu, P, P["SENT"][:r_ + 1, :c_])
        out, addend, overlap = parent.row_view(1, 1 + r_), parent.row_view(0, r_), True
        keep.append(parent)
    elif what == "out_is_a_row_view_of_lhs":
        # the alias must be the only fault: a window as wide as lhs
        out, addend, cols, overlap = lhs.row_view(0, rows), None, d, True
    elif what == "out_is_the_scalar":
        lhs, addend, out, cols, overlap = None, None, sc, 1, True  # 1 x 1 with d = 1
    elif what == "rhs_rows":
        rhs = dev(gpu, P, P["RH"][:d * k - 1, :c])
    elif what == "rhs_cols":
        rhs = dev(gpu, P, P["RH"][:d * k, :c - 1])
    elif what == "mixed_formats":
        addend = dev(gpu, P, P["AD"][:d, :c], False)
    elif what == "out_is_a_row_view_of_rhs":
        out, addend, overlap = rhs.row_view(1, 1 + d), None, True
    else:
        raise AssertionError(case)
    before = None if out is None else out.clone()
    tag = None if out is None else out.is_ntt
    gpu.gpu_device_sync()
    c0 = launches()
    if is_mg:
        rc = raw_mul_gadget(out, dst, lhs, sc, gc, cols, addend, False, base, False)
    else:
        rc = raw_gadget_mul(out, rhs, addend, False, base, False)
    msg = _ffi.last_error_string()
    assert launches() == c0, "a refused call launched a kernel"
    assert rc != 0 and (MG if is_mg else GM) in msg, msg
    if overlap:
        assert "overlaps" in msg, msg
    if out is not None:
        assert out.is_ntt == tag and raw_same(out, before), f"{case}: `out` changed (residues or tag)"


# ---- the host mirror ------------------------------------------------------------------------------------------------------
def test_mirror(gpu, oracle):
    n, depth, bits, base = RINGS["n16_18bit"]
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    d, k = 2, p.modulus_digits()
    g = M.gadget_matrix(p, d)
    s = M.from_rns(p, oracle.random_matrix(830, 1, d, moduli, n), True)
    x = M.from_rns(p, oracle.random_matrix(831, 1, 1, moduli, n), True)
    x_poly = gpu.GpuDCRTPoly(x)  # scalars may be polynomials or 1 x 1 matrices
    a = M.from_rns(p, oracle.random_matrix(832, d, d * k, moduli, n), True)
    assert s.mul_gadget() == s * g
    assert s.mul_gadget(scalar=x_poly) == (s * g).mul_scalar(x) and s.mul_gadget(scalar=x) == (s * g).mul_scalar(x)
    assert s.mul_gadget(col_start=k - 1, col_end=k + 2, negate=True) == -(s * g.slice(0, d, k - 1, k + 2))
    # A - G x, in place
    b = a.clone()
    v0 = b.content_version()
    b.add_scaled_gadget(scalar=x_poly, negate=True)
    assert b == a - g.mul_scalar(x) and b.content_version() != v0
    # A_chunk - G[:, chunk] y, out of place into a block of a wider matrix
    wide = a.clone()
    chunk = a.slice_columns(3, 6)
    got = M.identity(p, d).mul_gadget(scalar=x_poly, col_start=3, col_end=6, addend=a, negate=True, out=wide, dst_col=3)
    assert got is wide
    want = a.clone()
    want.copy_block_from(chunk - g.slice(0, d, 3, 6).mul_scalar(x), 0, 3, 0, 0, d, 3)
    assert wide == want
    assert M.gadget_block(p, d, 2, 7, scalar=x_poly, negate=True) == -(g.slice(0, d, 2, 7).mul_scalar(x))
    assert M.gadget_block(p, d, 0, d * 3, small=True) == M.small_gadget_matrix(p, d)
    assert M.gadget_block(p, 1, 0, 3 * 2, level=1).size() == (1, 6)
    rhs = M.from_rns(p, oracle.random_matrix(833, d * k, 3, moduli, n), True)
    add = M.from_rns(p, oracle.random_matrix(834, d, 3, moduli, n), True)
    assert M.gadget_mul(rhs) == g * rhs
    assert M.gadget_mul(rhs, addend=add, negate=True) == add - g * rhs
    coeff = M.from_rns(p, oracle.random_matrix(833, d * k, 3, moduli, n), False)
    out = M.gadget_mul(coeff)
    assert not out.is_ntt and np.array_equal(out.to_rns(), (g * rhs).to_rns())
