"""gpupoly_matrix_mul_decompose_pairs: outs[j] = addends[j] +- (lhss[j] * G^-1(rhss[j][:, window])) o scalars[j], every operand
against its OWN right operand, one gather + one digit transform + one grouped product per 64 operands.

Bit-exact against the CPU restatement (oracle), against the per-request sequence of the existing entry points (copy_block of
the window, gpupoly_matrix_mul_decompose, gpu_matrix_mul_scalar, gpu_matrix_add / _sub / gpupoly_matrix_neg) and, per width
class, against the plain big-integer reference (plainref); every register tile; the operand groups of a small budget; q - 1
operands at the lazy accumulators' bound and one past it; empty shapes; every refusal leaves outputs and the launch trace
alone; the launch count does not grow with the operand count."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_modulus_classes import SEED, _lazy_terms, _moduli, _params, _root

pytestmark = pytest.mark.gpu

# (n, depth, limb bits, base bits): 32-bit words on a tiny ring, 64-bit words, the fused 2^14 digit transform
RINGS = {"n16_18bit": (16, 3, 18, 6), "n256_51bit": (256, 3, 51, 17), "n16384_24bit": (16384, 2, 24, 12)}
# operand heights: two tile heights in one launch, 17 operands, a tile edge with an empty operand, the 65th operand (a
# second launch over the same digit matrix), and the 2- and 4-row tiles of 32-bit words
ROW_LISTS = {"1_4": [1, 4], "16x1_2": [1] * 16 + [2], "9_1_0_3": [9, 1, 0, 3], "65x1": [1] * 65, "2": [2], "3_1": [3, 1]}
POOL_ROWS, POOL_OPS, RHS_ROWS, RHS_COLS, COL_START, WIN = 65, 65, 2, 5, 1, 3
SHAPES = [(1, 1), (2, 3), (1, 3), (2, 1)]  # (r, c): the window [COL_START, COL_START + c) lies inside the 5 columns

_pool = {}


def pool(gpu, oracle, ring):
    """Inputs and CPU references of one ring, computed once and never written: POOL_OPS right operands (every j its own)
    with the digit matrices of their widest window, a pool of left rows, addend rows and three scalars."""
    if ring not in _pool:
        n, depth, bits, base = RINGS[ring]
        p = make_params(gpu, oracle, n, depth, bits, base)
        moduli = p.moduli()
        k = p.modulus_digits()
        B = oracle.random_matrix(930, POOL_OPS * RHS_ROWS, RHS_COLS, moduli, n).reshape(POOL_OPS, RHS_ROWS, RHS_COLS, depth, n)
        B_eval = oracle.matrix_ntt(B.reshape(POOL_OPS * RHS_ROWS, RHS_COLS, depth, n), moduli).reshape(B.shape)
        win = np.ascontiguousarray(B[:, :, COL_START:COL_START + WIN]).reshape(POOL_OPS * RHS_ROWS, WIN, depth, n)
        # G^-1 works entry by entry: row (j RHS_ROWS + i) k + e of the stacked decomposition is digit row i k + e of operand j
        D = oracle.matrix_ntt(oracle.decompose(win, moduli, base), moduli).reshape(POOL_OPS, RHS_ROWS * k, WIN, depth, n)
        S = oracle.random_matrix(931, POOL_ROWS, RHS_ROWS * k, moduli, n)
        A = oracle.random_matrix(932, POOL_ROWS, WIN, moduli, n)
        sc = oracle.random_matrix(933, 3, 1, moduli, n)
        for a in (B, B_eval, D, S, A, sc):
            a.setflags(write=False)
        _pool[ring] = dict(p=p, moduli=moduli, base=base, n=n, k=k, B=B, B_eval=B_eval, D=D, S=S, A=A, sc=sc, dev={})
    return _pool[ring]


def rhs_dev(gpu, P_, j, eval_form):
    """right operand j on the device (all RHS_ROWS rows), uploaded once per form and never written"""
    key = (j, eval_form)
    if key not in P_["dev"]:
        P_["dev"][key] = gpu.GpuDCRTPolyMatrix.from_rns(P_["p"], P_["B_eval" if eval_form else "B"][j], eval_form)
    return P_["dev"][key]


def mulmod(a, s, moduli):
    """a o s mod q in exact integer arithmetic; a: (rows, cols, L, n), s: (L, n)"""
    q = np.array([int(m) for m in moduli], dtype=object).reshape(1, 1, -1, 1)
    if max(int(m) for m in moduli) < 1 << 31:  # products below 2^62: exact in 64-bit integers
        return (a.astype(np.uint64) * s.astype(np.uint64)[None, None]) % q.astype(np.uint64)
    return ((a.astype(object) * s.astype(object)[None, None]) % q).astype(np.uint64)


def combine(addend, prod, negate, moduli):
    """addend +- prod, both below q < 2^62 (addend None: +- prod alone)"""
    q = np.array([int(m) for m in moduli], dtype=np.uint64).reshape(1, 1, -1, 1)
    term = (q - prod) % q if negate else prod
    return term if addend is None else (addend + term) % q


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag (a tag mismatch is 'not equal' there)"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value) or a.nrow * a.ncol == 0


def raw_call(outs, adds, lhss, rhss, scs, col_start, base, negate=0):
    from mxx_amd import _ffi

    n = len(outs)
    arr = lambda ms: (C.c_void_p * n)(*[None if m is None else m.raw.value for m in ms])  # noqa: E731
    return _ffi.lib().gpupoly_matrix_mul_decompose_pairs(arr(outs), arr(adds), arr(lhss), arr(rhss), arr(scs), n, col_start, base, negate)


def sequence(l_, rhs, col_start, c, s_, a_, negate):
    """the per-request sequence of the existing entry points"""
    out = l_.mul_decompose(rhs.slice_columns(col_start, col_start + c))
    if s_ is not None:
        out = out.mul_scalar(s_)
    if a_ is not None:
        return a_ - out if negate else a_ + out
    return -out if negate else out


def traced(gpu, fn):
    from mxx_amd import _ffi

    gpu.gpu_device_sync()
    _ffi.trace_begin()
    out = fn()
    gpu.gpu_device_sync()
    return out, _ffi.trace_end()


@pytest.mark.parametrize("rhs_eval", [False, True], ids=["rhs_coeff", "rhs_eval"])
@pytest.mark.parametrize("rows_id", list(ROW_LISTS))
@pytest.mark.parametrize("ring", list(RINGS))
def test_bit_exact_against_the_cpu_restatement(gpu, oracle, ring, rows_id, rhs_eval):
    """every j has its own right operand: a kernel that read operand 0's panel for every j fails here"""
    P_ = pool(gpu, oracle, ring)
    p, moduli, k = P_["p"], P_["moduli"], P_["k"]
    M = gpu.GpuDCRTPolyMatrix
    rows = ROW_LISTS[rows_id]
    for r, c in SHAPES:
        negate = (len(rows) + r + c) % 2 == 1
        lhss, adds, scs, rhss, want = [], [], [], [], []
        r0 = 0
        for j, h in enumerate(rows):
            sl = slice(r0, r0 + h)
            r0 += h
            lhs = np.ascontiguousarray(P_["S"][sl, : r * k])
            lhss.append(M.from_rns(p, lhs, True))
            full = rhs_dev(gpu, P_, j, rhs_eval)
            rhss.append(full if r == RHS_ROWS else full.row_view(0, r))
            w = oracle.matmul(lhs, np.ascontiguousarray(P_["D"][j, : r * k, :c]), moduli) if h else np.zeros((0, c) + lhs.shape[2:], dtype=np.uint64)
            if (j + len(rows)) % 2 == 0:  # scalar / none and addend / none mixed within the call
                s = P_["sc"][j % 3]
                scs.append(M.from_rns(p, s[None], True))
                w = mulmod(w, s[0], moduli)
            else:
                scs.append(None)
            if (j + len(rows)) % 3 != 0:
                a = np.ascontiguousarray(P_["A"][sl, :c])
                adds.append(M.from_rns(p, a, True))
            else:
                a = None
                adds.append(None)
            want.append(combine(a, w, negate, moduli))
        outs = M.mul_decompose_pairs(lhss, rhss, COL_START, c, scalars=scs, addends=adds, negate=negate)
        assert len(outs) == len(rows)
        for j, (o, w) in enumerate(zip(outs, want)):
            assert o.size() == (rows[j], c) and o.is_ntt
            assert np.array_equal(o.to_rns(), w), f"operand {j} of {rows}, r={r}, c={c}, negate={negate}"


@pytest.mark.parametrize("ring", list(RINGS))
def test_mixed_forms_of_the_right_operands_in_one_call(gpu, oracle, ring):
    P_ = pool(gpu, oracle, ring)
    p, moduli, k = P_["p"], P_["moduli"], P_["k"]
    M = gpu.GpuDCRTPolyMatrix
    lhss = [M.from_rns(p, np.ascontiguousarray(P_["S"][j:j + 1]), True) for j in range(5)]
    rhss = [rhs_dev(gpu, P_, j, j % 2 == 1) for j in range(5)]
    outs = M.mul_decompose_pairs(lhss, rhss, COL_START, WIN)
    for j, o in enumerate(outs):
        assert np.array_equal(o.to_rns(), oracle.matmul(np.ascontiguousarray(P_["S"][j:j + 1]), np.ascontiguousarray(P_["D"][j]), moduli)), j
        assert rhss[j].is_ntt == (j % 2 == 1)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("ring", ["n16_18bit", "n256_51bit"])
def test_a_level_below_the_top(gpu, oracle, ring, level):
    """Every matrix of the call at level 0 / 1 of the three-limb rings, through the raw entry (the mirror takes k from the
    context): k = dpt * (level + 1) with dpt from the CONTEXT's crt_bits, the module's CPU restatement at the truncated basis
    (same-width limbs: oracle.decompose derives the same dpt from it); own right operand per j, both forms, scalar and
    addend mixed, both signs."""
    n, depth, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    dpt = -(-p.crt_bits() // base)
    assert level < depth - 1 and oracle.digits_per_tower(moduli, base) == dpt
    k = dpt * (level + 1)
    rows = [2, 1, 0, 9, 3]
    sc = oracle.random_matrix(943, 1, 1, moduli, n)
    for negate in (0, 1):
        lhss, adds, scs, rhss, outs, want = [], [], [], [], [], []
        for j, h in enumerate(rows):
            B = oracle.random_matrix(940 + 7 * j + level, RHS_ROWS, RHS_COLS, moduli, n)
            D = oracle.matrix_ntt(oracle.decompose(np.ascontiguousarray(B[:, COL_START:COL_START + WIN]), moduli, base), moduli)
            S = oracle.random_matrix(941 + 7 * j + level, h, RHS_ROWS * k, moduli, n)
            A = oracle.random_matrix(942 + 7 * j + level, h, WIN, moduli, n)
            lhss.append(M.from_rns(p, S, True))
            rhss.append(M.from_rns(p, oracle.matrix_ntt(B, moduli) if j % 2 else B, j % 2 == 1))
            w = oracle.matmul(S, D, moduli) if h else np.zeros((0, WIN, level + 1, n), dtype=np.uint64)
            scs.append(M.from_rns(p, sc, True) if j % 2 == 0 else None)
            if j % 2 == 0:
                w = mulmod(w, sc[0, 0], moduli)
            adds.append(M.from_rns(p, A, True) if j % 3 != 0 else None)
            want.append(combine(A if j % 3 != 0 else None, w, negate, moduli))
            outs.append(M(p, h, WIN, level, False))
        assert raw_call(outs, adds, lhss, rhss, scs, COL_START, base, negate) == 0
        for j, (o, w) in enumerate(zip(outs, want)):
            o.is_ntt = True  # tagged EVAL by the entry: the store refuses any other tag
            assert o.level == level and np.array_equal(o.to_rns(), w), f"operand {j} of {rows} at level {level}, negate={negate}"


@pytest.mark.parametrize("rhs_eval", [False, True], ids=["rhs_coeff", "rhs_eval"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_bit_exact_against_the_existing_entry_points_and_inputs_untouched(gpu, oracle, ring, rhs_eval):
    """scalar / none x addend / none / addend is out, mixed within one call, for both signs"""
    P_ = pool(gpu, oracle, ring)
    p, k, base = P_["p"], P_["k"], P_["base"]
    M = gpu.GpuDCRTPolyMatrix
    rows = [2, 1, 3, 1, 9, 2, 0]
    c = WIN
    for negate in (0, 1):
        lhss, adds, scs, rhss, outs, seq = [], [], [], [], [], []
        r0 = 0
        for j, h in enumerate(rows):
            sl = slice(r0, r0 + h)
            r0 += h
            lhss.append(M.from_rns(p, np.ascontiguousarray(P_["S"][sl]), True))
            rhss.append(rhs_dev(gpu, P_, j, rhs_eval))
            scs.append(M.from_rns(p, P_["sc"][j % 3][None], True) if j % 2 == 0 else None)
            mode = j % 3  # 0: no addend, 1: a separate addend, 2: the addend is the output
            a = None if mode == 0 else M.from_rns(p, np.ascontiguousarray(P_["A"][sl]), True)
            # outputs hold other residues under the COEFF tag before the call
            outs.append(a if mode == 2 else M.from_rns(p, np.ascontiguousarray(P_["A"][10 + r0 - h:10 + r0]), False))
            adds.append(a)
            seq.append(sequence(lhss[j], rhss[j], COL_START, c, scs[j], a, negate))
        inputs = [m for j, m in enumerate(lhss + scs + rhss + [a for j, a in enumerate(adds) if j % 3 == 1]) if m is not None]
        before = [m.clone() for m in inputs]
        assert raw_call(outs, adds, lhss, rhss, scs, COL_START, base, negate) == 0
        for o in outs:
            o._touch()
            o.is_ntt = True
        for m, b in zip(inputs, before):  # residues and format tags as they were
            assert raw_same(m, b)
        for j in range(len(rows)):
            assert rhss[j].is_ntt == rhs_eval
            assert raw_same(outs[j], seq[j]), f"operand {j}, negate={negate}"


# shapes that reach every register tile: for 32-bit words the height follows the tallest operand of the launch (1, 2, 4 and 8
# rows; a digit matrix above 256 MB under one row tile per operand is streamed with non-temporal loads); for 64-bit words
# stacked_tile's rule of how far rows x columns fill the chip, asked with all rows of the launch, clamped to the tallest
# operand.  The operands are samples (PACKED24 where the ring allows it: unpacked first).
@pytest.mark.parametrize("ring,depth,rows,r,c,tile", [
    ("n256_51bit", 12, [4] * 43 + [3], 1, 8, "u64,4,4,2"), ("n256_51bit", 12, [3] * 58, 1, 8, "u64,2,4,2"),
    ("n256_51bit", 12, [1] * 64, 1, 24, "u64,1,4,2"), ("n256_51bit", 12, [2] * 42 + [1, 2], 1, 2, "u64,2,2,1"),
    ("n256_51bit", 12, [1] * 43, 1, 4, "u64,1,1,1"), ("n256_51bit", 12, [2, 1], 1, 3, "u64,1,1,1"),
    ("n16384_24bit", 2, [1] * 44, 2, 6, "u32,1,8,4"), ("n16384_24bit", 2, [2, 1], 1, 3, "u32,2,8,4"),
    ("n16384_24bit", 2, [3, 1, 4], 1, 3, "u32,4,8,1"), ("n16384_24bit", 2, [5, 9, 1], 1, 3, "u32,8,8,1"),
], ids=["u64_4x4x2", "u64_2x4x2", "u64_1x4x2", "u64_2x2x1", "u64_1x1x1_one_row", "u64_1x1x1", "u32_1x8x4_streamed_once", "u32_2x8x4",
        "u32_4x8x1", "u32_8x8x1"])
def test_every_tile_matches_the_per_request_sequence(gpu, oracle, ring, depth, rows, r, c, tile):
    n, _, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    us, dist = gpu.GpuDCRTPolyUniformSampler(), gpu.DistType.FinRingDist()
    k = p.modulus_digits()
    M = gpu.GpuDCRTPolyMatrix
    m = c + 2
    rhss = [us.sample_uniform(p, r, m, dist) for _ in rows]
    lhss = [us.sample_uniform(p, h, r * k, dist) for h in rows]
    adds = [us.sample_uniform(p, h, c, dist) if j % 3 else None for j, h in enumerate(rows)]
    scs = [us.sample_uniform(p, 1, 1, dist) if j % 2 == 0 else None for j in range(len(rows))]
    outs = M.mul_decompose_pairs(lhss, rhss, 1, c, scalars=scs, addends=adds, negate=True)
    assert tile in p.ctx().last_kernel(), p.ctx().last_kernel()
    for j in range(len(rows)):
        assert outs[j] == sequence(lhss[j], rhss[j], 1, c, scs[j], adds[j], True), f"operand {j}"


@pytest.mark.parametrize("ring", list(RINGS))
def test_operand_groups_give_the_uncut_result(gpu, oracle, hip_env, ring):
    n, depth, bits, base = RINGS[ring]
    P_ = pool(gpu, oracle, ring)
    p, k = P_["p"], P_["k"]
    M = gpu.GpuDCRTPolyMatrix
    rows = [1, 4, 0, 9, 1, 3]
    lhss, adds, scs, r0 = [], [], [], 0
    for j, h in enumerate(rows):
        lhss.append(M.from_rns(p, np.ascontiguousarray(P_["S"][r0:r0 + h]), True))
        adds.append(None if j % 3 == 0 else M.from_rns(p, np.ascontiguousarray(P_["A"][r0:r0 + h]), True))
        scs.append(M.from_rns(p, P_["sc"][j % 3][None], True) if j % 2 == 1 else None)
        r0 += h
    poly_bytes = depth * n * p.ctx().word_bytes()
    for rhs_eval in (False, True):
        rhss = [rhs_dev(gpu, P_, j, rhs_eval) for j in range(len(rows))]
        whole, recs_whole = traced(gpu, lambda: M.mul_decompose_pairs(lhss, rhss, COL_START, WIN, scalars=scs, addends=adds, negate=True))
        # room for the digit matrix of two operands: the five operands with rows go in groups of 2, 2 and 1
        hip_env.set("MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET", str(2 * RHS_ROWS * k * WIN * poly_bytes + poly_bytes // 2))
        cut, recs_cut = traced(gpu, lambda: M.mul_decompose_pairs(lhss, rhss, COL_START, WIN, scalars=scs, addends=adds, negate=True))
        hip_env.unset("MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET")
        count = lambda recs: sum("matmul_pairs_kernel" in x["kernel"] for x in recs)  # noqa: E731
        assert (count(recs_whole), count(recs_cut)) == (1, 3), (recs_whole, recs_cut)
        for j, (w, g) in enumerate(zip(whole, cut)):
            assert raw_same(w, g), f"operand {j}, rhs_eval={rhs_eval}"
            assert raw_same(w, sequence(lhss[j], rhss[j], COL_START, WIN, scs[j], adds[j], True)), f"operand {j} against the sequence"


# ---- worst-case inputs at the lazy accumulators' bound ---------------------------------------------------------------------
# One limb, base_bits = the limb's width, so a residue is its own single digit: a right operand whose every entry is the
# constant q - 1 has the constant q - 1 as digit polynomial, which is its own transform - every product entering an
# accumulator is (q - 1)^2, the largest there is, and the inner dimension r is exactly the number of products.  (A residue
# whose base-2^b digits are all ones, 2^bits - 1, is not below q; with several digits per residue, below, the low digits are
# all ones and the top digit is the largest that keeps the residue below q.)  lazy_terms = (2^acc - q) / (q - 1)^2.
@pytest.mark.parametrize("bits", [31, 62])
@pytest.mark.parametrize("past", [0, 1], ids=["at_the_bound", "one_past"])
def test_worst_case_inputs_at_the_lazy_bound(gpu, bits, past):
    n = 256
    q = P.primes(n, bits, 1)[0]
    lazy = _lazy_terms(q, bits > 31)
    assert lazy == (4 if bits == 31 else 16)
    M = gpu.GpuDCRTPolyMatrix

    def full(rows, cols, value):
        return np.full((rows, cols, 1, n), value, dtype=np.uint64)

    def const(rows, cols, value):
        a = np.zeros((rows, cols, 1, n), dtype=np.uint64)
        a[..., 0] = value
        return a

    for base, dpt in ((bits, 1), (bits // 2 + 1, 2)):
        p = _params(gpu, n, [q], base)
        assert p.modulus_digits() == dpt
        inner = lazy + past
        r = -(-inner // dpt)
        if r * dpt != inner:  # two digits per residue: the inner dimension moves in steps of two, to the bound or just past it
            assert dpt == 2 and r * dpt == inner + 1 and past == 1
        # the largest residue below q whose low digit is all ones (dpt = 1: q - 1 itself)
        top = q - 1 if dpt == 1 else ((((q - 1) >> base) - 1) << base) | ((1 << base) - 1)
        assert top < q
        digit_sum = sum((top >> (e * base)) & ((1 << base) - 1) for e in range(dpt))  # per source row, digits are constants
        prod = (q - 1) * r * digit_sum % q
        for rows, c in ((1, 1), (3, 2)):
            lhss = [M.from_rns(p, full(rows, r * dpt, q - 1), True) for _ in range(2)]
            # the constant polynomial `top` in either form: coefficient 0 alone, or the same value in every slot
            rhss = [M.from_rns(p, const(r, c + 1, top), False), M.from_rns(p, full(r, c + 1, top), True)]
            scs = [M.from_rns(p, full(1, 1, q - 1), True), None]
            adds = [M.from_rns(p, full(rows, c, q - 3), True), None]
            for negate in (False, True):
                outs = M.mul_decompose_pairs(lhss, rhss, 1, c, scalars=scs, addends=adds, negate=negate)
                t0 = prod * (q - 1) % q
                want0 = (q - 3 - t0) % q if negate else (q - 3 + t0) % q
                want1 = (q - prod) % q if negate else prod
                assert (outs[0].to_rns() == np.uint64(want0)).all(), (bits, base, inner, rows, c, negate)
                assert (outs[1].to_rns() == np.uint64(want1)).all(), (bits, base, inner, rows, c, negate)


# ---- width classes against the plain big-integer reference -----------------------------------------------------------------
@pytest.mark.parametrize("bits,base", [(24, 12), (31, 16), (33, 11), (51, 17), (62, 31)])
def test_width_classes_against_plainref(gpu, bits, base):
    """Two operands (1 and 2 rows) with their own 2 x 4 right operands, window [1, 4): the two largest and two smallest primes of
    the class in one context.  Expected from plainref alone: P.digits of the window's coefficients, taken to the sampled slots
    by P.ntt_slots, under P.slot_mul_sum with the scalar and addend terms in exact integers; and for the bare product the
    coefficients 0, 1 and n - 1 of entry (0, 0) by P.ring_matmul_coeffs on the inverse-transformed operands."""
    n = 256
    moduli = _moduli(n, bits)
    L = len(moduli)
    p = _params(gpu, n, moduli, base)
    M = gpu.GpuDCRTPolyMatrix
    dpt = P.digits_per_tower(moduli, base)
    k, r, m, cs, c = L * dpt, 2, 4, 1, 3
    assert p.modulus_digits() == k
    rng = np.random.default_rng(SEED + 7000 + bits)
    slots = sorted({0, 1, n - 1} | set(rng.choice(np.arange(2, n - 1), 5, replace=False).tolist()))
    rand = lambda rows, cols: np.stack([rng.integers(0, int(q), (rows, cols, n), dtype=np.uint64) for q in moduli], axis=2)  # noqa: E731
    top = np.asarray([q - 1 for q in moduli], dtype=np.uint64).reshape(1, 1, L, 1)
    qobj = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, -1, 1)
    Bc = [rand(r, m), rand(r, m)]
    Bc[1][0, cs] = np.broadcast_to(top[0, 0], (L, n))  # every coefficient q - 1
    digs, D = [], []
    for B in Bc:
        dig = np.zeros((r * k, c, L, n), dtype=np.uint64)
        for i in range(r):
            for cc in range(c):
                dig[i * k:(i + 1) * k, cc] = P.digits(B[i, cs + cc], moduli, base, dpt)
        digs.append(dig)
        flat = dig.reshape(-1, n)
        ms = [int(moduli[i % L]) for i in range(flat.shape[0])]
        D.append(P.ntt_slots(flat, ms, slots, [_root(q, n) for q in ms]).reshape(r * k, c, L, len(slots)))
    S = [rand(1, r * k), rand(2, r * k)]
    S[1][1, :dpt] = np.broadcast_to(top[0], (dpt, L, n))
    AD = rand(2, c)
    AD[0, 0] = np.broadcast_to(top[0, 0], (L, n))
    SC = rand(1, 1)
    SC[0, 0, :, slots[0]] = [q - 1 for q in moduli]
    up = lambda a, ev=True: M.from_rns(p, np.ascontiguousarray(a), ev)  # noqa: E731
    dS, dB = [up(s) for s in S], [up(Bc[0], False), up(Bc[1], False)]
    for negate in (False, True):
        # operand 0 bare; operand 1 with scalar and addend
        outs = M.mul_decompose_pairs(dS, dB, cs, c, scalars=[None, up(SC)], addends=[None, up(AD)], negate=negate)
        want0 = P.slot_mul_sum(None, [S[0][..., slots]], [D[0]], moduli, negate)
        assert np.array_equal(outs[0].to_rns()[..., slots], want0), (bits, negate, p.ctx().last_kernel())
        prod1 = P.slot_mul_sum(None, [S[1][..., slots]], [D[1]], moduli, False).astype(object)
        term = (prod1 * SC[..., slots].astype(object)) % qobj
        a = AD[..., slots].astype(object)
        want1 = ((a - term) % qobj if negate else (a + term) % qobj).astype(np.uint64)
        assert np.array_equal(outs[1].to_rns()[..., slots], want1), (bits, negate, p.ctx().last_kernel())
    # the bare product in the coefficient domain, from the defining negacyclic sums
    out = M.mul_decompose_pairs(dS[:1], dB[:1], cs, c)[0]
    idx = [0, 1, n - 1]
    ref = P.ring_matmul_coeffs(dS[0].to_coeff_rns(), digs[0], moduli, [(0, 0), (0, c - 1)], idx)
    got = out.to_coeff_rns()
    for (i, cc, l), vals in ref.items():
        assert [int(got[i, cc, l, x]) for x in idx] == [int(v) for v in vals], (bits, i, cc, l)


def test_empty_shapes(gpu, oracle):
    P_ = pool(gpu, oracle, "n256_51bit")
    p, k, moduli = P_["p"], P_["k"], P_["moduli"]
    M = gpu.GpuDCRTPolyMatrix
    lvl = p.crt_depth() - 1
    assert M.mul_decompose_pairs([], [], 0, 0) == []
    # r * k = 0: the addend term alone, the negated zero product without one
    rhs0 = [M(p, 0, RHS_COLS, lvl, True) for _ in range(3)]
    lhs0 = [M(p, 2, 0, lvl, True), M(p, 1, 0, lvl, True), M(p, 3, 0, lvl, True)]
    adds = [M.from_rns(p, np.ascontiguousarray(P_["A"][0:2]), True), None, M.from_rns(p, np.ascontiguousarray(P_["A"][2:5]), True)]
    scs = [M.from_rns(p, P_["sc"][0][None], True), None, None]
    outs = M.mul_decompose_pairs(lhs0, rhs0, COL_START, WIN, scalars=scs, addends=adds, negate=True)
    assert np.array_equal(outs[0].to_rns(), P_["A"][0:2])
    assert not outs[1].to_rns().any()
    assert np.array_equal(outs[2].to_rns(), P_["A"][2:5])
    # no columns, and only operands of height 0: nothing to launch
    two_rows = M.from_rns(p, np.ascontiguousarray(P_["S"][0:2]), True)
    _, recs = traced(gpu, lambda: M.mul_decompose_pairs([two_rows], [rhs_dev(gpu, P_, 0, True)], 2, 0))
    assert recs == []
    (out,), recs = traced(gpu, lambda: M.mul_decompose_pairs([M(p, 0, RHS_ROWS * k, lvl, True)], [rhs_dev(gpu, P_, 0, False)], COL_START, WIN))
    assert out.size() == (0, WIN) and out.is_ntt and recs == []
    # an operand of height 0 between two others
    lhss = [two_rows, M(p, 0, RHS_ROWS * k, lvl, True), M.from_rns(p, np.ascontiguousarray(P_["S"][2:3]), True)]
    outs = M.mul_decompose_pairs(lhss, [rhs_dev(gpu, P_, j, False) for j in range(3)], COL_START, WIN)
    assert outs[1].size() == (0, WIN)
    assert np.array_equal(outs[2].to_rns(), oracle.matmul(np.ascontiguousarray(P_["S"][2:3]), np.ascontiguousarray(P_["D"][2]), moduli))


REFUSALS = ["shape_mismatch_in_operand_2", "coeff_lhs_1", "coeff_scalar", "differing_c", "window_past_m", "out0_is_lhs1",
            "out0_is_a_shifted_row_view_of_rhs1s_parent", "same_output_twice", "addend_overlaps_its_output_by_one_row", "base_bits_zero",
            "base_bits_63"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing_and_leave_every_output_as_it_was(gpu, oracle, case):
    from mxx_amd import _ffi

    P_ = pool(gpu, oracle, "n256_51bit")
    p, base, k, moduli, n = P_["p"], P_["base"], P_["k"], P_["moduli"], P_["n"]
    M = gpu.GpuDCRTPolyMatrix
    rows = [1, 1, 2, 1]
    r, m, c, col_start = RHS_ROWS, RHS_COLS, WIN, COL_START
    if case == "out0_is_lhs1":  # an output row as wide as a left operand: c = m = r k with r = 1
        r, m, c, col_start = 1, k, k, 0
    elif case == "out0_is_a_shifted_row_view_of_rhs1s_parent":  # an output row as wide as a right operand's row
        m, c, col_start = WIN, WIN, 0
    rnd = lambda seed, rr, cc: oracle.random_matrix(seed, rr, cc, moduli, n)  # noqa: E731
    lhss = [M.from_rns(p, np.ascontiguousarray(P_["S"][j:j + h, : r * k]), True) for j, h in enumerate(rows)]
    rhss = [M.from_rns(p, rnd(940 + j, r, m), j % 2 == 0) for j in range(4)]
    adds = [M.from_rns(p, rnd(950 + j, h, c), True) for j, h in enumerate(rows)]
    scs = [M.from_rns(p, P_["sc"][j % 3][None], True) for j in range(4)]
    # outputs hold known residues under the COEFF tag: a refused call must leave both
    outs = [M.from_rns(p, rnd(960 + j, h, c), False) for j, h in enumerate(rows)]
    extra = []  # further blocks that must stay as they were
    if case == "shape_mismatch_in_operand_2":
        lhss[2] = M.from_rns(p, np.ascontiguousarray(P_["S"][0:2, : r * k - 1]), True)
    elif case == "coeff_lhs_1":
        lhss[1] = M.from_rns(p, np.ascontiguousarray(P_["S"][1:2]), False)
    elif case == "coeff_scalar":
        scs[3] = M.from_rns(p, P_["sc"][0][None], False)
    elif case == "differing_c":
        outs[2] = M.from_rns(p, rnd(970, 2, c - 1), False)
        adds[2] = None
    elif case == "window_past_m":
        col_start = m - c + 1
    elif case == "out0_is_lhs1":
        outs[0] = M.from_rns(p, rnd(971, 1, c), True)
        lhss[1] = outs[0]
    elif case == "out0_is_a_shifted_row_view_of_rhs1s_parent":
        parent = M.from_rns(p, rnd(972, r + 1, m), False)
        rhss[1] = parent.row_view(0, r)
        outs[0] = parent.row_view(r - 1, r)  # its one row is the last row of rhss[1]
        adds[0] = None
        extra.append(parent)
    elif case == "same_output_twice":
        outs[3] = outs[1]
    elif case == "addend_overlaps_its_output_by_one_row":
        parent = M.from_rns(p, rnd(973, 3, c), True)
        outs[2], adds[2] = parent.row_view(0, 2), parent.row_view(1, 3)
        extra.append(parent)
    distinct = list({o.raw.value: o for o in outs + extra}.values())
    before = [(o, o.clone()) for o in distinct]
    bb = 0 if case == "base_bits_zero" else (63 if case == "base_bits_63" else base)
    rc, recs = traced(gpu, lambda: raw_call(outs, adds, lhss, rhss, scs, col_start, bb, 1))
    assert recs == [], "a refused call launched a kernel"
    msg = _ffi.last_error_string()
    assert rc != 0 and "gpupoly_matrix_mul_decompose_pairs" in msg, msg
    if case in ("out0_is_lhs1", "out0_is_a_shifted_row_view_of_rhs1s_parent", "same_output_twice", "addend_overlaps_its_output_by_one_row"):
        assert "alias" in msg, msg
    for o, b in before:
        assert raw_same(o, b), f"{case}: an output changed (residues or tag)"


def test_an_addend_that_is_its_outputs_block_through_another_view_is_accepted(gpu, oracle):
    """the one exception to the overlap rule: addends[j] and outs[j] are two row views of the same rows"""
    P_ = pool(gpu, oracle, "n16_18bit")
    p = P_["p"]
    M = gpu.GpuDCRTPolyMatrix
    stack = M.from_rns(p, np.ascontiguousarray(P_["A"][0:3]), True)
    keep = stack.clone()
    lhss = [M.from_rns(p, np.ascontiguousarray(P_["S"][0:2]), True), M.from_rns(p, np.ascontiguousarray(P_["S"][2:3]), True)]
    rhss = [rhs_dev(gpu, P_, 0, False), rhs_dev(gpu, P_, 1, True)]
    outs = [stack.row_view(0, 2), stack.row_view(2, 3)]
    adds = [stack.row_view(0, 2), stack.row_view(2, 3)]
    M.mul_decompose_pairs(lhss, rhss, COL_START, WIN, addends=adds, negate=True, outs=outs)
    for j, (lo, hi) in enumerate(((0, 2), (2, 3))):
        assert raw_same(stack.row_view(lo, hi), sequence(lhss[j], rhss[j], COL_START, WIN, None, keep.row_view(lo, hi), True)), j


def test_launches_do_not_grow_with_the_operand_count(gpu, oracle):
    n, depth, bits, base = 256, 12, 51, 17  # the launch-bound GGH15 ring
    p = make_params(gpu, oracle, n, depth, bits, base)
    us, dist = gpu.GpuDCRTPolyUniformSampler(), gpu.DistType.FinRingDist()
    k = p.modulus_digits()
    M = gpu.GpuDCRTPolyMatrix
    count = 65
    rhss = [us.sample_uniform(p, 2, 2 * k, dist) for _ in range(count)]
    for m in rhss[1::2]:
        m.intt_all_in_place()  # right operands of both forms in every call
    lhss = [us.sample_uniform(p, 2, 2 * k, dist) for _ in range(count)]
    adds = [us.sample_uniform(p, 2, 4, dist) for _ in range(count)]
    scs = [us.sample_uniform(p, 1, 1, dist) for _ in range(count)]
    call = lambda t: M.mul_decompose_pairs(lhss[:t], rhss[:t], 4, 4, scalars=scs[:t], addends=adds[:t], negate=True)  # noqa: E731
    call(2)  # warm
    two, recs2 = traced(gpu, lambda: call(2))
    _, recs48 = traced(gpu, lambda: call(48))
    all65, recs65 = traced(gpu, lambda: call(65))
    seq, recs_seq = traced(gpu, lambda: sequence(lhss[0], rhss[0], 4, 4, scs[0], adds[0], True))
    print(f"launches: 2 operands {len(recs2)}, 48 operands {len(recs48)}, 65 operands {len(recs65)}, one per-request sequence {len(recs_seq)}")
    assert len(recs2) == len(recs48), ([x["kernel"] for x in recs2], [x["kernel"] for x in recs48])
    assert len(recs65) == len(recs48) + 1, [x["kernel"] for x in recs65]
    assert two[0] == seq and all65[0] == seq
    assert all65[64] == sequence(lhss[64], rhss[64], 4, 4, scs[64], adds[64], True)
