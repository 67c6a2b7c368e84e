"""gpupoly_matrix_mul_decompose_many: outs[j] = lhss[j] * G^-1(rhs) + addends[j] o scalars[j] with G^-1(rhs) built once.

Bit-exact against the CPU restatement (oracle) and against the per-operand sequence of the existing entry points
(gpupoly_matrix_mul_decompose, gpu_matrix_mul_scalar, gpu_matrix_add); inputs untouched; the multi-chunk path; every
refusal leaves outputs and the launch counter alone; one call's launch count does not grow with the operand count."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

# (n, depth, limb bits, base bits): 32-bit words on a tiny ring, 64-bit words, the fused 2^14 digit transform
RINGS = {"n16_18bit": (16, 3, 18, 6), "n256_51bit": (256, 3, 51, 17), "n16384_24bit": (16384, 2, 24, 12)}
# operand heights: a tile edge (5 and 13 stacked rows against 8-row tiles), an empty operand, three row tiles, a second
# group of 64 (the 65th operand), and the 1-, 2- and 4-row tiles of 32-bit words
ROW_LISTS = {"1_4": [1, 4], "16x1_2": [1] * 16 + [2], "9_1_0_3": [9, 1, 0, 3], "65x1": [1] * 65, "2": [2], "3_1": [3, 1]}
POOL_ROWS, RHS_ROWS, RHS_COLS = 65, 2, 3

_pool = {}


def pool(gpu, oracle, ring):
    """Inputs and CPU references of one ring, computed once and never written: a pool of POOL_ROWS left rows with their
    products against G^-1(B), as many addend rows, three scalars."""
    if ring not in _pool:
        n, depth, bits, base = RINGS[ring]
        p = make_params(gpu, oracle, n, depth, bits, base)
        moduli = p.moduli()
        k = p.modulus_digits()
        B = oracle.random_matrix(900, RHS_ROWS, RHS_COLS, moduli, n)  # read as coefficients
        D = oracle.matrix_ntt(oracle.decompose(B, moduli, base), moduli)
        S = oracle.random_matrix(901, POOL_ROWS, RHS_ROWS * k, moduli, n)
        A = oracle.random_matrix(902, POOL_ROWS, RHS_COLS, moduli, n)
        sc = oracle.random_matrix(903, 3, 1, moduli, n)
        prod = oracle.matmul(S, D, moduli)
        for a in (B, D, S, A, sc, prod):
            a.setflags(write=False)
        _pool[ring] = dict(p=p, moduli=moduli, base=base, n=n, B=B, B_eval=oracle.matrix_ntt(B, moduli), S=S, A=A, sc=sc, prod=prod)
    return _pool[ring]


def addend_term(a, s, moduli):
    """a o s mod q in exact integer arithmetic; a: (rows, cols, L, n), s: (L, n)"""
    q = np.array([int(m) for m in moduli], dtype=object).reshape(1, 1, -1, 1)
    if max(int(m) for m in moduli) < 1 << 31:  # products below 2^62: exact in 64-bit integers
        return (a.astype(np.uint64) * s.astype(np.uint64)[None, None]) % q.astype(np.uint64)
    return ((a.astype(object) * s.astype(object)[None, None]) % q).astype(np.uint64)


def add_mod(x, y, moduli):
    q = np.array([int(m) for m in moduli], dtype=np.uint64).reshape(1, 1, -1, 1)
    return (x + y) % q  # both below q < 2^62


def operands(gpu, P, rows, mode_of):
    """device operands cut from the pool, and the expected outputs; mode 0: no addend, 1: addend, 2: addend o scalar"""
    M = gpu.GpuDCRTPolyMatrix
    lhss, adds, scs, want = [], [], [], []
    r0 = 0
    for j, h in enumerate(rows):
        mode = mode_of(j)
        sl = slice(r0, r0 + h)
        r0 += h
        lhss.append(M.from_rns(P["p"], P["S"][sl], True))
        w = P["prod"][sl]
        if mode == 0:
            adds.append(None)
            scs.append(None)
        else:
            adds.append(M.from_rns(P["p"], P["A"][sl], True))
            if mode == 1:
                scs.append(None)
                w = add_mod(w, P["A"][sl], P["moduli"])
            else:
                s = P["sc"][j % 3]
                scs.append(M.from_rns(P["p"], s[None], True))
                w = add_mod(w, addend_term(P["A"][sl], s[0], P["moduli"]), P["moduli"])
        want.append(w)
    return lhss, adds, scs, want


def sequence(l_, rhs, a_, s_):
    """the per-operand sequence of the existing entry points"""
    out = l_.mul_decompose(rhs)
    if a_ is not None:
        out = out + (a_.mul_scalar(s_) if s_ is not None else a_)
    return out


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag (a tag mismatch is 'not equal' there)"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value) or a.nrow * a.ncol == 0


def raw_call(outs, lhss, adds, scs, rhs, base):
    from mxx_amd import _ffi

    n = len(outs)
    arr = lambda ms: (C.c_void_p * n)(*[None if m is None else m.raw.value for m in ms])
    return _ffi.lib().gpupoly_matrix_mul_decompose_many(arr(outs), arr(lhss), arr(adds), arr(scs), n, rhs.raw, base)


@pytest.mark.parametrize("rhs_eval", [False, True], ids=["rhs_coeff", "rhs_eval"])
@pytest.mark.parametrize("rows_id", list(ROW_LISTS))
@pytest.mark.parametrize("ring", list(RINGS))
def test_bit_exact_against_the_cpu_restatement(gpu, oracle, ring, rows_id, rhs_eval):
    P = pool(gpu, oracle, ring)
    rows = ROW_LISTS[rows_id]
    # the three addend cases mixed within the call, shifted by the operand count so that short lists differ
    lhss, adds, scs, want = operands(gpu, P, rows, lambda j: (j + len(rows)) % 3)
    rhs = gpu.GpuDCRTPolyMatrix.from_rns(P["p"], P["B_eval"] if rhs_eval else P["B"], rhs_eval)
    outs = gpu.GpuDCRTPolyMatrix.mul_decompose_many(lhss, rhs, adds, scs)
    assert len(outs) == len(rows)
    for j, (o, w) in enumerate(zip(outs, want)):
        assert o.size() == (rows[j], RHS_COLS) and o.is_ntt
        assert np.array_equal(o.to_rns(), w), f"operand {j} of {rows}"


@pytest.mark.parametrize("rhs_eval", [False, True], ids=["rhs_coeff", "rhs_eval"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_bit_exact_against_the_existing_entry_points_and_inputs_untouched(gpu, oracle, ring, rhs_eval):
    P = pool(gpu, oracle, ring)
    rows = [9, 1, 0, 3, 2]
    lhss, adds, scs, _ = operands(gpu, P, rows, lambda j: j % 3)
    rhs = gpu.GpuDCRTPolyMatrix.from_rns(P["p"], P["B_eval"] if rhs_eval else P["B"], rhs_eval)
    inputs = [m for m in lhss + adds + scs + [rhs] if m is not None]
    before = [m.clone() for m in inputs]
    outs = gpu.GpuDCRTPolyMatrix.mul_decompose_many(lhss, rhs, adds, scs)
    for m, b in zip(inputs, before):  # residues and format tags as they were
        assert raw_same(m, b)
    assert rhs.is_ntt == rhs_eval
    for j, (l_, a_, s_) in enumerate(zip(lhss, adds, scs)):
        assert raw_same(outs[j], sequence(l_, rhs, a_, s_)), f"operand {j}"


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("rhs_eval", [False, True], ids=["rhs_coeff", "rhs_eval"])
@pytest.mark.parametrize("ring", ["n16_18bit", "n256_51bit"])
def test_a_level_below_the_top(gpu, oracle, ring, rhs_eval, level):
    """Every matrix of the call at level 0 / 1 of the three-limb rings, through the raw entry (the mirror takes k from the
    context): k = dpt * (level + 1) digit rows per source row with dpt from the CONTEXT's crt_bits - the same number in
    these same-width bases as oracle.decompose derives from the truncated basis it is handed."""
    n, depth, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    dpt = -(-p.crt_bits() // base)
    assert level < depth - 1 and oracle.digits_per_tower(moduli, base) == dpt
    k = dpt * (level + 1)
    rows = [3, 1, 0, 9, 2]
    B = oracle.random_matrix(930 + level, RHS_ROWS, RHS_COLS, moduli, n)
    D = oracle.matrix_ntt(oracle.decompose(B, moduli, base), moduli)
    S = oracle.random_matrix(931 + level, sum(rows), RHS_ROWS * k, moduli, n)
    A = oracle.random_matrix(932 + level, sum(rows), RHS_COLS, moduli, n)
    sc = oracle.random_matrix(933 + level, 1, 1, moduli, n)
    prod = oracle.matmul(S, D, moduli)
    lhss, adds, scs, want, r0 = [], [], [], [], 0
    for j, h in enumerate(rows):
        sl = slice(r0, r0 + h)
        r0 += h
        lhss.append(M.from_rns(p, S[sl], True))
        adds.append(None if j % 3 == 0 else M.from_rns(p, A[sl], True))
        scs.append(M.from_rns(p, sc, True) if j % 3 == 2 else None)
        w = prod[sl]
        if j % 3 == 1:
            w = add_mod(w, A[sl], moduli)
        elif j % 3 == 2:
            w = add_mod(w, addend_term(A[sl], sc[0, 0], moduli), moduli)
        want.append(w)
    rhs = M.from_rns(p, oracle.matrix_ntt(B, moduli) if rhs_eval else B, rhs_eval)
    outs = [M(p, h, RHS_COLS, level, False) for h in rows]
    assert raw_call(outs, lhss, adds, scs, rhs, base) == 0
    for j, (o, w) in enumerate(zip(outs, want)):
        o.is_ntt = True  # tagged EVAL by the entry: the store refuses any other tag
        assert o.level == level and np.array_equal(o.to_rns(), w), f"operand {j} of {rows} at level {level}"
    assert np.array_equal(rhs.to_rns(), oracle.matrix_ntt(B, moduli) if rhs_eval else B)


# shapes that reach the tiles the small cases do not: 64-bit words' 4x4x2 / 2x4x2 / 1x4x2 / 2x2x1 register tiles (chosen by
# how far rows x columns fill the chip) and, for 32-bit words, a digit matrix above 256 MB under ONE row tile (streamed with
# non-temporal loads) and under several.  The operands are samples (PACKED24 where the ring allows it: unpacked first).
@pytest.mark.parametrize("ring,depth,rows,rhs_rows,cols", [
    ("n256_51bit", 12, [4, 1], 1, 176), ("n256_51bit", 12, [2, 1], 1, 344), ("n256_51bit", 12, [1], 1, 344),
    ("n256_51bit", 12, [2, 1], 1, 44), ("n16384_24bit", 2, [1], 2, 264), ("n16384_24bit", 2, [5, 4], 2, 264),
], ids=["u64_4x4x2", "u64_2x4x2", "u64_1x4x2", "u64_2x2x1", "u32_streamed_once", "u32_two_row_tiles"])
def test_every_tile_matches_the_per_operand_sequence(gpu, oracle, ring, depth, rows, rhs_rows, cols):
    n, _, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    us, dist = gpu.GpuDCRTPolyUniformSampler(), gpu.DistType.FinRingDist()
    k = p.modulus_digits()
    rhs = us.sample_uniform(p, rhs_rows, cols, dist)
    lhss = [us.sample_uniform(p, h, rhs_rows * k, dist) for h in rows]
    adds = [us.sample_uniform(p, h, cols, dist) for h in rows]
    scs = [us.sample_uniform(p, 1, 1, dist) if j % 2 == 0 else None for j in range(len(rows))]
    outs = gpu.GpuDCRTPolyMatrix.mul_decompose_many(lhss, rhs, adds, scs)
    for j, (l_, a_, s_) in enumerate(zip(lhss, adds, scs)):
        assert outs[j] == sequence(l_, rhs, a_, s_), f"operand {j}"


@pytest.mark.parametrize("ring", list(RINGS))
def test_column_chunks_give_the_unchunked_result(gpu, oracle, hip_env, ring):
    n, depth, bits, base = RINGS[ring]
    P = pool(gpu, oracle, ring)
    p, moduli = P["p"], P["moduli"]
    k = p.modulus_digits()
    cols = 7
    B = oracle.random_matrix(910, RHS_ROWS, cols, moduli, n)
    A = oracle.random_matrix(911, 18, cols, moduli, n)
    M = gpu.GpuDCRTPolyMatrix
    rows = [1, 4, 9, 1, 0, 3]
    lhss, adds, scs, r0 = [], [], [], 0
    for j, h in enumerate(rows):
        lhss.append(M.from_rns(p, P["S"][r0:r0 + h], True))
        adds.append(None if j % 3 == 0 else M.from_rns(p, A[r0:r0 + h], True))
        scs.append(M.from_rns(p, P["sc"][j % 3][None], True) if j % 3 == 2 else None)
        r0 += h
    poly_bytes = depth * n * p.ctx().word_bytes()
    for rhs_eval in (False, True):
        rhs = M.from_rns(p, oracle.matrix_ntt(B, moduli) if rhs_eval else B, rhs_eval)
        whole = M.mul_decompose_many(lhss, rhs, adds, scs)
        # room for two columns of the digit matrix: chunks of 2, 2, 2 and 1 columns
        hip_env.set("MXX_HIP_MUL_DECOMPOSE_MANY_BUDGET", str(2 * RHS_ROWS * k * poly_bytes + poly_bytes // 2))
        chunked = M.mul_decompose_many(lhss, rhs, adds, scs)
        hip_env.unset("MXX_HIP_MUL_DECOMPOSE_MANY_BUDGET")
        for j, (w, c) in enumerate(zip(whole, chunked)):
            assert raw_same(w, c), f"operand {j}, rhs_eval={rhs_eval}"
            assert raw_same(w, sequence(lhss[j], rhs, adds[j], scs[j])), f"operand {j} against the sequence"


def test_empty_shapes(gpu, oracle):
    from mxx_amd import _ffi

    P = pool(gpu, oracle, "n256_51bit")
    p = P["p"]
    M = gpu.GpuDCRTPolyMatrix
    k = p.modulus_digits()
    assert M.mul_decompose_many([], M.from_rns(p, P["B"], False)) == []
    # r * k = 0: the addend term alone (zero without an addend)
    rhs0 = M(p, 0, RHS_COLS, p.crt_depth() - 1, True)
    lhs0 = [M(p, 2, 0, p.crt_depth() - 1, True), M(p, 1, 0, p.crt_depth() - 1, True), M(p, 3, 0, p.crt_depth() - 1, True)]
    adds = [M.from_rns(p, P["A"][0:2], True), None, M.from_rns(p, P["A"][2:5], True)]
    scs = [M.from_rns(p, P["sc"][0][None], True), None, None]
    outs = M.mul_decompose_many(lhs0, rhs0, adds, scs)
    assert np.array_equal(outs[0].to_rns(), addend_term(P["A"][0:2], P["sc"][0][0], P["moduli"]))
    assert not outs[1].to_rns().any()
    assert np.array_equal(outs[2].to_rns(), P["A"][2:5])
    # no columns, and only empty operands: nothing to launch
    two_rows, rhs_eval = M.from_rns(p, P["S"][0:2], True), M.from_rns(p, P["B_eval"], True)
    gpu.gpu_device_sync()
    c0 = _ffi.lib().gpupoly_launch_count()
    out = M.mul_decompose_many([two_rows], M(p, RHS_ROWS, 0, p.crt_depth() - 1, True))
    assert out[0].size() == (2, 0)
    out = M.mul_decompose_many([M(p, 0, RHS_ROWS * k, p.crt_depth() - 1, True)], rhs_eval)
    assert out[0].size() == (0, RHS_COLS)
    assert _ffi.lib().gpupoly_launch_count() == c0


REFUSALS = ["shape_mismatch_in_operand_2", "coeff_lhs_1", "scalar_without_addend", "out0_is_lhs1", "same_output_twice",
            "operand_of_a_second_context", "base_bits_zero", "addend_not_eval"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing_and_leave_every_output_as_it_was(gpu, oracle, case):
    from mxx_amd import _ffi

    ring = "n256_51bit"
    P = pool(gpu, oracle, ring)
    p, base = P["p"], P["base"]
    M = gpu.GpuDCRTPolyMatrix
    k = p.modulus_digits()
    rows = [1, 1, 2, 1]
    lhss = [M.from_rns(p, P["S"][j:j + h], True) for j, h in enumerate(rows)]
    adds = [M.from_rns(p, P["A"][j:j + h], True) for j, h in enumerate(rows)]
    scs = [M.from_rns(p, P["sc"][j % 3][None], True) for j in range(4)]
    rhs = M.from_rns(p, P["B"], False)
    # outputs hold known residues under the COEFF tag: a refused call must leave both
    outs = [M.from_rns(p, P["A"][10 + j:10 + j + h], False) for j, h in enumerate(rows)]
    if case == "shape_mismatch_in_operand_2":
        lhss[2] = M.from_rns(p, P["S"][0:2, : RHS_ROWS * k - 1], True)
    elif case == "coeff_lhs_1":
        lhss[1] = M.from_rns(p, P["S"][1:2], False)
    elif case == "scalar_without_addend":
        adds[3] = None
    elif case == "out0_is_lhs1":
        # the alias must be the only fault: with a 2 x (2k) right operand an output row is as wide as a left operand
        rhs = M.from_rns(p, oracle.random_matrix(920, RHS_ROWS, RHS_ROWS * k, P["moduli"], P["n"]), False)
        adds = [None] * 4
        scs = [None] * 4
        outs = [M.from_rns(p, P["S"][20 + j:20 + j + h], j == 0) for j, h in enumerate(rows)]
        lhss[1] = outs[0]
    elif case == "same_output_twice":
        outs[3] = outs[1]
    elif case == "operand_of_a_second_context":
        n, depth, bits, _ = RINGS[ring]
        p2 = gpu.GpuDCRTPolyParams(n, P["moduli"], base, dnum=9)  # same ring and device, a context of its own
        assert p2.ctx_raw().value != p.ctx_raw().value
        adds[2] = M.from_rns(p2, P["A"][2:4], True)
    elif case == "addend_not_eval":
        adds[0] = M.from_rns(p, P["A"][0:1], False)
    distinct = {o.raw.value: o for o in outs}.values()
    before = [(o, o.clone()) for o in distinct]
    gpu.gpu_device_sync()
    c0 = _ffi.lib().gpupoly_launch_count()
    rc = raw_call(outs, lhss, adds, scs, rhs, 0 if case == "base_bits_zero" else base)
    assert _ffi.lib().gpupoly_launch_count() == c0, "a refused call launched a kernel"
    assert rc != 0 and "gpupoly_matrix_mul_decompose_many" in _ffi.last_error_string(), _ffi.last_error_string()
    for o, b in before:
        assert raw_same(o, b), f"{case}: an output changed (residues or tag)"


def test_launches_do_not_grow_with_the_operand_count(gpu, oracle):
    from mxx_amd import _ffi

    n, depth, bits, base = 256, 12, 51, 17  # the launch-bound GGH15 ring
    p = make_params(gpu, oracle, n, depth, bits, base)
    us, dist = gpu.GpuDCRTPolyUniformSampler(), gpu.DistType.FinRingDist()
    k = p.modulus_digits()
    M = gpu.GpuDCRTPolyMatrix
    rhs = us.sample_uniform(p, 2, 3, dist)
    lhss = [us.sample_uniform(p, 1, 2 * k, dist) for _ in range(16)]
    adds = [us.sample_uniform(p, 1, 3, dist) for _ in range(16)]
    scs = [us.sample_uniform(p, 1, 1, dist) for _ in range(16)]
    lib = _ffi.lib()
    M.mul_decompose_many(lhss, rhs, adds, scs)  # warm
    c0 = lib.gpupoly_launch_count()
    many = M.mul_decompose_many(lhss, rhs, adds, scs)
    c1 = lib.gpupoly_launch_count()
    one = M.mul_decompose_many(lhss[:1], rhs, adds[:1], scs[:1])
    c2 = lib.gpupoly_launch_count()
    seq = sequence(lhss[0], rhs, adds[0], scs[0])
    c3 = lib.gpupoly_launch_count()
    print(f"launches: 16 operands {c1 - c0}, 1 operand {c2 - c1}, one per-operand sequence {c3 - c2}")
    assert c1 - c0 == c2 - c1, f"16 operands took {c1 - c0} launches, one operand {c2 - c1}"
    assert c1 - c0 < c3 - c2, f"the call took {c1 - c0} launches, ONE per-operand sequence {c3 - c2}"
    assert one[0] == seq and many[0] == seq


def test_mirror_runs_the_reference_loop_when_the_chunk_switch_is_set(gpu, oracle, monkeypatch):
    P = pool(gpu, oracle, "n16_18bit")
    rows = [1, 4, 2]
    lhss, adds, scs, want = operands(gpu, P, rows, lambda j: (j + 1) % 3)
    rhs = gpu.GpuDCRTPolyMatrix.from_rns(P["p"], P["B"], False)
    monkeypatch.setenv("MXX_MUL_DECOMPOSE_COLUMN_CHUNK_WIDTH", "1")
    outs = gpu.GpuDCRTPolyMatrix.mul_decompose_many(lhss, rhs, adds, scs)
    monkeypatch.delenv("MXX_MUL_DECOMPOSE_COLUMN_CHUNK_WIDTH")
    direct = gpu.GpuDCRTPolyMatrix.mul_decompose_many(lhss, rhs, adds, scs)
    for j, (o, d, w) in enumerate(zip(outs, direct, want)):
        assert o.is_ntt and np.array_equal(o.to_rns(), w), f"operand {j} through the reference loop"
        assert o == d
