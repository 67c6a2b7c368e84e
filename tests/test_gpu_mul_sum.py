"""gpupoly_matrix_mul_sum / gpupoly_matrix_mul_acc: out[:, dst_col .. dst_col + cols) = addend block +- sum_t lhss[t] * rhss[t].

Bit-exact against the CPU restatement (oracle.matmul plus exact integer add / sub mod q on the host) and against the sequence
of the existing entry points (gpu_matrix_mul per term, gpu_matrix_add / gpu_matrix_sub or gpupoly_matrix_neg,
gpu_matrix_copy_block into place) through gpu_matrix_equal; the lazy window across a term boundary with all-(q - 1)
operands; inputs untouched; launch counts; every refusal leaves `out` and the launch counter alone; a level below the top; a
row view as `out`; the host mirror.  Every axis is covered against one default of the others."""
import ctypes as C

import numpy as np
import pytest

import plainref as PR
import ran
from conftest import make_params

pytestmark = pytest.mark.gpu

# (n, depth, limb bits, base bits): scalar loads of 32-bit words, 64-bit words, 16-byte loads
RINGS = {"n16_18bit": (16, 3, 18, 6), "n256_51bit": (256, 3, 51, 17), "n16384_24bit": (16384, 2, 24, 12)}
# inner sizes per term: one term, differing sizes, an empty term, a second launch (the 65th term), no term at all
KS = {"3": [3], "1_4_2": [1, 4, 2], "0_5": [0, 5], "65x1": [1] * 65, "none": []}
ROWS = [1, 2, 3, 5, 9, 0]  # tile edges of the 2-, 4- and 8-row tiles, two row tiles, nothing
RMAX, KMAX, CMAX, WIDE = 9, 8, 9, 7  # pool sizes; WIDE = columns of the `out` a block is placed into
D_ROWS, D_COLS, D_KS = 2, 3, "1_4_2"  # the defaults

_pool = {}


def pool(gpu, oracle, ring, limbs=None):
    """Host inputs of one ring, made once and never written; products of pool slices are cached per (offset, k)."""
    key = (ring, limbs)
    if key not in _pool:
        n, depth, bits, base = RINGS[ring]
        p = make_params(gpu, oracle, n, depth, bits, base)
        moduli = p.moduli()[: limbs or depth]
        P = dict(p=p, moduli=moduli, n=n, L=len(moduli), prod={}, oracle=oracle,
                 SA=oracle.random_matrix(700, RMAX, KMAX, moduli, n), SB=oracle.random_matrix(701, KMAX, CMAX, moduli, n),
                 AD=oracle.random_matrix(702, RMAX, CMAX, moduli, n), SENT=oracle.random_matrix(703, RMAX, max(WIDE, CMAX), moduli, n))
        for name in ("SA", "SB", "AD", "SENT"):
            P[name].setflags(write=False)
        _pool[key] = P
    return _pool[key]


def term_slices(ks):
    """where term t takes its k_t inner indices from the pool"""
    return [((3 * t) % (KMAX - k + 1), k) for t, k in enumerate(ks)]


def product(P, off, k):
    """SA[:, off:off+k] * SB[off:off+k, :] on the CPU (RMAX x CMAX), cached"""
    if (off, k) not in P["prod"]:
        w = P["oracle"].matmul(P["SA"][:, off:off + k], P["SB"][off:off + k, :], P["moduli"])
        w.setflags(write=False)
        P["prod"][(off, k)] = w
    return P["prod"][(off, k)]


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


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag (a tag mismatch is 'not equal' there)"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value) or a.nrow * a.ncol == 0


def launches():
    from mxx_amd import _ffi

    return _ffi.lib().gpupoly_launch_count()


def raw_mul_sum(out, dst_col, cols, addend, lhss, rhss, negate, n=None):
    from mxx_amd import _ffi

    n = len(lhss) if n is None else n
    arr = lambda ms: None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])
    return _ffi.lib().gpupoly_matrix_mul_sum(None if out is None else out.raw, dst_col, cols, None if addend is None else addend.raw,
                                             arr(lhss), arr(rhss), n, 1 if negate else 0)


def sequence(gpu, P, lhss, rhss, rows, cols, addend_block, negate):
    """the existing entry points: gpu_matrix_mul per term, then add / sub (or neg)"""
    acc = addend_block
    for l_, r_ in zip(lhss, rhss):
        prod = l_ * r_
        if acc is None:
            acc = -prod if negate else prod
        else:
            acc = acc - prod if negate else acc + prod
    if acc is None:
        acc = gpu.GpuDCRTPolyMatrix._new_zero_with_state(P["p"], rows, cols, P["L"] - 1, True)
    return acc


def run_case(gpu, oracle, ring, rows=D_ROWS, cols=D_COLS, ks_id=D_KS, addend="separate", negate=False, placed=False, limbs=None):
    """One call against the CPU restatement and against the sequence; inputs compared with their uploads afterwards.
    addend: "none", "separate" or "out".  placed: the block goes to columns [2, 2 + cols) of a WIDE-column sentinel."""
    P = pool(gpu, oracle, ring, limbs)
    M = gpu.GpuDCRTPolyMatrix
    q = qcol(P)
    terms = term_slices(KS[ks_id])
    lhss = [dev(gpu, P, P["SA"][:rows, off:off + k]) for off, k in terms]
    rhss = [dev(gpu, P, P["SB"][off:off + k, :cols]) for off, k in terms]
    dst = 2 if placed else 0
    width = WIDE if placed else cols
    assert dst + cols <= width
    # host: what `out` and the addend hold before the call (the addend's block is what counts)
    out_host = P["SENT"][:rows, :width]
    add_host = None if addend == "none" else (out_host if addend == "out" else P["AD"][:rows, :width])
    out = dev(gpu, P, out_host)
    add = None if addend == "none" else (out if addend == "out" else dev(gpu, P, add_host))
    total = np.zeros((rows, cols, P["L"], P["n"]), dtype=np.uint64)
    for off, k in terms:
        total = add_mod(total, product(P, off, k)[:rows, :cols], q)
    if add_host is None:
        block = sub_mod(np.zeros_like(total), total, q) if negate else total
    else:
        block = (sub_mod if negate else add_mod)(add_host[:, dst:dst + cols], total, q)
    want = out_host.copy()
    want[:, dst:dst + cols] = block
    # the sequence of existing entry points, placed with copy_block
    add_block = None if add is None else add.slice_columns(dst, dst + cols)
    seq_out = out.clone()
    seq_block = sequence(gpu, P, lhss, rhss, rows, cols, add_block, negate)
    seq_out.copy_block_from(seq_block, 0, dst, 0, 0, rows, cols)
    inputs = lhss + rhss + ([add] if addend == "separate" else [])
    before = [m.clone() for m in inputs]

    if terms or not placed:
        got = M.mul_sum(lhss, rhss, addend=add, negate=negate, out=out, dst_col=dst)
        assert got is out
    else:  # without a term the mirror takes the block to out's last column: the narrower block goes through the entry itself
        assert raw_mul_sum(out, dst, cols, add, [], [], negate) == 0
    assert out.is_ntt and out.size() == (rows, width)
    if rows:
        assert np.array_equal(out.to_rns(), want), "against the CPU restatement (columns outside the block included)"
    assert raw_same(out, seq_out), "against the sequence of existing entry points (residues and tag)"
    for j, (m, b) in enumerate(zip(inputs, before)):
        assert raw_same(m, b), f"input {j} changed"


@pytest.mark.parametrize("ks_id", list(KS))
@pytest.mark.parametrize("ring", list(RINGS))
def test_term_lists(gpu, oracle, ring, ks_id):
    run_case(gpu, oracle, ring, ks_id=ks_id)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("ring", list(RINGS))
def test_row_counts(gpu, oracle, ring, rows):
    run_case(gpu, oracle, ring, rows=rows)


@pytest.mark.parametrize("ring", list(RINGS))
def test_nine_columns(gpu, oracle, ring):
    run_case(gpu, oracle, ring, cols=9)


@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_placement_leaves_the_other_columns(gpu, oracle, ring, addend):
    run_case(gpu, oracle, ring, placed=True, addend=addend, negate=addend == "none")


@pytest.mark.parametrize("negate", [False, True], ids=["plus", "minus"])
@pytest.mark.parametrize("addend", ["none", "separate", "out"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_addend_modes(gpu, oracle, ring, addend, negate):
    run_case(gpu, oracle, ring, addend=addend, negate=negate)


@pytest.mark.parametrize("ks_id", ["1_4_2", "none", "0_5"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_nine_rows_placed_and_negated(gpu, oracle, ring, ks_id):
    """above 8 rows: the products into scratch and the combine pass, into a column block"""
    run_case(gpu, oracle, ring, rows=9, ks_id=ks_id, placed=True, negate=True)


@pytest.mark.parametrize("ks_id", ["1_4_2", "65x1"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_nine_rows_through_the_term_table_kernel(gpu, oracle, hip_env, ring, ks_id):
    """two row tiles of the 8-row tile: the switch keeps the term-table kernel above 8 rows"""
    hip_env.set("MXX_HIP_MUL_SUM_PATH", "tile")
    with ran.launches() as launched:
        run_case(gpu, oracle, ring, rows=9, ks_id=ks_id, placed=True, addend="out")
    if FORCED["test_nine_rows_through_the_term_table_kernel"]["pairs"][("MXX_HIP_MUL_SUM_PATH", "tile")](dict(ring=ring)):
        # the values cannot tell: above 8 rows the default is products into scratch and one combine pass per term
        launched.assert_ran("MXX_HIP_MUL_SUM_PATH", "tile", pool(gpu, oracle, ring)["moduli"])


def test_a_level_below_the_top(gpu, oracle):
    run_case(gpu, oracle, "n16_18bit", limbs=2, negate=True)
    run_case(gpu, oracle, "n16_18bit", limbs=2, rows=9, placed=True)


def test_a_row_view_of_a_taller_matrix_as_out(gpu, oracle):
    P = pool(gpu, oracle, "n256_51bit")
    q = qcol(P)
    M = gpu.GpuDCRTPolyMatrix
    rows, cols = 2, 3
    parent = dev(gpu, P, P["SENT"][:5, :cols])
    out = parent.row_view(1, 1 + rows)
    terms = term_slices(KS[D_KS])
    lhss = [dev(gpu, P, P["SA"][:rows, off:off + k]) for off, k in terms]
    rhss = [dev(gpu, P, P["SB"][off:off + k, :cols]) for off, k in terms]
    total = np.zeros((rows, cols, P["L"], P["n"]), dtype=np.uint64)
    for off, k in terms:
        total = add_mod(total, product(P, off, k)[:rows, :cols], q)
    want = P["SENT"][:5, :cols].copy()
    want[1:1 + rows] = add_mod(want[1:1 + rows], total, q)
    M.mul_sum(lhss, rhss, addend=out, out=out)  # accumulate in place through the view
    assert np.array_equal(parent.to_rns(), want)
    # a disjoint view of the same parent is an ordinary operand; one that reaches into the output is refused
    other = parent.row_view(3, 5)
    lhs = dev(gpu, P, P["SA"][:rows, :2])
    rhs2 = other  # 2 x cols
    want[1:1 + rows] = sub_mod(want[1:1 + rows], P["oracle"].matmul(P["SA"][:rows, :2], want[3:5], P["moduli"]), q)
    out.mul_sub_in_place(lhs, rhs2)
    assert np.array_equal(parent.to_rns(), want)


# ---- the lazy window across a term boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits,ks,window", [(31, [3, 3], 4), (61, [40, 30], 64)], ids=["31bit_3_3", "61bit_40_30"])
@pytest.mark.parametrize("negate", [False, True], ids=["plus", "minus"])
def test_lazy_window_carries_across_a_term_boundary(gpu, bits, ks, window, negate):
    """All operands q - 1, the largest prime of the class: the accumulator holds `window` products on top of a residue, no
    single term reaches it, both together pass it.  A kernel that resets its pending-product counter per term overflows.
    Expected: the closed form addend +- K (q - 1)^2 mod q."""
    n = 256
    qv = PR.primes(n, bits, 1)[0]
    acc_bits = 128 if qv >> 31 else 64
    assert ((1 << acc_bits) - qv) // (qv - 1) ** 2 == window and max(ks) <= window < sum(ks)
    p = gpu.GpuDCRTPolyParams(n, [qv], 1)
    M = gpu.GpuDCRTPolyMatrix
    full = lambda r, c, v: np.full((r, c, 1, n), v, dtype=np.uint64)  # noqa: E731
    rows, cols = 2, 3
    lhss = [M.from_rns(p, full(rows, k, qv - 1), True) for k in ks]
    rhss = [M.from_rns(p, full(k, cols, qv - 1), True) for k in ks]
    a = qv - 5
    addend = M.from_rns(p, full(rows, cols, a), True)
    term = sum(ks) * (qv - 1) ** 2
    want = (a - term) % qv if negate else (a + term) % qv
    out = M.mul_sum(lhss, rhss, addend=addend, negate=negate)
    assert np.array_equal(out.to_rns(), full(rows, cols, want))
    # and the same through the existing entry points
    acc = addend
    for l_, r_ in zip(lhss, rhss):
        acc = acc - l_ * r_ if negate else acc + l_ * r_
    assert raw_same(out, acc)


# ---- the other register tiles -------------------------------------------------------------------------------------------
# 64-bit words choose 4x4x2 / 2x4x2 / 1x4x2 / 2x2x1 / 1x1x1 by how far rows x columns fill the chip; 32-bit words stream
# right operands above 256 MB under one row tile with non-temporal loads.  The operands are samples (PACKED24 where the ring
# allows it: unpacked first).
@pytest.mark.parametrize("ring,depth,rows,cols,ks", [
    ("n256_51bit", 12, 4, 344, [2, 1]), ("n256_51bit", 12, 2, 344, [2, 1]), ("n256_51bit", 12, 1, 344, [2, 1]),
    ("n256_51bit", 12, 2, 88, [2, 1]), ("n256_51bit", 12, 5, 344, [1, 2]), ("n16384_24bit", 2, 1, 264, [6, 3]),
], ids=["u64_4x4x2", "u64_2x4x2", "u64_1x4x2", "u64_2x2x1", "u64_4x4x2_two_row_tiles", "u32_streamed_once"])
def test_every_tile_matches_the_sequence(gpu, oracle, ring, depth, rows, cols, ks):
    n, _, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    us, dist = gpu.GpuDCRTPolyUniformSampler(), gpu.DistType.FinRingDist()
    lhss = [us.sample_uniform(p, rows, k, dist) for k in ks]
    rhss = [us.sample_uniform(p, k, cols, dist) for k in ks]
    addend = us.sample_uniform(p, rows, cols, dist)
    out = gpu.GpuDCRTPolyMatrix.mul_sum(lhss, rhss, addend=addend, negate=True)
    acc = addend
    for l_, r_ in zip(lhss, rhss):
        acc = acc - l_ * r_
    assert out == acc


# ---- launch counts --------------------------------------------------------------------------------------------------------
def test_launch_counts(gpu, oracle):
    P = pool(gpu, oracle, "n256_51bit")
    rows, cols = 2, 3
    mk = lambda ks: ([dev(gpu, P, P["SA"][:rows, off:off + k]) for off, k in term_slices(ks)],  # noqa: E731
                     [dev(gpu, P, P["SB"][off:off + k, :cols]) for off, k in term_slices(ks)])
    addend = dev(gpu, P, P["AD"][:rows, :cols])
    out = dev(gpu, P, P["SENT"][:rows, :cols])
    counts = {}
    for name, ks in (("n3", [1, 4, 2]), ("n65", [1] * 65), ("n0", [])):
        lhss, rhss = mk(ks)
        assert all(m.layout == "words" for m in lhss + rhss + [addend, out])
        gpu.gpu_device_sync()
        c0 = launches()
        assert raw_mul_sum(out, 0, cols, addend, lhss, rhss, False) == 0
        counts[name] = launches() - c0
    print("launches:", counts)
    assert counts["n3"] == 1 and counts["n65"] == 2 and counts["n0"] <= 1
    assert np.array_equal(out.to_rns(), P["AD"][:rows, :cols])  # n = 0 with an addend copies the addend's block


def test_empty_shapes_launch_nothing(gpu, oracle):
    P = pool(gpu, oracle, "n256_51bit")
    M = gpu.GpuDCRTPolyMatrix
    level = P["L"] - 1
    lhs, rhs0, rhs = dev(gpu, P, P["SA"][:2, :3]), M(P["p"], 3, 0, level, True), dev(gpu, P, P["SB"][:3, :3])
    gpu.gpu_device_sync()
    c0 = launches()
    out = M.mul_sum([lhs], [rhs0])  # cols = 0
    assert out.size() == (2, 0) and out.is_ntt
    out = M.mul_sum([M(P["p"], 0, 3, level, True)], [rhs])  # r = 0
    assert out.size() == (0, 3) and out.is_ntt
    assert launches() == c0
    # n = 0 without an addend writes zeros into the block only
    wide = dev(gpu, P, P["SENT"][:2, :WIDE])
    assert raw_mul_sum(wide, 2, 3, None, [], [], False) == 0
    want = P["SENT"][:2, :WIDE].copy()
    want[:, 2:5] = 0
    assert np.array_equal(wide.to_rns(), want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
REFUSALS = ["null_out", "null_arrays", "null_lhss_only", "null_term", "operand_of_a_second_context", "addend_of_a_second_context",
            "level_mismatch", "inner_mismatch", "rows_mismatch", "cols_mismatch", "block_out_of_range", "addend_shape",
            "coeff_lhs", "coeff_rhs_in_term_2", "coeff_addend", "partial_block_into_coeff_out", "addend_is_a_shifted_view_of_out",
            "out_is_lhs", "out_is_a_row_view_of_rhs", "acc_shape_mismatch", "acc_coeff_out", "acc_out_is_rhs"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing_and_leave_out_as_it_was(gpu, oracle, case):
    from mxx_amd import _ffi

    ring = "n256_51bit"
    P = pool(gpu, oracle, ring)
    p = P["p"]
    M = gpu.GpuDCRTPolyMatrix
    rows, cols = 2, 3
    terms = term_slices([1, 4, 2])
    lhss = [dev(gpu, P, P["SA"][:rows, off:off + k]) for off, k in terms]
    rhss = [dev(gpu, P, P["SB"][off:off + k, :cols]) for off, k in terms]
    addend = dev(gpu, P, P["AD"][:rows, :cols])
    # `out` holds known residues under the COEFF tag wherever the rule allows it: a refused call must leave both
    out = dev(gpu, P, P["SENT"][:rows, :cols], False)
    dst, width, n, entry, overlap = 0, cols, None, "gpupoly_matrix_mul_sum", False
    keep = []
    if case == "null_out":
        out = None
    elif case == "null_arrays":
        lhss, rhss, n = None, None, 2
    elif case == "null_lhss_only":
        lhss, n = None, 3
    elif case == "null_term":
        rhss[1] = None
    elif case in ("operand_of_a_second_context", "addend_of_a_second_context"):
        n_, depth, bits, base = RINGS[ring]
        p2 = gpu.GpuDCRTPolyParams(n_, P["moduli"], base, dnum=9)  # same ring and device, a context of its own
        assert p2.ctx_raw().value != p.ctx_raw().value
        if case.startswith("operand"):
            lhss[2] = M.from_rns(p2, np.ascontiguousarray(P["SA"][:rows, 0:2]), True)
        else:
            addend = M.from_rns(p2, np.ascontiguousarray(P["AD"][:rows, :cols]), True)
    elif case == "level_mismatch":
        off, k = terms[1]
        rhss[1] = M.from_rns(p, np.ascontiguousarray(P["SB"][off:off + k, :cols, :2]), True)
    elif case == "inner_mismatch":
        lhss[1] = dev(gpu, P, P["SA"][:rows, 0:3])  # 3 against 4
    elif case == "rows_mismatch":
        lhss[2] = dev(gpu, P, P["SA"][:rows + 1, 0:2])
    elif case == "cols_mismatch":
        rhss[0] = dev(gpu, P, P["SB"][0:1, :cols + 1])
    elif case == "block_out_of_range":
        out = dev(gpu, P, P["SENT"][:rows, :WIDE])
        addend, dst = None, WIDE - cols + 1
    elif case == "addend_shape":
        addend = dev(gpu, P, P["AD"][:rows, :cols + 1])
    elif case == "coeff_lhs":
        lhss[0] = dev(gpu, P, P["SA"][:rows, 0:1], False)
    elif case == "coeff_rhs_in_term_2":
        off, k = terms[2]
        rhss[2] = dev(gpu, P, P["SB"][off:off + k, :cols], False)
    elif case == "coeff_addend":
        addend = dev(gpu, P, P["AD"][:rows, :cols], False)
    elif case == "partial_block_into_coeff_out":
        out = dev(gpu, P, P["SENT"][:rows, :WIDE], False)
        addend, dst = None, 2
    elif case == "addend_is_a_shifted_view_of_out":
        parent = dev(gpu, P, P["SENT"][:rows + 1, :cols])
        out, addend, overlap = parent.row_view(1, 1 + rows), parent.row_view(0, rows), True
        keep.append(parent)
    elif case == "out_is_lhs":
        # the alias must be the only fault: a term whose inner size is the block's width
        lhss, rhss = [dev(gpu, P, P["SA"][:rows, :cols])], [dev(gpu, P, P["SB"][:cols, :cols])]
        out, addend, overlap = lhss[0], None, True
    elif case == "out_is_a_row_view_of_rhs":
        lhss, rhss = [dev(gpu, P, P["SA"][:rows, :3])], [dev(gpu, P, P["SB"][:3, :cols])]
        out, addend, overlap = rhss[0].row_view(1, 1 + rows), None, True
    elif case.startswith("acc_"):
        entry = "gpupoly_matrix_mul_acc"
        lhs, rhs = dev(gpu, P, P["SA"][:rows, :cols]), dev(gpu, P, P["SB"][:cols, :cols])
        if case == "acc_shape_mismatch":
            out = dev(gpu, P, P["SENT"][:rows, :cols + 1])
        elif case == "acc_out_is_rhs":
            rhs = dev(gpu, P, P["SB"][:cols, :cols])
            lhs = dev(gpu, P, P["SA"][:cols, :cols])
            out, overlap = rhs, True
    before = None if out is None else out.clone()
    tag = None if out is None else out.is_ntt
    gpu.gpu_device_sync()
    c0 = launches()
    if case.startswith("acc_"):
        rc = _ffi.lib().gpupoly_matrix_mul_acc(out.raw, lhs.raw, rhs.raw, 0)
    else:
        rc = raw_mul_sum(out, dst, cols, addend, lhss, rhss, False, n)
    msg = _ffi.last_error_string()
    assert launches() == c0, "a refused call launched a kernel"
    assert rc != 0 and entry in msg, msg
    if overlap:
        assert "alias" in msg or "overlap" in msg, msg
    if out is not None:
        assert out.is_ntt == tag and raw_same(out, before), f"{case}: `out` changed (residues or tag)"


# ---- the host mirror ------------------------------------------------------------------------------------------------------
def test_mirror(gpu, oracle):
    P = pool(gpu, oracle, "n16_18bit")
    M = gpu.GpuDCRTPolyMatrix
    rows, cols = 3, 3
    l_, r_ = dev(gpu, P, P["SA"][:rows, :4]), dev(gpu, P, P["SB"][:4, :cols])
    a = dev(gpu, P, P["AD"][:rows, :cols])
    want_add, want_sub = a + l_ * r_, a - l_ * r_
    x = a.clone()
    v0 = x.content_version()
    x.mul_add_in_place(l_, r_)
    assert x == want_add and x.content_version() != v0
    y = a.clone()
    y.mul_sub_in_place(l_, r_)
    assert y == want_sub
    out = M.mul_sum([l_], [r_])
    assert out.is_ntt and out.size() == (rows, cols) and out == l_ * r_
    assert M.mul_sum([l_], [r_], negate=True) == -(l_ * r_)
    assert M.mul_sum([], [], addend=a) == a


# forced kernel paths (tests/ran.py): gpupoly_matrix_mul_sum keeps the term-table kernel at every height under the
# switch, with no condition of its own; evaluated over the parameter lists by tests/test_ran_table_host.py
FORCED = {
    "test_nine_rows_through_the_term_table_kernel": {"cls": lambda c: ran.Launched.word_class([1 << (RINGS[c["ring"]][2] - 1)]), "pairs": {
        ("MXX_HIP_MUL_SUM_PATH", "tile"): lambda c: True}},
}
