"""GPU: the preimage targets of many public-parameter indices x column parts of the Wee25 commitment in one call
(`gpupoly_matrix_wee25_targets`, mxx_amd/commit.py).

Everything in the target formula is exact arithmetic on canonical residues, so the bar is equality, bit for bit
(gpu_matrix_equal), with `t_top_target_block` - the reference's statements (src/commit/wee25.rs:536-584,696-719) restated with
the mirror's older operations, one target at a time.  That literal target is computed once per (context, secret size, index,
part) and shared by the block counts and windows.  Independently of the engine the same targets are computed with
tests/plainref.py fed with the CPU restatement's samples of W from the ORIGINAL formula, P.gadget times the digits of the
literal row_i minus the product, which the entry never evaluates: it writes row_i itself, so the comparison also proves
G G^-1(X) = X and the closed form of the index arithmetic.  The product kernel alone
(`gpupoly_matrix_wee25_targets_product`, which takes the stacked W as given) is held to plainref in every modulus width class
with operands no sampler produces: every residue of W and of T_bottom q - 1, an inner dimension m_b one past the class's lazy
window where operands of m_b x m_b polynomials allow it (a window of more than 71 products - 28 bits and below, 32 to 58 bits -
would take operands past a test's size: m_b = 8 there, the closed form without a fold inside the sum), indices that hit every
(limb, e, e'), and an all-zero W, which is the negation of 0."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import BASES, CLASSES, _cell, _eval_slots, _params, _top, _windows
from test_gpu_lut_targets import CONTEXTS
from test_gpu_lwe_targets import gadget_slots
from test_wee25_structure import literal_hits

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_wee25_targets"
PRODUCT = "gpupoly_matrix_wee25_targets_product"
KEY = bytes((13 * i + 3) & 0xFF for i in range(32))
SIGMA = 4.578
_SETUP, _LITERAL = {}, {}


def setup_of(gpu, oracle, ctx, s):
    """(Wee25Commit, T_bottom as an EVAL matrix, its residues): T_bottom is a random matrix - the targets are exact whatever it is"""
    from mxx_amd.commit import Wee25Commit

    if (ctx, s) not in _SETUP:
        p = make_params(gpu, oracle, *CONTEXTS[ctx])
        w = Wee25Commit(p, s, 2, SIGMA)
        w.hash_key = KEY
        tb = oracle.random_matrix(900 + 10 * s, w.m_b, w.j_2m_cols, p.moduli(), p.ring_dimension())
        _SETUP[(ctx, s)] = (w, gpu.GpuDCRTPolyMatrix.from_rns(p, tb, True), tb)
    return _SETUP[(ctx, s)]


def literal(gpu, oracle, ctx, s, idx, part):
    key = (ctx, s, idx, part)
    if key not in _LITERAL:
        w, t_bottom, _ = setup_of(gpu, oracle, ctx, s)
        _LITERAL[key] = w.t_top_target_block(idx, part * w.m_b, t_bottom.slice_columns(part * w.m_b, (part + 1) * w.m_b))
    return _LITERAL[key]


def straddles(w, bg):
    k = w.log_base_q
    return (bg * k) // w.m_b != (bg * k + k - 1) // w.m_b


def straddling_group(w):
    """a block group whose k columns cross a part boundary; where m_b = s (k + 2) is a multiple of k (s = 2 with k = 4) none
    does, and group 1 stands in"""
    assert any(straddles(w, bg) for bg in range(w.l)) == (w.m_b % w.log_base_q != 0)
    return next((bg for bg in range(w.l) if straddles(w, bg)), 1)


def pool_of(w):
    """indices that repeat and are not consecutive: 0 and pp_size - 1, every i*, a kk in each tower, a block group across a part
    boundary, one in the last part"""
    k, m_g = w.log_base_q, w.m_g
    L = w.params.crt_depth()
    dpt = k // L
    bg = straddling_group(w)
    pool = [0, w.pp_size - 1]
    pool += [2 * m_g + i * k + (i % k) for i in range(w.secret_size)]  # every i*
    pool += [m_g + tw * dpt + dpt - 1 for tw in range(L)]  # a kk in each tower
    pool += [bg * m_g + m_g - 1, bg * m_g, 0, (w.l - 1) * m_g + 1]
    assert {w.j_2m_hit(i)[0] for i in pool} == set(range(w.secret_size))
    assert {w.j_2m_hit(i)[1] // dpt for i in pool} == set(range(L))
    return pool


def windows_of(w):
    """(part_start, nparts): all parts, the part a straddling group ends in, a window not starting at 0"""
    bg = straddling_group(w)
    return {"all parts": (0, w.nparts), "one part": ((bg * w.log_base_q + w.log_base_q - 1) // w.m_b, 1), "inner window": (1, 2)}


def check_blocks(gpu, oracle, ctx, s, idxs, window, got, what):
    w = setup_of(gpu, oracle, ctx, s)[0]
    part_start, nparts = window
    assert len(got) == len(idxs)
    for t, idx in enumerate(idxs):
        assert len(got[t]) == nparts
        for q in range(nparts):
            assert got[t][q].size() == (s, w.m_b) and got[t][q].is_ntt
            assert got[t][q] == literal(gpu, oracle, ctx, s, idx, part_start + q), f"{what}: block {t} (index {idx}), part {part_start + q}"


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal leg; 2. a group boundary
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_one_call_equals_the_literal_leg_block_by_block(gpu, oracle, ctx, s):
    w, t_bottom, _ = setup_of(gpu, oracle, ctx, s)
    if ctx == "n16_24" and s == 1:
        assert (w.log_base_q, w.m_b, straddling_group(w)) == (4, 6, 1)  # columns 4..7 against the boundary at 6
    pool = pool_of(w)
    for name, window in windows_of(w).items():
        if name == "inner window":  # block group 0 lies wholly outside it
            assert w.log_base_q <= w.m_b * window[0]
        for T in (1, 3, 65):
            idxs = [pool[t % len(pool)] for t in range(T)]  # table tags
            check_blocks(gpu, oracle, ctx, s, idxs, window, w.t_top_target_blocks(t_bottom, idxs, *window), f"{name}, T = {T}")
        idxs = [pool[t % len(pool)] for t in range(7)][::-1]  # another order: every block's target is its own
        check_blocks(gpu, oracle, ctx, s, idxs, window, w.t_top_target_blocks(t_bottom, idxs, *window), f"{name}, reversed")
    # consecutive runs (indexed tags): three indices over all parts, the longest run of up to 65 over one part
    run = list(range(w.m_g - 1, w.m_g + 2))
    check_blocks(gpu, oracle, ctx, s, run, (0, w.nparts), w.t_top_target_blocks(t_bottom, run), "run of 3")
    count = min(65, w.pp_size)
    run = list(range(w.pp_size - count, w.pp_size))
    window = windows_of(w)["one part"]
    check_blocks(gpu, oracle, ctx, s, run, window, w.t_top_target_blocks(t_bottom, run, *window), f"run of {count}")
    assert w.t_top_target_blocks(t_bottom, []) == [] and w.t_top_target_blocks(t_bottom, [0, 1], 0, 0) == [[], []]


def test_a_group_boundary_inside_the_call(gpu, oracle):
    """More blocks than one group's W scratch holds cannot be reached with test-sized operands (the cap is 1 GiB); the blocks
    of a second call continue the first one's, which is what a group boundary does inside the entry: tags, hits and outputs
    start at the group's first block."""
    w, t_bottom, _ = setup_of(gpu, oracle, "n16_51", 2)
    for idxs in ([pool_of(w)[t % 5] for t in range(9)], list(range(3, 12))):
        whole = w.t_top_target_blocks(t_bottom, idxs, 1, 3)
        parts = w.t_top_target_blocks(t_bottom, idxs[:4], 1, 3) + w.t_top_target_blocks(t_bottom, idxs[4:], 1, 3)
        assert len(whole) == len(parts) == 9
        for a, b in zip(whole, parts):
            assert len(a) == len(b) == 3 and all(x == y for x, y in zip(a, b))


def test_a_grid_that_does_not_fit_is_split_by_blocks_then_by_columns(gpu, oracle):
    """The product's grid holds row tiles x column tiles <= 65535 in one extent.  At n = 16 with two 51-bit limbs the tile is
    4 x 4 for four stacked rows and 2 x 4 for two, so 2 blocks of 2 rows against 16385 parts of 16 columns (65540 column tiles)
    fit neither together nor block by block: the entry launches each block over two column halves, cut at column 131080 - inside
    part 8192 and inside the six hit columns 131076..131081 of the first block.  The reference is the same blocks one call each
    over the windows [0, 8192) and [8192, 16385), which fit (32768 and 32772 tiles).  The outputs are row views of one parent per
    leg, so one comparison covers all 32770 targets."""
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    w = setup_of(gpu, oracle, "n16_51", 2)[0]
    p, s, m_b, k = w.params, w.secret_size, w.m_b, w.log_base_q
    M, lib = gpu.GpuDCRTPolyMatrix, _ffi.lib()
    assert (s, m_b, k, p.ring_dimension()) == (2, 16, 6, 16)
    P_ = 16385
    wide = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, m_b, P_ * m_b, gpu.DistType.FinRingDist())
    idxs = [21846 * w.m_g + 10, 3 * w.m_g + 2]
    assert w.j_2m_hit(idxs[0]) == (1, 4, 131076) and (P_ * m_b + 1) // 2 == 131080
    tags = [w.tag(5), w.tag(9)]
    u64p = C.POINTER(C.c_uint64)

    def run(parent, blocks, part_start, nparts):
        """blocks `blocks` x parts [part_start, part_start + nparts) into their rows of `parent` (block-major over all P_ parts)"""
        views = [parent.row_view((t * P_ + q) * s, (t * P_ + q + 1) * s) for t in blocks for q in range(part_start, part_start + nparts)]
        arg, keep, _ = hash_tags_arg(KEY, [tags[t] for t in blocks])
        i_arr = np.array([idxs[t] for t in blocks], dtype=np.uint64)
        _ffi.trace_begin()
        rc = lib.gpupoly_matrix_wee25_targets(M._raw_array(views), len(blocks), nparts, wide.raw, part_start, s, p.base_bits(),
                                              i_arr.ctypes.data_as(u64p), C.byref(arg))
        names = [e["kernel"] for e in _ffi.trace_end() if e["threads"]]
        _ffi.check_status(rc, ENTRY)
        del keep
        return sum("wee25_targets_kernel" in name for name in names)

    split, ref = M(p, 2 * P_ * s, m_b, p.crt_depth() - 1, True), M(p, 2 * P_ * s, m_b, p.crt_depth() - 1, True)
    assert run(split, [0, 1], 0, P_) == 4  # two blocks x two column halves
    for t in (0, 1):
        assert run(ref, [t], 0, 8192) == 1 and run(ref, [t], 8192, P_ - 8192) == 1
    assert split == ref
    # the cut hit is in place: the constants of row 1 at columns 7, 8, 9 of part 8192 (the cut is at column 8), on top of the negated product
    blank = M(p, s, m_b, p.crt_depth() - 1, True)
    arg, keep, _ = hash_tags_arg(KEY, [tags[0]])
    i_arr = np.array([1 << 40], dtype=np.uint64)  # no column of T_bottom is hit
    _ffi.check_status(lib.gpupoly_matrix_wee25_targets(M._raw_array([blank]), 1, 1, wide.raw, 8192, s, p.base_bits(), i_arr.ctypes.data_as(u64p),
                                                       C.byref(arg)), ENTRY)
    diff = (split.row_view(8192 * s, 8193 * s) - blank).to_rns()
    moduli, dpt = p.moduli(), k // p.crt_depth()
    want = np.zeros_like(diff)
    for sp in range(k):  # kk = 4 = (tower 1, e = 1): 2^((1 + e') b) mod q_1 at the columns of tower 1
        if sp // dpt == 1:
            want[1, 131076 + sp - 8192 * m_b, 1, :] = pow(2, (1 + sp % dpt) * p.base_bits(), int(moduli[1]))
    assert want.any() and np.array_equal(diff, want)


# ---------------------------------------------------------------------------------------------------
# 3. independence from the engine: plainref fed with the CPU restatement's samples, the ORIGINAL formula
# ---------------------------------------------------------------------------------------------------
def literal_rows(w, idx, part, moduli, base, n):
    """the rows row_i of build_j_2m_block(idx, part * m_b) before decomposition, (s, m_b, L, n) coefficient residues, from the
    literal index arithmetic and P.gadget"""
    s, k, m_b, L = w.secret_size, w.log_base_q, w.m_b, len(moduli)
    g = P.gadget(1, moduli, base, n)[0]  # (k, L, n)
    rows = np.zeros((s, m_b, L, n), dtype=np.uint64)
    for i, kk, cols in literal_hits(idx, s, k, w.m_g):
        for sp, col in enumerate(cols):
            if part * m_b <= col < (part + 1) * m_b:
                for l in range(L):
                    rows[i, col - part * m_b, l, 0] = int(g[kk, l, 0]) * int(g[sp, l, 0]) % int(moduli[l])
    return rows


@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_targets_equal_the_plain_reference(gpu, oracle, ctx):
    s, T = 2, 3
    w, t_bottom, tb = setup_of(gpu, oracle, ctx, s)
    p = w.params
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k, m_b = L * dpt, w.m_b
    assert k == w.log_base_q
    slots = list(range(n))
    G = gadget_slots(moduli, base, n, s)
    bg = straddling_group(w)
    idxs = [bg * w.m_g + k + 1, w.pp_size - 1, bg * w.m_g + dpt]  # rows 1, s - 1 and 0; not consecutive
    part_start = bg * k // m_b
    got = w.t_top_target_blocks(t_bottom, idxs, part_start, 2)  # the two parts a straddling group touches
    hit_parts = set()
    for t, idx in enumerate(idxs[:T]):
        w_eval = _eval_slots(oracle.sample_distribution(s, m_b, moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, w.tag(idx))), moduli, slots)
        for q in range(2):
            part = part_start + q
            rows = literal_rows(w, idx, part, moduli, base, n)
            if rows.any():
                hit_parts.add((t, q))
            j = np.zeros((s * k, m_b, L, n), dtype=np.uint64)
            for i in range(s):
                for cc in range(m_b):
                    j[i * k:(i + 1) * k, cc] = _eval_slots(P.digits(rows[i, cc], moduli, base, dpt), moduli, slots)
            gj = P.slot_mul_sum(None, [G], [j], moduli, False)  # G_s J
            want = P.slot_mul_sum(gj, [w_eval], [tb[:, part * m_b:(part + 1) * m_b]], moduli, True)
            assert np.array_equal(got[t][q].to_rns(), want), (ctx, idx, part)
    assert {t for t, _ in hit_parts} == {0, 2}  # the last index's group lies outside the window
    if straddles(w, bg):  # the group's constants land in both parts (those of a tower only where its columns are)
        assert {q for _, q in hit_parts} == {0, 1}


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """T_bottom and the outputs at level 0 / 1 of a three-limb context: k = dpt * (level + 1) with dpt from the CONTEXT's
    crt_bits (one width per basis here, so plainref derives the same dpt from the truncated basis), m_g = s k and m_b = s (k + 2)
    at the level, W sampled in limbs 0..level only, and the plain reference above handed moduli[: level + 1]; the product
    entry with the stacked W given must write the same words."""
    from types import SimpleNamespace

    from mxx_amd.commit import Wee25Commit

    n, s = 16, 2
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    w = SimpleNamespace(secret_size=s, log_base_q=k, m_g=s * k, m_b=s * (k + 2))  # the sizes of a Wee25Commit at the level
    m_b = w.m_b
    tb = oracle.random_matrix(940 + level, m_b, 3 * m_b, moduli, n)
    t_bottom = M.from_rns(p, tb, True)
    slots = list(range(n))
    G = gadget_slots(moduli, base, n, s)
    idxs = [dpt - 1, w.m_g + k + 1, 2 * w.m_g + w.m_g - 1]  # block groups 0, 1, 2; rows 0, 1 and s - 1; not consecutive
    tags = [Wee25Commit.tag(i) for i in idxs]
    got = M.wee25_targets(t_bottom, 0, 2, s, idxs, KEY, tags)
    hits, stacked = 0, []
    for t, idx in enumerate(idxs):
        w_eval = _eval_slots(oracle.sample_distribution(s, m_b, moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tags[t])), moduli, slots)
        stacked.append(w_eval)
        for part in range(2):
            rows = literal_rows(w, idx, part, moduli, base, n)
            hits += bool(rows.any())
            j = np.zeros((s * k, m_b, L, n), dtype=np.uint64)
            for i in range(s):
                for cc in range(m_b):
                    j[i * k:(i + 1) * k, cc] = _eval_slots(P.digits(rows[i, cc], moduli, base, dpt), moduli, slots)
            gj = P.slot_mul_sum(None, [G], [j], moduli, False)  # G_s J
            want = P.slot_mul_sum(gj, [w_eval], [tb[:, part * m_b:(part + 1) * m_b]], moduli, True)
            assert got[t][part].level == level and got[t][part].is_ntt
            assert np.array_equal(got[t][part].to_rns(), want), (bits, level, idx, part)
    assert hits >= 2  # the constants of at least two blocks land inside the window
    given = M.wee25_targets_product(M.from_rns(p, np.concatenate(stacked, axis=0), True), t_bottom, 0, 2, s, idxs)
    for t in range(len(idxs)):
        for part in range(2):
            assert given[t][part] == got[t][part], (bits, level, t, part)


# ---------------------------------------------------------------------------------------------------
# 4. the product alone past the accumulator's window, in every width class
# ---------------------------------------------------------------------------------------------------
def inner_of(moduli):
    """m_b: one past the largest lazy window of the class, else one past the smallest, where the m_b x m_b operand stays
    test-sized (71 products at most); otherwise 8"""
    wins = _windows(moduli)
    for win in (max(wins), min(wins)):
        if win + 1 <= 72:
            return win + 1, True
    return 8, False


@pytest.mark.parametrize("bits", CLASSES)
def test_product_kernel_alone_in_every_width_class(gpu, bits):
    n, moduli, bases, slots = _cell(("class", bits))
    L = len(moduli)
    M = gpu.GpuDCRTPolyMatrix
    m_b, folds = inner_of(moduli)
    assert folds == (bits in (29, 31, 61, 62)), (bits, _windows(moduli))
    for base in BASES[bits]:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        s, k = 1, L * dpt
        nparts = -(-k // m_b)
        idxs = list(range(k))  # block group 0: kk = every (tower, e), columns s' = every (tower, e')
        T = len(idxs)
        g = P.gadget(1, moduli, base, n)[0]
        x = np.zeros((T, nparts * m_b, L, len(slots)), dtype=np.uint64)
        for kk in range(k):
            for sp in range(k):
                for l in range(L):
                    x[kk, sp, l, :] = int(g[kk, l, 0]) * int(g[sp, l, 0]) % int(moduli[l])
        for l in range(L):  # every (limb, e, e') is hit with the constant 2^((e + e') base) mod q_l
            for e in range(dpt):
                for e2 in range(dpt):
                    assert int(x[l * dpt + e, l * dpt + e2, l, 0]) == pow(2, (e + e2) * base, int(moduli[l]))
        tb = _top(m_b, nparts * m_b, moduli, n)
        t_bottom = M.from_rns(p, tb, True)
        for kind, w_np in (("top", _top(T * s, m_b, moduli, n)), ("zero", np.zeros((T * s, m_b, L, n), dtype=np.uint64))):
            got = M.wee25_targets_product(M.from_rns(p, w_np, True), t_bottom, 0, nparts, s, idxs)
            want = x  # W = 0: X itself, the negated sum stays 0
            if kind == "top":
                prod = P.slot_mul_sum(None, [w_np], [tb], moduli, False, slots)
                q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
                want = ((x.astype(object) - prod.astype(object)) % q_col).astype(np.uint64)
            for t in range(T):
                for q in range(nparts):
                    res = got[t][q].to_rns()
                    exp = want[t:t + 1, q * m_b:(q + 1) * m_b]
                    assert np.array_equal(res[..., slots], exp), (bits, base, kind, t, q)
                    assert np.array_equal(res, np.broadcast_to(exp[..., :1], res.shape)), (bits, base, kind, t, q)  # constant operands


# ---------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_depend_on_neither_blocks_nor_parts(gpu, oracle):
    from mxx_amd import _ffi

    w, t_bottom, _ = setup_of(gpu, oracle, "n256_51", 2)
    lib = _ffi.lib()

    def launches(fn):
        gpu.gpu_device_sync()
        c0 = lib.gpupoly_launch_count()
        _ffi.trace_begin()
        fn()
        names = [e["kernel"] for e in _ffi.trace_end() if e["threads"]]  # copies are traced with no threads
        return lib.gpupoly_launch_count() - c0, names

    many, many_names = launches(lambda: w.t_top_target_blocks(t_bottom, range(48), 0, 8))
    two, _ = launches(lambda: w.t_top_target_blocks(t_bottom, range(2), 0, 8))
    one_part, _ = launches(lambda: w.t_top_target_blocks(t_bottom, range(48), 0, 1))
    small, _ = launches(lambda: w.t_top_target_blocks(t_bottom, range(2), 0, 1))
    loop, _ = launches(lambda: [w.t_top_target_block(i, 0, t_bottom.slice_columns(0, w.m_b)) for i in range(2)])
    print(f"launches: 48 x 8 {many} {many_names}, 2 x 8 {two}, 48 x 1 {one_part}, 2 x 1 {small}, the literal loop for 2 x 1 {loop}")
    assert many == two == one_part == small and 0 < many < loop
    assert sum("wee25_targets_kernel" in name for name in many_names) == 1


# ---------------------------------------------------------------------------------------------------
# 6. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    ctx, s = "n16_24", 2
    w, t_bottom, _ = setup_of(gpu, oracle, ctx, s)
    p = w.params
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m_b, T, NP = w.m_b, 3, 2
    top = len(moduli) - 1
    sentinel = oracle.random_matrix(93, s, m_b, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    u64p = C.POINTER(C.c_uint64)
    i_arr = np.array([4, 9, 4], dtype=np.uint64)
    arg, keep, _ = hash_tags_arg(KEY, [w.tag(i) for i in (4, 9, 4)])
    bad_form, keep2, _ = hash_tags_arg(KEY, [w.tag(i) for i in (4, 9, 4)])
    bad_form.form = 9
    coeff_tb = t_bottom.clone()
    coeff_tb.intt_all_in_place()
    low = M(p, m_b, t_bottom.ncol, 0, True)
    ragged = M(p, m_b, t_bottom.ncol - 1, top, True)
    foreign = M(other, m_b, t_bottom.ncol, top, True)
    w_stacked = M.from_rns(p, oracle.random_matrix(95, T * s, m_b, moduli, n), True)

    def raw_outs(outs, arr=True):
        return None if not arr else (C.c_void_p * max(len(outs), 1))(*[None if o is None else o.raw.value for o in outs])

    def call(outs, T_=T, P_=NP, part_start=1, secret=s, base_bits=base, idx=i_arr, tags=arg, arr=True, tb=t_bottom):
        return lib.gpupoly_matrix_wee25_targets(raw_outs(outs, arr), T_, P_, None if tb is None else tb.raw, part_start, secret, base_bits,
                                                None if idx is None else idx.ctypes.data_as(u64p), None if tags is None else C.byref(tags))

    def call_product(outs, T_=T, P_=NP, part_start=1, secret=s, base_bits=base, idx=i_arr, arr=True, tb=t_bottom, ws=w_stacked):
        return lib.gpupoly_matrix_wee25_targets_product(raw_outs(outs, arr), T_, P_, None if ws is None else ws.raw, None if tb is None else tb.raw,
                                                        part_start, secret, base_bits, None if idx is None else idx.ctypes.data_as(u64p))

    def swap(o, j, m):
        return o[:j] + [m] + o[j + 1:]

    def view_of(m):
        return m.reshape_view(m.nrow * m.ncol // m_b, m_b)

    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call(swap(o, 4, None)), "null"),
        "null idx": (lambda o: call(o, idx=None), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "null t_bottom": (lambda o: call(o, tb=None), "null"),
        "context mismatch": (lambda o: call(o, tb=foreign), "mismatch"),
        "output of another context": (lambda o: call(swap(o, 1, M(other, s, m_b, top, True))), "mismatch"),
        "level mismatch": (lambda o: call(o, tb=low), "mismatch"),
        "output level": (lambda o: call(swap(o, 5, M(p, s, m_b, 0, True))), "mismatch"),
        "output rows": (lambda o: call(swap(o, 2, M(p, s + 1, m_b, top, True))), "shape"),
        "output columns": (lambda o: call(swap(o, 2, M(p, s, m_b - 1, top, True))), "shape"),
        "secret_size of other outputs": (lambda o: call(o, secret=s + 1), "shape"),
        "t_bottom not EVAL": (lambda o: call(o, tb=coeff_tb), "Eval"),
        "columns no multiple of m_b": (lambda o: call(o, tb=ragged), "multiple"),
        "parts past the columns": (lambda o: call(o, part_start=w.nparts - 1), "past"),
        "part_start past the columns": (lambda o: call(o, part_start=w.nparts + 1), "past"),
        "secret_size 0": (lambda o: call(o, secret=0), "secret_size"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "blocks x parts overflows": (lambda o: call(o, T_=2 ** 63, P_=2), "overflow"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "output overlaps t_bottom": (lambda o: call(swap(o, 3, view_of(t_bottom).row_view(s, 2 * s))), "overlap"),
        "the same output twice": (lambda o: call(swap(o, 5, o[0])), "overlap"),
    }
    product_cases = {
        "null outs": (lambda o: call_product(o, arr=False), "null"),
        "null output": (lambda o: call_product(swap(o, 0, None)), "null"),
        "null idx": (lambda o: call_product(o, idx=None), "null"),
        "null w_stacked": (lambda o: call_product(o, ws=None), "null"),
        "null t_bottom": (lambda o: call_product(o, tb=None), "null"),
        "w_stacked rows": (lambda o: call_product(o, ws=M(p, T * s + 1, m_b, top, True)), "shape"),
        "w_stacked columns": (lambda o: call_product(o, ws=M(p, T * s, m_b + 1, top, True)), "shape"),
        "w_stacked of another context": (lambda o: call_product(o, ws=M(other, T * s, m_b, top, True)), "mismatch"),
        "w_stacked level": (lambda o: call_product(o, ws=M(p, T * s, m_b, 0, True)), "mismatch"),
        "w_stacked not EVAL": (lambda o: call_product(o, ws=M(p, T * s, m_b, top, False)), "Eval"),
        "t_bottom not EVAL": (lambda o: call_product(o, tb=coeff_tb), "Eval"),
        "parts past the columns": (lambda o: call_product(o, part_start=w.nparts - 1), "past"),
        "secret_size 0": (lambda o: call_product(o, secret=0), "secret_size"),
        "base_bits 63": (lambda o: call_product(o, base_bits=63), "base_bits"),
        "output overlaps w_stacked": (lambda o: call_product(swap(o, 2, w_stacked.row_view(s, 2 * s))), "overlap"),
        "output overlaps t_bottom": (lambda o: call_product(swap(o, 0, view_of(t_bottom).row_view(0, s))), "overlap"),
    }
    kept = {"t_bottom": t_bottom.to_rns(), "w_stacked": w_stacked.to_rns()}

    def check(entry, name, fn, word):
        outs = [M.from_rns(p, sentinel, False) for _ in range(T * NP)]  # COEFF-tagged: a tag flipped to EVAL would change the read-out
        gpu.gpu_device_sync()
        c0 = lib.gpupoly_launch_count()
        _ffi.trace_begin()
        rc = fn(outs)
        msg = _ffi.last_error_string()
        trace = _ffi.trace_end()
        assert rc != 0, name
        assert entry + ":" in msg and word in msg, (name, msg)
        assert trace == [] and lib.gpupoly_launch_count() == c0, (name, trace)
        for o in outs:
            assert not o.is_ntt and np.array_equal(o.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(ENTRY, name, fn, word)
    for name, (fn, word) in product_cases.items():
        check(PRODUCT, name, fn, word)
    # an output that overlaps another output through a row view of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, T * NP * s, m_b, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(j * s, (j + 1) * s) for j in range(T * NP)]
    views[1] = parent.row_view(s - 1, 2 * s - 1)
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY + ":" in _ffi.last_error_string()
    assert call_product(views) != 0 and "overlap" in _ffi.last_error_string() and PRODUCT + ":" in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    assert np.array_equal(t_bottom.to_rns(), kept["t_bottom"]) and np.array_equal(w_stacked.to_rns(), kept["w_stacked"])
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and no blocks or no parts launch nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(T * NP)]
    assert call(outs) == 0
    disjoint = [parent.row_view(j * s, (j + 1) * s) for j in range(T * NP)]
    assert call(disjoint) == 0
    want = w.t_top_target_blocks(t_bottom, [4, 9, 4], 1, NP)
    for j, (o, v) in enumerate(zip(outs, disjoint)):
        o.is_ntt = v.is_ntt = True
        assert o == v and o == want[j // NP][j % NP]
    assert call_product([M.from_rns(p, sentinel, False) for _ in range(T * NP)]) == 0
    gpu.gpu_device_sync()
    c0 = lib.gpupoly_launch_count()
    _ffi.trace_begin()
    assert call([], T_=0) == 0 and call([], P_=0) == 0 and call([], T_=0, arr=False, idx=None, tags=None, tb=None) == 0
    assert call_product([], T_=0, arr=False, idx=None, tb=None, ws=None) == 0 and call_product([], P_=0) == 0
    assert _ffi.trace_end() == [] and lib.gpupoly_launch_count() == c0
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the literal loop
    default = w.t_top_target_blocks(t_bottom, [4, 9], 1, NP)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check(ENTRY, "reference keying", lambda o: call(o), "unsupported")
    assert call_product([M.from_rns(p, sentinel, False) for _ in range(T * NP)]) == 0  # no sampling: any keying
    fallen = w.t_top_target_blocks(t_bottom, [4, 9], 1, NP)
    for t, idx in enumerate((4, 9)):
        for q in range(NP):
            part = 1 + q
            assert fallen[t][q] == w.t_top_target_block(idx, part * m_b, t_bottom.slice_columns(part * m_b, (part + 1) * m_b))
            assert not (fallen[t][q] == default[t][q])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert w.t_top_target_blocks(t_bottom, [4, 9], 1, NP)[1][1] == default[1][1]
    del keep, keep2
