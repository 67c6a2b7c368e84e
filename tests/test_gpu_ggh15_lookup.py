"""GPU: the GGH15 online public lookup for many slots in one call (`gpupoly_matrix_ggh15_lookup`, mxx_amd/ggh15_eval.py;
DESIGN.md section 5w).

Everything in the lookup formula is exact arithmetic on canonical residues, so the bar is equality, bit for bit
(gpu_matrix_equal), with `build_public_lookup_output_chunk` - the reference's function (src/lookup/ggh15/encoding.rs:172-300)
restated with the mirror's older operations, one slot and one chunk at a time, in the reference's own association order.
The formula needs no real preimages, so the operands are uniform random; that literal output is computed once per (context,
d, r, chunk, slot definition) and shared by the slot counts.  Independently of the engine the same outputs are computed with
tests/plainref.py from the ORIGINAL association c_b0 (P rhs), fed with the CPU restatement's samples; the combine entry
alone (`gpupoly_matrix_ggh15_lookup_combine`, which takes the digits as given) is held to plainref in every modulus width
class with operands no sampler produces; and with real trapdoors and noise-free preimages the lookup returns exactly
s (A_out - G o y), the assertion of the reference's test_gpu_ggh15_plt_eval_multi_inputs (src/lookup/ggh15/gpu_tests.rs:161-175)."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import CELLS, _cell, _cell_id, _eval_slots, _params, _rand, _top, _windows
from test_gpu_lut_targets import full_modulus, gy_block, y_values

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_ggh15_lookup"
COMBINE = "gpupoly_matrix_ggh15_lookup_combine"
# (n, depth, bits, base_bits): one word per limb vector lane (n = 2: the scalar-word kernels), n = 4, 32-bit words packed and
# unpacked, 64-bit words, the GGH15 chain's ring
CONTEXTS = {"n2_17": (2, 1, 17, 17), "n4_24": (4, 2, 24, 12), "n16_24": (16, 2, 24, 12), "n16_28": (16, 2, 28, 14),
            "n16_51": (16, 2, 51, 17), "n256_51": (256, 3, 51, 17)}
KEY = bytes((7 * i + 5) & 0xFF for i in range(32))
GATE_ID, LUT_ID, LUT_SIZE = 11, 3, 8
NDEFS = 7  # slot t of a call is definition t % NDEFS
_WORLD, _LITERAL = {}, {}


def lut_of(moduli):
    """x -> (k, y): rows 9, 10, 11 are consecutive (the DECIMAL tag form grows a digit), the others are not"""
    ys = y_values(moduli)
    return {0: (9, ys[0]), 1: (10, ys[1]), LUT_SIZE - 1: (11, ys[2]), 2: (4, ys[3]), 3: (0, ys[4]), 4: ((1 << 40) + 3, 77)}


class World:
    """what the tests of one (context, d) share, computed once and left unchanged"""

    def __init__(self, gpu, oracle, ctx, d):
        from mxx_amd import ggh15_eval

        self.gpu, self.ctx, self.d = gpu, ctx, d
        p = self.p = make_params(gpu, oracle, *CONTEXTS[ctx])
        M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
        self.m_g, self.w = d * p.modulus_digits(), d * (p.modulus_digits() + 2)
        rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
        lut = lut_of(moduli)
        self.shared = ggh15_eval.PublicLookupShared(
            p, KEY, GATE_ID, LUT_ID, d, rand(700, self.w, self.w), *[rand(701 + i, self.w, self.m_g) for i in range(4)], lut,
            {k: rand(710 + i, self.w, self.m_g) for i, (k, _) in enumerate(lut.values())}, chunk_width=max(1, self.m_g // 2))
        nonconst = [2, 5, 0, 7][:n]
        xs = [[0], [1], [LUT_SIZE - 1], nonconst, [1], [3], [4]]  # definition 4 shares its LUT row with definition 1
        self.xs = [gpu.GpuDCRTPoly.from_biguints(p, x) for x in xs]
        self.c_b0 = [rand(730 + t, 3, self.w) for t in range(NDEFS)]
        self.c_in = [rand(740 + t, 3, self.m_g) for t in range(NDEFS)]
        self._rows = {}

    def slots(self, S, r, order=None):
        """(c_b0s, c_ins, xs, rows) of the slots `order` (default: 0 .. S - 1) with r rows each"""
        order = list(range(S)) if order is None else list(order)
        for t in {t % NDEFS for t in order}:
            if (t, r) not in self._rows:
                self._rows[(t, r)] = (self.c_b0[t].slice(0, r, 0, self.w), self.c_in[t].slice(0, r, 0, self.m_g))
        defs = [t % NDEFS for t in order]
        xs = [self.xs[t] for t in defs]
        return [self._rows[(t, r)][0] for t in defs], [self._rows[(t, r)][1] for t in defs], xs, [self.shared.get(x.const_coeff_u64()) for x in xs]

    def literal(self, r, chunk, t):
        from mxx_amd import ggh15_eval

        key = (self.ctx, self.d, r, chunk, t % NDEFS)
        if key not in _LITERAL:
            b0, cin, xs, _ = self.slots(1, r, [t])
            _LITERAL[key] = ggh15_eval.build_public_lookup_output_chunk(self.shared, b0[0], cin[0], xs[0], *chunk)
        return _LITERAL[key]

    def chunks(self):
        p, d, m_g = self.p, self.d, self.m_g
        dpt = -(-p.crt_bits() // p.base_bits())
        k = p.modulus_digits()
        out = {"first": (0, min(9, m_g)), "across a tower": (dpt - 1, min(3, m_g - dpt + 1)), "ragged last": (m_g - 1, 1)}
        if d > 1:
            out["across a block row"] = (k - 1, min(5, m_g - k + 1))
        return out

    def stage2(self, S, r, chunk, order=None):
        from mxx_amd import ggh15_eval

        b0, cin, xs, rows = self.slots(S, r, order)
        mids = ggh15_eval.public_lookup_stage1(self.shared, b0, cin)
        return ggh15_eval.public_lookup_stage2(self.shared, mids, rows, xs, chunk)


def world_of(gpu, oracle, ctx, d):
    if (ctx, d) not in _WORLD:
        _WORLD[(ctx, d)] = World(gpu, oracle, ctx, d)
    return _WORLD[(ctx, d)]


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal function
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_one_call_equals_the_literal_function_slot_by_slot(gpu, oracle, ctx, d):
    wd = world_of(gpu, oracle, ctx, d)
    sh = wd.shared
    operands = [sh.preimage_gate1, sh.preimage_gate2_identity, sh.preimage_gate2_gy, sh.preimage_gate2_v, sh.preimage_gate2_vx]
    operands += list(sh.lut_preimages.values()) + wd.c_b0 + wd.c_in + [x.inner for x in wd.xs]
    before = [(m.is_ntt, m.to_rns()) for m in operands]
    chunks = wd.chunks()
    for name, chunk in chunks.items():
        for S in (1, 3, 65):
            got = wd.stage2(S, 1, chunk)
            assert len(got) == S
            for t in range(S):
                assert got[t].size() == (1, chunk[1]) and got[t].is_ntt
                assert got[t] == wd.literal(1, chunk, t), f"{name} chunk {chunk}, slot {t} of {S}"
    # definitions 1 and 4 share a LUT row: the same K matrix and the same tag, each slot its own output
    _, _, xs, rows = wd.slots(5, 1)
    assert rows[1] == rows[4] and sh.lut_preimage_chunk(rows[1][0], 0, 1) is sh.lut_preimage_chunk(rows[4][0], 0, 1)
    assert not (wd.literal(1, chunks["first"], 1) == wd.literal(1, chunks["first"], 4))
    # more rows per encoding vector: the row tile and its ragged end
    chunk = chunks["across a tower"]
    for r in (2, 3):
        for t, out in enumerate(wd.stage2(3, r, chunk)):
            assert out.size() == (r, chunk[1]) and out == wd.literal(r, chunk, t), (r, t)
    # the same slots in another order: every slot's output is its own
    order = list(range(NDEFS))[::-1]
    for t, out in zip(order, wd.stage2(NDEFS, 1, chunk, order)):
        assert out == wd.literal(1, chunk, t), t
    # every input, residues and tag, as it was
    for m, (tag, res) in zip(operands, before):
        assert m.is_ntt == tag and np.array_equal(m.to_rns(), res)


def test_the_tag_forms_and_the_whole_width(gpu, oracle):
    from mxx_amd import ggh15_eval

    wd = world_of(gpu, oracle, "n16_51", 2)
    sh, M, chunk = wd.shared, gpu.GpuDCRTPolyMatrix, (3, 5)
    b0, cin, xs, rows = wd.slots(3, 1)
    assert isinstance(sh.v_tags([k for k, _ in rows]), gpu.IndexedTags)  # DECIMAL on the device: 9, 10, 11
    assert isinstance(sh.v_tags([k for k, _ in wd.slots(NDEFS, 1)[3]]), list)  # a table of literal tags
    mids = ggh15_eval.public_lookup_stage1(sh, b0, cin)
    ks = [sh.lut_preimage_chunk(k, *chunk) for k, _ in rows]
    x_mats = [x.inner for x in xs]
    ys = [y for _, y in rows]
    for decimal in (False, True):  # LE64 and DECIMAL generated on the device against the table of the same literal tags
        tags = gpu.IndexedTags(b"some_prefix_", (1 << 32) + 98, 3, decimal=decimal)
        indexed = M.ggh15_lookup(mids, ks, x_mats, chunk[0], chunk[1], ys, KEY, tags)
        table = M.ggh15_lookup(mids, ks, x_mats, chunk[0], chunk[1], ys, KEY, list(tags))
        assert all(a == b for a, b in zip(indexed, table)) and not (indexed[0] == indexed[1])
    # all chunks of the output row, concatenated: the public entry against the literal per-slot loop
    b0, cin, xs, rows = wd.slots(5, 2)
    got = ggh15_eval.public_lookup_slots(sh, b0, cin, xs, chunk_width=5)
    assert [y for _, y in got] == [y for _, y in rows]
    chunks = sh.column_chunks(5)
    assert wd.m_g == 12 and chunks == [(0, 5), (5, 5), (10, 2)]  # a ragged last chunk
    for t, (vec, _) in enumerate(got):
        assert vec.size() == (2, wd.m_g) and vec == ggh15_eval._literal_slot(sh, b0[t], cin[t], xs[t], chunks), t
    assert ggh15_eval.public_lookup_slots(sh, [], [], []) == []


def test_several_groups_equal_the_ungrouped_call(gpu, oracle, hip_env):
    wd = world_of(gpu, oracle, "n16_51", 2)
    p, chunk, r = wd.p, (3, 5), 2
    whole = wd.stage2(NDEFS, r, chunk)
    slot_bytes = (wd.m_g * chunk[1] + r * (wd.m_g + wd.w)) * len(p.moduli()) * p.ring_dimension() * 8
    for budget in (1, 3 * slot_bytes):  # one slot per group; groups of 3, 3 and 1
        hip_env.set("MXX_HIP_GGH15_LOOKUP_BUDGET", str(budget))
        for t, (a, b) in enumerate(zip(wd.stage2(NDEFS, r, chunk), whole)):
            assert a == b and a == wd.literal(r, chunk, t), (budget, t)
    hip_env.unset("MXX_HIP_GGH15_LOOKUP_BUDGET")


# ---------------------------------------------------------------------------------------------------
# 2. independence from the engine: plainref from the original association, fed with the CPU restatement's samples
# ---------------------------------------------------------------------------------------------------
def digits_eval(u, moduli, base, dpt, slots):
    """G^-1(u) in the evaluation domain: u (rows, cols, L, n) coefficient residues -> (rows * k, cols, L, len(slots))"""
    rows, cols, L, _ = u.shape
    k = L * dpt
    out = np.zeros((rows * k, cols, L, len(slots)), dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            out[r * k:(r + 1) * k, c] = _eval_slots(P.digits(u[r, c], moduli, base, dpt), moduli, slots)
    return out


@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_outputs_equal_the_plain_reference_in_the_original_association(gpu, oracle, ctx):
    d, S, r = 2, 3, 1
    wd = world_of(gpu, oracle, ctx, d)
    sh, p = wd.shared, wd.p
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k, m_g = L * dpt, wd.m_g
    slots = list(range(n))
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    p_g1, p_id, p_gy, p_v, p_vx = (m.to_rns() for m in (sh.preimage_gate1, sh.preimage_gate2_identity, sh.preimage_gate2_gy,
                                                        sh.preimage_gate2_v, sh.preimage_gate2_vx))
    u_g = oracle.sample_distribution(d, m_g, moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, sh.u_g_tag()), full_ncol=m_g, col_offset=0)
    u_g_dec = digits_eval(u_g, moduli, base, dpt, slots)
    prod = lambda a, b: P.slot_mul_sum(None, [a], [b], moduli, False)  # noqa: E731
    b0s, cins, xs, rows = wd.slots(3 + S, r, [3, 4, 5])  # the non-constant x, the shared LUT row, the three-word y
    for chunk in ((0, 4), (k - 1, 2)):
        got = wd.stage2(S, r, chunk, [3, 4, 5])
        for s in range(S):
            (row, y), x = rows[s], xs[s].inner.to_rns()[0, 0]
            c_b0, c_in = b0s[s].to_rns(), cins[s].to_rns()
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, sh.v_tag(row)),
                                           full_ncol=m_g, col_offset=chunk[0])
            v = digits_eval(u, moduli, base, dpt, slots)
            v_x = ((v.astype(object) * x.astype(object).reshape(1, 1, L, n)) % q_col).astype(np.uint64)
            k_chunk = sh.lut_preimages[row].to_rns()[:, chunk[0]:chunk[0] + chunk[1]]
            # c_b0 (P rhs), as the reference multiplies
            plus = P.slot_mul_sum(prod(c_b0, p_id[:, chunk[0]:chunk[0] + chunk[1]]), [c_b0, c_b0, c_b0, prod(c_in, u_g_dec)],
                                  [prod(p_gy, gy_block(moduli, n, base, dpt, y, d, chunk)), prod(p_v, v), prod(p_vx, v_x), v], moduli, False)
            want = P.slot_mul_sum(plus, [c_b0], [prod(p_g1, k_chunk)], moduli, True)
            assert np.array_equal(got[s].to_rns(), want), (ctx, chunk, s)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """Every matrix of the call at level 0 / 1 of a three-limb context (the refusal list below only shows that MIXED levels
    are turned away): m_g = d * dpt * (level + 1) with dpt from the CONTEXT's crt_bits (one width per basis here, so plainref
    derives the same dpt from the truncated basis), V_s sampled in limbs 0..level only, and the stage-2 formula of the header
    in plainref at moduli[: level + 1] - the stage-1 products are given as random matrices, the formula needs no more; the
    combine entry with the digits given must write the same words."""
    n, d, S, r = 16, 2, 3, 2
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    m_g, w = d * k, d * (k + 2)
    slots = list(range(n))
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    rnd = lambda seed, rows, cols: oracle.random_matrix(seed + level, rows, cols, moduli, n)  # noqa: E731
    mids_np = [rnd(760 + 3 * i, S * r, m_g) for i in range(5)] + [rnd(775, S * r, w)]
    mid_id, mid_gy, mid_v, mid_vx, mid_rand, mid_g1 = mids_np
    mids = [M.from_rns(p, a, True) for a in mids_np]
    xs_np = [rnd(780 + 3 * s, 1, 1) for s in range(S)]  # non-constant plaintexts: EVAL residues
    xs = [M.from_rns(p, x, True) for x in xs_np]
    ys = list(y_values(moduli)[2:5])  # Q - 1, Q + 5 and the three-word y
    tags = [b"ggh15_low_level_v_" + bytes([48 + s]) for s in range(S)]
    for chunk in ((0, min(4, m_g)), (k - 1, 2)):
        cols = slice(chunk[0], chunk[0] + chunk[1])
        ks_np = [rnd(790 + 3 * s, w, chunk[1]) for s in range(S)]
        ks = [M.from_rns(p, a, True) for a in ks_np]
        got = M.ggh15_lookup(mids, ks, xs, chunk[0], chunk[1], ys, KEY, tags)
        vs = []
        for s in range(S):
            rows = slice(s * r, (s + 1) * r)
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tags[s]),
                                           full_ncol=m_g, col_offset=chunk[0])
            v = digits_eval(u, moduli, base, dpt, slots)
            vs.append(v)
            x = xs_np[s][0, 0].astype(object).reshape(1, 1, L, n)
            lhs = ((mid_v[rows].astype(object) + x * mid_vx[rows].astype(object) + mid_rand[rows].astype(object)) % q_col).astype(np.uint64)
            plus = P.slot_mul_sum(mid_id[rows, cols], [mid_gy[rows], lhs], [gy_block(moduli, n, base, dpt, ys[s], d, chunk), v], moduli, False)
            want = P.slot_mul_sum(plus, [mid_g1[rows]], [ks_np[s]], moduli, True)
            assert got[s].level == level and got[s].is_ntt and got[s].size() == (r, chunk[1])
            assert np.array_equal(got[s].to_rns(), want), (bits, level, chunk, s)
        given = M.ggh15_lookup_combine(mids, ks, xs, M.from_rns(p, np.concatenate(vs, axis=1), True), chunk[0], chunk[1], ys)
        for s in range(S):
            assert given[s] == got[s], (bits, level, chunk, s)


# ---------------------------------------------------------------------------------------------------
# 3. the combine entry alone in every width class
# ---------------------------------------------------------------------------------------------------
SMALL_WINDOWS = {("class", 31), ("class", 62)}  # the classes whose lazy window is shorter than the term count
SECRET_SIZE = {(62, 31): 2}  # d per (bits, base_bits), 1 elsewhere: 62 bits, base 31 at d = 2 puts a fold on the V / K seam


def fold_places(window, m_g, w, dpt):
    """where the accumulator is folded before the final reduction, for terms 0 .. m_g + w + dpt - 1 in the kernel's order
    (V, K, the gy words): before every term t > 0 with t % window == 0"""
    places = set()
    for t in range(window, m_g + w + dpt, window):
        places.add("inside V" if t < m_g else "seam" if t == m_g else "inside K" if t < m_g + w else "epilogue")
    return places


def combine_want(mids, luts, xs, digits, moduli, n, base, dpt, d, chunk, ys, r, slots):
    """plainref: mid_id[:, chunk] + mid_gy gy + mid_v V + (x o mid_vx) V + mid_rand V + (-mid_g1) K, slot by slot"""
    L, c = len(moduli), chunk[1]
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    out = []
    for s in range(len(ys)):
        m_id, m_gy, m_v, m_vx, m_rand, m_g1 = (m[s * r:(s + 1) * r] for m in mids)
        x_vx = ((m_vx.astype(object) * xs[s].astype(object).reshape(1, 1, L, n)) % q_col).astype(np.uint64)
        neg_g1 = ((q_col - m_g1.astype(object)) % q_col).astype(np.uint64)
        v = digits[:, s * c:(s + 1) * c]
        out.append(P.slot_mul_sum(m_id[:, chunk[0]:chunk[0] + c], [m_gy, m_v, x_vx, m_rand, neg_g1],
                                  [gy_block(moduli, n, base, dpt, ys[s], d, chunk), v, v, v, luts[s]], moduli, False, slots))
    return out


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_combine_entry_alone_in_every_width_class(gpu, cell):
    n, moduli, bases, slots = _cell(cell)
    M, L = gpu.GpuDCRTPolyMatrix, len(moduli)
    bits = max(int(q).bit_length() for q in moduli)
    windows = _windows(moduli)
    seen = set()
    for base in bases:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        d = SECRET_SIZE.get((bits, base), 1)
        k = L * dpt
        m_g, w = d * k, d * (k + 2)
        chunk = (0, m_g)  # every (block row, tower, digit) column
        for window in windows:
            seen |= fold_places(window, m_g, w, dpt)
            if window < m_g + w + dpt:
                assert (m_g + w + dpt + 1) % window != 0
        rng = np.random.default_rng(2000 + bits + base)
        # the worst case: every residue of every operand q - 1 (x = q_t - 1 in every limb t) and y = 2^(bits - 1) - 1, below every
        # modulus of a class, whose digits below the last are 2^base - 1 in every tower
        for kind, S, r in (("top", 1, 1), ("random", 2, 2), ("gate1 zero", 2, 3)):
            make = (lambda rows, cols: _top(rows, cols, moduli, n)) if kind == "top" else (lambda rows, cols: _rand(rng, rows, cols, moduli, n))
            mids = [make(S * r, m_g) for _ in range(5)] + [make(S * r, w)]
            if kind == "gate1 zero":  # neg(0) = 0, not q
                mids[5][:] = 0
                mids[5][0, 1] = make(1, 1)[0, 0]
            luts, xs, digits = [make(w, m_g) for _ in range(S)], [make(1, 1)[0, 0] for _ in range(S)], make(m_g, S * m_g)
            ys = [(1 << (bits - 1)) - 1] * S if kind == "top" else [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(S)]
            got = M.ggh15_lookup_combine([M.from_rns(p, m, True) for m in mids], [M.from_rns(p, m, True) for m in luts],
                                         [M.from_rns(p, x.reshape(1, 1, L, n), True) for x in xs], M.from_rns(p, digits, True), chunk[0], chunk[1], ys)
            want = combine_want(mids, luts, xs, digits, moduli, n, base, dpt, d, chunk, ys, r, slots)
            for s in range(S):
                assert got[s].size() == (r, m_g) and got[s].is_ntt
                res = got[s].to_rns()
                assert np.array_equal(res[..., slots], want[s]), (cell, base, kind, s)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(res, np.broadcast_to(want[s][..., :1], res.shape)), (cell, base, s)
    if cell in SMALL_WINDOWS:  # a fold inside V, on the V / K seam and among the epilogue's terms
        assert {"inside V", "seam", "epilogue"} <= seen, seen


# ---------------------------------------------------------------------------------------------------
# 4. end to end, noise-free: real trapdoors, real preimages
# ---------------------------------------------------------------------------------------------------
def test_noise_free_lookup_returns_the_encoding_of_the_lut_value(gpu, oracle):
    from mxx_amd import ggh15_eval, lookup as L
    from test_gpu_gate_targets import BASE, BITS, DEPTH, N, gseed

    d, sigma = 1, 0.0
    p = make_params(gpu, oracle, N, DEPTH, BITS, BASE)
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    m_g, w = d * p.modulus_digits(), d * (p.modulus_digits() + 2)
    rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    (td0, b0), (td1, b1) = sampler.trapdoor(p, d), sampler.trapdoor(p, d)
    assert b0.size() == b1.size() == (d, w)
    w_id, w_gy, w_v, a_in = (rand(800 + i, d, m_g) for i in range(4))
    gates = L.GateShared(p, KEY, LUT_ID, b1, w_id, w_gy, w_v)
    w_vx = gates.w_vx_columns(0, m_g)
    hs = gates.sampler()
    a_out = hs.sample_hash(p, KEY, gates.a_out_tag(GATE_ID), d, m_g, gpu.DistType.FinRingDist())
    u_g = hs.sample_hash(p, KEY, gates.u_g_tag(GATE_ID), d, m_g, gpu.DistType.FinRingDist())
    s_seed = gseed(gpu, 900)
    # the five gate-stage targets with error_sigma = 0 and their preimages under B0
    targets = [L.build_gate_stage1_target_chunk(gates, s_seed, None, sigma, 0, w),
               L.build_gate_stage2_target_chunk(gates, GATE_ID, s_seed, None, sigma, 0, m_g),
               L.build_gate_stage3_target_chunk(gates, s_seed, None, sigma, 0, m_g),
               L.build_gate_stage4_target_chunk(gates, GATE_ID, s_seed, a_in, None, sigma, 0, m_g),
               L.build_gate_stage5_target_chunk(gates, s_seed, u_g, None, sigma, 0, m_g)]
    s_g = L.sample_gate_secret(p, d, s_seed)
    gadget = M.gadget_matrix(p, d)
    assert targets[0] == s_g * b1 and targets[1] == s_g * w_id + a_out and targets[2] == s_g * w_gy - gadget
    assert targets[3] == s_g * w_v - a_in * u_g.decompose() and targets[4] == s_g * w_vx + u_g
    p_g1, p_id, p_gy, p_v, p_vx = sampler.preimage_many_abi(p, td0, b0, targets)
    for pre, target in zip((p_g1, p_id, p_gy, p_v, p_vx), targets):
        assert b0 * pre == target
    # a 4-row LUT x -> (x, y_x) and its row preimages under B1
    ys = [5, full_modulus(moduli) - 1, 12345, 1]
    luts = L.LutShared(p, KEY, LUT_ID, w_id, w_gy, w_v, w_vx)
    pairs = L.sample_lut_preimages(luts, sampler, td1, b1, [(x, y) for x, y in enumerate(ys)], (0, m_g))
    for target, pre in pairs:
        assert b1 * pre == target
    shared = ggh15_eval.PublicLookupShared(p, KEY, GATE_ID, LUT_ID, d, p_g1, p_id, p_gy, p_v, p_vx, {x: (x, y) for x, y in enumerate(ys)},
                                           {x: pre for x, (_, pre) in enumerate(pairs)})
    # three slots, each with its own secret s: c_b0 = s B0, c_in = s (A_in - G o x)
    x_values = [0, 1, 3]
    secrets = [rand(820 + t, 1, d) for t in range(3)]
    xs = [gpu.GpuDCRTPoly.from_usize_to_constant(p, x) for x in x_values]
    c_b0s = [s * b0 for s in secrets]
    c_ins = [s * (a_in - gadget * x) for s, x in zip(secrets, xs)]
    got = ggh15_eval.public_lookup_slots(shared, c_b0s, c_ins, xs, chunk_width=4)
    assert len(got) == 3
    for s, x, (vec, y) in zip(secrets, x_values, got):
        assert y == ys[x]
        assert vec == s * (a_out - gadget * gpu.GpuDCRTPoly.from_elem_to_constant(p, y)), x


# ---------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_slot_count(gpu, oracle):
    from mxx_amd import _ffi, ggh15_eval

    wd = world_of(gpu, oracle, "n256_51", 2)
    sh, M, chunk = wd.shared, gpu.GpuDCRTPolyMatrix, (0, 4)

    def trace(fn):
        _ffi.trace_begin()
        fn()
        events = _ffi.trace_end()
        return [e["kernel"] for e in events if e["threads"]], [e["kernel"] for e in events if not e["threads"]]  # copies: no threads

    legs = {}
    for S in (2, 48):
        b0, cin, xs, rows = wd.slots(S, 1)
        mids = ggh15_eval.public_lookup_stage1(sh, b0, cin)
        tags = [sh.v_tag(k) for k, _ in rows]
        ks = [sh.lut_preimage_chunk(k, *chunk) for k, _ in rows]
        x_mats, ys = [x.inner for x in xs], [y for _, y in rows]
        legs[S] = dict(
            full=trace(lambda: M.ggh15_lookup(mids, ks, x_mats, chunk[0], chunk[1], ys, KEY, tags)),
            sampler=trace(lambda: M.sample_hash_decomposed_blocks(wd.p, KEY, tags, wd.d, wd.m_g, chunk[0], chunk[1], _ffi.GPU_MATRIX_DIST_UNIFORM)))
        digits = M.sample_hash_decomposed_blocks(wd.p, KEY, tags, wd.d, wd.m_g, chunk[0], chunk[1], _ffi.GPU_MATRIX_DIST_UNIFORM)
        legs[S]["combine"] = trace(lambda: M.ggh15_lookup_combine(mids, ks, x_mats, digits, chunk[0], chunk[1], ys))
    b0, cin, xs, _ = wd.slots(2, 1)
    loop = trace(lambda: [ggh15_eval.build_public_lookup_output_chunk(sh, b0[t], cin[t], xs[t], *chunk) for t in range(2)])
    two, many = legs[2], legs[48]
    print(f"stage 2 kernels: 48 slots {len(many['full'][0])} {many['full'][0]}, copies {many['full'][1]}; 2 slots {len(two['full'][0])}; "
          f"combine entry {len(many['combine'][0])}; sampler alone {len(many['sampler'][0])}; the literal loop for 2 slots "
          f"{len(loop[0])} kernels and {len(loop[1])} copies")
    assert many["full"] == two["full"] and many["combine"] == two["combine"]
    # the pre-pass and the main kernel behind the table copy; the sampling entry adds the sampler's launches and nothing else
    assert len(many["combine"][0]) == 2 and len(many["combine"][1]) == 1
    assert sorted(many["full"][0]) == sorted(many["sampler"][0] + many["combine"][0])
    assert sorted(many["full"][1]) == sorted(many["sampler"][1] + many["combine"][1])
    assert len(many["full"][0]) < len(loop[0])


# ---------------------------------------------------------------------------------------------------
# 6. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi, ggh15_eval
    from mxx_amd.matrix import hash_tags_arg

    wd = world_of(gpu, oracle, "n16_24", 2)
    sh, p = wd.shared, wd.p
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m_g, w, c, S, r, top = wd.m_g, wd.w, 2, 3, 2, len(p.moduli()) - 1
    b0, cin, xs, rows = wd.slots(S, r)
    names = ("mid_identity", "mid_gy", "mid_v", "mid_vx", "mid_rand", "mid_gate1")
    mids = dict(zip(names, ggh15_eval.public_lookup_stage1(sh, b0, cin)))
    luts = [sh.lut_preimage_chunk(k, 1, c) for k, _ in rows]
    x_mats = [x.inner for x in xs]
    sentinel = oracle.random_matrix(95, r, c, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    u64p = C.POINTER(C.c_uint64)
    y_arr = np.arange(1, 2 * S + 1, dtype=np.uint64)
    arg, keep, _ = hash_tags_arg(KEY, [b"a", b"bb", b"ccc"])
    bad_form, keep2, _ = hash_tags_arg(KEY, [b"a", b"bb", b"ccc"])
    bad_form.form = 9
    coeff_mid, coeff_k, coeff_x = mids["mid_v"].clone(), luts[1].clone(), x_mats[2].clone()
    for m in (coeff_mid, coeff_k, coeff_x):
        m.intt_all_in_place()

    def array(ms):
        return None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])

    def call(outs, S_=S, col_start=1, base_bits=base, y=y_arr, wpy=2, tags=arg, ks=luts, xv=x_mats, arr=True, **over):
        ms = dict(mids, **over)
        return lib.gpupoly_matrix_ggh15_lookup(array(outs) if arr else None, S_, *[None if ms[name] is None else ms[name].raw for name in names],
                                               array(ks), array(xv), col_start, base_bits, None if y is None else y.ctypes.data_as(u64p), wpy,
                                               None if tags is None else C.byref(tags))

    def rows_of(m, lo, hi):  # r x c views into an operand's storage
        return m.reshape_view(m.nrow * m.ncol // c, c).row_view(lo, hi)

    new = lambda rows, cols, params=p, level=top: M(params, rows, cols, level, True)  # noqa: E731
    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null lut_preimages": (lambda o: call(o, ks=None), "null"),
        "null lut_preimages entry": (lambda o: call(o, ks=[luts[0], None, luts[2]]), "null"),
        "null xs": (lambda o: call(o, xv=None), "null"),
        "null xs entry": (lambda o: call(o, xv=[None] + x_mats[1:]), "null"),
        "null y_words": (lambda o: call(o, y=None), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "null operand": (lambda o: call(o, mid_rand=None), "null"),
        "context mismatch": (lambda o: call(o, mid_vx=new(S * r, m_g, other)), "mismatch"),
        "K of another context": (lambda o: call(o, ks=[luts[0], new(w, c, other), luts[2]]), "mismatch"),
        "output of another context": (lambda o: call([o[0], new(r, c, other), o[2]]), "mismatch"),
        "level mismatch": (lambda o: call(o, mid_v=new(S * r, m_g, level=0)), "mismatch"),
        "x of another level": (lambda o: call(o, xv=[x_mats[0], new(1, 1, level=0), x_mats[2]]), "mismatch"),
        "mid columns": (lambda o: call(o, mid_gy=new(S * r, m_g - 1)), "shape"),
        "mid rows": (lambda o: call(o, mid_v=new(S * r + 1, m_g)), "shape"),
        "mid_gate1 columns": (lambda o: call(o, mid_gate1=new(S * r, m_g)), "shape"),
        "rows not divisible by S": (lambda o: call(o, **{name: new(S * r + 1, w if name == "mid_gate1" else m_g) for name in names}), "shape"),
        "K rows": (lambda o: call(o, ks=[luts[0], luts[1], new(m_g, c)]), "shape"),
        "K columns": (lambda o: call(o, ks=[new(w, c + 1), luts[1], luts[2]]), "shape"),
        "x not 1 x 1": (lambda o: call(o, xv=[x_mats[0], x_mats[1], new(1, 2)]), "shape"),
        "output rows": (lambda o: call([o[0], o[1], new(r + 1, c)]), "shape"),
        "outputs of different widths": (lambda o: call([o[0], o[1], new(r, c + 1)]), "width"),
        "mid not EVAL": (lambda o: call(o, mid_v=coeff_mid), "Eval"),
        "K not EVAL": (lambda o: call(o, ks=[luts[0], coeff_k, luts[2]]), "Eval"),
        "x not EVAL": (lambda o: call(o, xv=[x_mats[0], x_mats[1], coeff_x]), "Eval"),
        "chunk past m_g": (lambda o: call(o, col_start=m_g - 1), "past"),
        "col_start past m_g": (lambda o: call(o, col_start=m_g + 1), "past"),
        "words_per_y 0": (lambda o: call(o, wpy=0), "words_per_y"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
    }
    for name in names:  # every stage-1 product overlapped through a row view
        cases[f"output overlaps {name}"] = (lambda o, name=name: call([o[0], rows_of(mids[name], r, 2 * r), o[2]]), "overlap")
    # a K_s and an x_s overlapped through views: of the K's own rows, and of a parent whose first polynomial is the slot's x
    cases["output overlaps a K"] = (lambda o: call([o[0], o[1], rows_of(luts[0], 1, 1 + r)]), "overlap")
    x_parent = M.from_rns(p, oracle.random_matrix(96, 2 * r, c, moduli, n), True)
    x_view = x_parent.reshape_view(2 * r * c, 1).row_view(1, 2)
    cases["output overlaps an x"] = (lambda o: call([x_parent.row_view(0, r), o[1], o[2]], xv=[x_mats[0], x_view, x_mats[2]]), "overlap")
    operands = {name: m.to_rns() for name, m in mids.items()}
    held = [m.to_rns() for m in luts + x_mats + [x_parent]]

    def check(name, fn, word):
        outs = [M.from_rns(p, sentinel, False) for _ in range(S)]  # COEFF-tagged: a tag flipped to EVAL would change the read-out
        _ffi.trace_begin()
        c0 = lib.gpupoly_launch_count()
        rc = fn(outs)
        msg = _ffi.last_error_string()
        assert _ffi.trace_end() == [] and lib.gpupoly_launch_count() == c0, name
        assert rc != 0, name
        assert ENTRY in msg and word in msg, (name, msg)
        for o in outs:
            assert not o.is_ntt and np.array_equal(o.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # two outputs overlapping through views of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, 3 * r, c, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, r), parent.row_view(r - 1, 2 * r - 1), parent.row_view(2 * r, 3 * r)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for name, m in mids.items():
        assert np.array_equal(m.to_rns(), operands[name]), name
    for m, res in zip(luts + x_mats + [x_parent], held):
        assert np.array_equal(m.to_rns(), res)
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and S = 0, c = 0 launch nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(S)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * r, (t + 1) * r) for t in range(3)]
    assert call(disjoint) == 0
    for o, v in zip(outs, disjoint):
        o.is_ntt = v.is_ntt = True
        assert o == v
    c0 = lib.gpupoly_launch_count()
    assert call([], S_=0) == 0 and call([], S_=0, arr=False, y=None, tags=None, ks=None, xv=None) == 0
    assert call([new(r, 0) for _ in range(S)], ks=[new(w, 0) for _ in range(S)]) == 0
    assert lib.gpupoly_launch_count() == c0
    # the combine entry names itself
    assert lib.gpupoly_matrix_ggh15_lookup_combine(array(outs), S, *[mids[name].raw for name in names], array(luts), array(x_mats), 1, base,
                                                   y_arr.ctypes.data_as(u64p), 2, new(m_g, S * c + 1).raw) != 0
    assert COMBINE in _ffi.last_error_string() and "shape" in _ffi.last_error_string()
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the literal loop
    default = ggh15_eval.public_lookup_slots(sh, b0, cin, xs, chunk_width=3)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    fallen = ggh15_eval.public_lookup_slots(sh, b0, cin, xs, chunk_width=3)
    for t in range(S):
        assert fallen[t][0] == ggh15_eval._literal_slot(sh, b0[t], cin[t], xs[t], sh.column_chunks(3)) and fallen[t][1] == default[t][1]
        assert not (fallen[t][0] == default[t][0])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert ggh15_eval.public_lookup_slots(sh, b0, cin, xs, chunk_width=3)[2][0] == default[2][0]
    del keep, keep2
