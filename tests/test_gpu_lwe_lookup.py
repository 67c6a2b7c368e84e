"""GPU: the LWE online public lookup for many slots in one call (`gpupoly_matrix_lwe_lookup`, mxx_amd/lwe_lookup.py; DESIGN.md
section 5x).

out_s[:, dst_col .. dst_col + c) = c_b_s K_high_s + c_z_s G^-1(U_s[:, chunk]) is exact arithmetic on canonical residues, so
the bar is equality, bit for bit (gpu_matrix_equal), with the reference's sequence through the mirror's older operations:
`mul` + `mul` + `add` (+ `copy_block` into place) per slot and chunk, and `public_lookup` per slot over the whole width.  The
formula needs no real preimages, so the operands are uniform random; a literal output is computed once per (context, d, r,
chunk, slot definition) and shared by the slot counts.  Independently of the engine the same outputs are computed with
tests/plainref.py fed with the oracle's samples of U_s; the combine entry alone (`gpupoly_matrix_lwe_lookup_combine`, which
takes the digits as given) is held to plainref in every modulus width class with operands no sampler produces; and with a
real trapdoor and noise-free encodings the lookup returns exactly s (A_lt - G o y_s)."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import CELLS, _cell, _cell_id, _params, _rand, _top, _windows
from test_gpu_ggh15_lookup import CONTEXTS, digits_eval
from test_gpu_lut_targets import full_modulus

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_lwe_lookup"
COMBINE = "gpupoly_matrix_lwe_lookup_combine"
KEY = bytes((13 * i + 3) & 0xFF for i in range(32))
GATE_ID, LUT_ID = 23, 5
# slot definition t: (LUT row, slot index); slot t of a call is definition t % NDEFS.  Definitions 1 and 4 share one c_b and
# one K_high matrix (each has its own tag, input vector and output)
DEFS = [(7, 0), (3, 1), (100, 2), (7, 3), (12, 4), ((1 << 40) + 3, 5), (0, None)]
NDEFS = len(DEFS)
_WORLD, _LITERAL = {}, {}


class World:
    """what the tests of one (context, d) share, computed once and left unchanged"""

    def __init__(self, gpu, oracle, ctx, d):
        from mxx_amd import lwe_lookup

        self.gpu, self.ctx, self.d = gpu, ctx, d
        p = self.p = make_params(gpu, oracle, *CONTEXTS[ctx])
        M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
        self.m_g = d * p.modulus_digits()
        self.w = self.m_g + 2 * d if d == 1 else 5  # the library does not tie w to d
        rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
        a = rand(600, d, self.m_g)  # the online side reads neither A_z nor A_lt: LweShared takes d from them
        self.shareds = [lwe_lookup.LweShared(p, KEY, GATE_ID, LUT_ID, slot, a, a) for _, slot in DEFS]
        self.entries = [entry for entry, _ in DEFS]
        self.c_b = [rand(610 + t, 3, self.w) for t in range(NDEFS)]
        self.k_high = [rand(620 + t, self.w, self.m_g) for t in range(NDEFS)]
        self.c_b[4], self.k_high[4] = self.c_b[1], self.k_high[1]
        self.c_z = [rand(630 + t, 3, self.m_g) for t in range(NDEFS)]
        self._rows, self._chunks = {}, {}

    def operands(self):
        return self.c_b + self.k_high + self.c_z

    def k_chunk(self, t, chunk):
        key = (1 if t % NDEFS == 4 else t % NDEFS, chunk)
        if key not in self._chunks:
            self._chunks[key] = self.k_high[t % NDEFS].slice_columns(chunk[0], chunk[0] + chunk[1])
        return self._chunks[key]

    def rows(self, kind, t, r):
        """the first r rows of definition t's c_b ("b"; definition 4 uses definition 1's matrix) or c_z ("z"), made once"""
        t = 1 if (kind, t) == ("b", 4) else t
        if (kind, t, r) not in self._rows:
            full = self.c_b[t] if kind == "b" else self.c_z[t]
            self._rows[(kind, t, r)] = full.slice(0, r, 0, full.ncol)
        return self._rows[(kind, t, r)]

    def slots(self, S, r, chunk, order=None):
        """(c_bs, K_high chunks, c_zs, tags) of the slots `order` (default: 0 .. S - 1) with r rows each"""
        defs = [t % NDEFS for t in (range(S) if order is None else order)]
        return ([self.rows("b", t, r) for t in defs], [self.k_chunk(t, chunk) for t in defs], [self.rows("z", t, r) for t in defs],
                [self.shareds[t].tag(self.entries[t]) for t in defs])

    def literal(self, r, chunk, t):
        """two gpu_matrix_mul and one gpu_matrix_add, K_low from the one-tag sampler"""
        from mxx_amd import lwe_lookup

        t %= NDEFS
        key = (self.ctx, self.d, r, chunk, t)
        if key not in _LITERAL:
            cb, kh, cz, _ = self.slots(1, r, chunk, [t])
            k_low = lwe_lookup.derive_k_low_chunk(self.shareds[t], self.entries[t], *chunk)
            _LITERAL[key] = (cb[0] * kh[0]) + (cz[0] * k_low)
        return _LITERAL[key]

    def chunks(self):
        p, d, m_g = self.p, self.d, self.m_g
        dpt = -(-p.crt_bits() // p.base_bits())
        k = p.modulus_digits()
        out = {"first": (0, min(9, m_g)), "across a tower": (dpt - 1, min(3, m_g - dpt + 1)), "last column": (m_g - 1, 1)}
        if d > 1:
            out["across a block row"] = (k - 1, min(5, m_g - k + 1))
        return out

    def lookup(self, S, r, chunk, order=None):
        cb, kh, cz, tags = self.slots(S, r, chunk, order)
        return self.gpu.GpuDCRTPolyMatrix.lwe_lookup(None, cb, kh, cz, chunk[0], KEY, tags)


def world_of(gpu, oracle, ctx, d):
    if (ctx, d) not in _WORLD:
        _WORLD[(ctx, d)] = World(gpu, oracle, ctx, d)
    return _WORLD[(ctx, d)]


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal per-slot sequence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_one_call_equals_the_literal_sequence_slot_by_slot(gpu, oracle, ctx, d):
    wd = world_of(gpu, oracle, ctx, d)
    M = gpu.GpuDCRTPolyMatrix
    before = [(m.is_ntt, m.to_rns()) for m in wd.operands()]
    chunks = wd.chunks()
    for name, chunk in chunks.items():
        for S in (1, 3, 65):
            got = wd.lookup(S, 1, chunk)
            assert len(got) == S
            for t in range(S):
                assert got[t].size() == (1, chunk[1]) and got[t].is_ntt
                assert got[t] == wd.literal(1, chunk, t), f"{name} chunk {chunk}, slot {t} of {S}"
    # definitions 1 and 4 share one c_b and one K_high matrix; their tags and input vectors differ
    cb, kh, _, tags = wd.slots(5, 1, chunks["first"])
    assert cb[1] is cb[4] and kh[1] is kh[4] and tags[1] != tags[4]
    assert not (wd.literal(1, chunks["first"], 1) == wd.literal(1, chunks["first"], 4))
    # more rows per encoding vector: the row tile and its ragged end
    chunk = chunks["across a tower"]
    for r in (2, 3):
        for t, out in enumerate(wd.lookup(3, r, chunk)):
            assert out.size() == (r, chunk[1]) and out == wd.literal(r, chunk, t), (r, t)
    # the same slots in another order: every slot's output is its own
    order = list(range(NDEFS))[::-1]
    for t, out in zip(order, wd.lookup(NDEFS, 1, chunk, order)):
        assert out == wd.literal(1, chunk, t), t
    # a block at dst_col = 2 of a wider sentinel: the other columns keep their words (copy_block puts the literal in place)
    r, c = 2, chunk[1]
    cbs, khs, czs, tags = wd.slots(3, r, chunk)
    sentinel = oracle.random_matrix(97, r, c + 5, wd.p.moduli(), wd.p.ring_dimension())
    outs = [M.from_rns(wd.p, sentinel, True) for _ in range(3)]
    assert M.lwe_lookup(outs, cbs, khs, czs, chunk[0], KEY, tags, dst_col=2) is not None
    for t, out in enumerate(outs):
        want = M.from_rns(wd.p, sentinel, True)
        want.copy_block_from(wd.literal(r, chunk, t), 0, 2, 0, 0, r, c)
        assert out == want, t
        res = out.to_rns()
        assert np.array_equal(res[:, :2], sentinel[:, :2]) and np.array_equal(res[:, 2 + c:], sentinel[:, 2 + c:])
    # every input, residues and tag, as it was
    for m, (tag, res) in zip(wd.operands(), before):
        assert m.is_ntt == tag and np.array_equal(m.to_rns(), res)


def test_w_zero_gives_the_digits_term_alone(gpu, oracle):
    from mxx_amd import lwe_lookup

    wd = world_of(gpu, oracle, "n16_51", 2)
    M, chunk, r = gpu.GpuDCRTPolyMatrix, (3, 5), 2
    _, _, czs, tags = wd.slots(3, r, chunk)
    got = M.lwe_lookup(None, [M(wd.p, r, 0, czs[0].level, True)] * 3, [M(wd.p, 0, chunk[1], czs[0].level, True)] * 3, czs, chunk[0], KEY, tags)
    for t in range(3):
        assert got[t] == czs[t] * lwe_lookup.derive_k_low_chunk(wd.shareds[t], wd.entries[t], *chunk), t


def test_the_whole_width_through_public_lookup_slots(gpu, oracle):
    from mxx_amd import lwe_lookup

    wd = world_of(gpu, oracle, "n16_51", 2)
    widths = [5, 5, 2]  # a ragged last chunk
    assert wd.m_g == sum(widths)
    S, r = 5, 2
    starts = [0, 5, 10]
    cbs, _, czs, _ = wd.slots(S, r, (0, 5))
    by_slot = [[wd.k_chunk(t, (c0, cw)) for c0, cw in zip(starts, widths)] for t in range(S)]
    got = lwe_lookup.public_lookup_slots(wd.shareds[:S], cbs, czs, by_slot, wd.entries[:S])
    assert len(got) == S
    for t in range(S):
        assert got[t].size() == (r, wd.m_g) and got[t].is_ntt
        assert got[t] == lwe_lookup.public_lookup(wd.shareds[t], cbs[t], czs[t], by_slot[t], wd.entries[t]), t
        parts = [wd.literal(r, (c0, cw), t) for c0, cw in zip(starts, widths)]
        assert got[t] == parts[0].concat_columns(parts[1:]), t
    assert lwe_lookup.public_lookup_slots([], [], [], [], []) == []


def test_public_lookup_poly_is_the_slot_loop(gpu, oracle):
    """the body of public_lookup_poly_gpu: the rows from the plaintexts, A_lt per slot, the K_high chunks from compact bytes"""
    from mxx_amd import lwe_lookup

    wd = world_of(gpu, oracle, "n16_51", 2)
    p, M, r = wd.p, gpu.GpuDCRTPolyMatrix, 1
    widths, starts = [5, 5, 2], [0, 5, 10]
    plt = {0: (7, 11), 1: (3, full_modulus(p.moduli()) - 1), 5: (100, 12345)}
    x_values = [1, 5, 0, 1]
    k_of = {7: 0, 3: 1, 100: 2}  # LUT row -> the definition whose K_high stands for the stored preimage
    blobs = {k: M.to_compact_bytes_many([wd.k_chunk(t, (c0, cw)) for c0, cw in zip(starts, widths)]) for k, t in k_of.items()}
    asked = []

    def k_high_blobs(k, slot_idx):
        asked.append((k, slot_idx))
        return blobs[k]

    cbs = [wd.c_b[t].slice(0, r, 0, wd.w) for t in range(4)]
    czs = [wd.c_z[t].slice(0, r, 0, wd.m_g) for t in range(4)]
    xs = [gpu.GpuDCRTPoly.from_usize_to_constant(p, x) for x in x_values]
    for wave in (None, 3):
        del asked[:]
        vectors, a_lts, ys = lwe_lookup.public_lookup_poly(p, KEY, GATE_ID, LUT_ID, plt, wd.d, cbs, czs, xs, k_high_blobs, wave_slots=wave)
        assert ys == [plt[x][1] for x in x_values] and len(vectors) == len(a_lts) == 4
        assert asked == ([(3, None), (100, None), (7, None)] if wave is None else [(3, None), (100, None), (7, None), (3, None)])
        for s, x in enumerate(x_values):
            k = plt[x][0]
            assert a_lts[s] == lwe_lookup.derive_a_lt_matrix(p, wd.d, KEY, GATE_ID, None)
            sh = lwe_lookup.LweShared(p, KEY, GATE_ID, LUT_ID, None, None, a_lts[s])
            chunks = [wd.k_chunk(k_of[k], (c0, cw)) for c0, cw in zip(starts, widths)]
            assert vectors[s] == lwe_lookup.public_lookup(sh, cbs[s], czs[s], chunks, k), (wave, s)
    with pytest.raises(KeyError):
        lwe_lookup.public_lookup_poly(p, KEY, GATE_ID, LUT_ID, plt, wd.d, cbs[:1], czs[:1], [gpu.GpuDCRTPoly.from_usize_to_constant(p, 9)], k_high_blobs)


def test_several_groups_equal_the_ungrouped_call(gpu, oracle, hip_env):
    wd = world_of(gpu, oracle, "n16_51", 2)
    p, chunk, r = wd.p, (3, 5), 2
    whole = wd.lookup(NDEFS, r, chunk)
    slot_bytes = wd.m_g * chunk[1] * len(p.moduli()) * p.ring_dimension() * 8
    for budget in (1, 3 * slot_bytes):  # one slot per group; groups of 3, 3 and 1
        hip_env.set("MXX_HIP_LWE_LOOKUP_BUDGET", str(budget))
        for t, (a, b) in enumerate(zip(wd.lookup(NDEFS, r, chunk), whole)):
            assert a == b and a == wd.literal(r, chunk, t), (budget, t)
    hip_env.unset("MXX_HIP_LWE_LOOKUP_BUDGET")


# ---------------------------------------------------------------------------------------------------
# 2. independence from the engine: plainref fed with the oracle's samples of U_s
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_outputs_equal_the_plain_reference(gpu, oracle, ctx):
    d, S, r = 2, 3, 1
    wd = world_of(gpu, oracle, ctx, d)
    p = wd.p
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k, m_g = L * dpt, wd.m_g
    slots = list(range(n))
    order = [3, 4, 5]
    for chunk in ((0, 4), (k - 1, 2)):
        cbs, khs, czs, tags = wd.slots(S, r, chunk, order)
        got = wd.lookup(S, r, chunk, order)
        for s in range(S):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tags[s]), full_ncol=m_g,
                                           col_offset=chunk[0])
            want = P.slot_mul_sum(None, [cbs[s].to_rns(), czs[s].to_rns()], [khs[s].to_rns(), digits_eval(u, moduli, base, dpt, slots)], moduli, False)
            assert np.array_equal(got[s].to_rns(), want), (ctx, chunk, s)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """Every matrix of the call at level 0 / 1 of a three-limb context (the refusal list below only shows that MIXED levels
    are turned away): m_g = d * dpt * (level + 1) with dpt from the CONTEXT's crt_bits (one width per basis here, so plainref
    derives the same dpt from the truncated basis), U_s sampled in limbs 0..level only, the plain reference above at
    moduli[: level + 1]; into fresh outputs and into a column block of wider ones, and the combine entry with the digits given."""
    n, d, S, r = 16, 2, 3, 2
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    m_g, w = d * k, 5
    slots = list(range(n))
    rnd = lambda seed, rows, cols: oracle.random_matrix(seed + level, rows, cols, moduli, n)  # noqa: E731
    cbs_np, czs_np = [rnd(650 + 3 * s, r, w) for s in range(S)], [rnd(660 + 3 * s, r, m_g) for s in range(S)]
    cbs, czs = [M.from_rns(p, a, True) for a in cbs_np], [M.from_rns(p, a, True) for a in czs_np]
    tags = [b"lwe_low_level_" + bytes([48 + s]) for s in range(S)]
    for chunk in ((0, min(4, m_g)), (k - 1, 2)):
        khs_np = [rnd(670 + 3 * s, w, chunk[1]) for s in range(S)]
        khs = [M.from_rns(p, a, True) for a in khs_np]
        got = M.lwe_lookup(None, cbs, khs, czs, chunk[0], KEY, tags)
        frame = rnd(680, r, chunk[1] + 3)
        wide = [M.from_rns(p, frame, True) for _ in range(S)]
        M.lwe_lookup(wide, cbs, khs, czs, chunk[0], KEY, tags, dst_col=2)
        vs = []
        for s in range(S):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tags[s]), full_ncol=m_g,
                                           col_offset=chunk[0])
            vs.append(digits_eval(u, moduli, base, dpt, slots))
            want = P.slot_mul_sum(None, [cbs_np[s], czs_np[s]], [khs_np[s], vs[s]], moduli, False)
            assert got[s].level == level and got[s].is_ntt and np.array_equal(got[s].to_rns(), want), (bits, level, chunk, s)
            placed = frame.copy()
            placed[:, 2:2 + chunk[1]] = want
            assert np.array_equal(wide[s].to_rns(), placed), (bits, level, chunk, s, "a block of a wider output")
        given = M.lwe_lookup_combine(None, cbs, khs, czs, M.from_rns(p, np.concatenate(vs, axis=1), True), chunk[0])
        for s in range(S):
            assert given[s] == got[s], (bits, level, chunk, s)


# ---------------------------------------------------------------------------------------------------
# 3. the combine entry alone in every width class
# ---------------------------------------------------------------------------------------------------
SMALL_WINDOWS = {("class", 31), ("class", 62)}  # the classes whose lazy window is shorter than the term count


def fold_places(window, w, m_g):
    """where the accumulator is folded before the final reduction, for terms 0 .. w + m_g - 1 in the kernel's order (K_high,
    the digits): before every term t > 0 with t % window == 0"""
    places = set()
    for t in range(window, w + m_g, window):
        places.add("inside K_high" if t < w else "seam" if t == w else "inside the digits")
    return places


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_combine_entry_alone_in_every_width_class(gpu, cell):
    n, moduli, bases, slots = _cell(cell)
    M, L = gpu.GpuDCRTPolyMatrix, len(moduli)
    bits = max(int(q).bit_length() for q in moduli)
    windows = _windows(moduli)
    small = min(windows)
    for base in bases:
        p = _params(gpu, n, moduli, base)
        k = L * P.digits_per_tower(moduli, base)
        if cell in SMALL_WINDOWS:
            # w two of the shortest window: a fold inside K_high (term `small`) and on the seam (term w); enough block rows of
            # G for the digits to reach past one more window (term w + small)
            w, d = 2 * small, small // k + 1
        else:
            w, d = 3, 1
        m_g = d * k
        c = min(m_g, 5)  # the ragged column tile
        col_start = m_g - c
        seen = set()
        for window in windows:
            seen |= fold_places(window, w, m_g)
        if cell in SMALL_WINDOWS:
            assert {"inside K_high", "seam", "inside the digits"} <= seen, (base, windows, w, m_g, seen)
        rng = np.random.default_rng(3000 + bits + base)
        for kind, S, r in (("top", 1, 1), ("random", 2, 2), ("c_b zero", 2, 3)):
            make = (lambda rows, cols: _top(rows, cols, moduli, n)) if kind == "top" else (lambda rows, cols: _rand(rng, rows, cols, moduli, n))
            cbs = [make(r, w) for _ in range(S)]
            if kind == "c_b zero":
                for cb in cbs:
                    cb[:] = 0
            khs, czs, digits = [make(w, c) for _ in range(S)], [make(r, m_g) for _ in range(S)], make(m_g, S * c)
            up = lambda a: M.from_rns(p, a, True)  # noqa: E731
            got = M.lwe_lookup_combine(None, [up(a) for a in cbs], [up(a) for a in khs], [up(a) for a in czs], up(digits), col_start)
            for s in range(S):
                want = P.slot_mul_sum(None, [cbs[s], czs[s]], [khs[s], digits[:, s * c:(s + 1) * c]], moduli, False, slots)
                assert got[s].size() == (r, c) and got[s].is_ntt
                res = got[s].to_rns()
                assert np.array_equal(res[..., slots], want), (cell, base, kind, s)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(res, np.broadcast_to(want[..., :1], res.shape)), (cell, base, s)


# ---------------------------------------------------------------------------------------------------
# 4. end to end, noise-free: a real trapdoor, real preimages
# ---------------------------------------------------------------------------------------------------
def test_noise_free_lookup_returns_the_encoding_of_the_lut_value(gpu, oracle):
    from mxx_amd import lwe_lookup
    from test_gpu_preimage_abi import explicit_seeds, seed_bytes, trapdoor_and_oracle

    d = 2
    p = make_params(gpu, oracle, *CONTEXTS["n256_51"])
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    m = d * p.modulus_digits()
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, p.base_bits(), d, seed_bytes(9))
    a_z = M.from_rns(p, oracle.random_matrix(650, d, m, moduli, n), True)
    rows = [(5, 12345, full_modulus(moduli) - 1), (41, (1 << 32) + 5, 3), (6, 0, 77)]  # (entry, x, y): three LUT rows
    shareds = [lwe_lookup.LweShared(p, KEY, GATE_ID, LUT_ID, slot, a_z, lwe_lookup.derive_a_lt_matrix(p, d, KEY, GATE_ID, slot)) for slot in range(3)]
    chunks = [(c0, min(4, m - c0)) for c0 in range(0, m, 4)]
    assert chunks[-1][1] < 4  # a ragged last chunk
    k_high = [[] for _ in rows]
    for s, (sh, row) in enumerate(zip(shareds, rows)):
        for j, chunk in enumerate(chunks):  # no error term enters the targets: error sigma 0
            (target, x_high), = lwe_lookup.sample_lwe_preimages(sh, sampler, td, A, [row], chunk, _seeds=explicit_seeds(gpu, 1, 900 + 10 * j + s))
            assert A * x_high == target
            k_high[s].append(x_high)
    G = M.gadget_matrix(p, d)
    secrets = [M.from_rns(p, oracle.random_matrix(660 + s, 1, d, moduli, n), True) for s in range(3)]
    c_bs = [s * A for s in secrets]  # noise-free encodings
    c_zs = [s * (a_z - G * gpu.GpuDCRTPoly.from_usize_to_constant(p, x)) for s, (_, x, _) in zip(secrets, rows)]
    got = lwe_lookup.public_lookup_slots(shareds, c_bs, c_zs, k_high, [entry for entry, _, _ in rows])
    assert len(got) == 3
    for s, sh, (entry, x, y), vec in zip(secrets, shareds, rows, got):
        assert vec.size() == (1, m) and vec.is_ntt
        assert vec == s * (sh.a_lt - G * gpu.GpuDCRTPoly.from_elem_to_constant(p, y)), (entry, x, y)


# ---------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_slot_count(gpu, oracle):
    from mxx_amd import _ffi, lwe_lookup

    wd = world_of(gpu, oracle, "n256_51", 2)
    M, chunk = gpu.GpuDCRTPolyMatrix, (0, 4)

    def trace(fn):
        _ffi.trace_begin()
        fn()
        events = _ffi.trace_end()
        return [e["kernel"] for e in events if e["threads"]], [e["kernel"] for e in events if not e["threads"]]  # copies: no threads

    legs = {}
    for S in (2, 48):
        cbs, khs, czs, tags = wd.slots(S, 1, chunk)
        # the library call behind sample_hash_decomposed_columns_many for the same tags (the mirror's split into S matrices,
        # which the lookup has no use for, is not part of it)
        legs[S] = dict(full=trace(lambda: M.lwe_lookup(None, cbs, khs, czs, chunk[0], KEY, tags)),
                       sampler=trace(lambda: M.sample_hash_decomposed_blocks(wd.p, KEY, tags, wd.d, wd.m_g, chunk[0], chunk[1],
                                                                             _ffi.GPU_MATRIX_DIST_UNIFORM)))
    cbs, khs, czs, _ = wd.slots(2, 1, chunk)
    # what `public_lookup` runs per slot for this chunk: the one-tag decomposed sample and one mul_sum
    loop = trace(lambda: [M.mul_sum([cbs[t], czs[t]], [khs[t], lwe_lookup.derive_k_low_chunk(wd.shareds[t], wd.entries[t], *chunk)]) for t in range(2)])
    two, many = legs[2], legs[48]
    print(f"kernels: 48 slots {len(many['full'][0])} {many['full'][0]}, copies {many['full'][1]}; 2 slots {len(two['full'][0])}; sampler alone "
          f"{len(many['sampler'][0])} and {len(many['sampler'][1])} copies; the per-slot loop for 2 slots {len(loop[0])} kernels and {len(loop[1])} copies")
    assert many["full"] == two["full"]
    # exactly one kernel and one copy more than the sampler's call
    assert len(many["full"][0]) == len(many["sampler"][0]) + 1 and len(many["full"][1]) == len(many["sampler"][1]) + 1
    extra = list(many["full"][0])
    for name in many["sampler"][0]:
        extra.remove(name)
    assert len(extra) == 1 and "lwe_lookup_kernel" in extra[0]
    assert len(two["full"][0]) + len(two["full"][1]) < len(loop[0]) + len(loop[1])
    assert len(two["full"][0]) < len(loop[0])


# ---------------------------------------------------------------------------------------------------
# 6. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi, lwe_lookup
    from mxx_amd.matrix import hash_tags_arg

    wd = world_of(gpu, oracle, "n16_24", 2)
    p = wd.p
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m_g, w, c, S, r, top = wd.m_g, wd.w, 2, 3, 2, len(p.moduli()) - 1
    chunk = (1, c)
    cbs, khs, czs, tag_list = wd.slots(S, r, chunk, [0, 2, 3])
    sentinel = oracle.random_matrix(95, r, c, moduli, n)
    wide_sentinel = oracle.random_matrix(93, r, c + 3, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    arg, keep, _ = hash_tags_arg(KEY, tag_list)
    bad_form, keep2, _ = hash_tags_arg(KEY, tag_list)
    bad_form.form = 9
    coeff = {name: m.clone() for name, m in (("c_b", cbs[1]), ("k_high", khs[1]), ("c_z", czs[2]))}
    for m in coeff.values():
        m.intt_all_in_place()

    def array(ms):
        return None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])

    def call(outs, S_=S, dst_col=0, col_start=1, base_bits=base, tags=arg, b=cbs, k=khs, z=czs, arr=True):
        return lib.gpupoly_matrix_lwe_lookup(array(outs) if arr else None, S_, dst_col, array(b), array(k), array(z), col_start, base_bits,
                                             None if tags is None else C.byref(tags))

    def rows_of(m, lo, hi):  # r x c views into an operand's storage
        return m.reshape_view(m.nrow * m.ncol // c, c).row_view(lo, hi)

    def swap(ms, at, m):
        return [m if j == at else x for j, x in enumerate(ms)]

    new = lambda rows, cols, params=p, level=top: M(params, rows, cols, level, True)  # noqa: E731
    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null c_bs": (lambda o: call(o, b=None), "null"),
        "null c_bs entry": (lambda o: call(o, b=swap(cbs, 1, None)), "null"),
        "null k_highs": (lambda o: call(o, k=None), "null"),
        "null k_highs entry": (lambda o: call(o, k=swap(khs, 2, None)), "null"),
        "null c_zs": (lambda o: call(o, z=None), "null"),
        "null c_zs entry": (lambda o: call(o, z=swap(czs, 0, None)), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "c_b of another context": (lambda o: call(o, b=swap(cbs, 1, new(r, w, other))), "context mismatch (slot 1)"),
        "K_high of another context": (lambda o: call(o, k=swap(khs, 2, new(w, c, other))), "context mismatch (slot 2)"),
        "c_z of another context": (lambda o: call(o, z=swap(czs, 1, new(r, m_g, other))), "context mismatch (slot 1)"),
        "output of another context": (lambda o: call(swap(o, 1, new(r, c, other))), "context mismatch (slot 1)"),
        "c_b of another level": (lambda o: call(o, b=swap(cbs, 2, new(r, w, level=0))), "level mismatch (slot 2)"),
        "K_high of another level": (lambda o: call(o, k=swap(khs, 1, new(w, c, level=0))), "level mismatch (slot 1)"),
        "c_z of another level": (lambda o: call(o, z=swap(czs, 2, new(r, m_g, level=0))), "level mismatch (slot 2)"),
        "output of another level": (lambda o: call(swap(o, 2, new(r, c, level=0))), "level mismatch (slot 2)"),
        "c_b rows": (lambda o: call(o, b=swap(cbs, 1, new(r + 1, w))), "shape mismatch"),
        "c_b columns": (lambda o: call(o, b=swap(cbs, 2, new(r, w + 1))), "(slot 2)"),
        "K_high rows": (lambda o: call(o, k=swap(khs, 1, new(w + 1, c))), "shape mismatch"),
        "K_high chunks of different widths": (lambda o: call(o, k=swap(khs, 2, new(w, c + 1))), "width"),
        "c_z rows": (lambda o: call(o, z=swap(czs, 1, new(r + 1, m_g))), "shape mismatch"),
        "c_z columns": (lambda o: call(o, z=swap(czs, 2, new(r, m_g + wd.p.modulus_digits()))), "(slot 2)"),
        "m_g not a multiple of k": (lambda o: call(o, z=[new(r, m_g + 1)] * 3), "shape mismatch"),
        "output rows": (lambda o: call(swap(o, 2, new(r + 1, c))), "shape mismatch"),
        "outputs of different widths": (lambda o: call(swap(o, 2, new(r, c + 1))), "width"),
        "c_b not EVAL": (lambda o: call(o, b=swap(cbs, 1, coeff["c_b"])), "Eval"),
        "K_high not EVAL": (lambda o: call(o, k=swap(khs, 1, coeff["k_high"])), "Eval"),
        "c_z not EVAL": (lambda o: call(o, z=swap(czs, 2, coeff["c_z"])), "Eval"),
        "chunk past m_g": (lambda o: call(o, col_start=m_g - 1), "past"),
        "col_start past m_g": (lambda o: call(o, col_start=m_g + 1), "past"),
        "block past the outputs": (lambda o: call(o, dst_col=1), "past"),
        "dst_col past the outputs": (lambda o: call(o, dst_col=c + 1), "past"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
        # each operand kind overlapped through a row view
        "output overlaps a c_z": (lambda o: call(swap(o, 1, rows_of(czs[0], 1, 1 + r))), "overlap"),
        "output overlaps a K_high": (lambda o: call(swap(o, 2, rows_of(khs[0], 1, 1 + r))), "overlap"),
    }
    kh_parent = M.from_rns(p, oracle.random_matrix(92, w + r, c, moduli, n), True)
    cases["output overlaps a K_high of one parent"] = (lambda o: call(swap(o, 0, kh_parent.row_view(w - 1, w - 1 + r)),
                                                                      k=swap(khs, 2, kh_parent.row_view(0, w))), "overlap")
    cb_wide = M.from_rns(p, oracle.random_matrix(91, 2 * r, w, moduli, n), True)
    cb_as_out = cb_wide.reshape_view(2 * r * w // c, c)  # its first r rows lie inside the first r rows of cb_wide
    cases["output overlaps a c_b"] = (lambda o: call(swap(o, 1, cb_as_out.row_view(0, r)), b=swap(cbs, 0, cb_wide.row_view(0, r))), "overlap")
    held_mats = cbs + khs + czs + [kh_parent, cb_wide]
    held = [m.to_rns() for m in held_mats]

    def check(name, fn, word, entry=ENTRY, fresh=None):
        # COEFF-tagged: a tag flipped to EVAL would change the read-out
        outs = [M.from_rns(p, sentinel, False) for _ in range(S)] if fresh is None else fresh()
        before = [(o.is_ntt, o.to_rns()) for o in outs]
        _ffi.trace_begin()
        c0 = lib.gpupoly_launch_count()
        rc = fn(outs)
        msg = _ffi.last_error_string()
        assert _ffi.trace_end() == [] and lib.gpupoly_launch_count() == c0, name
        assert rc != 0, name
        assert entry in msg and word in msg, (name, msg)
        for o, (tag, res) in zip(outs, before):
            assert o.is_ntt == tag and np.array_equal(o.to_rns(), res), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # a partial block needs outputs already tagged EVAL: one COEFF output among EVAL ones, every output left alone
    def partial_outs():
        return [M.from_rns(p, wide_sentinel, t != 1) for t in range(S)]

    check("partial block into a non-EVAL output", lambda o: call(o, dst_col=1), "partial", fresh=partial_outs)
    # two outputs overlapping through views of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, 3 * r, c, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, r), parent.row_view(r - 1, 2 * r - 1), parent.row_view(2 * r, 3 * r)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for m, res in zip(held_mats, held):
        assert np.array_equal(m.to_rns(), res)
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and S = 0, c = 0, r = 0 launch nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(S)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * r, (t + 1) * r) for t in range(3)]
    assert call(disjoint) == 0
    for t, (o, v) in enumerate(zip(outs, disjoint)):
        o.is_ntt = v.is_ntt = True
        assert o == v and o == wd.literal(r, chunk, [0, 2, 3][t])
    partial = partial_outs()
    partial[1].ntt_all_in_place()
    assert call(partial, dst_col=1) == 0
    c0 = lib.gpupoly_launch_count()
    assert call([], S_=0) == 0 and call([], S_=0, arr=False, tags=None, b=None, k=None, z=None) == 0
    assert call([new(r, 0) for _ in range(S)], k=[new(w, 0) for _ in range(S)]) == 0
    assert call([new(0, c) for _ in range(S)], b=[new(0, w)] * S, z=[new(0, m_g)] * S) == 0
    assert lib.gpupoly_launch_count() == c0
    # the combine entry names itself, counts the digits as an operand and takes any keying
    digits = new(m_g, S * c)

    def combine(outs, d=digits):
        return lib.gpupoly_matrix_lwe_lookup_combine(array(outs), S, 0, array(cbs), array(khs), array(czs), 1, base, None if d is None else d.raw)

    check("combine: digits shape", lambda o: combine(o, new(m_g, S * c + 1)), "shape", COMBINE)
    check("combine: null digits", lambda o: combine(o, None), "null", COMBINE)
    check("combine: output overlaps the digits", lambda o: combine(swap(o, 1, rows_of(digits, 0, r))), "overlap", COMBINE)
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the per-slot loop
    widths, starts = [5, 3], [0, 5]
    assert sum(widths) == m_g
    by_slot = [[wd.k_chunk(t, (c0, cw)) for c0, cw in zip(starts, widths)] for t in (0, 2, 3)]
    shareds, entries = [wd.shareds[t] for t in (0, 2, 3)], [wd.entries[t] for t in (0, 2, 3)]
    default = lwe_lookup.public_lookup_slots(shareds, cbs, czs, by_slot, entries)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    assert combine([M.from_rns(p, sentinel, False) for _ in range(S)]) == 0  # no sampling: any keying
    fallen = lwe_lookup.public_lookup_slots(shareds, cbs, czs, by_slot, entries)
    for t in range(S):
        assert fallen[t] == lwe_lookup.public_lookup(shareds[t], cbs[t], czs[t], by_slot[t], entries[t])
        assert not (fallen[t] == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert lwe_lookup.public_lookup_slots(shareds, cbs, czs, by_slot, entries)[2] == default[2]
    del keep, keep2
