"""GPU: the slot-transfer online evaluation for many destination slots in one call (`gpupoly_matrix_slot_transfer_eval`,
mxx_amd/slot_transfer.py).

out_s = c_b0 Pg_s + sum_t x^shift_t o kappa_t o (c_in_t G^-1(A_s) + mu_t o ((c_b0 P0_src_t) P1_s)) is exact arithmetic on canonical
residues, so the bar is equality, bit for bit (gpu_matrix_equal), with the reference's two functions restated through the
mirror's older operations (`output_slot`, `slot_reduce_output_slot`) and, for arbitrary shifts, with the `mul_monomial` +
`mul_scalar` + `add` sequence.  The formula needs no real preimages, so the operands are uniform random; a literal output is
computed once per (context, d, r, destination) and shared.  Independently of the engine the same outputs are computed with
tests/plainref.py in the reference's original association, fed with the oracle's samples of A_s; the combine entry alone
(`gpupoly_matrix_slot_transfer_eval_combine`, which takes the digits as given) is held to plainref in every modulus width class
with operands no sampler produces; and with real trapdoors and noise-free encodings the gate returns exactly
(s S_dst)(A_out - G o (kappa mu_src))."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import CELLS, STATED_WINDOWS, _cell, _cell_id, _params, _rand, _top, _windows
from test_gpu_ggh15_lookup import CONTEXTS, digits_eval
from test_gpu_lut_targets import full_modulus

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_slot_transfer_eval"
COMBINE = "gpupoly_matrix_slot_transfer_eval_combine"
KEY = bytes((11 * i + 7) & 0xFF for i in range(32))
GATE = 19
NSRC, NDEF, NVEC = 4, 7, 5  # source slots; stored P1 / Pg definitions (destination t uses definition t % NDEF); reduce input vectors
KAPPAS = [None, 1, 3, (1 << 32) - 1]
CHUNK = 5  # the column chunk of the whole-width runs: a ragged last chunk wherever m_g is no multiple of 5
_WORLD, _LITERAL = {}, {}


def src_slot_of(t):
    """destination t's (source slot, scalar): sources repeat, None mixes with Some(kappa)"""
    return ((5 * t + 2) % NSRC, KAPPAS[(t + t // 4) % 4])


class _Cyclic:
    """stored preimages by slot: slot t holds definition t % NDEF (the tags of A_t are the slots' own)"""

    def __init__(self, mats, gate=False):
        self.mats, self.gate = mats, gate

    def __getitem__(self, key):
        return self.mats[(key[1] if self.gate else key) % len(self.mats)]


class World:
    """what the tests of one (context, d) share, computed once and left unchanged"""

    def __init__(self, gpu, oracle, ctx, d):
        from mxx_amd import slot_transfer as ST

        self.gpu, self.ctx, self.d = gpu, ctx, d
        p = self.p = make_params(gpu, oracle, *CONTEXTS[ctx])
        M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
        k = p.modulus_digits()
        self.m_g = d * k
        self.w0, self.w1 = (d * (k + 2), 2 * d * (k + 2)) if d == 1 else (5, 7)  # the library ties neither to d
        rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
        Q = full_modulus(moduli)
        self.mus = [12345 % Q, Q - 1, 1, ((1 << 70) + 7) % Q]
        self.c_b0_full = rand(700, 3, self.w0)
        self.vec_full = [rand(710 + t, 3, self.m_g) for t in range(NVEC)]
        self.p0 = [rand(720 + t, self.w0, self.w1) for t in range(NSRC)]
        self.p1 = [rand(730 + t, self.w1, self.m_g) for t in range(NDEF)]
        self.pg = [rand(740 + t, self.w0, self.m_g) for t in range(NDEF)]
        self.plaintexts = [gpu.GpuDCRTPoly.from_biguint_to_constant(p, mu) for mu in self.mus]
        self._rows, self._shared, self.ST = {}, {}, ST

    def operands(self):
        return [self.c_b0_full] + self.vec_full + self.p0 + self.p1 + self.pg

    def rows(self, kind, t, r):
        if (kind, t, r) not in self._rows:
            full = self.c_b0_full if kind == "b" else self.vec_full[t]
            self._rows[(kind, t, r)] = full.slice(0, r, 0, full.ncol)
        return self._rows[(kind, t, r)]

    def shared(self, r):
        if r not in self._shared:
            self._shared[r] = self.ST.SlotEvalShared.from_matrices(self.p, KEY, self.d, self.rows("b", 0, r), _Cyclic(self.p0), _Cyclic(self.p1),
                                                                   _Cyclic(self.pg, True))
        return self._shared[r]

    def inputs(self, r):
        return [self.rows("v", t, r) for t in range(NSRC)]

    def literal(self, r, dst):
        """output_slot for destination dst: the reference's sequence, one chunk over the whole width"""
        key = (self.ctx, self.d, r, dst)
        if key not in _LITERAL:
            src_slots = [src_slot_of(t) for t in range(dst + 1)]
            _LITERAL[key] = self.ST.output_slot(self.shared(r), GATE, self.inputs(r), self.plaintexts, src_slots, dst, self.m_g)
        return _LITERAL[key]

    def chunks(self):
        p, d, m_g = self.p, self.d, self.m_g
        dpt = -(-p.crt_bits() // p.base_bits())
        k = p.modulus_digits()
        out = {"first": (0, min(9, m_g)), "across a tower": (dpt - 1, min(3, m_g - dpt + 1)), "last column": (m_g - 1, 1)}
        if d > 1:
            out["across a block row"] = (k - 1, min(5, m_g - k + 1))
        return out

    def transfer_terms(self, S, r, mids):
        out = []
        for t in range(S):
            src, kappa = src_slot_of(t)
            out.append([(self.rows("v", src, r), mids[src], 0, 1 if kappa is None else kappa, self.mus[src])])
        return out

    def eval_chunk(self, S, r, chunk, terms=None, outs=None, dst_col=0, dsts=None):
        sh = self.shared(r)
        dsts = list(range(S)) if dsts is None else dsts
        if terms is None:
            terms = self.transfer_terms(S, r, self.ST.transfer_mids(sh, range(NSRC)))
        return self.gpu.GpuDCRTPolyMatrix.slot_transfer_eval(outs, sh.c_b0, [sh.gate_chunk(GATE, s, *chunk) for s in dsts],
                                                             [sh.p1_chunk(s, *chunk) for s in dsts], terms, chunk[0], KEY, sh.slot_a_tags(dsts),
                                                             dst_col=dst_col)


def world_of(gpu, oracle, ctx, d):
    if (ctx, d) not in _WORLD:
        _WORLD[(ctx, d)] = World(gpu, oracle, ctx, d)
    return _WORLD[(ctx, d)]


def cols(m, chunk):
    return m.slice_columns(chunk[0], chunk[0] + chunk[1])


# ---------------------------------------------------------------------------------------------------
# 1. the transfer gate against the literal per-slot function
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_transfer_equals_output_slot_slot_by_slot(gpu, oracle, ctx, d):
    wd = world_of(gpu, oracle, ctx, d)
    ST = wd.ST
    before = [(m.is_ntt, m.to_rns()) for m in wd.operands()]
    defs = [src_slot_of(t) for t in range(65)]
    assert len({s for s, _ in defs[:3]}) == 3 and len({s for s, _ in defs}) == NSRC  # sources repeat past the fourth slot
    assert {k for _, k in defs[:8]} == set(KAPPAS)
    for S in (1, 3, 65):
        got = ST.slot_transfer_slots(wd.shared(1), GATE, wd.inputs(1), wd.mus, defs[:S], CHUNK)
        assert len(got) == S
        for t in range(S):
            assert got[t].size() == (1, wd.m_g) and got[t].is_ntt
            assert got[t] == wd.literal(1, t)[0], f"slot {t} of {S}"
    # single chunks through the entry: the first, across a tower, across a block row, the last column
    for name, chunk in wd.chunks().items():
        for S in (3, 65):
            for t, out in enumerate(wd.eval_chunk(S, 1, chunk)):
                assert out.size() == (1, chunk[1]) and out == cols(wd.literal(1, t)[0], chunk), f"{name} chunk {chunk}, slot {t} of {S}"
    # more rows per encoding vector: the row tile and its ragged end
    chunk = wd.chunks()["across a tower"]
    for r in (2, 3):
        got = ST.slot_transfer_slots(wd.shared(r), GATE, wd.inputs(r), wd.mus, defs[:3], CHUNK)
        for t in range(3):
            assert got[t].size() == (r, wd.m_g) and got[t] == wd.literal(r, t)[0], (r, t)
        for t, out in enumerate(wd.eval_chunk(3, r, chunk)):
            assert out == cols(wd.literal(r, t)[0], chunk), (r, t)
    # the whole gate: the vectors and const(mu_src) * kappa
    vectors, plaintexts = ST.slot_transfer(wd.shared(1), GATE, wd.inputs(1), wd.plaintexts, defs[:5], CHUNK)
    for t in range(5):
        assert vectors[t] == wd.literal(1, t)[0] and plaintexts[t] == wd.literal(1, t)[1], t
    # destinations that are not consecutive: the table form of the tags
    dsts = [4, 0, 2]
    mids = ST.transfer_mids(wd.shared(1), range(NSRC))
    terms = [wd.transfer_terms(5, 1, mids)[t] for t in dsts]
    for t, out in zip(dsts, wd.eval_chunk(3, 1, chunk, terms=terms, dsts=dsts)):
        assert out == cols(wd.literal(1, t)[0], chunk), t
    # every input, residues and tag, as it was
    for m, (tag, res) in zip(wd.operands(), before):
        assert m.is_ntt == tag and np.array_equal(m.to_rns(), res)


def test_w0_and_w1_zero_are_legal(gpu, oracle):
    wd = world_of(gpu, oracle, "n16_51", 2)
    M, p, r, chunk = gpu.GpuDCRTPolyMatrix, wd.p, 2, (3, 5)
    sh = wd.shared(r)
    level = sh.c_b0.level
    new = lambda rows, ncols: M(p, rows, ncols, level, True)  # noqa: E731
    vec = wd.rows("v", 1, r)
    digits = [cols(sh.slot_a(s), chunk).decompose() for s in range(2)]
    kappa = gpu.GpuDCRTPoly.from_usize_to_constant(p, 3)
    # w1 = 0: the gate preimage and the A segment alone
    got = M.slot_transfer_eval(None, sh.c_b0, [sh.gate_chunk(GATE, s, *chunk) for s in range(2)], [new(0, chunk[1])] * 2,
                               [[(vec, new(r, 0), 0, 1, 5)], [(vec, new(r, 0), 0, 3, 5)]], chunk[0], KEY, sh.slot_a_tags([0, 1]))
    assert got[0] == sh.c_b0 * sh.gate_chunk(GATE, 0, *chunk) + vec * digits[0]
    assert got[1] == sh.c_b0 * sh.gate_chunk(GATE, 1, *chunk) + (vec * digits[1]).mul_scalar(kappa)
    # w0 = 0: no gate term
    mid = sh.c_b0 * wd.p0[0]
    got = M.slot_transfer_eval(None, new(r, 0), [new(0, chunk[1])] * 2, [sh.p1_chunk(s, *chunk) for s in range(2)],
                               [[(vec, mid, 0, 1, 1)], [(vec, mid, 0, 0, 1)]], chunk[0], KEY, sh.slot_a_tags([0, 1]))
    assert got[0] == vec * digits[0] + mid * sh.p1_chunk(0, *chunk)
    assert got[1] == M.zero(p, r, chunk[1])  # scalar 0 is a legal weight


# ---------------------------------------------------------------------------------------------------
# 2. the reduce gate, and arbitrary shifts through the entry
# ---------------------------------------------------------------------------------------------------
def reduce_case(wd, r, ndst):
    inputs = [[wd.rows("v", (3 * dst + src) % NVEC, r) for src in range(16)] for dst in range(ndst)]
    mus = [[wd.mus[(dst + src) % len(wd.mus)] for src in range(16)] for dst in range(ndst)]
    return inputs, mus


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_reduce_equals_slot_reduce_output_slot(gpu, oracle, ctx, d):
    wd = world_of(gpu, oracle, ctx, d)
    ST, p, n = wd.ST, wd.p, wd.p.ring_dimension()
    r, ndst = 1, 2
    sh = wd.shared(r)
    inputs, mus = reduce_case(wd, r, ndst)
    for num_slots in [s for s in (1, 3) if s <= n] + ([n] if n <= 16 else []):  # the literal's one-hot monomial has n places
        pts = [[gpu.GpuDCRTPoly.from_biguint_to_constant(p, mu) for mu in row[:num_slots]] for row in mus]
        vectors, plaintexts = ST.slot_reduce(sh, GATE, inputs, pts, num_slots, CHUNK)
        assert len(vectors) == len(plaintexts) == ndst
        for dst in range(ndst):
            want = ST.slot_reduce_output_slot(sh, GATE, inputs, pts, dst, num_slots, wd.m_g)
            assert vectors[dst].size() == (r, wd.m_g) and vectors[dst] == want[0], (num_slots, dst)
            assert plaintexts[dst] == want[1], (num_slots, dst)


@pytest.mark.parametrize("ctx", ["n2_17", "n16_24", "n256_51"])
def test_shifts_against_the_monomial_sequence(gpu, oracle, ctx):
    d, r = 2, 2
    wd = world_of(gpu, oracle, ctx, d)
    p, n, M = wd.p, wd.p.ring_dimension(), gpu.GpuDCRTPolyMatrix
    sh = wd.shared(r)
    shifts = [0, 1, n - 1, n, 2 * n - 1, 2 * n + 3]  # the sign half and the reduction mod 2N
    mids = wd.ST.transfer_mids(sh, range(NSRC))
    chunk = wd.chunks()["across a block row"]
    terms = [[(wd.rows("v", j % NVEC, r), mids[j % NSRC], s, [1, 3, (1 << 32) - 1][j % 3], wd.mus[j % 4]) for j, s in enumerate(shifts)],
             [(wd.rows("v", 2, r), mids[1], shifts[5], 1, wd.mus[1])], [(wd.rows("v", 3, r), mids[2], shifts[3], 1, wd.mus[3])]]
    got = wd.eval_chunk(3, r, chunk, terms=terms)
    for dst in range(3):
        digits = cols(sh.slot_a(dst), chunk).decompose()
        want = sh.c_b0 * sh.gate_chunk(GATE, dst, *chunk)
        for c_in, mid, shift, kappa, mu in terms[dst]:
            pre = c_in * digits + (mid * sh.p1_chunk(dst, *chunk)).mul_scalar(gpu.GpuDCRTPoly.from_biguint_to_constant(p, mu))
            want = want + pre.mul_monomial(shift).mul_scalar(gpu.GpuDCRTPoly.from_usize_to_constant(p, kappa))
        assert got[dst] == want, dst


# ---------------------------------------------------------------------------------------------------
# 3. independence from the engine: plainref in the original association
# ---------------------------------------------------------------------------------------------------
def plain_eval(c_b0, pg, p1, digits, terms, moduli, n, slots=None):
    """c_b0 Pg + sum_t x^shift o kappa o (c_in D + mu o (mid P1)) on (rows, cols, L, n) residue arrays, slot by slot, in Python
    integers; terms = [(c_in, mid, shift, kappa, mu)].  x^shift in slot k of limb l is psi_l^(shift (2 bitrev(k) + 1))."""
    L, logn = len(moduli), n.bit_length() - 1
    which = list(range(n)) if slots is None else [int(s) for s in slots]
    q = np.asarray([int(v) for v in moduli], dtype=object).reshape(1, 1, L, 1)
    total = P.slot_mul_sum(None, [c_b0], [pg], moduli, False, slots).astype(object)
    for c_in, mid, shift, kappa, mu in terms:
        pre = P.slot_mul_sum(None, [c_in], [digits], moduli, False, slots).astype(object)
        pre = (pre + P.slot_mul_sum(None, [mid], [p1], moduli, False, slots).astype(object) * (int(mu) % q)) % q
        f = np.asarray([[pow(P.min_root(int(ql), n), (shift % (2 * n)) * (2 * P.bitrev(k, logn) + 1), int(ql)) for k in which] for ql in moduli],
                       dtype=object).reshape(1, 1, L, len(which))
        total = (total + pre * f % q * (int(kappa) % q)) % q
    return total.astype(np.uint64)


@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_outputs_equal_the_plain_reference_in_the_original_association(gpu, oracle, ctx):
    d, r = 2, 1
    wd = world_of(gpu, oracle, ctx, d)
    p, sh = wd.p, wd.shared(r)
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k, m_g = L * dpt, wd.m_g
    slots = list(range(n))
    mids = wd.ST.transfer_mids(sh, range(NSRC))
    c_b0 = sh.c_b0.to_rns()
    # (source, shift, kappa) per term: two transfers, one reduce over three sources
    specs = [[(src, 0, 1 if kappa is None else kappa)] for src, kappa in (src_slot_of(0), src_slot_of(2))] + [[(src, src, 1) for src in range(3)]]
    terms = [[(wd.rows("v", src, r), mids[src], shift, kappa, wd.mus[src]) for src, shift, kappa in spec] for spec in specs]
    for chunk in ((0, 4), (k - 1, 2)):
        got = wd.eval_chunk(3, r, chunk, terms=terms)
        for s in range(3):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, sh.slot_a_tag(s)), full_ncol=m_g,
                                           col_offset=chunk[0])
            # the reference's association: (c_b0 P0_src) P1_s, with plainref's own products
            plain_terms = [(wd.rows("v", src, r).to_rns(), P.slot_mul_sum(None, [c_b0], [wd.p0[src].to_rns()], moduli, False), shift, kappa, wd.mus[src])
                           for src, shift, kappa in specs[s]]
            want = plain_eval(c_b0, sh.gate_chunk(GATE, s, *chunk).to_rns(), sh.p1_chunk(s, *chunk).to_rns(), digits_eval(u, moduli, base, dpt, slots),
                              plain_terms, moduli, n)
            assert np.array_equal(got[s].to_rns(), want), (ctx, chunk, s)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """Every matrix of the call at level 0 / 1 of a three-limb context (the refusal list below only shows that MIXED levels
    are turned away): m_g = d * dpt * (level + 1) with dpt from the CONTEXT's crt_bits (one width per basis here, so plainref
    derives the same dpt from the truncated basis), A_s sampled in limbs 0..level only, x^shift from the roots of limbs
    0..level, and plain_eval above at moduli[: level + 1]; one and two terms per output, the combine entry with the digits
    given."""
    n, d, r, w0, w1 = 16, 2, 2, 3, 4
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    m_g = d * k
    slots = list(range(n))
    rnd = lambda seed, rows, ncols: oracle.random_matrix(seed + level, rows, ncols, moduli, n)  # noqa: E731
    up = lambda a: M.from_rns(p, a, True)  # noqa: E731
    c_b0 = rnd(850, r, w0)
    specs = [[(0, 1, full_modulus(moduli) - 1)], [(3, 3, 5), (2 * n - 1, (1 << 32) - 1, (1 << 70) + 9)]]  # (shift, kappa, mu) per term
    terms_np = [[(rnd(860 + 10 * s + 2 * t, r, m_g), rnd(861 + 10 * s + 2 * t, r, w1)) + spec for t, spec in enumerate(ts)] for s, ts in enumerate(specs)]
    terms = [[(up(c_in), up(mid), shift, kappa, mu) for c_in, mid, shift, kappa, mu in ts] for ts in terms_np]
    tags = [b"slot_low_level_" + bytes([48 + s]) for s in range(2)]
    g_c_b0 = up(c_b0)
    for chunk in ((0, min(4, m_g)), (k - 1, 2)):
        pg_np, p1_np = [rnd(880 + s, w0, chunk[1]) for s in range(2)], [rnd(890 + s, w1, chunk[1]) for s in range(2)]
        pgs, p1s = [up(a) for a in pg_np], [up(a) for a in p1_np]
        got = M.slot_transfer_eval(None, g_c_b0, pgs, p1s, terms, chunk[0], KEY, tags)
        ds = []
        for s in range(2):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tags[s]), full_ncol=m_g,
                                           col_offset=chunk[0])
            ds.append(digits_eval(u, moduli, base, dpt, slots))
            want = plain_eval(c_b0, pg_np[s], p1_np[s], ds[s], terms_np[s], moduli, n)
            assert got[s].level == level and got[s].is_ntt and np.array_equal(got[s].to_rns(), want), (bits, level, chunk, s)
        given = M.slot_transfer_eval_combine(None, g_c_b0, pgs, p1s, terms, up(np.concatenate(ds, axis=1)), chunk[0])
        for s in range(2):
            assert given[s] == got[s], (bits, level, chunk, s)


# ---------------------------------------------------------------------------------------------------
# 4. the combine entry alone in every width class: the lazy windows of both kernels
# ---------------------------------------------------------------------------------------------------
REACHABLE = 64  # cells whose shortest lazy window is at most this get sizes that pass it in every segment


def fold_places(window, w0, m_g, w1):
    """where the main kernel folds before the final reduction, for terms 0 .. w0 + m_g + w1 - 1 in its order (Pg, the digits,
    P1): before every term t > 0 with t % window == 0"""
    places = set()
    for t in range(window, w0 + m_g + w1, window):
        places.add("inside Pg" if t < w0 else "first seam" if t == w0 else "inside the digits" if t < w0 + m_g else
                   "second seam" if t == w0 + m_g else "inside P1")
    return places


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_combine_entry_alone_in_every_width_class(gpu, cell):
    """All operands q - 1 ("top"), then random ones, against plainref.  A limb's window is the number of (q - 1)^2 products its
    accumulator holds on top of a residue; where the shortest window of a cell is at most REACHABLE the inner sizes are two
    windows per segment, so that the main kernel folds inside Pg, on the Pg / digits seam, inside the digits, on the digits /
    P1 seam and inside P1 (asserted below from the kernel's term order).  The other cells' windows (thousands of terms, 2^20
    where the library caps them) are past what a test of a few seconds can stream with plainref behind it; there the entry
    runs at small sizes.  In the 31- and 62-bit classes the term count passes the largest window (17 and 65 terms), so the
    pre-pass folds as well, with its products at (q - 1)^2: kappa mu = -1 mod every q_l, or kappa = -1 mod the limb of the
    shortest window."""
    n, moduli, bases, slots = _cell(cell)
    M, L = gpu.GpuDCRTPolyMatrix, len(moduli)
    bits = max(int(q).bit_length() for q in moduli)
    windows = _windows(moduli)
    small = min(windows)
    Q = full_modulus(moduli)
    q_small = moduli[windows.index(small)]
    for base in bases[:1] if small <= REACHABLE else bases:
        p = _params(gpu, n, moduli, base)
        k = L * P.digits_per_tower(moduli, base)
        if small <= REACHABLE:
            # two of the shortest window per segment: a fold inside each (terms small, w0 + small, w0 + m_g + small) and on both
            # seams (terms w0 and w0 + m_g); m_g a multiple of k as well
            w0 = w1 = 2 * small
            m_g = 2 * small * k // int(np.gcd(2 * small, k))
            seen = set()
            for window in windows:
                seen |= fold_places(window, w0, m_g, w1)
            assert {"inside Pg", "first seam", "inside the digits", "second seam", "inside P1"} <= seen, (base, windows, w0, m_g, w1, seen)
        else:
            w0, m_g, w1 = 3, k, 2
        c = min(m_g, 5)  # the ragged column tile
        col_start = m_g - c
        nterms = 3
        if cell[0] == "class" and cell[1] in (31, 62):  # a term count past the largest window: the pre-pass folds too
            assert (small, max(windows)) == STATED_WINDOWS[cell[1]]
            nterms = {31: 17, 62: 65}[cell[1]]
            assert nterms > max(windows)
        rng = np.random.default_rng(4000 + bits + base)
        up = lambda a: M.from_rns(p, a, True)  # noqa: E731
        top = lambda rows, ncols: _top(rows, ncols, moduli, n)  # noqa: E731
        for kind, S, r in (("top", 2, 1), ("top terms", 2, 2), ("random", 2, 3)):
            make = (lambda rows, ncols: _rand(rng, rows, ncols, moduli, n)) if kind == "random" else top
            c_b0, pgs, p1s, digits = make(r, w0), [make(w0, c) for _ in range(S)], [make(w1, c) for _ in range(S)], make(m_g, S * c)
            if kind == "top":
                # mu = 1, kappa = 1: LhsA = c_in and LhsB = mid, every word q - 1 in all three streams of the main kernel; output 0
                # reads c_in in place, output 1 goes through the pre-pass (shift 2N)
                plain = [[(top(r, m_g), top(r, w1), 0, 1, 1)], [(top(r, m_g), top(r, w1), 2 * n, 1, 1)]]
            elif kind == "top terms":
                # output 0: kappa mu = -1 in every limb, the B segment's products at (q - 1)^2; output 1: kappa = -1 in the limb of the
                # shortest window, both segments at (q - 1)^2 there
                plain = [[(top(r, m_g), top(r, w1), 0, 1, Q - 1) for _ in range(nterms)], [(top(r, m_g), top(r, w1), 0, q_small - 1, 1) for _ in range(nterms)]]
            else:
                plain = [[(make(r, m_g), make(r, w1), int(rng.integers(0, 4 * n)), int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 62)) ** 2 % Q)
                          for _ in range(nterms)] for _ in range(S)]
            terms = [[(up(a), up(b), sh, ka, mu) for a, b, sh, ka, mu in ts] for ts in plain]
            got = M.slot_transfer_eval_combine(None, up(c_b0), [up(a) for a in pgs], [up(a) for a in p1s], terms, up(digits), col_start)
            for s in range(S):
                want = plain_eval(c_b0, pgs[s], p1s[s], digits[:, s * c:(s + 1) * c], plain[s], moduli, n, slots)
                assert got[s].size() == (r, c) and got[s].is_ntt
                res = got[s].to_rns()
                assert np.array_equal(res[..., slots], want), (cell, base, kind, s)
                if kind != "random":  # constant operands, shifts that are multiples of 2N: every slot holds the same word
                    assert np.array_equal(res, np.broadcast_to(want[..., :1], res.shape)), (cell, base, kind, s)


# ---------------------------------------------------------------------------------------------------
# 5. the output read in place and the same output through the pre-pass
# ---------------------------------------------------------------------------------------------------
def test_in_place_output_equals_the_pre_pass_forms(gpu, oracle):
    wd = world_of(gpu, oracle, "n16_51", 2)
    r, chunk, n = 2, (3, 5), wd.p.ring_dimension()
    sh = wd.shared(r)
    mids = wd.ST.transfer_mids(sh, range(NSRC))
    vec, mid, mu = wd.rows("v", 1, r), mids[1], wd.mus[1]
    forms = {"in place": [(vec, mid, 0, 1, mu)], "shift 2N": [(vec, mid, 2 * n, 1, mu)], "shift 4N": [(vec, mid, 4 * n, 1, mu)]}
    outs = {name: wd.eval_chunk(2, r, chunk, terms=[ts, ts])[1] for name, ts in forms.items()}
    want = cols(wd.ST.output_slot(sh, GATE, wd.inputs(r), wd.plaintexts, [(1, None), (1, None)], 1, wd.m_g)[0], chunk)
    for name, out in outs.items():
        assert out == want, name
    # the term split in two of scalar 1: the input vector as a sum of two vectors, mu as a sum of two integers mod Q
    Q = full_modulus(wd.p.moduli())
    half = wd.rows("v", 2, r)
    split = [(half, mid, 0, 1, 12345), (vec - half, mid, 0, 1, (mu - 12345) % Q)]
    assert wd.eval_chunk(2, r, chunk, terms=[forms["in place"], split])[1] == want


# ---------------------------------------------------------------------------------------------------
# 6. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_depend_on_neither_the_slot_count_nor_the_term_count(gpu, oracle):
    from mxx_amd import _ffi

    wd = world_of(gpu, oracle, "n256_51", 2)
    M, chunk, r = gpu.GpuDCRTPolyMatrix, (0, 4), 1
    sh = wd.shared(r)
    mids = wd.ST.transfer_mids(sh, range(NSRC))

    def trace(fn):
        _ffi.trace_begin()
        fn()
        events = _ffi.trace_end()
        return [e["kernel"] for e in events if e["threads"]], [e["kernel"] for e in events if not e["threads"]]  # copies: no threads

    def terms_of(S, per_out):
        if per_out == 1:
            return [[(wd.rows("v", t % NVEC, r), mids[t % NSRC], 0, 3, wd.mus[t % 4])] for t in range(S)]
        return [[(wd.rows("v", (t + j) % NVEC, r), mids[j % NSRC], j, 1, wd.mus[j % 4]) for j in range(per_out)] for t in range(S)]

    for s in range(48):  # the stored chunks are cut once, outside the traces
        sh.gate_chunk(GATE, s, *chunk), sh.p1_chunk(s, *chunk)
    legs = {}
    for S in (2, 48):
        for per_out in (1, 8):
            terms = terms_of(S, per_out)
            legs[(S, per_out)] = trace(lambda: wd.eval_chunk(S, r, chunk, terms=terms))
    sampler = trace(lambda: M.sample_hash_decomposed_blocks(wd.p, KEY, sh.slot_a_tags(range(48)), wd.d, wd.m_g, chunk[0], chunk[1],
                                                            _ffi.GPU_MATRIX_DIST_UNIFORM))
    first = legs[(2, 1)]
    for key, leg in legs.items():
        assert leg == first, key
    # exactly two kernels and one copy more than the sampler's call
    assert len(first[0]) == len(sampler[0]) + 2 and len(first[1]) == len(sampler[1]) + 1
    extra = list(first[0])
    for name in sampler[0]:
        extra.remove(name)
    assert len(extra) == 2 and "slot_eval_lhs_kernel" in extra[0] and "slot_eval_kernel" in extra[1]
    # the whole gate for 2 destinations, stage 1 included, against the literal sequence over the same column chunks
    src_slots = [src_slot_of(t) for t in range(2)]
    for c0, cl in sh.column_chunks(CHUNK):
        for s in range(2):
            sh.gate_chunk(GATE, s, c0, cl), sh.p1_chunk(s, c0, cl)
    gate = trace(lambda: wd.ST.slot_transfer_slots(sh, GATE, wd.inputs(r), wd.mus, src_slots, CHUNK))
    loop = trace(lambda: [wd.ST.output_slot(sh, GATE, wd.inputs(r), wd.plaintexts, src_slots, t, CHUNK) for t in range(2)])
    print(f"one call: {len(first[0])} kernels {first[0]}, copies {first[1]}; sampler alone {len(sampler[0])} and {len(sampler[1])} copies; the gate "
          f"for 2 slots over {len(sh.column_chunks(CHUNK))} chunks {len(gate[0])} kernels and {len(gate[1])} copies, the literal sequence "
          f"{len(loop[0])} kernels and {len(loop[1])} copies")
    assert len(gate[0]) + len(gate[1]) < len(loop[0]) + len(loop[1]) and len(gate[0]) < len(loop[0])
    assert len(first[0]) + len(first[1]) < len(loop[0]) + len(loop[1])


# ---------------------------------------------------------------------------------------------------
# 7. groups
# ---------------------------------------------------------------------------------------------------
def test_three_groups_equal_the_ungrouped_call(gpu, oracle, hip_env):
    wd = world_of(gpu, oracle, "n16_51", 2)
    p, chunk, r, S = wd.p, (3, 5), 2, 7
    whole = wd.eval_chunk(S, r, chunk)
    poly_bytes = len(p.moduli()) * p.ring_dimension() * 8
    slot_bytes = (wd.m_g * chunk[1] + r * (wd.m_g + wd.w1)) * poly_bytes
    for budget in (1, 3 * slot_bytes):  # one output per group; groups of 3, 3 and 1
        hip_env.set("MXX_HIP_SLOT_EVAL_BUDGET", str(budget))
        for t, (a, b) in enumerate(zip(wd.eval_chunk(S, r, chunk), whole)):
            assert a == b and a == cols(wd.literal(r, t)[0], chunk), (budget, t)
    hip_env.unset("MXX_HIP_SLOT_EVAL_BUDGET")


# ---------------------------------------------------------------------------------------------------
# 8. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    wd = world_of(gpu, oracle, "n16_24", 2)
    p, ST = wd.p, wd.ST
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m_g, w0, w1, c, S, r, top = wd.m_g, wd.w0, wd.w1, 2, 3, 2, len(p.moduli()) - 1
    chunk = (1, c)
    sh = wd.shared(r)
    c_b0 = sh.c_b0
    mids = ST.transfer_mids(sh, range(NSRC))
    pgs, p1s = [sh.gate_chunk(GATE, s, *chunk) for s in range(S)], [sh.p1_chunk(s, *chunk) for s in range(S)]
    # output 0: one term read in place; output 1: two terms; output 2: one term with a scalar - four terms in all
    term_list = [(wd.rows("v", 0, r), mids[0], 0, 1, wd.mus[0]), (wd.rows("v", 1, r), mids[1], 1, 1, wd.mus[1]),
                 (wd.rows("v", 2, r), mids[2], 2, 1, wd.mus[2]), (wd.rows("v", 3, r), mids[3], 0, 3, wd.mus[3])]
    offsets = [0, 1, 3, 4]
    sentinel = oracle.random_matrix(85, r, c, moduli, n)
    wide_sentinel = oracle.random_matrix(83, r, c + 3, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    arg, keep, _ = hash_tags_arg(KEY, sh.slot_a_tags(range(S)))
    bad_form, keep2, _ = hash_tags_arg(KEY, sh.slot_a_tags(range(S)))
    bad_form.form = 9
    coeff = {name: m.clone() for name, m in (("c_b0", c_b0), ("pg", pgs[1]), ("p1", p1s[2]), ("c_in", term_list[1][0]), ("mid", term_list[2][1]))}
    for m in coeff.values():
        m.intt_all_in_place()
    mu_arr, wpm = M._int_rows([t[4] for t in term_list])

    def array(ms):
        return None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])

    def term_array(ts):
        if ts is None:
            return None
        arr = (_ffi.GpuSlotTerm * max(len(ts), 1))()
        for j, (c_in, mid, shift, scalar, _) in enumerate(ts):
            arr[j].c_in, arr[j].mid = None if c_in is None else c_in.raw.value, None if mid is None else mid.raw.value
            arr[j].shift, arr[j].scalar = shift, scalar
        return arr

    def call(outs, S_=S, dst_col=0, col_start=1, base_bits=base, tags=arg, b0=c_b0, g=pgs, b1=p1s, ts=term_list, offs=offsets, mus=True, words=wpm,
             arr=True, entry=None, digits=None):
        fn = getattr(lib, entry or ENTRY)
        last = (None if tags is None else C.byref(tags)) if entry is None else (None if digits is None else digits.raw)
        return fn(array(outs) if arr else None, S_, dst_col, None if b0 is None else b0.raw, array(g), array(b1), term_array(ts),
                  None if offs is None else (C.c_size_t * len(offs))(*offs), mu_arr.ctypes.data_as(C.POINTER(C.c_uint64)) if mus else None, words,
                  col_start, base_bits, last)

    def rows_of(m, lo, hi):  # r x c views into an operand's storage
        return m.reshape_view(m.nrow * m.ncol // c, c).row_view(lo, hi)

    def swap(ms, at, m):
        return [m if j == at else x for j, x in enumerate(ms)]

    def term(at, c_in=Ellipsis, mid=Ellipsis):
        t = term_list[at]
        return swap(term_list, at, (t[0] if c_in is Ellipsis else c_in, t[1] if mid is Ellipsis else mid) + t[2:])

    new = lambda rows, ncols, params=p, level=top: M(params, rows, ncols, level, True)  # noqa: E731
    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null output (slot 1)"),
        "null c_b0": (lambda o: call(o, b0=None), "null"),
        "null gate_preimages": (lambda o: call(o, g=None), "null"),
        "null gate_preimages entry": (lambda o: call(o, g=swap(pgs, 1, None)), "null operand (slot 1)"),
        "null b1_preimages": (lambda o: call(o, b1=None), "null"),
        "null b1_preimages entry": (lambda o: call(o, b1=swap(p1s, 2, None)), "null operand (slot 2)"),
        "null terms": (lambda o: call(o, ts=None), "null"),
        "null c_in": (lambda o: call(o, ts=term(2, c_in=None)), "null operand (term 2)"),
        "null mid": (lambda o: call(o, ts=term(3, mid=None)), "null operand (term 3)"),
        "null term_offsets": (lambda o: call(o, offs=None), "null"),
        "null mu_words": (lambda o: call(o, mus=False), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "term_offsets not from 0": (lambda o: call(o, offs=[1, 2, 3, 4]), "term_offsets"),
        "term_offsets decreasing": (lambda o: call(o, offs=[0, 2, 1, 4]), "term_offsets"),
        "an output without terms": (lambda o: call(o, offs=[0, 1, 1, 4]), "without terms (slot 1)"),
        "words_per_mu 0": (lambda o: call(o, words=0), "words_per_mu"),
        "c_b0 of another context": (lambda o: call(o, b0=new(r, w0, other)), "context mismatch"),
        "Pg of another context": (lambda o: call(o, g=swap(pgs, 1, new(w0, c, other))), "context mismatch (slot 1)"),
        "P1 of another context": (lambda o: call(o, b1=swap(p1s, 2, new(w1, c, other))), "context mismatch (slot 2)"),
        "c_in of another context": (lambda o: call(o, ts=term(1, c_in=new(r, m_g, other))), "context mismatch (term 1)"),
        "mid of another context": (lambda o: call(o, ts=term(3, mid=new(r, w1, other))), "context mismatch (term 3)"),
        "output of another context": (lambda o: call(swap(o, 1, new(r, c, other))), "context mismatch (slot 1)"),
        "Pg of another level": (lambda o: call(o, g=swap(pgs, 2, new(w0, c, level=0))), "level mismatch (slot 2)"),
        "P1 of another level": (lambda o: call(o, b1=swap(p1s, 1, new(w1, c, level=0))), "level mismatch (slot 1)"),
        "c_in of another level": (lambda o: call(o, ts=term(2, c_in=new(r, m_g, level=0))), "level mismatch (term 2)"),
        "mid of another level": (lambda o: call(o, ts=term(0, mid=new(r, w1, level=0))), "level mismatch (term 0)"),
        "output of another level": (lambda o: call(swap(o, 2, new(r, c, level=0))), "level mismatch (slot 2)"),
        "Pg rows": (lambda o: call(o, g=swap(pgs, 1, new(w0 + 1, c))), "shape mismatch"),
        "P1 rows": (lambda o: call(o, b1=swap(p1s, 1, new(w1 + 1, c))), "(slot 1)"),
        "Pg chunks of different widths": (lambda o: call(o, g=swap(pgs, 2, new(w0, c + 1))), "width"),
        "P1 chunks of different widths": (lambda o: call(o, b1=swap(p1s, 2, new(w1, c + 1))), "width"),
        "c_in rows": (lambda o: call(o, ts=term(1, c_in=new(r + 1, m_g))), "(term 1)"),
        "c_in columns": (lambda o: call(o, ts=term(2, c_in=new(r, m_g + p.modulus_digits()))), "shape mismatch"),
        "mid columns": (lambda o: call(o, ts=term(3, mid=new(r, w1 + 1))), "(term 3)"),
        "m_g not a multiple of k": (lambda o: call(o, ts=[(new(r, m_g + 1),) + t[1:] for t in term_list]), "shape mismatch"),
        "output rows": (lambda o: call(swap(o, 2, new(r + 1, c))), "shape mismatch"),
        "outputs of different widths": (lambda o: call(swap(o, 2, new(r, c + 1))), "width"),
        "c_b0 not EVAL": (lambda o: call(o, b0=coeff["c_b0"]), "Eval"),
        "Pg not EVAL": (lambda o: call(o, g=swap(pgs, 1, coeff["pg"])), "Eval"),
        "P1 not EVAL": (lambda o: call(o, b1=swap(p1s, 2, coeff["p1"])), "Eval"),
        "c_in not EVAL": (lambda o: call(o, ts=term(1, c_in=coeff["c_in"])), "Eval"),
        "mid not EVAL": (lambda o: call(o, ts=term(2, mid=coeff["mid"])), "Eval"),
        "chunk past m_g": (lambda o: call(o, col_start=m_g - 1), "past"),
        "col_start past m_g": (lambda o: call(o, col_start=m_g + 1), "past"),
        "block past the outputs": (lambda o: call(o, dst_col=1), "past"),
        "dst_col past the outputs": (lambda o: call(o, dst_col=c + 1), "past"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
        # each operand kind overlapped through a row view
        "output overlaps a c_in": (lambda o: call(swap(o, 1, rows_of(term_list[2][0], 1, 1 + r))), "overlap"),
        "output overlaps a Pg": (lambda o: call(swap(o, 1, rows_of(pgs[0], 1, 1 + r))), "overlap"),
        "output overlaps a P1": (lambda o: call(swap(o, 2, rows_of(p1s[0], 1, 1 + r))), "overlap"),
    }
    mid_wide = M.from_rns(p, oracle.random_matrix(82, 2 * r, w1 * c, moduli, n), True)  # rows of c columns inside a mid's storage
    mid_view = mid_wide.reshape_view(2 * r * c, w1).row_view(0, r)
    cases["output overlaps a mid"] = (lambda o: call(swap(o, 1, rows_of(mid_wide, 0, r)), ts=term(0, mid=mid_view)), "overlap")
    b0_wide = M.from_rns(p, oracle.random_matrix(81, 2 * r, w0 * c, moduli, n), True)
    cases["output overlaps c_b0"] = (lambda o: call(swap(o, 2, rows_of(b0_wide, 0, r)), b0=b0_wide.reshape_view(2 * r * c, w0).row_view(0, r)), "overlap")
    held_mats = [c_b0] + pgs + p1s + [t[0] for t in term_list] + [t[1] for t in term_list] + [mid_wide, b0_wide]
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
    parent = M.from_rns(p, oracle.random_matrix(84, 3 * r, c, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, r), parent.row_view(r - 1, 2 * r - 1), parent.row_view(2 * r, 3 * r)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for m, res in zip(held_mats, held):
        assert np.array_equal(m.to_rns(), res)
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and S = 0, c = 0, r = 0 launch nothing
    terms_by_out = [term_list[offsets[s]:offsets[s + 1]] for s in range(S)]
    want = wd.eval_chunk(S, r, chunk, terms=terms_by_out)
    outs = [M.from_rns(p, sentinel, False) for _ in range(S)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * r, (t + 1) * r) for t in range(3)]
    assert call(disjoint) == 0
    for o, v, good in zip(outs, disjoint, want):
        o.is_ntt = v.is_ntt = True
        assert o == v and o == good
    # the partial-block rule: into outputs already EVAL the block lands at dst_col and the other columns keep their words
    partial = partial_outs()
    partial[1].ntt_all_in_place()
    kept = [o.to_rns() for o in partial]
    assert call(partial, dst_col=1) == 0
    for o, was, good in zip(partial, kept, want):
        res = o.to_rns()
        assert np.array_equal(res[:, 1:1 + c], good.to_rns()) and np.array_equal(res[:, :1], was[:, :1]) and np.array_equal(res[:, 1 + c:], was[:, 1 + c:])
    c0 = lib.gpupoly_launch_count()
    assert call([], S_=0) == 0 and call([], S_=0, arr=False, tags=None, b0=None, g=None, b1=None, ts=None, offs=None, mus=False) == 0
    assert call([new(r, 0) for _ in range(S)], g=[new(w0, 0)] * S, b1=[new(w1, 0)] * S) == 0
    assert call([new(0, c) for _ in range(S)], b0=new(0, w0), ts=[(new(0, m_g), new(0, w1)) + t[2:] for t in term_list]) == 0
    assert lib.gpupoly_launch_count() == c0
    # the combine entry names itself, counts the digits as an operand and takes any keying
    digits = new(m_g, S * c)
    check("combine: digits shape", lambda o: call(o, entry=COMBINE, digits=new(m_g, S * c + 1)), "shape", COMBINE)
    check("combine: null digits", lambda o: call(o, entry=COMBINE), "null", COMBINE)
    check("combine: output overlaps the digits", lambda o: call(swap(o, 1, rows_of(digits, 0, r)), entry=COMBINE, digits=digits), "overlap", COMBINE)
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the per-slot functions
    src_slots = [src_slot_of(t) for t in range(S)]
    default = ST.slot_transfer_slots(sh, GATE, wd.inputs(r), wd.mus, src_slots, CHUNK)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    assert call([M.from_rns(p, sentinel, False) for _ in range(S)], entry=COMBINE, digits=digits) == 0  # no sampling: any keying
    fallen = ST.slot_transfer_slots(sh, GATE, wd.inputs(r), wd.mus, src_slots, CHUNK)
    reduce_in, reduce_mu = reduce_case(wd, r, 2)
    fallen_reduce = ST.slot_reduce_slots(sh, GATE, reduce_in, reduce_mu, 3, CHUNK)
    pts = [[gpu.GpuDCRTPoly.from_biguint_to_constant(p, mu) for mu in row[:3]] for row in reduce_mu]
    for t in range(S):
        assert fallen[t] == ST.output_slot(sh, GATE, wd.inputs(r), wd.plaintexts, src_slots, t, CHUNK)[0]
        assert not (fallen[t] == default[t])  # the other keying
    for dst in range(2):
        assert fallen_reduce[dst] == ST.slot_reduce_output_slot(sh, GATE, reduce_in, pts, dst, 3, CHUNK)[0]
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert ST.slot_transfer_slots(sh, GATE, wd.inputs(r), wd.mus, src_slots, CHUNK)[2] == default[2]
    del keep, keep2


# ---------------------------------------------------------------------------------------------------
# 9. end to end, noise-free: real trapdoors, real preimages
# ---------------------------------------------------------------------------------------------------
def test_noise_free_transfer_matches_the_slot_relation(gpu, oracle):
    """test_slot_transfer_bgg_poly_encoding_matches_slot_relation (src/slot_transfer/bgg_poly_encoding.rs:746-882) at n = 16:
    B0 P0_j = [S_j | I] B1, B1 P1_j = [A_j ; -S_j G], B0 Pg_dst = S_dst A_out - kappa (S_src A_in) G^-1(A_dst), error sigma 0."""
    from mxx_amd import slot_transfer as ST
    from test_gpu_preimage_abi import seed_bytes, trapdoor_and_oracle

    d, num_slots, gate_id = 2, 3, 7
    src_slots = [(2, None), (0, 3), (1, 2)]
    p = make_params(gpu, oracle, *CONTEXTS["n16_51"])
    M, Poly, moduli, n = gpu.GpuDCRTPolyMatrix, gpu.GpuDCRTPoly, p.moduli(), p.ring_dimension()
    m_g = d * p.modulus_digits()
    rand = lambda seed, rows, ncols: M.from_rns(p, oracle.random_matrix(seed, rows, ncols, moduli, n), True)  # noqa: E731
    sampler0, td0, B0, _ = trapdoor_and_oracle(gpu, oracle, p, n, p.base_bits(), d, seed_bytes(21))
    sampler1, td1, B1, _ = trapdoor_and_oracle(gpu, oracle, p, n, p.base_bits(), 2 * d, seed_bytes(22))
    G = M.gadget_matrix(p, d)
    gate_shared = ST.SlotGateShared(p, KEY, d)
    a_out = gate_shared.a_out_columns(gate_shared.a_out_tag(gate_id), 0, m_g)
    a_in = rand(800, d, m_g)
    slot_secrets = [rand(810 + j, d, d) for j in range(num_slots)]
    eval_probe = ST.SlotEvalShared(p, KEY, d, None, None, None, None)
    slot_as = [eval_probe.slot_a(j) for j in range(num_slots)]
    identity = M.identity(p, d)
    p0 = sampler0.preimage_many_abi(p, td0, B0, [S.concat_columns([identity]) * B1 for S in slot_secrets])
    p1 = sampler1.preimage_many_abi(p, td1, B1, [ST._stack_rows([A, -(S * G)]) for A, S in zip(slot_as, slot_secrets)])
    for j in range(num_slots):
        assert B0 * p0[j] == slot_secrets[j].concat_columns([identity]) * B1 and p0[j].size() == (B0.ncol, B1.ncol)
        assert p1[j].size() == (B1.ncol, m_g)
    # the gate preimages from the preprocessing half, one column chunk at a time
    chunks = [(c0, min(4, m_g - c0)) for c0 in range(0, m_g, 4)]
    scalars = [None if k is None else Poly.from_usize_to_constant(p, k).inner for _, k in src_slots]
    pg_chunks = [[] for _ in src_slots]
    for chunk in chunks:
        targets = ST.gate_target_chunks(gate_shared, gate_id, [slot_secrets[s] * a_in for s, _ in src_slots], slot_secrets, slot_as, scalars,
                                        [gpu.GpuRngSeed.from_bytes(seed_bytes(830 + t)) for t in range(num_slots)], 0.0, chunk)
        for dst, (_, x) in enumerate(ST.sample_gate_preimages(gate_shared, sampler0, td0, B0, targets)):
            pg_chunks[dst].append(x)
    pg = {(gate_id, dst): xs[0].concat_columns(xs[1:]) for dst, xs in enumerate(pg_chunks)}
    # noise-free encodings under the secret s
    s = rand(840, 1, d)
    mus = [5, 9, 4]
    plaintexts = [Poly.from_usize_to_constant(p, mu) for mu in mus]
    input_vectors = [(s * slot_secrets[j]) * (a_in - G * plaintexts[j]) for j in range(num_slots)]
    shared = ST.SlotEvalShared.from_matrices(p, KEY, d, s * B0, p0, p1, pg)
    vectors, out_plaintexts = ST.slot_transfer(shared, gate_id, input_vectors, plaintexts, src_slots, 4)
    assert len(vectors) == len(out_plaintexts) == num_slots
    for dst, (src, kappa) in enumerate(src_slots):
        scaled = Poly.from_usize_to_constant(p, mus[src] * (1 if kappa is None else kappa))
        assert vectors[dst].size() == (1, m_g) and vectors[dst] == (s * slot_secrets[dst]) * (a_out - G * scaled), dst
        assert out_plaintexts[dst] == scaled, dst
        assert vectors[dst] == ST.output_slot(shared, gate_id, input_vectors, plaintexts, src_slots, dst, 4)[0], dst
