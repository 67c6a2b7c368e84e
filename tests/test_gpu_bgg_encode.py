"""GPU: the BGG+ encodings of many slots in one call (`gpupoly_matrix_bgg_encode_slots`, mxx_amd/bgg.py).

outs[i][s, c] = sum_j T[s, j] A_i[j, c] - pt[s, i] o T[s, c / k] w(c) + E[s, i m + c] is exact arithmetic on canonical
residues.  The combine entry (`gpupoly_matrix_bgg_encode_slots_combine`, the errors given or absent) is held to that formula
in plain Python integers with the gadget's weights from tests/plainref.py - nothing from oracle/ or another entry point -,
in every modulus width class with operands no sampler produces; the sampling entry is held, bit for bit through
gpu_matrix_equal, to the reference's per-slot sequence restated with the mirror's older operations
(`sample_poly_encoding_vectors_literal`) under the same seeds, and its error term to the CPU restatement of the sampler.

The folds of the lazy accumulator are asserted in the 31- and 62-bit classes alone, where a secret size within reach passes
the window.  Every other class and the mixed-width cells - those with a 31-bit limb included, whose window is long in 64-bit
words - run d = 2 and reach the final reduction only."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bgg_levels  # noqa: F401  (the entries' rows of the lower-level coverage table)
import plainref as P
import ran
from conftest import make_params
from test_gpu_fused_width_classes import CELLS, _cell, _cell_id, _params, _rand, _top, _windows

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_bgg_encode_slots"
COMBINE = "gpupoly_matrix_bgg_encode_slots_combine"
KERNEL = "bgg_encode_kernel"
Y_MAX = 65535


def seed_bytes(tag):
    return bytes((tag * 29 + 7 * i + 3) & 0xFF for i in range(32))


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(seed_bytes(tag))


def slot_tile(S):
    """the launcher's rule: the slots of one tile"""
    return 4 if S >= 3 else S


def grid_of(n, word_bytes, S, P_, m, L):
    """the launcher's grid rule: (threads, gx, entries) - a lane owns 16 bytes of a limb vector (one word where that is narrower),
    a workgroup 64 .. 256 lanes, at most 64 workgroups stride a limb vector; one (input, column, limb, slot tile) per (y, z)"""
    vn = 16 // word_bytes if n % (16 // word_bytes) == 0 else 1
    vecs = n // vn
    threads = min(256, -(-vecs // 64) * 64)
    return threads, min(-(-vecs // threads), 64), P_ * m * L * -(-S // slot_tile(S))


def formula(T, As, pt, E, moduli, base, dpt, slots=None):
    """the outputs [(S, m, L, slots)] in Python integers: T (S, d, L, n), As[i] (d, m, L, n), pt (S, P - 1, L, n) or None,
    E (S, P m, L, n) or None"""
    L, n = T.shape[2], T.shape[3]
    slots = list(range(n)) if slots is None else slots
    assert P.digits_per_tower(moduli, base) == dpt  # plainref's gadget has the context's digit count
    S, d = T.shape[:2]
    k = L * dpt
    m = d * k
    G = P.gadget(d, moduli, base, n)  # constants: the evaluation of a constant is that constant in every slot
    assert not G[..., 1:].any()
    w = G[np.arange(m) // k, np.arange(m), :, 0].astype(object)  # (m, L): non-zero in limb tower(c) alone
    assert all(np.count_nonzero(w[c]) == 1 and w[c][(c % k) // dpt] != 0 for c in range(m))
    q = np.asarray([int(x) for x in moduli], dtype=object).reshape(1, 1, L, 1)
    To = T[..., slots].astype(object)
    Tg = To[:, np.arange(m) // k]  # (S, m, L, slots): T[s, c / k]
    outs = []
    for i, A in enumerate(As):
        Ao = A[..., slots].astype(object)
        acc = sum(To[:, j, None] * Ao[None, j] for j in range(d))
        pti = 1 if i == 0 else pt[:, i - 1, None][..., slots].astype(object)
        acc = acc - pti * Tg * w[None, :, :, None]
        if E is not None:
            acc = acc + E[:, i * m:(i + 1) * m][..., slots].astype(object)
        outs.append((acc % q).astype(np.uint64))
    return outs


def up(gpu, p, a):
    return gpu.GpuDCRTPolyMatrix.from_rns(p, a, True)


# ---------------------------------------------------------------------------------------------------
# 1. the combine entry against plain Python integers
# ---------------------------------------------------------------------------------------------------
def spanning_n(word_bytes):
    """the smallest n at which a limb vector spans more than one workgroup under the launcher's rule"""
    n = 2
    while grid_of(n, word_bytes, 1, 1, 1, 1)[1] < 2:
        n *= 2
    return n


# (n, depth, bits, base): n = 2 is the scalar-word path; "span": the first ring with two workgroups per limb vector
RINGS = {"n2_17": (2, 1, 17, 17), "n4_24": (4, 2, 24, 12), "n16_24": (16, 2, 24, 12), "n16_28": (16, 2, 28, 14), "n16_51": (16, 2, 51, 17),
         "n256_51": (256, 3, 51, 17), "span_24": (spanning_n(4), 2, 24, 12)}
# (ring, d, S, P): d = 1, 2, 3; S = 1, 3, 65; P = 1 (no plaintext matrix), 2, 5
COMBINE_CASES = [("n2_17", 1, 3, 2), ("n2_17", 2, 65, 5), ("n4_24", 2, 65, 5), ("n4_24", 3, 1, 1), ("n16_24", 3, 1, 1), ("n16_24", 2, 3, 5),
                 ("n16_28", 1, 65, 2), ("n16_51", 3, 3, 2), ("n16_51", 2, 65, 1), ("n16_51", 1, 1, 5), ("n256_51", 2, 3, 5), ("span_24", 1, 3, 2)]


@pytest.mark.parametrize("ring,d,S,P_", COMBINE_CASES)
def test_combine_entry_equals_the_formula_in_python_integers(gpu, oracle, ring, d, S, P_):
    n, depth, bits, base = RINGS[ring]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
    L, dpt = len(moduli), -(-p.crt_bits() // base)
    m = d * L * dpt
    assert m == d * p.modulus_digits()
    if ring.startswith("span"):
        assert grid_of(n, 4, S, P_, m, L)[1] == 2 and grid_of(n // 2, 4, S, P_, m, L)[1] == 1
    slots = None if n <= 16 else sorted({0, 1, 2, 3, 4, n // 2 - 1, n // 2, n - 5, n - 4, n - 1} | ({1023, 1024, 1027, 1028} if n > 1028 else set()))
    rng = np.random.default_rng(4000 + n + 10 * d + S + P_)
    T = _rand(rng, S, d, moduli, n)
    keys = [_rand(rng, d, m, moduli, n) for _ in range(min(P_, 3))]
    which = [0, 1, 0, 2, 1][:P_]  # one public key given for two inputs
    pt = _rand(rng, S, P_ - 1, moduli, n) if P_ > 1 else None
    E = _rand(rng, S, P_ * m, moduli, n)
    gT, gkeys, gpt, gE = up(gpu, p, T), [up(gpu, p, a) for a in keys], None if pt is None else up(gpu, p, pt), up(gpu, p, E)
    pubkeys = [gkeys[j] for j in which]
    for errors, e_np in ((gE, E), (None, None)):
        got = M.bgg_encode_slots_combine(gT, pubkeys, gpt, errors)
        want = formula(T, [keys[j] for j in which], pt, e_np, moduli, base, dpt, slots)
        assert len(got) == P_
        for i in range(P_):
            assert got[i].size() == (S, m) and got[i].is_ntt and got[i].level == L - 1
            res = got[i].to_rns()
            assert np.array_equal(res if slots is None else res[..., slots], want[i]), (ring, d, S, P_, i, errors is not None)
    # the sampling entry without an error is the same kernel: sigma 0, no seeds
    plain = M.bgg_encode_slots(gT, pubkeys, gpt, 0.0, None)
    for i in range(P_):
        assert plain[i] == got[i]
    # every input, residues and tag, as it was
    for mat, a in [(gT, T), (gE, E)] + list(zip(gkeys, keys)) + ([(gpt, pt)] if pt is not None else []):
        assert mat.is_ntt and np.array_equal(mat.to_rns(), a)


def test_a_packed24_public_key_is_unpacked_first(gpu, oracle):
    n, depth, bits, base = RINGS["n16_24"]
    p = make_params(gpu, oracle, n, depth, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
    d, S = 2, 3
    m = d * p.modulus_digits()
    A = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, d, m, gpu.DistType.FinRingDist())
    assert A.layout == "packed24"
    rng = np.random.default_rng(4100)
    T, pt, E = _rand(rng, S, d, moduli, n), _rand(rng, S, 1, moduli, n), _rand(rng, S, 2 * m, moduli, n)
    got = M.bgg_encode_slots_combine(up(gpu, p, T), [A, A], up(gpu, p, pt), up(gpu, p, E))
    assert A.layout == "words"
    a = A.to_rns()
    want = formula(T, [a, a], pt, E, moduli, base, -(-p.crt_bits() // base))
    for i in range(2):
        assert np.array_equal(got[i].to_rns(), want[i]), i


# ---------------------------------------------------------------------------------------------------
# 2. every width class, random and worst-case operands, the folds of the lazy accumulator
# ---------------------------------------------------------------------------------------------------
SMALL_WINDOWS = {("class", 31), ("class", 62)}  # the classes whose lazy window a secret size within reach can pass
MAX_KEY_POLYS = 16384  # a d x m public key beyond this is not built: d stays at one window


def fold_places(window, d):
    """where a limb with this window folds before the final reduction: the accumulator starts at the error's residue, takes
    the d products as terms 0 .. d - 1 and the gadget term as term d, and folds before every term t > 0 with t % window == 0"""
    return {"among the products" if t < d else "on the gadget term" for t in range(window, d + 1, window)}


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_combine_entry_in_every_width_class(gpu, cell):
    n, moduli, bases, slots = _cell(cell)
    M, L = gpu.GpuDCRTPolyMatrix, len(moduli)
    windows = _windows(moduli)  # (q - 1) + terms (q - 1)^2 below 2^64, or 2^128 for 64-bit words: runtime.hip's lazy_terms
    wide = max(moduli) >> 31 != 0
    assert windows == [min(((1 << (128 if wide else 64)) - q) // (q - 1) ** 2, 1 << 20) for q in moduli]
    small = min(windows)
    seen = set()
    for base in bases:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        k = L * dpt
        if cell in SMALL_WINDOWS:
            # d + 1 terms past the shortest window: d = two windows folds among the products (term `small`) and on the gadget
            # term (term d) in the limbs of that window; one window where the key would be too large folds on the gadget term
            d = 2 * small if 2 * small * 2 * small * k <= MAX_KEY_POLYS else small
            assert d + 1 > small
        else:
            d = 2
        m = d * k
        for window in windows:
            seen |= fold_places(window, d)
        rng = np.random.default_rng(5000 + 7 * base + n + L)
        for kind, S, P_ in (("top", 1, 2), ("random", 3, 2)):
            make = (lambda rows, cols: _top(rows, cols, moduli, n)) if kind == "top" else (lambda rows, cols: _rand(rng, rows, cols, moduli, n))
            T, A, pt, E = make(S, d), make(d, m), make(S, P_ - 1), make(S, P_ * m)
            gA = up(gpu, p, A)
            got = M.bgg_encode_slots_combine(up(gpu, p, T), [gA] * P_, up(gpu, p, pt), up(gpu, p, E))
            want = formula(T, [A] * P_, pt, E, moduli, base, dpt, slots)
            for i in range(P_):
                res = got[i].to_rns()
                assert np.array_equal(res[..., slots], want[i]), (cell, base, kind, i)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(res, np.broadcast_to(res[..., :1], res.shape)), (cell, base, i)
    if cell in SMALL_WINDOWS:
        assert "among the products" in seen, (cell, windows, seen)
        assert "on the gadget term" in seen, (cell, windows, seen)


# ---------------------------------------------------------------------------------------------------
# 3. the sampling entry against the literal per-slot sequence
# ---------------------------------------------------------------------------------------------------
SAMPLING = {"n128_28": (128, 2, 28, 14), "n256_51": (256, 3, 51, 17), "n1024_24": (1024, 2, 24, 12)}
_WORLD = {}


class World:
    """what the tests of one (context, d) share, made once and left unchanged: 17 slots, 3 inputs"""

    S, P_ = 17, 3

    def __init__(self, gpu, oracle, ctx, d):
        from mxx_amd import bgg

        self.gpu, self.d = gpu, d
        p = self.p = make_params(gpu, oracle, *SAMPLING[ctx])
        M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
        self.m = d * p.modulus_digits()
        rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
        self.secret = rand(700 + d, 1, d)
        self.sampler = bgg.BGGPolyEncodingSampler(p, [self.secret.entry(0, j) for j in range(d)], None)
        self.masks = self.sampler.sample_slot_secret_mats(p, self.S, _seeds=[gseed(gpu, 800 + s) for s in range(self.S)])
        self.mask_list = [self.masks.slice_columns(s * d, (s + 1) * d) for s in range(self.S)]
        self.T = self.sampler.slot_secrets(p, self.masks, self.S).clone()
        if ctx == "n1024_24":  # the packed storage a hash-sampled public key starts in
            hashed = gpu.GpuDCRTPolyHashSampler()
            self.keys = [hashed.sample_hash(p, bytes(32), b"bgg_key_%d" % i, d, self.m, gpu.DistType.FinRingDist()) for i in range(self.P_)]
            assert all(k.layout == "packed24" for k in self.keys)
        else:
            self.keys = [rand(710 + i, d, self.m) for i in range(self.P_)]
        self.pt = rand(720, self.S, self.P_ - 1)
        self.pt_rows = [[self.pt.entry(s, i) for s in range(self.S)] for i in range(self.P_ - 1)]
        self.seeds = [gseed(gpu, 900 + s) for s in range(self.S)]
        self._literal = {}

    def literal(self, sigma):
        """[input][slot] of the per-slot sequence for all 17 slots: slot s does not depend on the slot count"""
        from mxx_amd import bgg

        if sigma not in self._literal:
            M, p = self.gpu.GpuDCRTPolyMatrix, self.p
            all_keys = self.keys[0].concat_columns(self.keys[1:])
            self._literal[sigma] = bgg.sample_poly_encoding_vectors_literal(p, self.secret, all_keys, M.gadget_matrix(p, self.d), self.pt_rows,
                                                                            self.mask_list, self.S, self.P_, self.m, sigma, _seeds=self.seeds)
        return self._literal[sigma]

    def encode(self, S, sigma):
        M = self.gpu.GpuDCRTPolyMatrix
        return M.bgg_encode_slots(self.T.row_view(0, S), self.keys, self.pt.row_view(0, S), sigma, self.seeds[:S])


def world_of(gpu, oracle, ctx, d):
    if (ctx, d) not in _WORLD:
        _WORLD[(ctx, d)] = World(gpu, oracle, ctx, d)
    return _WORLD[(ctx, d)]


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(SAMPLING))
def test_sampling_entry_equals_the_literal_sequence(gpu, oracle, ctx, d):
    wd = world_of(gpu, oracle, ctx, d)
    for sigma in (3.5, 4.578, 0.0):
        gots = {S: wd.encode(S, sigma) for S in (1, 3, 17)}  # before the literal leg: packed keys are unpacked by the entry itself
        assert all(k.layout == "words" for k in wd.keys)
        want = wd.literal(sigma)
        for S, got in gots.items():
            assert len(got) == wd.P_
            for i in range(wd.P_):
                assert got[i].size() == (S, wd.m) and got[i].is_ntt
                for s in range(S):
                    assert got[i].row_view(s, s + 1) == want[i][s], (ctx, d, sigma, S, i, s)
    assert not (wd.literal(3.5)[0][0] == wd.literal(0.0)[0][0])


def test_the_error_term_is_the_plain_samplers_row_under_the_slots_seed(gpu, oracle):
    wd = world_of(gpu, oracle, "n256_51", 2)
    p, S, sigma = wd.p, 3, 4.578
    moduli, n = p.moduli(), p.ring_dimension()
    noisy, clean = wd.encode(S, sigma), wd.encode(S, 0.0)
    for s in range(S):
        e = oracle.matrix_ntt(oracle.sample_distribution(1, wd.P_ * wd.m, moduli, n, "gauss", sigma, seed_bytes(900 + s)), moduli)
        for i in range(wd.P_):
            diff = (noisy[i] - clean[i]).to_rns()[s:s + 1]
            assert np.array_equal(diff, e[:, i * wd.m:(i + 1) * wd.m]), (s, i)


def test_several_groups_equal_the_ungrouped_call(gpu, oracle, hip_env):
    wd = world_of(gpu, oracle, "n128_28", 2)
    p, S, sigma = wd.p, 7, 3.5
    whole = wd.encode(S, sigma)
    # a slot's scratch: its 1 x P m error row and the int64 samples staged for it
    slot_bytes = wd.P_ * wd.m * (len(p.moduli()) * p.ring_dimension() * p.ctx().word_bytes() + p.ring_dimension() * 8)
    for budget, groups in ((1, 7), (3 * slot_bytes, 3)):  # one slot per group; groups of 3, 3 and 1
        hip_env.set("MXX_HIP_BGG_ENCODE_BUDGET", str(budget))
        with ran.launches() as seen:
            got = wd.encode(S, sigma)
        assert len(seen.blocks_of(KERNEL)) == groups, (budget, list(seen))
        for i in range(wd.P_):
            assert got[i] == whole[i], (budget, i)
    hip_env.unset("MXX_HIP_BGG_ENCODE_BUDGET")
    with ran.launches() as seen:
        wd.encode(S, sigma)
    assert len(seen.blocks_of(KERNEL)) == 1


# ---------------------------------------------------------------------------------------------------
# 4. the mirror
# ---------------------------------------------------------------------------------------------------
def relation_holds(gpu, p, sampler, public_keys, sampled, masks, num_slots, d):
    """the predicate of the reference's test: vector(slot) == t A - t (G o pt) for every input and slot"""
    M = gpu.GpuDCRTPolyMatrix
    gadget = M.gadget_matrix(p, d)
    assert len(sampled) == len(public_keys)
    for slot in range(num_slots):
        assert sampled[0].plaintext(slot) == gpu.GpuDCRTPoly.const_one(p)
    for idx, enc in enumerate(sampled):
        assert enc.pubkey is public_keys[idx] and enc.num_slots == num_slots
        for slot in range(num_slots):
            t = sampler.secret_vec * masks.slice_columns(slot * d, (slot + 1) * d)
            pt = enc.plaintext(slot)
            assert pt is not None
            assert enc.vector(slot) == t * enc.pubkey.matrix - (t * (gadget * pt)), (idx, slot)


def mirror_setup(gpu, oracle, ring, d, num_slots, sigma, tag):
    from mxx_amd import bgg

    p = make_params(gpu, oracle, *ring)
    moduli, n = p.moduli(), p.ring_dimension()
    M = gpu.GpuDCRTPolyMatrix
    keys = bgg.BGGPublicKeySampler(bytes(range(32)), d).sample(p, tag, [True, True])
    assert len(keys) == 3 and all(k.matrix.size() == (d, d * p.modulus_digits()) for k in keys)
    uni = gpu.GpuDCRTPolyUniformSampler()
    secrets = [uni.sample_poly(p, gpu.DistType.TernaryDist()) for _ in range(d)]
    sampler = bgg.BGGPolyEncodingSampler(p, secrets, sigma)
    plaintexts = [[gpu.GpuDCRTPoly(M.from_rns(p, oracle.random_matrix(730 + 10 * i + s, 1, 1, moduli, n), True)) for s in range(num_slots)] for i in range(2)]
    return p, keys, sampler, plaintexts


def test_mirror_replays_the_references_relation_test(gpu, oracle):
    """test_bgg_poly_encoding_sampler_relation_with_slot_secret_mats (src/bgg/sampler.rs:466-528): n = 4, depth 2, 17 bits,
    base 1, d = 3, 2 slots, no error; the masks go in as compact bytes as there, and as the stacked matrix"""
    d, num_slots = 3, 2
    p, keys, sampler, plaintexts = mirror_setup(gpu, oracle, (4, 2, 17, 1), d, num_slots, None, b"relation")
    masks = sampler.sample_slot_secret_mats(p, num_slots)
    blobs = [masks.slice_columns(s * d, (s + 1) * d).into_compact_bytes() for s in range(num_slots)]
    sampled = sampler.sample(p, keys, plaintexts, blobs)
    relation_holds(gpu, p, sampler, keys, sampled, masks, num_slots, d)
    again = sampler.sample(p, keys, [[pt.to_compact_bytes() for pt in row] for row in plaintexts], masks)
    for a, b in zip(sampled, again):
        assert a.matrix == b.matrix
    fresh, fresh_masks = sampler.sample_with_fresh_slot_secret_mats(p, keys, plaintexts)
    relation_holds(gpu, p, sampler, keys, fresh, fresh_masks, num_slots, d)


def test_mirror_relation_at_n256_and_the_noise_bound(gpu, oracle):
    from mxx_amd import bgg

    d, num_slots, sigma = 2, 3, 4.578
    p, keys, sampler, plaintexts = mirror_setup(gpu, oracle, (256, 3, 51, 17), d, num_slots, 0.0, b"n256")
    masks = sampler.sample_slot_secret_mats(p, num_slots)
    clean = sampler.sample(p, keys, plaintexts, masks)
    relation_holds(gpu, p, sampler, keys, clean, masks, num_slots, d)
    noisy_sampler = bgg.BGGPolyEncodingSampler(p, [sampler.secret_vec.entry(0, j) for j in range(d)], sigma)
    noisy = noisy_sampler.sample(p, keys, plaintexts, masks)
    for a, b in zip(noisy, clean):
        bound = int((a.matrix - b.matrix).centered_max_abs())
        assert 0 < bound < 6 * sigma, bound


def test_slot_secret_mats_are_the_plain_ternary_sampler_block_by_block(gpu, oracle):
    from mxx_amd import bgg

    p = make_params(gpu, oracle, 16, 2, 51, 17)
    d, S = 3, 5
    sampler = bgg.BGGPolyEncodingSampler(p, [gpu.GpuDCRTPoly.const_one(p)] * d, None)
    seeds = [gseed(gpu, 1000 + s) for s in range(S)]
    stacked = sampler.sample_slot_secret_mats(p, S, _seeds=seeds)
    assert stacked.size() == (d, d * S) and stacked.is_ntt
    for s in range(S):
        alone = gpu.sample_gpu_matrix_with_seed(p, d, d, gpu.DistType.TernaryDist(), seeds[s])
        assert stacked.slice_columns(s * d, (s + 1) * d) == alone, s


def test_encoding_sampler_equals_its_literal_form(gpu, oracle):
    from mxx_amd import bgg

    for ring, sigma in (((256, 3, 51, 17), 3.5), ((256, 3, 51, 17), None), ((16, 2, 24, 12), 0.0)):
        p = make_params(gpu, oracle, *ring)
        M, moduli, n, d = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), 2
        keys = bgg.BGGPublicKeySampler(bytes(32), d).sample(p, b"enc", [True, False])
        poly = lambda seed: gpu.GpuDCRTPoly(M.from_rns(p, oracle.random_matrix(seed, 1, 1, moduli, n), True))  # noqa: E731
        sampler = bgg.BGGEncodingSampler(p, [poly(740), poly(741)], sigma)
        plaintexts = [poly(742), poly(743)]
        got = sampler.sample(p, keys, plaintexts, _seeds=[gseed(gpu, 1100)])
        want = sampler.sample_literal(p, keys, plaintexts, _seeds=[gseed(gpu, 1100)])
        assert len(got) == 3
        for g, w in zip(got, want):
            assert g.vector.size() == (1, d * p.modulus_digits()) and g.vector == w.vector and g.pubkey is w.pubkey
        assert got[0].plaintext == gpu.GpuDCRTPoly.const_one(p) and got[1].plaintext == plaintexts[0] and got[2].plaintext is None


def test_unsupported_rings_fall_back_to_the_plain_sampler(gpu, oracle):
    """n = 16 with sigma > 0: the library answers "unsupported", the mirror samples the rows and calls the combine entry"""
    from mxx_amd import _ffi, bgg

    d, num_slots, sigma = 2, 3, 3.5
    p, keys, sampler, plaintexts = mirror_setup(gpu, oracle, (16, 2, 51, 17), d, num_slots, sigma, b"small")
    M = gpu.GpuDCRTPolyMatrix
    masks = sampler.sample_slot_secret_mats(p, num_slots)
    seeds = [gseed(gpu, 1200 + s) for s in range(num_slots)]
    T = sampler.slot_secrets(p, masks, num_slots)
    with pytest.raises(_ffi.GpuPolyError, match="unsupported"):
        M.bgg_encode_slots(T, [k.matrix for k in keys], bgg._plaintext_matrix(p, plaintexts, num_slots), sigma, seeds)
    got = sampler.sample(p, keys, plaintexts, masks, _seeds=seeds)
    all_keys = keys[0].matrix.concat_columns([k.matrix for k in keys[1:]])
    want = bgg.sample_poly_encoding_vectors_literal(p, sampler.secret_vec, all_keys, M.gadget_matrix(p, d), plaintexts,
                                                    [masks.slice_columns(s * d, (s + 1) * d) for s in range(num_slots)], num_slots, 3,
                                                    d * p.modulus_digits(), sigma, _seeds=seeds)
    for i in range(3):
        for s in range(num_slots):
            assert got[i].vector(s) == want[i][s], (i, s)


# ---------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_depend_on_neither_slots_nor_inputs(gpu, oracle):
    from mxx_amd import _ffi, bgg

    p = make_params(gpu, oracle, 256, 3, 51, 17)
    M, moduli, n, d = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), 2
    m = d * p.modulus_digits()
    rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
    T, keys, pt = rand(750, 48, d), [rand(751 + i, d, m) for i in range(5)], rand(760, 48, 4)
    pt1 = pt.slice_columns(0, 1)
    seeds = [gseed(gpu, 1300 + s) for s in range(48)]

    def trace(fn):
        _ffi.trace_begin()
        fn()
        events = _ffi.trace_end()
        return [e["kernel"] for e in events if e["threads"]], [e["kernel"] for e in events if not e["threads"]]  # copies: no threads

    def call(S, P_, sigma):
        return trace(lambda: M.bgg_encode_slots(T.row_view(0, S), keys[:P_], (pt if P_ == 5 else pt1).row_view(0, S), sigma, seeds[:S]))

    base = call(2, 2, 3.5)
    for S, P_ in ((48, 2), (2, 5), (48, 5)):  # the sampler picks its lane kernel by size: the counts are what must not move
        kernels, copies = call(S, P_, 3.5)
        assert (len(kernels), len(copies)) == (len(base[0]), len(base[1])), (S, P_, kernels, copies)
        assert len([k for k in kernels if KERNEL in k]) == 1
    sampler = trace(lambda: M.sample_gauss_blocks(p, seeds[:2], 3.5, block_polys=2 * m))
    assert len(base[0]) == len(sampler[0]) + 1 and len(base[1]) == len(sampler[1]) + 1
    extra = list(base[0])
    for name in sampler[0]:
        extra.remove(name)
    assert len(extra) == 1 and KERNEL in extra[0]
    quiet = call(48, 5, 0.0)
    assert len(quiet[0]) == 1 and KERNEL in quiet[0][0] and len(quiet[1]) == 1
    # ONE slot of the literal sequence, its operands on the device already
    secret, mask = rand(770, 1, d), rand(771, d, d)
    all_keys, gadget = keys[0].concat_columns(keys[1:2]), M.gadget_matrix(p, d)
    rows = [[pt.entry(0, 0)]]
    loop = trace(lambda: bgg.sample_poly_encoding_vectors_literal(p, secret, all_keys, gadget, rows, [mask], 1, 2, m, 3.5, _seeds=seeds[:1]))
    print(f"one call: {len(base[0])} kernels {base[0]}, {len(base[1])} copies; one slot of the literal sequence: {len(loop[0])} kernels, {len(loop[1])} copies")
    assert len(base[0]) + len(base[1]) < len(loop[0]) + len(loop[1])
    assert len(base[0]) < len(loop[0])


# ---------------------------------------------------------------------------------------------------
# 6. the grid past 65535 tiles
# ---------------------------------------------------------------------------------------------------
def test_the_grid_folds_past_65535_tiles(gpu, oracle):
    """n = 4 in 32-bit words, two 24-bit limbs, d = 2: P m L = 32 limb vectors per slot tile, 2049 tiles of 4 slots (the last one
    ragged) give 65568 entries; every word against numpy (the products stay below 2^64)"""
    p = make_params(gpu, oracle, 4, 2, 24, 12)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    assert p.ctx().word_bytes() == 4
    L, dpt, d, P_, S = len(moduli), P.digits_per_tower(moduli, base), 2, 2, 8193
    k = L * dpt
    m = d * k
    threads, gx, entries = grid_of(n, 4, S, P_, m, L)
    assert (threads, gx) == (64, 1) and entries == 65568 > Y_MAX
    gy = min(entries, Y_MAX)
    gz = -(-entries // gy)
    assert gz == 2
    rng = np.random.default_rng(6000)
    T, A, pt, E = _rand(rng, S, d, moduli, n), [_rand(rng, d, m, moduli, n) for _ in range(P_)], _rand(rng, S, 1, moduli, n), _rand(rng, S, P_ * m, moduli, n)
    with ran.launches() as seen:
        got = M.bgg_encode_slots_combine(up(gpu, p, T), [up(gpu, p, a) for a in A], up(gpu, p, pt), up(gpu, p, E))
    assert seen.blocks_of(KERNEL) == [gx * gy * gz], seen.records
    q = np.asarray(moduli, dtype=np.uint64).reshape(1, 1, L, 1)
    G = P.gadget(d, moduli, base, n)
    w = G[np.arange(m) // k, np.arange(m), :, 0]  # (m, L)
    Tg = T[:, np.arange(m) // k]
    for i in range(P_):
        acc = E[:, i * m:(i + 1) * m].copy()
        for j in range(d):
            acc = (acc + T[:, j, None] * A[i][None, j]) % q
        hit = Tg if i == 0 else (pt[:, 0, None] * Tg) % q
        acc = (acc + (q - hit) % q * w[None, :, :, None]) % q
        assert np.array_equal(got[i].to_rns(), acc), i


# ---------------------------------------------------------------------------------------------------
# 7. below the top level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base,n", [(24, 12, 16), (51, 17, 128)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, n, level):
    """Every matrix of the call at level 0 / 1 of a three-limb context: m = d * dpt * (level + 1) with dpt from the CONTEXT's
    crt_bits (one width per basis here, so plainref derives the same dpt from the truncated basis), the integer formula over
    moduli[: level + 1]; the combine entry with errors, and at n = 128 the sampling entry, whose error row is the plain
    sampler's at that level"""
    d, S, P_ = 2, 3, 3
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    m = d * L * dpt
    slots = list(range(n)) if n <= 16 else [0, 1, 63, 64, n - 1]
    rnd = lambda seed, rows, cols: oracle.random_matrix(seed + level, rows, cols, moduli, n)  # noqa: E731
    T, A, pt, E = rnd(780, S, d), [rnd(781 + i, d, m) for i in range(P_)], rnd(790, S, P_ - 1), rnd(791, S, P_ * m)
    gT, gA, gpt = up(gpu, p, T), [up(gpu, p, a) for a in A], up(gpu, p, pt)
    assert gT.level == level
    got = M.bgg_encode_slots_combine(gT, gA, gpt, up(gpu, p, E))
    want = formula(T, A, pt, E, moduli, base, dpt, slots)
    for i in range(P_):
        assert got[i].level == level and got[i].is_ntt and got[i].size() == (S, m)
        assert np.array_equal(got[i].to_rns()[..., slots], want[i]), (bits, level, i)
    if n >= 128:
        sigma = 3.5
        noisy = M.bgg_encode_slots(gT, gA, gpt, sigma, [gseed(gpu, 1400 + s) for s in range(S)])
        rows = [oracle.matrix_ntt(oracle.sample_distribution(1, P_ * m, moduli, n, "gauss", sigma, seed_bytes(1400 + s)), moduli) for s in range(S)]
        want = formula(T, A, pt, np.concatenate(rows, axis=0), moduli, base, dpt, slots)
        for i in range(P_):
            assert noisy[i].level == level and np.array_equal(noisy[i].to_rns()[..., slots], want[i]), (bits, level, i, "sampled")


# ---------------------------------------------------------------------------------------------------
# 8. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi

    p = make_params(gpu, oracle, 128, 2, 28, 14)
    small = make_params(gpu, oracle, 16, 2, 28, 14)
    other = make_params(gpu, oracle, 128, 2, 24, 12)
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    d, S, P_, top = 2, 3, 3, len(p.moduli()) - 1
    m = d * p.modulus_digits()
    rand = lambda seed, rows, cols, params=p: M.from_rns(params, oracle.random_matrix(seed, rows, cols, params.moduli(), params.ring_dimension()), True)  # noqa: E731
    T, keys, pt, E = rand(800, S, d), [rand(801 + i, d, m) for i in range(P_)], rand(810, S, P_ - 1), rand(811, S, P_ * m)
    seeds = (gpu.GpuRngSeed * S)(*[gseed(gpu, 1500 + s) for s in range(S)])
    sentinel = oracle.random_matrix(812, S, m, moduli, n)
    coeff = {name: x.clone() for name, x in (("T", T), ("key", keys[1]), ("pt", pt), ("E", E))}
    for x in coeff.values():
        x.intt_all_in_place()

    def array(ms):
        return None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if x is None else x.raw.value for x in ms])

    raw = lambda x: None if x is None else x.raw  # noqa: E731

    def call(outs, count=P_, secrets=T, ks=keys, pts=pt, base_bits=base, sigma=3.5, sd=seeds, arr=True):
        return lib.gpupoly_matrix_bgg_encode_slots(array(outs) if arr else None, count, raw(secrets), array(ks), raw(pts), base_bits, sigma, sd)

    def combine(outs, errors=E, count=P_, secrets=T, ks=keys, pts=pt):
        return lib.gpupoly_matrix_bgg_encode_slots_combine(array(outs), count, raw(secrets), array(ks), raw(pts), base, raw(errors))

    def swap(ms, at, x):
        return [x if j == at else y for j, y in enumerate(ms)]

    def rows_of(x, lo, hi):  # S x m views into an operand's storage
        return x.reshape_view(x.nrow * x.ncol // m, m).row_view(lo, hi)

    new = lambda rows, cols, params=p, level=top: M(params, rows, cols, level, True)  # noqa: E731
    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null secrets": (lambda o: call(o, secrets=None), "null"),
        "null pubkeys": (lambda o: call(o, ks=None), "null"),
        "null pubkeys entry": (lambda o: call(o, ks=swap(keys, 1, None)), "null"),
        "null plaintexts with P > 1": (lambda o: call(o, pts=None), "plaintexts"),
        "plaintexts with P == 1": (lambda o: call(o[:1], count=1, ks=keys[:1]), "plaintexts"),
        "null seeds with sigma > 0": (lambda o: call(o, sd=None), "null seeds"),
        "key of another context": (lambda o: call(o, ks=swap(keys, 1, new(d, m, other))), "context mismatch (input 1)"),
        "plaintexts of another context": (lambda o: call(o, pts=new(S, P_ - 1, other)), "context mismatch"),
        "output of another context": (lambda o: call(swap(o, 2, new(S, m, other))), "context mismatch (input 2)"),
        "key of another level": (lambda o: call(o, ks=swap(keys, 2, new(d, m, level=0))), "level mismatch (input 2)"),
        "plaintexts of another level": (lambda o: call(o, pts=new(S, P_ - 1, level=0)), "level mismatch"),
        "output of another level": (lambda o: call(swap(o, 1, new(S, m, level=0))), "level mismatch (input 1)"),
        "key rows": (lambda o: call(o, ks=swap(keys, 1, new(d + 1, m))), "shape mismatch"),
        "m is not d k": (lambda o: call(o, ks=swap(keys, 0, new(d, m + 1))), "(input 0)"),
        "every key with m not d k": (lambda o: call(o, ks=[new(d, m - 1)] * 3), "shape mismatch"),
        "plaintext rows": (lambda o: call(o, pts=new(S + 1, P_ - 1)), "shape mismatch"),
        "plaintext columns": (lambda o: call(o, pts=new(S, P_)), "shape mismatch"),
        "output rows": (lambda o: call(swap(o, 1, new(S + 1, m))), "(input 1)"),
        "output columns": (lambda o: call(swap(o, 2, new(S, m + 1))), "shape mismatch"),
        "secrets not EVAL": (lambda o: call(o, secrets=coeff["T"]), "Eval"),
        "key not EVAL": (lambda o: call(o, ks=swap(keys, 1, coeff["key"])), "Eval"),
        "plaintexts not EVAL": (lambda o: call(o, pts=coeff["pt"]), "Eval"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "negative sigma": (lambda o: call(o, sigma=-1.0), "sigma"),
        "infinite sigma": (lambda o: call(o, sigma=math.inf), "sigma"),
        "sigma not a number": (lambda o: call(o, sigma=math.nan), "sigma"),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
        # each operand kind overlapped through a row view
        "output overlaps a key": (lambda o: call(swap(o, 1, rows_of(E, 0, S)), ks=swap(keys, 2, rows_of(E, 1, 1 + d))), "overlap"),
    }
    t_wide = rand(813, S * m, d)  # its reshape holds S x m views; rows 0 .. S of it are the secrets of the case
    cases["output overlaps the secrets"] = (lambda o: call(swap(o, 0, t_wide.reshape_view(S * d, m).row_view(0, S)), secrets=t_wide.row_view(0, S)), "overlap")
    pt_wide = rand(814, S * m, P_ - 1)
    cases["output overlaps the plaintexts"] = (lambda o: call(swap(o, 2, pt_wide.reshape_view(S * (P_ - 1), m).row_view(0, S)), pts=pt_wide.row_view(0, S)),
                                               "overlap")
    held_mats = [T, pt, E, t_wide, pt_wide] + keys
    held = [x.to_rns() for x in held_mats]

    def check(name, fn, word, entry=ENTRY):
        # COEFF-tagged: a tag flipped to EVAL would change the read-out
        outs = [M.from_rns(p, sentinel, False) for _ in range(P_)]
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
    # more than 2^20 slots: matrices of zero columns hold no storage
    check("too many slots", lambda o: call(o[:1], count=1, secrets=new((1 << 20) + 1, 0), ks=[new(0, 0)], pts=None), "2^20")
    # the combine entry names itself and counts the errors as an operand
    check("combine: errors shape", lambda o: combine(o, new(S, P_ * m + 1)), "shape", COMBINE)
    check("combine: errors not EVAL", lambda o: combine(o, coeff["E"]), "Eval", COMBINE)
    check("combine: output overlaps the errors", lambda o: combine(swap(o, 1, rows_of(E, 0, S))), "overlap", COMBINE)
    check("combine: null secrets", lambda o: combine(o, secrets=None), "null", COMBINE)
    # two outputs overlapping through views of one parent
    parent = M.from_rns(p, oracle.random_matrix(815, 3 * S, m, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, S), parent.row_view(S - 1, 2 * S - 1), parent.row_view(2 * S, 3 * S)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    # "unsupported": what the Gaussian block sampler refuses - a ring below n = 128, the reference's keying; the combine entry takes both
    sT, skeys, spt = rand(820, S, d, small), [rand(821 + i, d, m, small) for i in range(P_)], rand(830, S, P_ - 1, small)
    s_sentinel = oracle.random_matrix(831, S, m, small.moduli(), small.ring_dimension())
    souts = [M.from_rns(small, s_sentinel, False) for _ in range(P_)]
    c0 = lib.gpupoly_launch_count()
    assert call(souts, secrets=sT, ks=skeys, pts=spt) != 0
    assert "unsupported" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string() and lib.gpupoly_launch_count() == c0
    assert all(not o.is_ntt and np.array_equal(o.to_rns(), s_sentinel) for o in souts)
    # "unsupported" is judged last: a mistake in the operands is named first
    assert call(souts, secrets=sT, ks=swap(skeys, 1, M(small, d, m + 1, top, True)), pts=spt) != 0
    assert "shape mismatch" in _ffi.last_error_string() and "unsupported" not in _ffi.last_error_string()
    assert all(not o.is_ntt and np.array_equal(o.to_rns(), s_sentinel) for o in souts)
    assert call(souts, secrets=sT, ks=skeys, pts=spt, sigma=0.0, sd=None) == 0  # nothing to sample: any ring
    assert combine([M.from_rns(small, s_sentinel, False) for _ in range(P_)], rand(832, S, P_ * m, small), secrets=sT, ks=skeys, pts=spt) == 0
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    assert combine([M.from_rns(p, sentinel, False) for _ in range(P_)]) == 0  # no sampling: any keying
    assert call([M.from_rns(p, sentinel, False) for _ in range(P_)], sigma=0.0, sd=None) == 0
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    for x, res in zip(held_mats, held):
        assert np.array_equal(x.to_rns(), res)
    # the same call succeeds once the fault is gone - disjoint row views as outputs included
    outs = [M.from_rns(p, sentinel, False) for _ in range(P_)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * S, (t + 1) * S) for t in range(3)]
    assert call(disjoint) == 0
    want = M.bgg_encode_slots(T, keys, pt, 3.5, list(seeds))
    for o, v, w in zip(outs, disjoint, want):
        o.is_ntt = v.is_ntt = True
        assert o == v and o == w
    # the empty shapes launch nothing
    c0 = lib.gpupoly_launch_count()
    assert call([], count=0) == 0 and call(None, count=0, secrets=None, ks=None, pts=None, sd=None, arr=False) == 0  # P = 0
    assert call([new(0, m)] * 1, count=1, secrets=new(0, d), ks=keys[:1], pts=None) == 0  # S = 0
    empties = [new(0, m) for _ in range(P_)]
    assert call(empties, secrets=new(0, d), pts=new(0, P_ - 1)) == 0
    assert call([new(S, 0) for _ in range(P_)], secrets=new(S, 0), ks=[new(0, 0)] * P_) == 0  # d = 0, m = 0
    assert lib.gpupoly_launch_count() == c0
