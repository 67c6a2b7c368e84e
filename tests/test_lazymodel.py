"""CPU: the lazy-reduction model (tests/lazymodel.py) against plainref, its worst-case inputs, and every threshold shift
of the transform families settled - either the shifted setting gives a wrong residue on a worst-case vector (so the
GPU file tests/test_gpu_lazy_bounds.py, which runs those vectors at the shifted width, catches it), or the analytical
worst case over the real schedule stays under the word limit (the shift is slack).

The analytical bound (Peak.bound / bound_exact) propagates every operation's proven output range through the exact
schedule the kernel runs, element by element:
- Shoup products V w - hi(V ws) q: [0, 2q) for any V < 2^W;  fold_2q: [0, 2q);  csub(x, m): x < 2m -> [0, m);
- forward butterflies U + r, U + 2q - r: the bound grows by 2q per stage, only prefolds and the final fold cut it;
- inverse A = X + Y: bounds add; D = X + 2^e q - Y: below X's bound + 2^e q, and Y below 2^e q (checked);
- signed smul_lazy / folds: (-q |D| / 2^32, q + q |D| / 2^32), intervals add and subtract;
- f64 mulmod: |T| <= q / 2 + |V| w (2u + u^2) (two roundings in the quotient estimate, u = 2^-53), with h - c q within
  ulp(|V| w) / 2 of T; folds: |x - q rint(x / q)| <= q / 2 + |x| (2u + u^2).
"""
import numpy as np
import pytest

import lazymodel as LM
import plainref as P

SEED = 20261016


def _edge(n, bits):
    return [P.primes(n, bits, 1)[0], P.primes(n, bits, 1, low=True)[0]]


# (bits, logn, path): every family at its tightest shipped width, at sizes whose schedules differ
FAMILIES = [
    (25, 10, "default"), (25, 13, "default"), (25, 14, "unsigned"), (25, 14, "whole"), (25, 16, "default"),
    (24, 14, "default"), (28, 12, "default"), (28, 14, "default"), (28, 16, "default"),
    (57, 11, "default"), (57, 15, "default"), (51, 12, "int"),
    (51, 8, "default"), (51, 13, "default"), (51, 15, "default"), (49, 12, "default"), (40, 13, "default"),
]


def _schedule(q, n, path):
    bits = q.bit_length()
    W = LM.word_size(bits)
    if W == 64 and bits <= 51 and path != "int":
        return W, None, 31
    lazy, tight, _ = LM.forms(bits)
    _, _, ip = LM.int_schedule(W, n.bit_length() - 1, "whole" if path == "whole" else "grouped")
    return W, ip, LM.TIGHT_CAP if tight else 31


# split sizes (2^15 and up) cost seconds per run: the largest prime with every other candidate, and the smallest
# prime with the remaining ones at this one (every candidate of every split size runs on the GPU)
SPLIT_BOTH_PRIMES = {(28, 16)}


@pytest.mark.parametrize("bits,logn,path", FAMILIES)
def test_model_matches_plainref(bits, logn, path):
    """Forward residues on sampled slots equal plainref's; the inverse of plainref's slots gives the input back -
    for random and constructed inputs, on the largest and the smallest prime of the class (split sizes: see
    SPLIT_BOTH_PRIMES)."""
    n = 1 << logn
    slots = sorted(set(range(0, n, max(1, n // 64))) | {n - 1})
    for i, q in enumerate(_edge(n, bits)):
        if logn >= 15 and i == 1 and (bits, logn) not in SPLIT_BOTH_PRIMES:
            continue
        W, ip, cap = _schedule(q, n, path)
        X = LM.candidates(q, n, W, ip, cap, seed=SEED + bits, randoms=1)
        for x in X if logn < 15 else X[1 - i::2]:
            y, _, _ = LM.transform(x, q, False, path=path)
            assert np.array_equal(y[slots], P.ntt_slots(x.reshape(1, -1), [q], slots)[0]), ("forward", q)
        # evaluation-domain inputs: the constructed vectors themselves; their inverse must transform back to them
        for x in X[:3]:
            z, _, _ = LM.transform(x, q, True, path=path)
            assert np.array_equal(P.ntt_slots(z.reshape(1, -1), [q], slots)[0], x[slots]), ("inverse", q)


# worst-case floors: what the constructions reach (largest prime of the class), as a fraction of the word limit,
# next to the proven bound of the same schedule.  (family, forward floor, inverse floor)
FLOORS = {
    (25, 13, "default"): (0.16, 0.37),    # proven 0.211 / 0.500
    (25, 14, "unsigned"): (0.16, 0.27),   # proven 0.225 / 0.496
    (24, 14, "default"): (0.08, 0.36),    # proven 0.112 / 0.386 (signed inverse)
    (28, 13, "default"): (0.81, 0.77),    # proven 0.875 / 1.000 (TIGHT)
    (28, 16, "default"): (0.89, 0.98),    # proven 0.999 / 0.999 (TIGHT)
    (57, 13, "default"): (0.16, 0.37),    # proven 0.211 / 0.500
    (51, 13, "default"): (0.49, 0.49),    # proven 0.875 / 0.500 (f64, ELIM 15)
    (51, 8, "default"): (0.49, 0.49),     # proven 0.875 / 0.500 (f64 small_kernel)
    (49, 13, "default"): (0.15, 0.49),    # proven 0.313 / 0.500 (f64, ELIM 63)
}


@pytest.mark.parametrize("fam", sorted(FLOORS))
def test_worst_case_peaks(fam):
    """The candidate inputs reach at least the stated floor and never pass the proven bound."""
    bits, logn, path = fam
    n = 1 << logn
    q = P.primes(n, bits, 1)[0]
    W, ip, cap = _schedule(q, n, path)
    X = LM.candidates(q, n, W, ip, cap, seed=SEED + bits, randoms=0)
    for inverse, floor in zip((False, True), FLOORS[fam]):
        peaks = [LM.transform(x, q, inverse, path=path)[1] for x in X]
        best = max(p.value for p in peaks)
        assert best >= floor, (inverse, best, floor)
        assert all(p.value <= p.bound for p in peaks), "a value past its proven bound: the model is wrong"
        assert peaks[0].bound_exact() < 1, "the shipped width must be proven"


@pytest.mark.parametrize("bits", [25, 28])
def test_mulw_operand(bits):
    """The fused product + inverse loads REDC(a w) = a w 2^-32: mulw_operand gives the a whose load is the constructed
    vector itself, word for word, on both edge primes."""
    n = 1 << 12
    rng = np.random.default_rng(SEED + bits)
    for q in _edge(n, bits):
        W, ip, cap = _schedule(q, n, "default")
        c = LM.candidates(q, n, W, ip, cap, seed=SEED, randoms=1)
        w = rng.integers(1, q, n, dtype=np.uint64)
        a = LM.mulw_operand(c, w, q)
        assert np.array_equal(LM.mont_load(a, w, q), c)
        # and the product mod q is c 2^32: the constant the kernels' last stage takes out again
        want = (c.astype(object) * ((1 << 32) % q)) % q
        assert np.array_equal((a.astype(object) * w.astype(object)) % q, want)


# ---------------------------------------------------------------------------------------------- shifts
def _bound(bits, logn, inverse, path="default", **shift):
    n = 1 << logn
    q = P.primes(n, bits, 1)[0]
    _, pk, fam = LM.transform(np.zeros(n, dtype=np.uint64), q, inverse, path=path, **shift)
    return pk.bound_exact(), fam


@pytest.mark.parametrize("logn", range(10, 18))
def test_shift_lazy_one_bit_wider_is_slack(logn):
    """runtime.hip lazy_ok `crt_bits + 7` -> `+ 6`: 26-bit moduli in 32-bit words, 58-bit in 64-bit words, on the lazy
    forms.  Forward: below (1 + 2 logN) q <= 35 q < 2^(W-0.8).  Inverse: a pass of at most 5 stages from inputs below 2q
    keeps A below 2^6 q and D below 2^5 q + 2^5 q; with q < 2^(W-6) both stay below 2^W.  The model evaluates that
    worst case over every size's real pass split (LDS, ntt14 grouped, head / tail split) and finds it under 2^W: the
    shift is slack (the comment in ntt_lds.h already states q < 2^(W-6) as the condition)."""
    for bits in (26, 58):
        for inverse in (False, True):
            b, fam = _bound(bits, logn, inverse, lazy_margin=6)
            assert ":tight" not in fam and not fam.startswith("f64")
            assert b < 1, (bits, logn, inverse, float(b))
    # one bit more is not, wherever a pass has 5 stages: the inverse can reach 2^W
    b, _ = _bound(27, logn, True, lazy_margin=5)
    assert (b >= 1) == (logn in (13, 14, 15, 17)), float(b)


def test_shift_signed_25_bits_is_slack():
    """runtime.hip signed_ok `crt_bits <= 24` -> `<= 25`: the signed grouped 2^14 inverse at 25 bits.  Every product and
    fold leaves (-q |x| / 2^32, q + q |x| / 2^32), so the A path of the 5-stage register pass sums 32 values of at most
    ~1.5 q and the last stage's A + 2^6 q, D + 2^6 q stay inside [0, 2^32); nothing reaches 2^31 in between.  The model's
    interval propagation over the real pass schedule (folds (0,2), (2,3), (3,1)) stays under the limit: slack.  At 26
    bits it does not."""
    b, fam = _bound(25, 14, True, signed_max=25)
    assert fam == "ntt14:signed"
    assert b < 1, float(b)
    b, fam = _bound(26, 14, True, signed_max=26, lazy_margin=6)
    assert fam == "ntt14:signed" and b >= 1


@pytest.mark.parametrize("logn", range(10, 18))
def test_shift_elim63_at_50_bits_is_slack(logn):
    """ntt_lds_u64.hip `crt_bits <= 49` -> `<= 50` (ELIM 63 for 50-bit moduli).  fwd_next's (1/2 + e/2) q per product is
    loose below 51 bits: the quotient estimate's error is |V| w 2^-52, a quarter of that at 50 bits, so a 5-stage
    forward pass from canonical inputs stays near 6.7 q < 8 q = 2^53 / 2^50.  The inverse A path folds after four
    additions of values within q/2 + 4: below 8 q + 64 < 2^53 for every 50-bit NTT prime.  Slack at every size."""
    for inverse in (False, True):
        b, fam = _bound(50, logn, inverse, elim=63)
        assert fam.startswith("f64")
        assert b < 1, (logn, inverse, float(b))


@pytest.mark.parametrize("logn", range(10, 18))
def test_shift_elim4095_at_41_bits_is_slack(logn):
    """`crt_bits <= 40` -> `<= 41` (ELIM 4095, no fold inside a pass, at 41 bits): the worst case stays below 1 % of
    2^53 - confirmed slack."""
    for inverse in (False, True):
        b, _ = _bound(41, logn, inverse, elim=4095)
        assert b < 0.01, (logn, inverse, float(b))


@pytest.mark.parametrize("logn", [12, 14, 16])
def test_shift_tight_29_bits_is_caught(logn):
    """runtime.hip tight_ok `crt_bits + 4` -> `+ 3`: TIGHT forms at 29 bits.  Pass ends reach 16 q > 2^32, and the model
    gives a wrong residue on every constructed vector: tests/test_gpu_lazy_bounds.py runs the same vectors at 29 bits
    and catches the shift."""
    n = 1 << logn
    q = P.primes(n, 29, 1)[0]
    _, _, ip = LM.int_schedule(32, logn)
    slots = list(range(0, n, n // 64))
    for x in LM.candidates(q, n, 32, ip, LM.TIGHT_CAP, seed=SEED, randoms=0):
        y, pk, fam = LM.transform(x, q, False, tight_margin=3)
        assert fam.endswith(":tight") and pk.value >= 1
        assert not np.array_equal(y[slots], P.ntt_slots(x.reshape(1, -1), [q], slots)[0])
