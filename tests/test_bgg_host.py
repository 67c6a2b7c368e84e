"""CPU-only: what the BGG+ mirror (mxx_amd/bgg.py) decides on the host - the reference's two assertion messages,
effective_gauss_sigma, the order in which a call draws its seeds (the slots' masks first, then the slots' errors, each in slot
order) and how a BggPolyEncoding indexes slots and inputs.  The device is replaced by recording stand-ins."""
import pytest

from mxx_amd import bgg
from mxx_amd.sampler import seed_source


class FakeMatrix:
    def __init__(self, nrow, ncol, name="m"):
        self.nrow, self.ncol, self.name = nrow, ncol, name

    def row_view(self, lo, hi):
        return (self.name, "rows", lo, hi)

    def entry(self, i, j):
        return (self.name, "entry", i, j)


class FakePoly:
    @staticmethod
    def const_one(params):
        return ("one", params)


def bare_sampler(d, sigma):
    s = object.__new__(bgg.BGGPolyEncodingSampler)
    s.secret_vec, s.gauss_sigma = FakeMatrix(1, d, "s"), sigma
    return s


def test_the_references_two_assertion_messages():
    s = bare_sampler(2, None)
    keys = [bgg.BggPublicKey(None, True)] * 3
    with pytest.raises(AssertionError, match="requires all plaintext rows to have the same num_slots"):
        s.sample(None, keys, [[b"a", b"b"], [b"c"]])
    with pytest.raises(AssertionError, match=r"requires public_keys.len\(\) == plaintexts.len\(\) \+ 1"):
        s.sample(None, keys[:2], [[b"a", b"b"], [b"c", b"d"]])
    with pytest.raises(AssertionError, match=r"requires public_keys.len\(\) == plaintexts.len\(\) \+ 1"):
        s.sample(None, keys, [[b"a", b"b"]])
    assert bgg.RAGGED == "BGGPolyEncodingSampler::sample requires all plaintext rows to have the same num_slots"
    assert bgg.KEY_COUNT == "BGGPolyEncodingSampler::sample requires public_keys.len() == plaintexts.len() + 1"
    assert bgg.BGGPolyEncodingSampler.assert_uniform_num_slots([]) == 0
    assert bgg.BGGPolyEncodingSampler.assert_uniform_num_slots([[1, 2, 3], [4, 5, 6]]) == 3


def test_effective_gauss_sigma():
    assert bgg.effective_gauss_sigma(None) is None and bgg.effective_gauss_sigma(0.0) is None and bgg.effective_gauss_sigma(0) is None
    assert bgg.effective_gauss_sigma(4.578) == 4.578 and bgg.effective_gauss_sigma(1e-9) == 1e-9


def test_seeds_are_drawn_per_slot_in_slot_order(monkeypatch):
    """one fresh seed per slot for the masks, then one per slot for the errors; none for the errors without a sigma"""
    S, d = 4, 2
    stream = [bytes([16 * j + i for i in range(32)]) for j in range(2 * S)]
    seen = {}

    def fake_blocks(params, seeds, dist, *, nrow, seg_cols):
        seen["mask"] = (list(seeds), nrow, list(seg_cols))
        return FakeMatrix(nrow, sum(seg_cols), "masks")

    def fake_encode(secrets, pubkeys, plaintexts, sigma, seeds, outs=None):
        seen["encode"] = (secrets, list(pubkeys), plaintexts, sigma, None if seeds is None else list(seeds))
        return [FakeMatrix(S, 7, f"out{i}") for i in range(len(pubkeys))]

    monkeypatch.setattr(bgg.GpuDCRTPolyMatrix, "sample_distribution_blocks", staticmethod(fake_blocks))
    monkeypatch.setattr(bgg.GpuDCRTPolyMatrix, "bgg_encode_slots", staticmethod(fake_encode))
    monkeypatch.setattr(bgg.BGGPolyEncodingSampler, "slot_secrets", lambda self, params, mats, n: ("T", mats.name, n))
    monkeypatch.setattr(bgg, "_plaintext_matrix", lambda params, rows, n: FakeMatrix(n, len(rows), "pt"))

    class Params:
        @staticmethod
        def modulus_digits():
            return 3

    words = lambda seeds: [tuple(s.words) for s in seeds]  # noqa: E731
    from mxx_amd._ffi import GpuRngSeed

    want = [tuple(GpuRngSeed.from_bytes(b).words) for b in stream]
    keys = [bgg.BggPublicKey(f"A{i}", i != 2) for i in range(3)]
    rows = [[f"p{i}{s}" for s in range(S)] for i in range(2)]
    with seed_source(stream):
        got = bare_sampler(d, 3.5).sample(Params, keys, rows)
    assert words(seen["mask"][0]) == want[:S] and seen["mask"][1:] == (d, [d] * S)
    secrets, pubkeys, pt, sigma, seeds = seen["encode"]
    assert secrets == ("T", "masks", S) and pubkeys == ["A0", "A1", "A2"] and pt.name == "pt" and sigma == 3.5
    assert words(seeds) == want[S:]
    assert [e.matrix.name for e in got] == ["out0", "out1", "out2"] and [e.index for e in got] == [0, 1, 2]
    # no error: the masks' seeds alone are drawn, and the library call gets sigma 0 without seeds
    for quiet in (None, 0.0):
        with seed_source(stream[:S]):
            bare_sampler(d, quiet).sample(Params, keys, rows)
        assert words(seen["mask"][0]) == want[:S] and seen["encode"][3:] == (0.0, None)
    # masks given: the errors' seeds alone; `_seeds` gives them instead
    with seed_source(stream[:S]):
        bare_sampler(d, 3.5).sample(Params, keys, rows, FakeMatrix(d, d * S, "given"))
    assert seen["encode"][0] == ("T", "given", S) and words(seen["encode"][4]) == want[:S]
    explicit = [GpuRngSeed.from_bytes(b) for b in stream[S:]]
    with seed_source([]):
        bare_sampler(d, 3.5).sample(Params, keys, rows, FakeMatrix(d, d * S, "given"), _seeds=explicit)
    assert words(seen["encode"][4]) == want[S:]
    with pytest.raises(AssertionError, match="one seed per slot"):
        bare_sampler(d, 3.5).sample(Params, keys, rows, FakeMatrix(d, d * S, "given"), _seeds=explicit[:2])


def test_poly_encoding_indexes_slots_and_inputs(monkeypatch):
    monkeypatch.setattr(bgg, "GpuDCRTPoly", FakePoly)
    pt = FakeMatrix(3, 2, "pt")
    shown, hidden = bgg.BggPublicKey("A", True), bgg.BggPublicKey("B", False)
    enc = [bgg.BggPolyEncoding("params", FakeMatrix(3, 5, f"v{i}"), key, pt, i) for i, key in enumerate((shown, shown, hidden))]
    assert [e.num_slots for e in enc] == [3, 3, 3]
    assert enc[0].vector(0) == ("v0", "rows", 0, 1) and enc[1].vector(2) == ("v1", "rows", 2, 3)
    # input 0's plaintext is the constant 1; input i's plaintext in slot s is entry (s, i - 1); a hidden one is None
    assert enc[0].plaintext(1) == ("one", "params")
    assert enc[1].plaintext(2) == ("pt", "entry", 2, 0)
    assert enc[2].plaintext(0) is None
    shown2 = bgg.BggPolyEncoding("params", FakeMatrix(3, 5, "v2"), shown, pt, 2)
    assert shown2.plaintext(1) == ("pt", "entry", 1, 1)
    for bad in (-1, 3):
        with pytest.raises(AssertionError, match="slot out of range"):
            enc[0].vector(bad)
        with pytest.raises(AssertionError, match="slot out of range"):
            enc[1].plaintext(bad)
