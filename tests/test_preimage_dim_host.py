"""Host side of the batched preimage at trapdoor dimensions 3 and 4: which shapes the mirror hands to the segmented
samplers (`GpuDCRTPolyTrapdoorSampler._segments_supported`).  No device: the parameters and the trapdoor are stubs."""
import pytest


class _Params:
    def __init__(self, n, bits, base):
        self._n, self._bits, self._base = n, bits, base

    def ring_dimension(self):
        return self._n

    def crt_bits(self):
        return self._bits

    def base_bits(self):
        return self._base


class _Rows:
    def __init__(self, d):
        self._d = d

    def row_size(self):
        return self._d


class _Trapdoor:
    def __init__(self, d):
        self.r = _Rows(d)


@pytest.fixture
def supported(monkeypatch):
    from mxx_amd.trapdoor import GpuDCRTPolyTrapdoorSampler

    for name in ("MXX_HIP_RNG_COMPAT", "MXX_HIP_P1", "MXX_PREIMAGE_BATCH"):
        monkeypatch.delenv(name, raising=False)
    return lambda n, bits, base, d: GpuDCRTPolyTrapdoorSampler._segments_supported(_Params(n, bits, base), _Trapdoor(d))


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_dimensions_up_to_four_are_batched(supported, d):
    assert supported(256, 51, 17, d) is True


def test_what_the_segmented_samplers_do_not_cover_stays_one_by_one(supported, monkeypatch):
    assert supported(256, 51, 17, 5) is False   # the p1 lane kernel holds 2d <= 8 rows
    assert supported(64, 51, 17, 3) is False    # n not a multiple of 128
    assert supported(256, 24, 5, 3) is False    # five digits per tower
    assert supported(256, 24, 6, 4) is True     # four digits per tower
    monkeypatch.setenv("MXX_HIP_P1", "simple")
    assert supported(256, 51, 17, 3) is False
