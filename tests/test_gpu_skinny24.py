"""GPU: the one-row product against a 3-byte right operand (csrc/matmul_skinny24.hip).

Every instantiated shape of the kernel (MXX_HIP_SKINNY24=force:TC,G,WPE,MAP) must return exactly what the register-tile
kernel returns for the same seeded sample drawn in 4-byte words (MXX_HIP_PACK24=0, MXX_HIP_SKINNY24=0), and two output
columns per case are checked against the CPU restatement.  Rings below a whole wave run the 12-byte map whatever was asked.
"""
import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

# TC, G, WPE, MAP: MXX_SKINNY24_SHAPES of csrc/matmul_skinny24.hip
SHAPES = [(8, 1, 5, 12), (8, 2, 5, 12), (8, 4, 5, 12), (8, 8, 5, 12), (8, 8, 4, 12),
          (8, 1, 5, 16), (8, 2, 5, 16), (8, 4, 5, 16),
          (4, 1, 8, 12), (4, 2, 8, 12), (4, 4, 8, 12), (4, 1, 8, 16), (4, 2, 8, 16), (4, 4, 8, 16)]


def _seed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(bytes([(tag * 31 + i * 11 + 5) & 0xFF for i in range(32)]))


def _uniform(gpu, p, rows, cols, tag, level=None):
    if level is None:
        return gpu.GpuDCRTPolyMatrix.sample_distribution(p, rows, cols, gpu.DistType.FinRingDist().as_ffi(), 0.0, _seed(gpu, tag))
    m = gpu.GpuDCRTPolyMatrix(p, rows, cols, level, True)
    assert gpu._ffi.lib().gpu_matrix_sample_distribution(m.raw, gpu.DistType.FinRingDist().as_ffi(), 0.0, _seed(gpu, tag)) == 0
    return m


def _pair(gpu, hip_env, p, rows, cols, tag, level=None):
    """(packed, words): the same uniform sample in both layouts"""
    packed = _uniform(gpu, p, rows, cols, tag, level)
    hip_env.set("MXX_HIP_PACK24", "0")
    words = _uniform(gpu, p, rows, cols, tag, level)
    hip_env.unset("MXX_HIP_PACK24")
    assert packed.layout == "packed24" and words.layout == "words"
    return packed, words


def _label_map(label):
    return label.split("MAP=")[1].split(",")[0]


def _check_every_shape(gpu, oracle, hip_env, p, a_w, b_p, b_w, level=None):
    """a_w * b_p under every shape and under 0 against a_w * b_w by the register-tile kernel; two columns against the oracle"""
    n = p.ring_dimension()
    cols = b_p.ncol
    hip_env.set("MXX_HIP_SKINNY24", "0")
    want_m = a_w * b_w
    assert "skinny24" not in p.ctx().last_kernel()
    want = want_m.to_rns()
    moduli = p.moduli() if level is None else p.moduli()[: level + 1]
    a_h = a_w.to_rns()
    for col in (0, cols - 1):
        assert np.array_equal(want[:, col:col + 1], oracle.matmul(a_h, b_w.slice_columns(col, col + 1).to_rns(), moduli)), col
    got = a_w * b_p
    assert "skinny24" not in p.ctx().last_kernel() and "packed24 B" in p.ctx().last_kernel()
    assert got == want_m and np.array_equal(got.to_rns(), want)
    for tc, g, wpe, mp in SHAPES:
        hip_env.set("MXX_HIP_SKINNY24", f"force:{tc},{g},{wpe},{mp}")
        got = a_w * b_p
        label = p.ctx().last_kernel()
        assert "skinny24" in label and "packed24 B" in label and f"TC={tc},G={g},WPE={wpe}," in label, label
        if mp == 16 and n % 256:
            assert _label_map(label) == "12 (16 asked: partial wave)", label
        else:
            assert _label_map(label) == str(mp), label
        assert got == want_m, label
        assert np.array_equal(got.to_rns(), want), label
        assert b_p.layout == "packed24"
    hip_env.unset("MXX_HIP_SKINNY24")
    assert np.array_equal(b_p.to_rns(), b_w.to_rns())  # last: reading it back unpacks it


# every ring, column count, inner dimension and limb count of the issue, each at least once; cols 8 and 16 end on the last
# bytes of B's allocation (last column, last k, last limb of the last tile), n = 256 with one wave and one workgroup
CASES = [(256, 3, 5, 9), (1024, 3, 3, 17), (4096, 3, 2, 16), (64, 3, 5, 15), (16, 3, 30, 8), (256, 1, 1, 8),
         (1024, 15, 30, 9), (4096, 1, 5, 15), (16, 15, 2, 17), (64, 1, 3, 16), (256, 15, 2, 15), (1024, 1, 1, 16)]


@pytest.mark.parametrize("n,limbs,inner,cols", CASES)
def test_every_shape_matches_words_product(gpu, oracle, hip_env, n, limbs, inner, cols):
    p = make_params(gpu, oracle, n, limbs, 24, 12)
    _, a_w = _pair(gpu, hip_env, p, 1, inner, 60 + inner)
    b_p, b_w = _pair(gpu, hip_env, p, inner, cols, 70 + cols)
    _check_every_shape(gpu, oracle, hip_env, p, a_w, b_p, b_w)


def test_lazy_window_plus_one_term(gpu, oracle, hip_env):
    """2^16 products of 24-bit residues fill a 64-bit accumulator: with 2^16 + 1 terms the reduction inside the loop runs."""
    p = make_params(gpu, oracle, 16, 1, 24, 12)
    inner = (1 << 16) + 1
    _, a_w = _pair(gpu, hip_env, p, 1, inner, 80)
    b_p, b_w = _pair(gpu, hip_env, p, inner, 8, 81)
    _check_every_shape(gpu, oracle, hip_env, p, a_w, b_p, b_w)


def test_output_below_the_context_level(gpu, oracle, hip_env):
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    _, a_w = _pair(gpu, hip_env, p, 1, 3, 82, level=1)
    b_p, b_w = _pair(gpu, hip_env, p, 3, 9, 83, level=1)
    _check_every_shape(gpu, oracle, hip_env, p, a_w, b_p, b_w, level=1)


def test_packed_a_is_unpacked_and_b_stays_packed(gpu, oracle, hip_env):
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    a_p, a_w = _pair(gpu, hip_env, p, 1, 5, 84)
    b_p, b_w = _pair(gpu, hip_env, p, 5, 9, 85)
    hip_env.set("MXX_HIP_SKINNY24", "0")
    want = a_w * b_w
    hip_env.set("MXX_HIP_SKINNY24", "force")
    got = a_p * b_p
    assert "skinny24" in p.ctx().last_kernel() and "packed24 B" in p.ctx().last_kernel()
    assert a_p.layout == "words" and b_p.layout == "packed24"
    assert got == want and np.array_equal(got.to_rns(), want.to_rns())


def test_ineligible_products_keep_their_kernel(gpu, oracle, hip_env):
    """7 columns, two rows, B in words: the dispatch is the parent's and the results are equal."""
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    for rows, inner, cols, packed_b in ((1, 5, 7, True), (2, 5, 9, True), (1, 5, 9, False)):
        _, a_w = _pair(gpu, hip_env, p, rows, inner, 86 + rows)
        b_p, b_w = _pair(gpu, hip_env, p, inner, cols, 88 + cols)
        b = b_p if packed_b else b_w
        hip_env.set("MXX_HIP_SKINNY24", "0")
        want = a_w * b_w
        ref = a_w * b
        label0 = p.ctx().last_kernel()
        hip_env.set("MXX_HIP_SKINNY24", "force")
        got = a_w * b
        assert p.ctx().last_kernel() == label0 and "skinny24" not in label0
        assert got == want and ref == want and np.array_equal(got.to_rns(), want.to_rns())
        assert b.layout == ("packed24" if packed_b else "words")


def test_a_shape_that_is_not_instantiated_is_refused(gpu, oracle, hip_env):
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    _, a_w = _pair(gpu, hip_env, p, 1, 2, 90)
    b_p, _ = _pair(gpu, hip_env, p, 2, 8, 91)
    for bad in ("force:8,3,5,12", "force:nonsense"):
        hip_env.set("MXX_HIP_SKINNY24", bad)
        with pytest.raises(gpu.GpuPolyError, match="not instantiated"):
            a_w * b_p
