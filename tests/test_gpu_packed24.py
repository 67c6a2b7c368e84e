"""GPU: the 3-byte residue layout (GPU_MATRIX_LAYOUT_PACKED24, csrc/layout.hip).

A uniform sample of a 32-bit context whose moduli are all below 2^24 is stored with 3 bytes per residue; the register-tile
product reads it as it is and every other operation unpacks it once.  Results must not depend on the layout: every check
here compares a packed operand with the same operand sampled under MXX_HIP_PACK24=0.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu


def _seed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(bytes([(tag * 29 + i * 13 + 7) & 0xFF for i in range(32)]))


def _uniform(gpu, p, rows, cols, tag):
    return gpu.GpuDCRTPolyMatrix.sample_distribution(p, rows, cols, gpu.DistType.FinRingDist().as_ffi(), 0.0, _seed(gpu, tag))


def _pair(gpu, hip_env, p, rows, cols, tag):
    """(packed, words): the same uniform sample in both layouts"""
    packed = _uniform(gpu, p, rows, cols, tag)
    hip_env.set("MXX_HIP_PACK24", "0")
    words = _uniform(gpu, p, rows, cols, tag)
    hip_env.unset("MXX_HIP_PACK24")
    assert packed.layout == "packed24" and words.layout == "words"
    return packed, words


@pytest.mark.parametrize("n", [1024, 16384])  # separate pack kernel / packed store of the 2^14 transform
def test_uniform_samples_are_packed_where_eligible(gpu, oracle, hip_env, n):
    p = make_params(gpu, oracle, n, 3, 24, 12)
    m = _uniform(gpu, p, 2, 3, 1)
    assert m.layout == "packed24"
    hip_env.set("MXX_HIP_PACK24", "off")
    assert _uniform(gpu, p, 2, 3, 1).layout == "words"
    hip_env.unset("MXX_HIP_PACK24")
    # other distributions, a modulus of 2^24 or more, 64-bit words: words
    assert gpu.GpuDCRTPolyMatrix.sample_distribution(p, 2, 3, gpu.DistType.BitDist().as_ffi(), 0.0, _seed(gpu, 2)).layout == "words"
    assert _uniform(gpu, make_params(gpu, oracle, n, 2, 28, 12), 2, 3, 3).layout == "words"
    assert _uniform(gpu, make_params(gpu, oracle, 1024, 2, 51, 12), 2, 3, 4).layout == "words"


def test_views_device_ptr_and_conversion(gpu, oracle, hip_env):
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    packed, words = _pair(gpu, hip_env, p, 4, 3, 5)
    want = words.to_rns()
    v = packed.row_view(1, 3)  # a view shares words: the parent is unpacked first
    assert packed.layout == "words" and v.layout == "words"
    assert np.array_equal(v.to_rns(), want[1:3])
    assert np.array_equal(packed.to_rns(), want)
    # a matrix with a live row view is not packed again by a new sample into it
    st = gpu._ffi.lib().gpu_matrix_sample_distribution(packed.raw, gpu.DistType.FinRingDist().as_ffi(), 0.0, _seed(gpu, 6))
    assert st == 0 and packed.layout == "words"
    del v
    q, _ = _pair(gpu, hip_env, p, 2, 2, 7)
    ptr, size = C.c_void_p(), C.c_size_t()
    assert gpu._ffi.lib().gpupoly_matrix_device_ptr(q.raw, C.byref(ptr), C.byref(size)) == 0
    assert q.layout == "words" and size.value == 2 * 2 * 3 * 1024 * 4


@pytest.mark.parametrize("n", [1024, 16384])
def test_every_operation_family_matches_words(gpu, oracle, hip_env, n):
    p = make_params(gpu, oracle, n, 3, 24, 12)
    for rows, k, cols in ((1, 5, 9), (3, 4, 4), (2, 3, 8)):
        a_p, a_w = _pair(gpu, hip_env, p, rows, k, 10 + rows)
        b_p, b_w = _pair(gpu, hip_env, p, k, cols, 20 + rows)
        want = (a_w * b_w).to_rns()
        assert np.array_equal((a_p * b_w).to_rns(), want)           # A packed only
        assert np.array_equal((a_w * b_p).to_rns(), want)           # B packed only
        assert a_p.layout == "packed24" and b_p.layout == "packed24"  # the register tile read them as they are
        assert np.array_equal((a_p * b_p).to_rns(), want)           # both: A is unpacked, B read packed
        assert a_p.layout == "words" and b_p.layout == "packed24"
    x_p, x_w = _pair(gpu, hip_env, p, 2, 3, 30)
    y_p, y_w = _pair(gpu, hip_env, p, 2, 3, 31)
    assert np.array_equal((x_p + y_p).to_rns(), (x_w + y_w).to_rns())  # element-wise: unpacks
    assert np.array_equal(x_p.to_coeff_rns(), x_w.to_coeff_rns())
    assert np.array_equal(x_p.decompose().to_rns(), x_w.decompose().to_rns())
    z_p, z_w = _pair(gpu, hip_env, p, 2, 3, 32)
    assert z_p == z_w and z_p.layout == "words"
    c_p, c_w = _pair(gpu, hip_env, p, 3, 2, 33)
    assert np.array_equal(c_p.slice_columns(1, 2).to_rns(), c_w.slice_columns(1, 2).to_rns())


def test_m2a_shape_packed_against_words_and_oracle(gpu, oracle, hip_env):
    """The bench shape (n = 2^14, L = 15, (1 x 30)(30 x 120)): the packed product equals the words product, and output
    columns equal the CPU restatement."""
    p = make_params(gpu, oracle, 16384, 15, 24, 12)
    a_p, a_w = _pair(gpu, hip_env, p, 1, 30, 40)
    b_p, b_w = _pair(gpu, hip_env, p, 30, 120, 41)
    c_p = a_p * b_p
    assert "packed24 B" in p.ctx().last_kernel()
    c_w = a_w * b_w
    assert "packed24" not in p.ctx().last_kernel()
    assert c_p == c_w
    a_h = a_w.to_rns()
    for col in (0, 119):
        want = oracle.matmul(a_h, b_w.slice_columns(col, col + 1).to_rns(), p.moduli())
        assert np.array_equal(c_p.slice_columns(col, col + 1).to_rns(), want), col


def test_threads_share_one_packed_matrix(gpu, oracle, hip_env):
    """Four host threads on one context use the same packed operands: some products read them packed, the first
    words consumer unpacks them under the context's layout lock; every result equals the words reference."""
    p = make_params(gpu, oracle, 1024, 3, 24, 12)
    a_p, a_w = _pair(gpu, hip_env, p, 1, 6, 50)
    b_p, b_w = _pair(gpu, hip_env, p, 6, 8, 51)
    want_prod, want_sum = (a_w * b_w).to_rns(), (b_w + b_w).to_rns()
    errors = []

    def work(t):
        try:
            for i in range(6):
                if (i + t) % 3 == 2:
                    assert np.array_equal((b_p + b_p).to_rns(), want_sum)
                else:
                    assert np.array_equal((a_p * b_p).to_rns(), want_prod)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert b_p.layout == "words"
