"""GPU parity: the batched preimage at trapdoor dimensions d = 3 and d = 4 (m = 2d = 6 and 8 perturbation rows: the eight-row
instantiations of `p1_sample_lanes_kernel`, plain, SEG and KEYED).

m = 6 leaves the eight mean registers partly filled, m = 8 fills them; n = 128 is the smallest ring the segmented samplers
take; column counts that are no multiple of d pad every request's perturbation; both word widths; both superstep forms of
the sampler (one element per lane by default at these sizes, several with MXX_HIP_SAMPLER_PER_LANE).  The bar is the one of
the d <= 2 tests: bit for bit the matrix the request gets alone, and the CPU restatement (`oracle/`) for some of them.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params
from test_gpu_preimage_abi import SIGMA, assert_refused, eval_targets, explicit_seeds, seed_bytes, sentinel_outputs, trapdoor_and_oracle
from test_gpu_preimage_batch import gseed
from test_gpu_preimage_batch import seed_bytes as batch_seed_bytes
from test_gpu_preimage_keyed import assert_refused as assert_keyed_refused

pytestmark = pytest.mark.gpu

PER_LANE = pytest.mark.parametrize("per_lane", ["", "3"], ids=["one_per_lane", "three_per_lane"])


def _per_lane(hip_env, per_lane):
    if per_lane:  # several elements per lane: the sampler's KARNEY_SERVICES superstep form
        hip_env.set("MXX_HIP_SAMPLER_PER_LANE", per_lane)
    else:
        hip_env.unset("MXX_HIP_SAMPLER_PER_LANE")


# ---------------------------------------------------------------------------------------------------
# 1. the plain p1 entry against the CPU restatement, from either kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,bits", [(3, 32, 24), (4, 16, 51), (4, 64, 24)])
@PER_LANE
def test_p1_plain_bit_exact_from_either_kernel(gpu, oracle, hip_env, per_lane, d, n, bits):
    _per_lane(hip_env, per_lane)
    depth, base = 2, 12 if bits == 24 else 17
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    rng = np.random.default_rng(d * 100 + n)

    def small(rows, cols, bound):
        v = rng.integers(-bound, bound + 1, size=(rows, cols, n))
        return np.stack([np.mod(v, q).astype(np.uint64) for q in moduli], axis=-2)

    M = gpu.GpuDCRTPolyMatrix
    a, b, dm = small(d, d, 60), small(d, d, 25), small(d, d, 60)
    sigma, s_par, dgg = 12.0, 900.0, 4.578
    cols = 3
    tp2 = small(2 * d, cols, 5000)
    ga, gb, gd = (M.from_rns(p, x, False) for x in (a, b, dm))
    cache = M.create_p1_covariance_cache(ga, gb, gd, sigma, s_par, dgg)
    s = gseed(gpu, 9)
    out = M.sample_p1_full_cached(cache, M.from_rns(p, tp2, False), s)
    assert out.is_ntt and out.size() == (2 * d, cols)
    sv, up = oracle.p1_covariance(a, b, dm, moduli, sigma, s_par, dgg)
    c_scale = -(sigma * sigma) / (s_par * s_par - sigma * sigma)
    want = oracle.sample_p1(tp2, moduli, sv, up, c_scale, s)
    assert np.array_equal(out.to_coeff_rns(), want)
    hip_env.set("MXX_HIP_P1", "simple")  # one thread per element
    assert M.sample_p1_full_cached(cache, M.from_rns(p, tp2, False), s) == out.ensure_eval()


# ---------------------------------------------------------------------------------------------------
# 2. p1 over segments
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,depth,bits,base,d,seg_cols", [(128, 2, 24, 12, 3, [2, 1, 4]), (256, 3, 51, 17, 4, [4, 1, 3])])
@PER_LANE
def test_p1_segments_equal_the_plain_sampler_per_segment(gpu, oracle, hip_env, per_lane, n, depth, bits, base, d, seg_cols):
    from mxx_amd.sampler import seed_source
    from mxx_amd.trapdoor import GpuDCRTTrapdoor, p1_covariance_parameters

    _per_lane(hip_env, per_lane)
    p = make_params(gpu, oracle, n, depth, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
    with seed_source([batch_seed_bytes(1), batch_seed_bytes(2)]):
        td = GpuDCRTTrapdoor.new(p, d, SIGMA)
    c, s, dgg = p1_covariance_parameters(p, d, SIGMA)
    cache = td.p1_covariance_cache(c, s, dgg)
    tp2 = M.sample_distribution(p, 2 * d, sum(seg_cols), gpu.DistType.GaussDist(3.0e5).as_ffi(), 3.0e5, gseed(gpu, 9))
    seeds = [gseed(gpu, 40 + j) for j in range(len(seg_cols))]
    got = M.sample_p1_full_cached_segments(cache, tp2.clone(), seeds, seg_cols)
    assert got.is_ntt and got.size() == (2 * d, sum(seg_cols))
    parts, tparts = got.split_columns(seg_cols), tp2.split_columns(seg_cols)
    for j, (part, t) in enumerate(zip(parts, tparts)):
        assert part == M.sample_p1_full_cached(cache, t.clone(), seeds[j]), f"segment {j} differs from the plain p1 sampler"
    # one segment against the CPU restatement too
    inv = lambda m: oracle.matrix_ntt(m, moduli, inverse=True)
    r, e = td.r.to_rns(), td.e.to_rns()
    rt, et = np.swapaxes(r, 0, 1), np.swapaxes(e, 0, 1)
    sv, up = oracle.p1_covariance(inv(oracle.matmul(r, rt, moduli)), inv(oracle.matmul(r, et, moduli)), inv(oracle.matmul(e, et, moduli)),
                                  moduli, c, s, dgg)
    want = oracle.matrix_ntt(oracle.sample_p1(inv(tparts[1].to_rns()), moduli, sv, up, -(c * c) / (s * s - c * c), batch_seed_bytes(41)), moduli)
    assert np.array_equal(parts[1].to_rns(), want)


# ---------------------------------------------------------------------------------------------------
# 3. gpupoly_trapdoor_preimage_many
# ---------------------------------------------------------------------------------------------------
def _cache(sampler, p, td, d):
    from mxx_amd.trapdoor import preimage_smoothing_parameter

    s = preimage_smoothing_parameter(sampler.base, sampler.sigma, d, p.ring_dimension(), p.modulus_digits())
    return td.p1_covariance_cache(sampler.c, s, sampler.sigma)


def _outputs(gpu, p, d, targets):
    k = p.modulus_digits()
    return [gpu.GpuDCRTPolyMatrix(p, (k + 2) * d, t.col_size(), t.level, True) for t in targets]


def _many(gpu, sampler, p, td, A, targets, seeds):
    """one accepted gpupoly_trapdoor_preimage_many call: (outputs, launches)"""
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    cache = _cache(sampler, p, td, A.row_size())
    outs = _outputs(gpu, p, A.row_size(), targets)
    flat = (_ffi.GpuRngSeed * (3 * len(seeds)))(*[x for t in seeds for x in t])
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    rc = lib.gpupoly_trapdoor_preimage_many(td.re.raw, cache.raw, A.raw, p.base_bits(), M._raw_array(targets), len(targets), flat,
                                            M._raw_array(outs))
    launched = lib.gpupoly_launch_count() - c0
    assert rc == 0, _ffi.last_error_string()
    return outs, launched


def _keyed(gpu, sampler, p, keys, key_of, targets, seeds):
    """one accepted gpupoly_trapdoor_preimage_keyed call: (outputs, launches)"""
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    d = keys[0][1].row_size()
    caches = [_cache(sampler, p, td, d) for td, _ in keys]
    outs = _outputs(gpu, p, d, targets)
    flat = (_ffi.GpuRngSeed * (3 * len(seeds)))(*[x for t in seeds for x in t])
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    rc = lib.gpupoly_trapdoor_preimage_keyed(M._raw_array([td.re for td, _ in keys]), M._raw_array(caches), M._raw_array([a for _, a in keys]),
                                             len(keys), p.base_bits(), (C.c_uint32 * len(key_of))(*key_of), M._raw_array(targets),
                                             len(targets), flat, M._raw_array(outs))
    launched = lib.gpupoly_launch_count() - c0
    assert rc == 0, _ffi.last_error_string()
    return outs, launched


def _master_seeds(gpu, oracle, masters):
    """the (p2, p1, z) triple oracle.preimage derives from each request's master seed"""
    return [tuple(gpu.GpuRngSeed.from_bytes(oracle._seed_from(m, i).tobytes()) for i in (3, 4, 5)) for m in masters]


@pytest.mark.parametrize("n,depth,bits,base,d,cols", [(128, 2, 24, 12, 3, [1, 2, 4, 3]), (256, 3, 51, 17, 4, [3, 1, 4, 2, 5])])
def test_one_call_equals_the_requests_alone_and_the_oracle(gpu, oracle, n, depth, bits, base, d, cols):
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    sampler, td, A, (r, e, a) = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(1))
    targets_np, targets = eval_targets(gpu, oracle, p, d, cols, 8000)
    masters = [seed_bytes(60 + j) for j in range(len(cols))]
    seeds = _master_seeds(gpu, oracle, masters)
    got, launched = _many(gpu, sampler, p, td, A, targets, seeds)
    k = p.modulus_digits()
    for j, (x, t) in enumerate(zip(got, targets)):
        assert x.size() == ((k + 2) * d, cols[j]) and x.is_ntt
        assert x == sampler.preimage(p, td, A, t, _seeds=seeds[j]), f"request {j}: differs from the preimage sampled alone"
        assert A * x == t
    want = oracle.preimage(moduli, n, base, SIGMA, r, e, a, targets_np[1], masters[1])
    assert np.array_equal(got[1].to_rns(), want)
    # the launches of a group do not depend on the number of requests in it
    two, launched_two = _many(gpu, sampler, p, td, A, targets[:2], seeds[:2])
    five = targets + targets[:1] if len(targets) == 4 else targets
    _, launched_five = _many(gpu, sampler, p, td, A, five, (seeds + seeds[:1])[:5])
    assert two[0] == got[0] and two[1] == got[1]
    assert launched_two > 0 and launched_two == launched_five, f"2 requests: {launched_two} launches, 5 requests: {launched_five}"


# ---------------------------------------------------------------------------------------------------
# 4. gpupoly_trapdoor_preimage_keyed
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,depth,bits,base,d", [(256, 3, 51, 17, 3), (128, 2, 24, 12, 3)], ids=["u64", "u32_eight_row_tile"])
@PER_LANE
def test_keyed_call_equals_every_request_with_its_key_alone(gpu, oracle, hip_env, per_lane, n, depth, bits, base, d):
    from test_gpu_preimage_keyed import make_key

    _per_lane(hip_env, per_lane)
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    keys = [make_key(gpu, oracle, p, n, base, d, seed_bytes(20 + k))[:2] for k in range(3)]
    key_of, cols = [0, 1, 2, 1, 0], [2, 1, 3, 2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 8100)
    seeds = explicit_seeds(gpu, len(cols), 1400)
    got, launched = _keyed(gpu, sampler, p, keys, key_of, targets, seeds)
    for j, k in enumerate(key_of):
        td, A = keys[k]
        assert got[j] == sampler.preimage_many_abi(p, td, A, [targets[j]], _seeds=[seeds[j]])[0], f"request {j}: differs from the one-key entry"
        assert A * got[j] == targets[j]
    _, launched_one_key = _keyed(gpu, sampler, p, keys[:1], [0] * len(cols), targets, seeds)
    assert launched > 0 and launched == launched_one_key, f"3 keys: {launched} launches, 1 key: {launched_one_key}"


# ---------------------------------------------------------------------------------------------------
# 5. what stays refused
# ---------------------------------------------------------------------------------------------------
def test_dimension_five_is_refused_and_the_wrapper_falls_back(gpu, oracle):
    from mxx_amd._ffi import GpuPolyError

    n, depth, bits, base, d = 256, 2, 24, 12, 5
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(7))
    k = p.modulus_digits()
    cols = [2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 8200)
    seeds = explicit_seeds(gpu, len(cols), 1500)
    data, outs = sentinel_outputs(gpu, oracle, p, (k + 2) * d, cols, 8300)
    msg = assert_refused(gpu, sampler, p, td, A, targets, outs, data, seeds, "unsupported")
    assert "dimension above 4" in msg
    msg = assert_keyed_refused(gpu, sampler, p, [(td, A), (td, A)], [1, 0], targets, outs, data, seeds, "unsupported")
    assert "dimension above 4" in msg
    M = gpu.GpuDCRTPolyMatrix
    tp2 = M.sample_distribution(p, 2 * d, 3, gpu.DistType.GaussDist(3.0e5).as_ffi(), 3.0e5, gseed(gpu, 9))
    with pytest.raises(GpuPolyError, match="unsupported: trapdoor dimension above 4"):
        M.sample_p1_full_cached_segments(_cache(sampler, p, td, d), tp2, [gseed(gpu, 1), gseed(gpu, 2)], [2, 1])
    got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    for x, t, sd in zip(got, targets, seeds):
        assert x == sampler.preimage(p, td, A, t, _seeds=sd) and A * x == t


def test_the_simple_p1_kernel_is_refused_in_its_own_words(gpu, oracle, monkeypatch):
    from mxx_amd import _ffi
    from mxx_amd._ffi import GpuPolyError

    n, depth, bits, base, d = 128, 2, 24, 12, 3
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(8))
    k = p.modulus_digits()
    cols = [2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 8400)
    seeds = explicit_seeds(gpu, len(cols), 1600)
    data, outs = sentinel_outputs(gpu, oracle, p, (k + 2) * d, cols, 8500)
    M = gpu.GpuDCRTPolyMatrix
    tp2 = M.sample_distribution(p, 2 * d, 3, gpu.DistType.GaussDist(3.0e5).as_ffi(), 3.0e5, gseed(gpu, 9))
    cache = _cache(sampler, p, td, d)
    monkeypatch.setenv("MXX_HIP_P1", "simple")
    _ffi.reload_env()
    try:
        for msg in (assert_refused(gpu, sampler, p, td, A, targets, outs, data, seeds, "unsupported"),
                    assert_keyed_refused(gpu, sampler, p, [(td, A), (td, A)], [1, 0], targets, outs, data, seeds, "unsupported")):
            assert "MXX_HIP_P1=simple" in msg and "dimension" not in msg
        with pytest.raises(GpuPolyError, match="unsupported under MXX_HIP_P1=simple"):
            M.sample_p1_full_cached_segments(cache, tp2, [gseed(gpu, 1), gseed(gpu, 2)], [2, 1])
        got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)  # the wrapper: one by one
    finally:
        monkeypatch.delenv("MXX_HIP_P1")
        _ffi.reload_env()
    for x, t, sd in zip(got, targets, seeds):
        assert x == sampler.preimage(p, td, A, t, _seeds=sd) and A * x == t


# ---------------------------------------------------------------------------------------------------
# 6. the mirror
# ---------------------------------------------------------------------------------------------------
def test_the_python_segments_path_batches_dimension_three(gpu, oracle):
    from mxx_amd import _ffi

    n, depth, bits, base, d = 128, 2, 24, 12, 3
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(9))
    assert sampler._segments_supported(p, td)
    cols = [2, 1, 3]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 8600)
    seeds = explicit_seeds(gpu, len(cols), 1700)
    lib = _ffi.lib()
    sampler.preimage_many(p, td, A, targets, _seeds=seeds)  # warm: covariance cache, public-matrix blocks
    c0 = lib.gpupoly_launch_count()
    many = sampler.preimage_many(p, td, A, targets, _seeds=seeds)
    c1 = lib.gpupoly_launch_count()
    alone = [sampler.preimage(p, td, A, t, _seeds=sd) for t, sd in zip(targets, seeds)]
    c2 = lib.gpupoly_launch_count()
    for j, (x, y, t) in enumerate(zip(many, alone, targets)):
        assert x == y, f"request {j}: batched preimage differs from the one sampled alone"
        assert A * x == t
    print(f"launches for {len(cols)} requests: preimage_many {c1 - c0}, one by one {c2 - c1}")
    assert 0 < (c1 - c0) < (c2 - c1), f"preimage_many took {c1 - c0} launches, the loop {c2 - c1}"
