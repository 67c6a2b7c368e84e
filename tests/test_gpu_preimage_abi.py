"""GPU parity: several preimage requests against one trapdoor through ONE C-ABI call (`gpupoly_trapdoor_preimage_many`,
`GpuDCRTPolyTrapdoorSampler.preimage_many_abi`).

Every request must get the matrix it would get alone - bit for bit, for the same seeds - which is also what the Python
sequence `preimage_many` gives, and the first requests are checked against the CPU restatement (oracle.preimage).  A
refused call must launch nothing and leave every output's contents and format tag as they were.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

SIGMA = 4.578


def seed_bytes(tag):
    return bytes((tag * 31 + 5 * i + 11) & 0xFF for i in range(32))


def trapdoor_and_oracle(gpu, oracle, p, n, base, d, master):
    from mxx_amd.sampler import seed_source

    r, e, a = oracle.trapdoor_gen(p.moduli(), n, base, SIGMA, d, master)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    with seed_source([oracle._seed_from(master, i).tobytes() for i in range(3)]):
        td, A = sampler.trapdoor(p, d)
    assert np.array_equal(A.to_rns(), a)
    return sampler, td, A, (r, e, a)


def eval_targets(gpu, oracle, p, d, cols, tag):
    moduli, n = p.moduli(), p.ring_dimension()
    t_np = [oracle.matrix_ntt(oracle.random_matrix(tag + j, d, c, moduli, n), moduli) for j, c in enumerate(cols)]
    return t_np, [gpu.GpuDCRTPolyMatrix.from_rns(p, t, True) for t in t_np]


def explicit_seeds(gpu, count, tag):
    return [tuple(gpu.GpuRngSeed.from_bytes(seed_bytes(tag + 3 * j + i)) for i in range(3)) for j in range(count)]


@pytest.mark.parametrize("n,depth,bits,base,d,cols", [
    (256, 12, 51, 17, 2, [4] * 8),         # the M4 request, eight at a time
    (256, 3, 51, 17, 2, [3, 1, 4, 2, 5]),  # odd column counts: every request's perturbation is padded to a multiple of d
    (1024, 3, 24, 12, 1, [1, 2, 3, 1]),    # u32 words, d = 1
    (128, 2, 24, 12, 1, [1] * 67),         # more requests than one group of 64
    (16384, 2, 24, 12, 1, [1, 2]),         # several elements per lane
])
def test_one_call_equals_preimage_many_alone_and_the_oracle(gpu, oracle, n, depth, bits, base, d, cols):
    from mxx_amd.sampler import seed_source

    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    sampler, td, A, (r, e, a) = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(1))
    targets_np, targets = eval_targets(gpu, oracle, p, d, cols, 5000)
    masters = [seed_bytes(60 + j) for j in range(len(cols))]
    draws = [oracle._seed_from(m, i).tobytes() for m in masters for i in (3, 4, 5)]  # request by request: p2, p1, z
    with seed_source(draws):
        got = sampler.preimage_many_abi(p, td, A, targets)
    with seed_source(draws):
        many = sampler.preimage_many(p, td, A, targets)
    with seed_source(draws):
        alone = [sampler.preimage(p, td, A, t) for t in targets]
    k = p.modulus_digits()
    assert len(got) == len(cols)
    for j, (x, xm, xa, t) in enumerate(zip(got, many, alone, targets)):
        assert x.size() == ((k + 2) * d, cols[j]) and x.is_ntt
        assert x == xm, f"request {j}: the C entry differs from preimage_many"
        assert x == xa, f"request {j}: the C entry differs from the preimage sampled alone"
        assert A * x == t
    for j in range(min(3, len(cols))):
        want = oracle.preimage(moduli, n, base, SIGMA, r, e, a, targets_np[j], masters[j])
        assert np.array_equal(got[j].to_rns(), want)


def test_zero_column_requests_and_trivial_counts(gpu, oracle):
    from mxx_amd import _ffi

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(2))
    k = p.modulus_digits()
    # a zero-column request among others
    _, (t0, t2) = eval_targets(gpu, oracle, p, d, [2, 3], 5100)
    targets = [t0, gpu.GpuDCRTPolyMatrix(p, d, 0, depth - 1, True), t2]
    seeds = explicit_seeds(gpu, 3, 700)
    got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    assert got[1].size() == ((k + 2) * d, 0) and got[1].is_ntt
    for j in (0, 2):
        assert got[j] == sampler.preimage(p, td, A, targets[j], _seeds=seeds[j]) and A * got[j] == targets[j]
    # one request
    one = sampler.preimage_many_abi(p, td, A, targets[2:], _seeds=seeds[2:])
    assert len(one) == 1 and one[0] == got[2]
    # none: nothing launched, by the wrapper or by the entry itself
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    assert sampler.preimage_many_abi(p, td, A, []) == []
    empty = (C.c_void_p * 1)()
    assert lib.gpupoly_trapdoor_preimage_many(td.re.raw, td.p1_covariance_cache(*cache_widths(sampler, p, d)).raw, A.raw,
                                              p.base_bits(), empty, 0, None, empty) == 0
    assert lib.gpupoly_launch_count() == c0


def cache_widths(sampler, p, d):
    from mxx_amd.trapdoor import preimage_smoothing_parameter

    s = preimage_smoothing_parameter(sampler.base, sampler.sigma, d, p.ring_dimension(), p.modulus_digits())
    return sampler.c, s, sampler.sigma


def test_one_call_issues_fewer_launches_than_preimage_many(gpu, oracle):
    from mxx_amd import _ffi

    n, depth, bits, base, d = 256, 12, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(3))
    _, targets = eval_targets(gpu, oracle, p, d, [3, 1, 5, 3, 1, 3, 5, 1], 5200)
    seeds = explicit_seeds(gpu, len(targets), 800)
    lib = _ffi.lib()
    sampler.preimage_many(p, td, A, targets, _seeds=seeds)  # warm: covariance cache, public-matrix blocks
    sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    c0 = lib.gpupoly_launch_count()
    many = sampler.preimage_many(p, td, A, targets, _seeds=seeds)
    c1 = lib.gpupoly_launch_count()
    got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    c2 = lib.gpupoly_launch_count()
    print(f"launches for {len(targets)} requests: preimage_many {c1 - c0}, gpupoly_trapdoor_preimage_many {c2 - c1}")
    assert all(x == y for x, y in zip(got, many))
    assert (c2 - c1) < (c1 - c0), f"the C entry took {c2 - c1} launches, preimage_many {c1 - c0}"


# ---------------------------------------------------------------------------------------------------
# refusals: a clean error, no launch, every output as it was (contents AND format tag)
# ---------------------------------------------------------------------------------------------------
def sentinel_outputs(gpu, oracle, p, rows, cols, tag):
    """outputs pre-filled with known COEFF-tagged contents: to_rns() reads them back only while the library's tag is
    still COEFF, so a refused call that touched a tag or a word shows up"""
    moduli, n = p.moduli(), p.ring_dimension()
    data = [oracle.random_matrix(tag + j, rows, c, moduli, n) for j, c in enumerate(cols)]
    return data, [gpu.GpuDCRTPolyMatrix.from_rns(p, x, False) for x in data]


def raw_call(gpu, sampler, p, td, A, targets, outs, seeds):
    from mxx_amd import _ffi

    d = A.row_size()
    cache = td.p1_covariance_cache(*cache_widths(sampler, p, d))
    M = gpu.GpuDCRTPolyMatrix
    flat = (_ffi.GpuRngSeed * (3 * len(seeds)))(*[x for t in seeds for x in t])
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    rc = lib.gpupoly_trapdoor_preimage_many(td.re.raw, cache.raw, A.raw, p.base_bits(), M._raw_array(targets), len(targets),
                                            flat, M._raw_array(outs))
    launched = lib.gpupoly_launch_count() - c0
    return rc, (_ffi.last_error_string() if rc else ""), launched


def assert_refused(gpu, sampler, p, td, A, targets, outs, data, seeds, match):
    rc, msg, launched = raw_call(gpu, sampler, p, td, A, targets, outs, seeds)
    assert rc != 0 and match in msg, msg
    assert launched == 0
    for o, want in zip(outs, data):
        assert not o.is_ntt and np.array_equal(o.to_rns(), want)
    return msg


def test_unsupported_ring_is_refused_and_the_wrapper_falls_back(gpu, oracle):
    n, depth, bits, base, d = 64, 2, 24, 12, 1  # below the segmented samplers' 128
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(4))
    k = p.modulus_digits()
    cols = [1, 2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 5300)
    seeds = explicit_seeds(gpu, len(cols), 900)
    data, outs = sentinel_outputs(gpu, oracle, p, (k + 2) * d, cols, 5400)
    assert_refused(gpu, sampler, p, td, A, targets, outs, data, seeds, "unsupported")
    got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
    for x, t, sd in zip(got, targets, seeds):
        assert x == sampler.preimage(p, td, A, t, _seeds=sd) and A * x == t


def test_reference_rng_keying_is_refused_and_the_wrapper_falls_back(gpu, oracle, monkeypatch):
    from mxx_amd import _ffi

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(5))
    k = p.modulus_digits()
    cols = [2, 3]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 5500)
    seeds = explicit_seeds(gpu, len(cols), 1000)
    data, outs = sentinel_outputs(gpu, oracle, p, (k + 2) * d, cols, 5600)
    monkeypatch.setenv("MXX_HIP_RNG_COMPAT", "reference")
    _ffi.reload_env()
    try:
        assert_refused(gpu, sampler, p, td, A, targets, outs, data, seeds, "unsupported")
        got = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)
        for x, t, sd in zip(got, targets, seeds):
            assert x == sampler.preimage(p, td, A, t, _seeds=sd) and A * x == t
    finally:
        monkeypatch.delenv("MXX_HIP_RNG_COMPAT")
        _ffi.reload_env()


def test_bad_arguments_are_refused_without_writing(gpu, oracle):
    from mxx_amd._ffi import GpuPolyError
    from mxx_amd.trapdoor import worker_params

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(6))
    k = p.modulus_digits()
    rows = (k + 2) * d
    cols = [2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 5700)
    seeds = explicit_seeds(gpu, len(cols), 1100)
    data, outs = sentinel_outputs(gpu, oracle, p, rows, cols, 5800)
    # a target in another context (a worker context of the same device)
    pw = worker_params(p, 1)
    assert_refused(gpu, sampler, p, td, A, [targets[0], targets[1].to_params(pw)], outs, data, seeds, "context mismatch")
    # a wrong output shape
    wdata, wrong = sentinel_outputs(gpu, oracle, p, rows, [2, 2], 5900)
    assert_refused(gpu, sampler, p, td, A, targets, wrong, wdata, seeds, "output 1")
    # an output whose storage holds a target: the target is a row view of the output
    host_np = oracle.matrix_ntt(oracle.random_matrix(6000, rows, 1, p.moduli(), n), p.moduli())
    host = gpu.GpuDCRTPolyMatrix.from_rns(p, host_np, True)
    view = host.row_view(0, d)
    rc, msg, launched = raw_call(gpu, sampler, p, td, A, [targets[0], view], [outs[0], host], seeds)
    assert rc != 0 and "aliases" in msg and launched == 0, msg
    assert np.array_equal(host.to_rns(), host_np) and np.array_equal(outs[0].to_rns(), data[0])
    # the same output twice
    assert_refused(gpu, sampler, p, td, A, [targets[0], targets[0]], [outs[0], outs[0]], data[:1], seeds, "aliases")
    # a COEFF-form target
    coeff = targets[1].clone().into_coeff_domain()
    assert_refused(gpu, sampler, p, td, A, [targets[0], coeff], outs, data, seeds, "EVAL")
    with pytest.raises(GpuPolyError, match="EVAL"):
        sampler.preimage_many_abi(p, td, A, [coeff])
