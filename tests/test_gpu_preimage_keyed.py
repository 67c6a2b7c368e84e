"""GPU parity: preimage requests that do NOT all share a trapdoor through ONE C-ABI call (`gpupoly_trapdoor_preimage_keyed`,
`GpuDCRTPolyTrapdoorSampler.preimage_many_keys`).

Every request must get the matrix it would get alone with its own key - bit for bit, for the same seeds - whatever the
spread of the requests over the keys; the first request of every key is checked against the CPU restatement
(oracle.preimage).  The number of launches must not depend on the number of keys.  A refused call must launch nothing and
leave every output's contents and format tag as they were.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

SIGMA = 4.578


def seed_bytes(tag):
    return bytes((tag * 31 + 5 * i + 11) & 0xFF for i in range(32))


def make_key(gpu, oracle, p, n, base, d, master):
    """(trapdoor, A, (r, e, a)) generated from `master` as oracle.trapdoor_gen generates it"""
    from mxx_amd.sampler import seed_source

    r, e, a = oracle.trapdoor_gen(p.moduli(), n, base, SIGMA, d, master)
    with seed_source([oracle._seed_from(master, i).tobytes() for i in range(3)]):
        td, A = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA).trapdoor(p, d)
    assert np.array_equal(A.to_rns(), a)
    return td, A, (r, e, a)


def eval_targets(gpu, oracle, p, d, cols, tag):
    moduli, n = p.moduli(), p.ring_dimension()
    t_np = [oracle.matrix_ntt(oracle.random_matrix(tag + j, d, c, moduli, n), moduli) for j, c in enumerate(cols)]
    return t_np, [gpu.GpuDCRTPolyMatrix.from_rns(p, t, True) for t in t_np]


def master_seeds(gpu, oracle, masters):
    """the (p2, p1, z) triple oracle.preimage derives from each request's master seed"""
    return [tuple(gpu.GpuRngSeed.from_bytes(oracle._seed_from(m, i).tobytes()) for i in (3, 4, 5)) for m in masters]


def explicit_seeds(gpu, count, tag):
    return [tuple(gpu.GpuRngSeed.from_bytes(seed_bytes(tag + 3 * j + i)) for i in range(3)) for j in range(count)]


def cache_of(sampler, p, td, d):
    from mxx_amd.trapdoor import preimage_smoothing_parameter

    s = preimage_smoothing_parameter(sampler.base, sampler.sigma, d, p.ring_dimension(), p.modulus_digits())
    return td.p1_covariance_cache(sampler.c, s, sampler.sigma)


def raw_call(gpu, sampler, p, keys, key_of, targets, outs, seeds, caches=None, nkeys=None):
    """the entry itself (no wrapper, no fallback): (status, message, launches)"""
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    if caches is None:
        caches = [cache_of(sampler, p, td, A.row_size()) for td, A in keys]
    flat = (_ffi.GpuRngSeed * max(1, 3 * len(seeds)))(*[x for t in seeds for x in t])
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    rc = lib.gpupoly_trapdoor_preimage_keyed(M._raw_array([td.re for td, _ in keys]), M._raw_array(caches), M._raw_array([A for _, A in keys]),
                                             len(keys) if nkeys is None else nkeys, p.base_bits(), (C.c_uint32 * max(1, len(key_of)))(*key_of),
                                             M._raw_array(targets), len(targets), flat, M._raw_array(outs))
    launched = lib.gpupoly_launch_count() - c0
    return rc, (_ffi.last_error_string() if rc else ""), launched


def run_keyed(gpu, sampler, p, keys, key_of, targets, seeds):
    """outputs of one accepted call, and its launch count"""
    k, d = p.modulus_digits(), keys[0][1].row_size()
    outs = [gpu.GpuDCRTPolyMatrix(p, (k + 2) * d, t.col_size(), t.level, True) for t in targets]  # tagged EVAL by the call
    rc, msg, launched = raw_call(gpu, sampler, p, keys, key_of, targets, outs, seeds)
    assert rc == 0, msg
    return outs, launched


# (key, columns) per request, in the order of the call: interleaved, not sorted by key
def interleave(col_lists):
    reqs, at = [], [0] * len(col_lists)
    while any(a < len(c) for a, c in zip(at, col_lists)):
        for k in reversed(range(len(col_lists))) if len(reqs) % 2 else range(len(col_lists)):
            if at[k] < len(col_lists[k]):
                reqs.append((k, col_lists[k][at[k]]))
                at[k] += 1
    return reqs


@pytest.mark.parametrize("n,depth,bits,base,d,requests", [
    (128, 2, 24, 12, 1, interleave([[3, 1], [2], [1, 4, 2]])),   # one wave chunk per column; u32 words
    (256, 3, 51, 17, 2, interleave([[3, 1], [5], [1, 2]])),      # u64 words; padding to a multiple of d at key boundaries
    (128, 2, 24, 12, 1, [(j % 2, 1) for j in range(67)]),        # a group boundary inside a key's run (34 + 33 requests)
    (16384, 2, 24, 12, 1, [(0, 1), (1, 1), (0, 2)]),             # several elements per lane; a cache per wave chunk
], ids=["n128_u32_3keys", "n256_u64_d2_odd", "n128_67_requests_2keys", "n16384_2keys"])
def test_every_request_equals_its_key_alone_and_the_oracle(gpu, oracle, n, depth, bits, base, d, requests):
    p = make_params(gpu, oracle, n, depth, bits, base)
    moduli = p.moduli()
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    key_of = [k for k, _ in requests]
    assert key_of != sorted(key_of)
    nkeys = max(key_of) + 1
    made = [make_key(gpu, oracle, p, n, base, d, seed_bytes(20 + k)) for k in range(nkeys)]
    keys = [(td, A) for td, A, _ in made]
    targets_np, targets = eval_targets(gpu, oracle, p, d, [c for _, c in requests], 7000)
    masters = [seed_bytes(90 + j) for j in range(len(requests))]
    seeds = master_seeds(gpu, oracle, masters)
    got, _ = run_keyed(gpu, sampler, p, keys, key_of, targets, seeds)
    kd = p.modulus_digits()
    for j, (k, c) in enumerate(requests):
        td, A = keys[k]
        x = got[j]
        assert x.size() == ((kd + 2) * d, c)
        assert x == sampler.preimage_many_abi(p, td, A, [targets[j]], _seeds=[seeds[j]])[0], f"request {j}: differs from the one-key entry"
        assert x == sampler.preimage(p, td, A, targets[j], _seeds=seeds[j]), f"request {j}: differs from the preimage sampled alone"
        assert A * x == targets[j]
    for k in range(nkeys):  # the first request of every key against the CPU restatement
        j = key_of.index(k)
        r, e, a = made[k][2]
        want = oracle.preimage(moduli, n, base, SIGMA, r, e, a, targets_np[j], masters[j])
        assert np.array_equal(got[j].to_rns(), want), f"key {k}"
    # the wrapper draws the seeds request by request in the order given and returns the same matrices
    from mxx_amd.sampler import seed_source

    with seed_source([oracle._seed_from(m, i).tobytes() for m in masters for i in (3, 4, 5)]):
        wrapped = sampler.preimage_many_keys(p, keys, key_of, targets)
    assert all(x == y for x, y in zip(wrapped, got))


def test_launches_and_results_do_not_depend_on_the_spread_over_keys(gpu, oracle):
    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    td, A, _ = make_key(gpu, oracle, p, n, base, d, seed_bytes(30))
    cols = [3, 1, 4, 2, 5, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 7100)
    seeds = explicit_seeds(gpu, len(cols), 1200)
    want = sampler.preimage_many_abi(p, td, A, targets, _seeds=seeds)  # the one-key entry; also warms the covariance cache
    launches = []
    for key_of in ([0] * 6, [0, 1, 0, 1, 1, 0], [0, 1, 2, 2, 1, 0]):
        nkeys = max(key_of) + 1
        got, launched = run_keyed(gpu, sampler, p, [(td, A)] * nkeys, key_of, targets, seeds)
        assert all(x == y for x, y in zip(got, want)), f"{nkeys} keys: differs from the one-key entry"
        launches.append(launched)
    print(f"launches for 6 requests over 1, 2, 3 keys: {launches}")
    assert launches[0] > 0 and launches[0] == launches[1] == launches[2]


def test_trivial_cases(gpu, oracle):
    from mxx_amd import _ffi

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    keys = [make_key(gpu, oracle, p, n, base, d, seed_bytes(40 + k))[:2] for k in range(3)]
    kd = p.modulus_digits()
    # key 1 has no requests; request 1 has no columns
    _, (t0, t2) = eval_targets(gpu, oracle, p, d, [2, 3], 7200)
    targets = [t0, gpu.GpuDCRTPolyMatrix(p, d, 0, depth - 1, True), t2]
    key_of = [2, 0, 0]
    seeds = explicit_seeds(gpu, 3, 1300)
    got, _ = run_keyed(gpu, sampler, p, keys, key_of, targets, seeds)
    assert got[1].size() == ((kd + 2) * d, 0)
    for j in (0, 2):
        td, A = keys[key_of[j]]
        assert got[j] == sampler.preimage(p, td, A, targets[j], _seeds=seeds[j]) and A * got[j] == targets[j]
    # one key: the existing entry's matrices
    one, _ = run_keyed(gpu, sampler, p, keys[:1], [0, 0], [t0, t2], [seeds[0], seeds[2]])
    many = sampler.preimage_many_abi(p, keys[0][0], keys[0][1], [t0, t2], _seeds=[seeds[0], seeds[2]])
    assert one[0] == many[0] and one[1] == many[1]
    # no request: nothing launched, with keys or without
    assert sampler.preimage_many_keys(p, keys, [], []) == []
    rc, msg, launched = raw_call(gpu, sampler, p, keys, [], [], [], [])
    assert rc == 0 and launched == 0, msg
    lib = _ffi.lib()
    c0 = lib.gpupoly_launch_count()
    assert lib.gpupoly_trapdoor_preimage_keyed(None, None, None, 0, p.base_bits(), None, None, 0, None, None) == 0
    assert lib.gpupoly_launch_count() == c0


# ---------------------------------------------------------------------------------------------------
# refusals: a clean error, no launch, every output as it was (contents AND format tag)
# ---------------------------------------------------------------------------------------------------
def sentinel_outputs(gpu, oracle, p, rows, cols, tag):
    """outputs pre-filled with known COEFF-tagged contents: to_rns() reads them back only while the library's tag is
    still COEFF, so a refused call that touched a tag or a word shows up"""
    moduli, n = p.moduli(), p.ring_dimension()
    data = [oracle.random_matrix(tag + j, rows, c, moduli, n) for j, c in enumerate(cols)]
    return data, [gpu.GpuDCRTPolyMatrix.from_rns(p, x, False) for x in data]


def assert_refused(gpu, sampler, p, keys, key_of, targets, outs, data, seeds, match, caches=None):
    rc, msg, launched = raw_call(gpu, sampler, p, keys, key_of, targets, outs, seeds, caches=caches)
    assert rc != 0 and match in msg and "gpupoly_trapdoor_preimage_keyed" in msg, msg
    assert launched == 0
    for o, want in zip(outs, data):
        assert not o.is_ntt and np.array_equal(o.to_rns(), want)
    return msg


def test_bad_arguments_are_refused_without_writing(gpu, oracle, monkeypatch):
    from mxx_amd import _ffi
    from mxx_amd.trapdoor import worker_params

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    keys = [make_key(gpu, oracle, p, n, base, d, seed_bytes(50 + k))[:2] for k in range(2)]
    rows = (p.modulus_digits() + 2) * d
    cols, key_of = [2, 1], [1, 0]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 7300)
    seeds = explicit_seeds(gpu, len(cols), 1400)
    data, outs = sentinel_outputs(gpu, oracle, p, rows, cols, 7400)
    caches = [cache_of(sampler, p, td, d) for td, _ in keys]
    # key_of out of range
    assert_refused(gpu, sampler, p, keys, [1, 2], targets, outs, data, seeds, "key_of")
    # keys of different d
    small = make_key(gpu, oracle, p, n, base, 1, seed_bytes(58))[:2]
    assert_refused(gpu, sampler, p, [keys[0], small], key_of, targets, outs, data, seeds, " d ")
    # a cache of another context (a worker context of the same device)
    pw = worker_params(p, 1)
    foreign = cache_of(sampler, pw, keys[1][0].to_params(pw), d)
    assert_refused(gpu, sampler, p, keys, key_of, targets, outs, data, seeds, "context mismatch", caches=[caches[0], foreign])
    # a COEFF-form target
    coeff = targets[1].clone().into_coeff_domain()
    assert_refused(gpu, sampler, p, keys, key_of, [targets[0], coeff], outs, data, seeds, "EVAL")
    # an output that is a row view of some key's A
    a_before = keys[0][1].to_rns()
    rc, msg, launched = raw_call(gpu, sampler, p, keys, key_of, targets, [outs[0], keys[0][1].row_view(0, 1)], seeds)
    assert rc != 0 and "alias" in msg and launched == 0, msg
    assert keys[0][1].is_ntt and np.array_equal(keys[0][1].to_rns(), a_before) and np.array_equal(outs[0].to_rns(), data[0])
    # two outputs sharing storage
    assert_refused(gpu, sampler, p, keys, key_of, [targets[0], targets[0]], [outs[0], outs[0]], data[:1], seeds, "alias")
    # MXX_HIP_RNG_COMPAT=reference
    monkeypatch.setenv("MXX_HIP_RNG_COMPAT", "reference")
    _ffi.reload_env()
    try:
        assert_refused(gpu, sampler, p, keys, key_of, targets, outs, data, seeds, "unsupported")
    finally:
        monkeypatch.delenv("MXX_HIP_RNG_COMPAT")
        _ffi.reload_env()


def test_caches_of_different_widths_are_unsupported_and_the_wrapper_falls_back(gpu, oracle):
    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    keys = [make_key(gpu, oracle, p, n, base, d, seed_bytes(60 + k))[:2] for k in range(2)]
    rows = (p.modulus_digits() + 2) * d
    cols, key_of = [2, 1, 3], [1, 0, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 7500)
    seeds = explicit_seeds(gpu, len(cols), 1500)
    data, outs = sentinel_outputs(gpu, oracle, p, rows, cols, 7600)
    # key 1's trapdoor hands out a cache with another s (the same one to every caller, so the paths stay comparable)
    td1 = keys[1][0]
    plain = td1.p1_covariance_cache
    td1.p1_covariance_cache = lambda c, s, dgg: plain(c, 1.25 * s, dgg)
    caches = [cache_of(sampler, p, td, d) for td, _ in keys]
    assert_refused(gpu, sampler, p, keys, key_of, targets, outs, data, seeds, "unsupported", caches=caches)
    calls = type(sampler).keyed_calls
    got = sampler.preimage_many_keys(p, keys, key_of, targets, _seeds=seeds)
    assert type(sampler).keyed_calls == calls + 1
    for j, k in enumerate(key_of):
        td, A = keys[k]
        assert got[j] == sampler.preimage_many_abi(p, td, A, [targets[j]], _seeds=[seeds[j]])[0]
        assert A * got[j] == targets[j]


def test_batched_sharded_takes_the_entry_only_when_asked(gpu, oracle, monkeypatch):
    from mxx_amd.sampler import seed_source

    n, depth, bits, base, d = 256, 3, 51, 17, 2
    p = make_params(gpu, oracle, n, depth, bits, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
    keys = [make_key(gpu, oracle, p, n, base, d, seed_bytes(70 + k))[:2] for k in range(3)]
    key_of, cols = [0, 1, 2, 1, 0], [2, 1, 3, 2, 1]
    _, targets = eval_targets(gpu, oracle, p, d, cols, 7700)
    requests = [(100 + j, p, keys[k][0], keys[k][1], t) for j, (k, t) in enumerate(zip(key_of, targets))]
    draws = [seed_bytes(200 + i) for i in range(3 * len(requests))]
    monkeypatch.delenv("MXX_PREIMAGE_MIXED", raising=False)
    calls = type(sampler).keyed_calls
    with seed_source(draws):
        default = sampler.preimage_batched_sharded(requests)
    assert type(sampler).keyed_calls == calls, "the default path must not reach gpupoly_trapdoor_preimage_keyed"
    monkeypatch.setenv("MXX_PREIMAGE_MIXED", "abi")
    with seed_source(draws):
        mixed = sampler.preimage_batched_sharded(requests)
    assert type(sampler).keyed_calls == calls + 1
    assert [i for i, _ in mixed] == [i for i, _ in default] == [100 + j for j in range(len(requests))]
    for j, ((_, x), (_, y)) in enumerate(zip(mixed, default)):
        assert x == y, f"request {j}"
        assert keys[key_of[j]][1] * x == targets[j]
