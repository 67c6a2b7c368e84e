"""A wave of preimage requests that do not all share a trapdoor (tools/README.md), four ways in one process:
  keyed    one `gpupoly_trapdoor_preimage_keyed` call (`preimage_many_keys`): one sequence of launches for all keys
  workers  `preimage_batched_sharded` as it is by default: key groups dealt to worker contexts, replicas, copies back
  loop     one `gpupoly_trapdoor_preimage_many` call per key on one stream (`preimage_many_abi`)
  floor    the same requests against ONE key in one `gpupoly_trapdoor_preimage_many` call
on two shapes: the M4 ring of tools/time_mixed_keys.py (n = 256, 12 x 51 bits, base 2^17, d = 2; 8 keys x 2 requests of 4
columns) and a 32-bit one (n = 2^14, 10 x 24 bits, base 2^12, d = 1; 4 keys x 4 single-column requests).  The outputs of
keyed, workers and loop are compared first (`gpu_matrix_equal`, same seeds).  Then the legs alternate; every leg is
bracketed by device events on the requests' stream (the workers leg ends with its copies back onto that stream) and by the
host clock until the device is idle; median of REPS (6) after a warm-up, launches per call from gpupoly_launch_count, and
the launch trace of the keyed and the workers leg summed per kernel."""
import collections
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402
from mxx_amd.sampler import seed_source  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "6")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, keys, requests per key, columns
    ("m4 (u64)", 256, 12, 51, 17, 2, 8, 2, 4),
    ("n16384 (u32)", 16384, 10, 24, 12, 1, 4, 4, 1),
]
os.environ.pop("MXX_PREIMAGE_MIXED", None)  # the workers leg is the default path
lib = _ffi.lib()


def run_shape(name, n, limbs, bits, base, d, nkeys, per_key, cols):
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    us = mx.GpuDCRTPolyUniformSampler()
    keys = [sampler.trapdoor(p, d) for _ in range(nkeys)]
    key_of = [k for k in range(nkeys) for _ in range(per_key)]
    targets = [us.sample_uniform(p, d, cols, mx.DistType.FinRingDist()) for _ in key_of]
    draws = [os.urandom(32) for _ in range(3 * len(targets))]
    seeds = [tuple(mx.GpuRngSeed.from_bytes(draws[3 * j + i]) for i in range(3)) for j in range(len(targets))]
    requests = [(j, p, keys[k][0], keys[k][1], t) for j, (k, t) in enumerate(zip(key_of, targets))]

    def keyed():
        return sampler.preimage_many_keys(p, keys, key_of, targets, _seeds=seeds)

    def workers():
        with seed_source(draws):
            return [x for _, x in sampler.preimage_batched_sharded(requests)]

    def loop():
        out = []
        for k, (td, a) in enumerate(keys):
            mine = [j for j, kk in enumerate(key_of) if kk == k]
            out += sampler.preimage_many_abi(p, td, a, [targets[j] for j in mine], _seeds=[seeds[j] for j in mine])
        return out

    def floor():
        return sampler.preimage_many_abi(p, keys[0][0], keys[0][1], targets, _seeds=seeds)

    legs = [("keyed", keyed), ("workers", workers), ("loop", loop), ("floor", floor)]
    print(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}; {nkeys} keys x {per_key} requests of {cols} column(s)")
    calls = type(sampler).keyed_calls
    got = {nm: fn() for nm, fn in legs}  # also warms covariance caches, replicas and worker contexts
    assert type(sampler).keyed_calls == calls + 1, "only the keyed leg reaches gpupoly_trapdoor_preimage_keyed"
    for nm in ("workers", "loop"):
        assert all(x == y for x, y in zip(got["keyed"], got[nm])), f"keyed differs from {nm}"
    assert all(keys[k][1] * x == t for k, x, t in zip(key_of, got["keyed"], targets))
    assert all(keys[0][1] * x == t for x, t in zip(got["floor"], targets))
    print("outputs: keyed == workers == loop for the same seeds (gpu_matrix_equal); A_key x == target")
    del got
    ctx = p.ctx()
    for _ in range(WARMUP):
        for _, fn in legs:
            fn()
    dev, wall, launches = collections.defaultdict(list), collections.defaultdict(list), {}
    for _ in range(REPS):
        for nm, fn in legs:  # the legs alternate
            mx.gpu_device_sync()
            c0 = lib.gpupoly_launch_count()
            t0 = time.perf_counter()
            ctx.timer_mark(0)
            out = fn()
            ctx.timer_mark(1)
            mx.gpu_device_sync()
            wall[nm].append((time.perf_counter() - t0) * 1e3)
            dev[nm].append(ctx.timer_elapsed(0, 1))
            launches[nm] = lib.gpupoly_launch_count() - c0
            del out
    for nm, _ in legs:
        print(f"{nm:8s} device events median {statistics.median(dev[nm]):.3f} ms (min {min(dev[nm]):.3f}), "
              f"host until idle median {statistics.median(wall[nm]):.3f} ms, {launches[nm]} launches per call")
    for nm, fn in legs[:2]:
        mx.gpu_device_sync()
        _ffi.trace_begin()
        fn()
        mx.gpu_device_sync()
        per = collections.OrderedDict()
        for rec in _ffi.trace_end():
            e = per.setdefault(rec["kernel"].split("<")[0].strip("( "), [0, 0.0])
            e[0] += 1
            e[1] += rec["ms"]
        print(f"-- launch trace, {nm} leg ({sum(v[0] for v in per.values())} traced launches and copies, "
              f"{sum(v[1] for v in per.values()):.3f} ms summed over streams):")
        for k, (cnt, ms) in per.items():
            print(f"   {cnt:4d} x {k:48s} {ms:8.3f} ms")
    return {nm: statistics.median(dev[nm]) for nm, _ in legs}


for shape in SHAPES:
    med = run_shape(*shape)
    print(f"keyed / floor = {med['keyed'] / med['floor']:.2f}, workers / keyed = {med['workers'] / med['keyed']:.2f}, "
          f"loop / keyed = {med['loop'] / med['keyed']:.2f}")
