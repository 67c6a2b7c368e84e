"""Sixteen preimage requests against one trapdoor on the GGH15 chain's ring (M4: n = 256, 12 limbs of 51 bits, base 2^17,
d = 2, four columns each): the one C-ABI call (`preimage_many_abi` -> gpupoly_trapdoor_preimage_many) against the Python
sequence of the same launches (`preimage_many`) and sixteen single requests (`preimage`).  Wall time per call from the host,
device synchronised before and after (the calls are asynchronous; the chain consumes the result), and the launches each
call issues (gpupoly_launch_count).  Prints one line per path and a JSON summary."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

N, LIMBS, BITS, BASE, D, REQUESTS, COLS = 256, 12, 51, 17, 2, 16, 4
REPS, WARMUP = int(os.environ.get("REPS", "30")), 5

p = mx.GpuDCRTPolyParams(N, mx.gen_crt_basis(N, LIMBS, BITS), BASE)
sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
td, A = sampler.trapdoor(p, D)
us = mx.GpuDCRTPolyUniformSampler()
targets = [us.sample_uniform(p, D, COLS, mx.DistType.FinRingDist()) for _ in range(REQUESTS)]
lib = _ffi.lib()

paths = {
    "preimage_many_abi": lambda: sampler.preimage_many_abi(p, td, A, targets),
    "preimage_many": lambda: sampler.preimage_many(p, td, A, targets),
    "preimage x16": lambda: [sampler.preimage(p, td, A, t) for t in targets],
}
for name, fn in paths.items():  # correctness once, and warm caches (covariance cache, public-matrix blocks)
    assert all(A * x == t for x, t in zip(fn(), targets)), name
mx.gpu_device_sync()

summary = {}
for name, fn in paths.items():
    for _ in range(WARMUP):
        fn()
    mx.gpu_device_sync()
    times, launches = [], []
    for _ in range(REPS):
        mx.gpu_device_sync()
        c0 = lib.gpupoly_launch_count()
        t0 = time.perf_counter()
        fn()
        mx.gpu_device_sync()
        times.append((time.perf_counter() - t0) * 1e3)
        launches.append(lib.gpupoly_launch_count() - c0)
    times.sort()
    summary[name] = {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "launches": launches[0]}
    print(f"{name:18s} median {summary[name]['median_ms']:.3f} ms  min {summary[name]['min_ms']:.3f} ms  "
          f"{launches[0]} launches per call ({REQUESTS} requests x {COLS} columns)")
print(json.dumps({"shape": {"n": N, "limbs": LIMBS, "bits": BITS, "base_bits": BASE, "d": D, "requests": REQUESTS, "cols": COLS},
                  "reps": REPS, "paths": summary}))
