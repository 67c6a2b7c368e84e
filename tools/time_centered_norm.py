"""The centred infinity norm of every entry: the device entry (`gpupoly_matrix_centered_max_abs`, through
`centered_max_abs(axis="entries")`) against the host form the callers run (`_centered_max_abs_host`: coeffs(), then
min(v, Q - v) and a max over python ints).

Shapes: 1 x 64 at the reference's parameter-search ring (n = 2^16, 53 limbs of 28 bits) holding uniform residues (every
coefficient through the Garner path) and Gaussian errors (sigma 3.2: the first fast path), and the M3A preimage
(n = 2^14, 10 limbs of 24 bits, base 2^12, d = 1, 50 target columns: 22 x 50; the second fast path) as the sampler
returns it (EVAL: the call inverse-transforms a scratch copy first) and in COEFF form.  One further call per case runs
under the library's launch trace and prints what each launch took.  The host
form runs on HOST_COLS columns (default 4) and its figure is scaled to the whole matrix.  Wall time from the host, device
synchronised before and after.  Prints one line per case and a JSON summary."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402
from mxx_amd.trapdoor import compute_preimage_norm  # noqa: E402

REPS = int(os.environ.get("REPS", "10"))
HOST_COLS = int(os.environ.get("HOST_COLS", "4"))


def timed(fn, reps):
    fn()  # warm
    mx.gpu_device_sync()
    times = []
    for _ in range(reps):
        mx.gpu_device_sync()
        t0 = time.perf_counter()
        fn()
        mx.gpu_device_sync()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2]


def case(name, m):
    part = m.slice_columns(0, HOST_COLS)
    dev = m.centered_max_abs(axis="entries")
    assert [row[:HOST_COLS] for row in dev] == part._centered_max_abs_host(axis="entries"), name
    device_ms = timed(lambda: m.centered_max_abs(axis="entries"), REPS)
    host_ms = timed(lambda: part._centered_max_abs_host(axis="entries"), 1) * m.ncol / HOST_COLS
    worst = max(max(r) for r in dev)
    _ffi.trace_begin()
    m.centered_max_abs(axis="entries")
    launches = [{"kernel": r["kernel"][:60], "ms": round(r["ms"], 4), "GB/s": round(r["bytes"] / r["ms"] / 1e6, 0) if r["bytes"] and r["ms"] else None}
                for r in _ffi.trace_end()]
    print(f"{name:28s} {m.nrow} x {m.ncol}: device {device_ms:10.3f} ms   host {host_ms:10.1f} ms (scaled from "
          f"{HOST_COLS} columns)   max |x| 2^{math.log2(worst) if worst else 0:.1f}")
    for r in launches:
        print(f"{'':28s}   {r['kernel']:60s} {r['ms']:8.4f} ms  {r['GB/s'] or '':>8} GB/s")
    return {"rows": m.nrow, "cols": m.ncol, "device_ms": round(device_ms, 3), "host_ms": round(host_ms, 1),
            "log2_max": round(math.log2(worst), 2) if worst else None, "launches": launches}


summary = {}
n, limbs, bits = 1 << 16, 53, 28
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 1)
us = mx.GpuDCRTPolyUniformSampler()
summary["csv_2^16_53x28_uniform"] = case("2^16 53x28 uniform", us.sample_uniform(p, 1, 64, mx.DistType.FinRingDist()))
summary["csv_2^16_53x28_gauss"] = case("2^16 53x28 gauss 3.2", us.sample_uniform(p, 1, 64, mx.DistType.GaussDist(3.2)))
del p, us

n, depth, bits, base = 1 << 14, 10, 24, 12
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, depth, bits), base)
sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
td, A = sampler.trapdoor(p, 1)
target = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, 50, mx.DistType.FinRingDist())
x = sampler.preimage(p, td, A, target)
summary["m3a_preimage"] = case("M3A preimage (EVAL)", x)
summary["m3a_preimage_coeff"] = case("M3A preimage (COEFF)", x.ensure_coeff())
bound = compute_preimage_norm(math.sqrt(n), p.modulus_digits(), float(1 << base))
summary["m3a_preimage"]["log2_preimage_norm"] = round(math.log2(bound), 2)
print(json.dumps({"reps": REPS, "host_cols": HOST_COLS, "cases": summary}))
