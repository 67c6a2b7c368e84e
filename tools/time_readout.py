"""Bits and machine integers off the device: the mirror methods on `gpupoly_matrix_extract_bits` /
`gpupoly_matrix_store_coeff_ints` against the host forms they replace (`_extract_bits_with_threshold_host`,
`_const_coeff_u64_host`, coeffs() and a host pass), alternating in one process.

Shapes: the reference's parameter-search ring (n = 2^16, 53 limbs of 28 bits) with uniform coefficients -
`extract_bits_with_threshold` and `const_coeff_u64` of one polynomial, `extract_bits` of a 1 x 64 matrix - and the M3A
preimage (n = 2^14, 10 limbs of 24 bits, base 2^12, d = 1, 50 target columns: 22 x 50) read as int64 through
`coeffs_ints` against coeffs() and a centring pass, as the sampler returns it (EVAL: the call inverse-transforms a scratch
copy first) and in COEFF form; `const_coeffs_u64` of the 1 x 64 matrix against the per-entry `_const_coeff_u64_host` loop.
Median of REPS calls (default 11) of EACH side after a warm-up, wall time around the whole call, device synchronised before
and after; the host forms of the matrix cases run on HOST_COLS columns and are scaled to the whole matrix.  One
further device call per case runs under the library's launch trace and gives the kernels' own time.  Prints one line per
case and a JSON summary."""
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS = int(os.environ.get("REPS", "11"))
HOST_COLS = int(os.environ.get("HOST_COLS", "2"))


def once(fn):
    mx.gpu_device_sync()
    t0 = time.perf_counter()
    fn()
    mx.gpu_device_sync()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def case(name, device, host, host_scale=1.0):
    """device() and host() alternate, REPS timed calls each after one warm-up call each"""
    device()
    host()
    dev_ms, host_ms = [], []
    for i in range(REPS):
        dev_ms.append(once(device))
        host_ms.append(once(host))
    _ffi.trace_begin()
    device()
    launches = [{"kernel": r["kernel"][:48], "ms": round(r["ms"], 4)} for r in _ffi.trace_end()]
    kernel_ms = sum(r["ms"] for r in launches if "extract_bits_kernel" in r["kernel"] or "coeff_ints_kernel" in r["kernel"])
    d, h = median(dev_ms), median(host_ms) * host_scale
    scaled = f" (scaled x{host_scale:g})" if host_scale != 1.0 else ""
    print(f"{name:58s} device {d:9.3f} ms   of which the read-out kernel {kernel_ms:8.4f} ms   host form {h:10.1f} ms{scaled}   x{h / d:8.1f}")
    for r in launches:
        print(f"{'':58s}   {r['kernel']:48s} {r['ms']:8.4f} ms")
    return {"device_ms": round(d, 3), "kernel_ms": round(kernel_ms, 4), "host_ms": round(h, 1), "launches": launches}


summary = {}
rnd = random.Random(1)
n, limbs, bits = 1 << 16, 53, 28
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 1)
Q = p.modulus()
us = mx.GpuDCRTPolyUniformSampler()

poly = us.sample_poly(p, mx.DistType.FinRingDist())
assert poly.extract_bits_with_threshold() == poly._extract_bits_with_threshold_host()
summary["poly_extract_bits_with_threshold"] = case("2^16 53x28 uniform, poly: extract_bits_with_threshold",
                                                   poly.extract_bits_with_threshold, poly._extract_bits_with_threshold_host)

small = mx.GpuDCRTPoly.from_biguints(p, [rnd.getrandbits(64)] + [rnd.randrange(Q) for _ in range(n - 1)])
assert small.const_coeff_u64() == small._const_coeff_u64_host()
summary["poly_const_coeff_u64"] = case("2^16 53x28 uniform, poly: const_coeff_u64", small.const_coeff_u64, small._const_coeff_u64_host)

m = us.sample_uniform(p, 1, 64, mx.DistType.FinRingDist())
quarter = (Q // 2) >> 1
part = m.slice_columns(0, HOST_COLS)


def host_bits(mat):
    return [[[quarter <= c < 3 * quarter for c in poly_] for poly_ in row] for row in mat.coeffs()]


assert m.extract_bits(quarter, 3 * quarter)[:, :HOST_COLS].tolist() == host_bits(part)
summary["matrix_extract_bits"] = case("2^16 53x28 uniform, 1 x 64: extract_bits", lambda: m.extract_bits(quarter, 3 * quarter),
                                      lambda: host_bits(part), m.ncol / HOST_COLS)


def host_consts(mat):  # the per-entry loop of the callers; a uniform constant does not fit and raises after the CRT
    for c in range(mat.ncol):
        try:
            mat.entry(0, c)._const_coeff_u64_host()
        except OverflowError:
            pass


summary["matrix_const_coeffs_u64"] = case("2^16 53x28 uniform, 1 x 64: const_coeffs_u64", lambda: m.const_coeffs_u64(strict=False),
                                          lambda: host_consts(part), m.ncol / HOST_COLS)
del p, us, poly, small, m, part

n, depth, bits, base = 1 << 14, 10, 24, 12
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, depth, bits), base)
Q = p.modulus()
sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
td, A = sampler.trapdoor(p, 1)
target = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, 50, mx.DistType.FinRingDist())
x = sampler.preimage(p, td, A, target)


def host_ints(mat):
    return np.array([[[c if c <= Q // 2 else c - Q for c in poly_] for poly_ in row] for row in mat.coeffs()], dtype=np.int64)


for name, mat in (("EVAL", x), ("COEFF", x.ensure_coeff())):
    part = mat.slice_columns(0, HOST_COLS)
    assert np.array_equal(mat.coeffs_ints(np.int64)[:, :HOST_COLS], host_ints(part))
    summary[f"m3a_preimage_coeffs_ints_{name.lower()}"] = case(f"M3A preimage 22 x 50 ({name}): coeffs_ints(int64)",
                                                                lambda mat=mat: mat.coeffs_ints(np.int64),
                                                                lambda part=part: host_ints(part), mat.ncol / HOST_COLS)
print(json.dumps({"reps": REPS, "host_cols": HOST_COLS, "cases": summary}))
