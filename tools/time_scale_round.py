"""modulus_switch and the centred decode on a 1 x 64 matrix: the device path (`gpupoly_matrix_scale_round`, then the
forward transform the result is returned in) against the host path the mirror keeps (`_modulus_switch_host`,
`_decode_centered_host`: coeffs -> big-integer rescale -> from_coeffs / from_biguints), at the shape of the reference's
parameter search (n = 2^16, 53 limbs of 28 bits; bench/security_bits_100_diamond_io_simulation_parameters.csv) and at
M3A (n = 2^14, 10 limbs of 24 bits).

The host paths take seconds per entry, so they run on HOST_COLS entries (default 1) and the 64-entry figure is that
time scaled up; "host (old coeffs)" is the host path with the residue-by-residue CRT coeffs() had before the device
word store.  Wall time from the host, device synchronised before and after.  Prints one line per path and a JSON
summary."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402

COLS, REPS = 64, int(os.environ.get("REPS", "5"))
HOST_COLS = int(os.environ.get("HOST_COLS", "1"))
SHAPES = {"csv_2^16_53x28": (1 << 16, 53, 28), "m3a_2^14_10x24": (1 << 14, 10, 24)}
T = 1 << 20


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


def old_host_switch(m, t):
    from mxx_amd.poly import GpuDCRTPoly

    Q = m.params.modulus()
    rows = [[GpuDCRTPoly.from_coeffs(m.params, [(c * t // Q) % t for c in poly]) for poly in row] for row in m._coeffs_host()]
    return mx.GpuDCRTPolyMatrix.from_poly_vec(m.params, rows)


summary = {}
for name, (n, limbs, bits) in SHAPES.items():
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 1)
    m = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, COLS, mx.DistType.FinRingDist())
    part = m.slice(0, 1, 0, HOST_COLS)
    dev_sw = m.modulus_switch(T)
    assert np.array_equal(dev_sw.slice(0, 1, 0, HOST_COLS).to_rns(), part._modulus_switch_host(T).to_rns()), name
    row = {
        "device modulus_switch": timed(lambda: m.modulus_switch(T), REPS),
        "device decode_centered": timed(lambda: m.decode_centered(T), REPS),
        "device coeffs()": timed(lambda: m.coeffs(), 1),
        "host modulus_switch": timed(lambda: part._modulus_switch_host(T), 1) * COLS / HOST_COLS,
        "host decode_centered": timed(lambda: part._decode_centered_host(T), 1) * COLS / HOST_COLS,
        "host (old coeffs) modulus_switch": timed(lambda: old_host_switch(part, T), 1) * COLS / HOST_COLS,
        "host (old coeffs) coeffs()": timed(lambda: part._coeffs_host(), 1) * COLS / HOST_COLS,
    }
    for k, v in row.items():
        scaled = " (scaled from %d entr%s)" % (HOST_COLS, "y" if HOST_COLS == 1 else "ies") if k.startswith("host") else ""
        print(f"{name:16s} {k:34s} {v:12.1f} ms for 1 x {COLS}{scaled}")
    summary[name] = {"n": n, "limbs": limbs, "bits": bits, "log2_Q": round(math.log2(p.modulus()), 1),
                     "ms_1x64": {k: round(v, 2) for k, v in row.items()}}
print(json.dumps({"cols": COLS, "host_cols": HOST_COLS, "t": T, "reps": REPS, "shapes": summary}))
