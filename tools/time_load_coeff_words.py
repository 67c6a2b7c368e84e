"""The exact coefficient load on a 1 x 64 matrix (`gpupoly_matrix_load_coeff_words`) at the two shapes of
§5d's table: n = 2^16 with 53 limbs of 28 bits, and M3A (n = 2^14, 10 limbs of 24 bits).

  (a) the device entry from a ready word array (pageable numpy memory), COEFF and EVAL: whole-call wall time, and from
      the launch trace the host-to-device copy, the load kernel and the transform apart; next to it a bare hipMemcpy of
      the same bytes from the same array, the floor an input in host memory cannot beat;
  (b) `GpuDCRTPolyMatrix.from_coeffs` from Python ints (ints -> bytes -> words on the host, then (a));
  (c) the path before the device load, `GpuDCRTPoly._from_biguints_host` + `from_poly_vec`, on HOST_COLS entries (default
      1) scaled to 64.

Wall time from the host, device synchronised before and after; median of REPS for (a), one run each for (b) and (c), which
take seconds.  Prints one line per figure and a JSON summary."""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

COLS, REPS = 64, int(os.environ.get("REPS", "5"))
HOST_COLS = int(os.environ.get("HOST_COLS", "1"))
SHAPES = {"csv_2^16_53x28": (1 << 16, 53, 28), "m3a_2^14_10x24": (1 << 14, 10, 24)}
HBM_GBS = 8000.0  # MI355X peak HBM3E bandwidth


def wall(fn, reps, warm=True):
    if warm:
        fn()
    times = []
    for _ in range(reps):
        mx.gpu_device_sync()
        t0 = time.perf_counter()
        fn()
        mx.gpu_device_sync()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2]


def bare_copy_ms(host: np.ndarray, reps: int) -> float:
    """hipMemcpy of the array into a device block, nothing else"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), host.nbytes) == 0

    def copy():
        assert hip.hipMemcpy(dev, host.ctypes.data, host.nbytes, 1) == 0

    ms = wall(copy, reps)
    hip.hipFree(dev)
    return ms


def traced(fn):
    _ffi.trace_begin()
    fn()
    mx.gpu_device_sync()
    out = {"copy": 0.0, "kernel": 0.0, "transform": 0.0}
    for rec in _ffi.trace_end():
        key = "copy" if rec["kernel"].startswith("copy") else "kernel" if "load_coeff_words" in rec["kernel"] else "transform"
        out[key] += rec["ms"]
    return out


summary = {}
for name, (n, limbs, bits) in SHAPES.items():
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 1)
    M = mx.GpuDCRTPolyMatrix
    m = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, COLS, mx.DistType.FinRingDist())
    m.intt_all_in_place()
    want = m.to_rns()
    wpc = -(-p.modulus().bit_length() // 64)
    words = np.empty((1, COLS, n, wpc), dtype=np.uint64)
    _ffi.check_status(_ffi.lib().gpupoly_matrix_store_coeff_words(m.raw, words.ctypes.data_as(C.POINTER(C.c_uint64)), wpc), "store")
    out = M(p, 1, COLS, limbs - 1, False)
    out.load_coeff_words(words, eval_format=False)
    assert np.array_equal(out.to_rns(), want), name
    word_bytes = 8 if bits > 31 else 4
    kernel_bytes = COLS * n * (8 * wpc + word_bytes * limbs)
    row = {
        "(a) device call, COEFF": wall(lambda: out.load_coeff_words(words, eval_format=False), REPS),
        "(a) device call, EVAL": wall(lambda: out.load_coeff_words(words, eval_format=True), REPS),
        "bare hipMemcpy of the words": bare_copy_ms(words, REPS),
    }
    tr_c = traced(lambda: out.load_coeff_words(words, eval_format=False))
    tr_e = traced(lambda: out.load_coeff_words(words, eval_format=True))
    row["(a) traced copy"] = tr_c["copy"]
    row["(a) traced load kernel"] = tr_c["kernel"]
    row["(a) traced transform (EVAL)"] = tr_e["transform"]
    ints = m.coeffs()
    row["(b) from_coeffs from ints, EVAL"] = wall(lambda: M.from_coeffs(p, ints, True), 1, warm=False)
    got = M.from_coeffs(p, [ints[0][:HOST_COLS]], True)

    def parent_path():
        polys = [mx.GpuDCRTPoly._from_biguints_host(p, c) for c in ints[0][:HOST_COLS]]
        return M.from_poly_vec(p, [polys])

    assert np.array_equal(got.to_rns(), parent_path().to_rns()), name
    row["(c) host loop + from_poly_vec, EVAL"] = wall(parent_path, 1, warm=False) * COLS / HOST_COLS
    for k, v in row.items():
        scaled = " (scaled from %d entr%s)" % (HOST_COLS, "y" if HOST_COLS == 1 else "ies") if k.startswith("(c)") else ""
        print(f"{name:16s} {k:38s} {v:12.3f} ms for 1 x {COLS}{scaled}")
    gbs = kernel_bytes / (row["(a) traced load kernel"] * 1e-3) / 1e9
    print(f"{name:16s} load kernel: {kernel_bytes / 1e6:.1f} MB in and out, {gbs:.0f} GB/s = {100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM peak; "
          f"whole COEFF call / bare copy = {row['(a) device call, COEFF'] / row['bare hipMemcpy of the words']:.2f}")
    summary[name] = {"n": n, "limbs": limbs, "bits": bits, "log2_Q": round(math.log2(p.modulus()), 1), "words_per_coeff": wpc,
                     "input_MB": round(words.nbytes / 1e6, 1), "kernel_bytes_MB": round(kernel_bytes / 1e6, 1),
                     "kernel_GBs": round(gbs, 1), "ms_1x64": {k: round(v, 3) for k, v in row.items()}}
print(json.dumps({"cols": COLS, "host_cols": HOST_COLS, "reps": REPS, "shapes": summary}))
