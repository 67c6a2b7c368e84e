"""The compact wire format for many matrices: the loop over gpu_matrix_store_compact_bytes / gpu_matrix_load_compact_bytes
(a) against ONE gpupoly_matrix_store_compact_bytes_many / _load_ call (b), alternated in one process.

Host clock around calls that end in the entries' own synchronise, pinned destination / source, every shape warmed up.
Shapes: the 16 outputs (76 x 4, n = 256, 12 limbs of 51 bits) of one gpupoly_trapdoor_preimage_many call, in COEFF and in
EVAL form (the inverse transforms are then part of both forms); 64 such; four M3A preimages (22 x 50, n = 2^14, 10 limbs
of 24 bits) as the large, copy-bound case.  Per shape: median and the 10th..90th percentile of ms per call, the ratio
(a) / (b), launches per call (gpupoly_launch_count) and synchronises per call (from the code: 2 per matrix in the loop's
store, 1 in its load; 2 and 1 per batched call), and for the small shape the preimage call's own time next to it.
Prints one line per measurement and a JSON summary.  REPS / REPS_LARGE set the repetitions (200 / 10)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS, REPS_LARGE, WARMUP = int(os.environ.get("REPS", "200")), int(os.environ.get("REPS_LARGE", "10")), 3
lib = _ffi.lib()


def check(st, what):
    _ffi.check_status(st, what)


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


class Batch:
    def __init__(self, mats):
        self.mats, self.n = mats, len(mats)
        self.raws = (C.c_void_p * self.n)(*[m.raw for m in mats])
        self.bits, self.bpcs = (C.c_uint16 * self.n)(), (C.c_uint16 * self.n)()
        self.offs, self.lens, self.total = (C.c_size_t * self.n)(), (C.c_size_t * self.n)(), C.c_size_t(0)
        self.ptrs = (C.c_void_p * self.n)()
        # the lengths first (a call without room reports them), then pinned slots of the longest payload
        st = lib.gpupoly_matrix_store_compact_bytes_many(self.raws, self.n, None, 0, self.bits, self.bpcs, self.offs, self.lens, C.byref(self.total))
        assert st == 0 or "payload buffer too small" in _ffi.last_error_string(), _ffi.last_error_string()
        self.slot = (max(self.lens) + 7) // 8 * 8 + 8
        self.cap = self.slot * self.n
        self.pinned = lib.gpu_pinned_alloc(self.cap)
        assert self.pinned, "gpu_pinned_alloc failed"

    def to_eval(self):
        for m in self.mats:
            m.is_ntt = False
            m.ntt_all_in_place()
        mx.gpu_device_sync()

    def store_loop(self):
        b, c, ln = C.c_uint16(0), C.c_uint16(0), C.c_size_t(0)
        for j, m in enumerate(self.mats):
            check(lib.gpu_matrix_store_compact_bytes(m.raw, C.c_void_p(self.pinned + j * self.slot), self.slot, C.byref(b), C.byref(c), C.byref(ln)),
                  "gpu_matrix_store_compact_bytes")
            self.bits[j], self.offs[j], self.lens[j] = b.value, j * self.slot, ln.value

    def store_many(self):
        check(lib.gpupoly_matrix_store_compact_bytes_many(self.raws, self.n, C.c_void_p(self.pinned), self.cap, self.bits, self.bpcs, self.offs,
                                                          self.lens, C.byref(self.total)), "gpupoly_matrix_store_compact_bytes_many")

    def payloads(self):
        return [C.string_at(self.pinned + self.offs[j], self.lens[j]) for j in range(self.n)]

    def load_loop(self):
        for j, m in enumerate(self.mats):
            check(lib.gpu_matrix_load_compact_bytes(m.raw, C.cast(C.c_void_p(self.pinned + self.offs[j]), C.POINTER(C.c_uint8)), self.lens[j],
                                                    self.bits[j]), "gpu_matrix_load_compact_bytes")

    def load_many(self):
        for j in range(self.n):
            self.ptrs[j] = self.pinned + self.offs[j]
        check(lib.gpupoly_matrix_load_compact_bytes_many(self.raws, self.n, self.ptrs, self.lens, self.bits), "gpupoly_matrix_load_compact_bytes_many")

    def release(self):
        lib.gpu_pinned_free(C.c_void_p(self.pinned))


def timed(fn, before=None):
    if before:
        before()
    mx.gpu_device_sync()
    c0 = lib.gpupoly_launch_count()
    t0 = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t0) * 1e3
    return dt, lib.gpupoly_launch_count() - c0


def measure(name, batch, reps, eval_in, extra=None):
    """store in `eval_in` form and load, the loop and the batched call alternated"""
    before = batch.to_eval if eval_in else None
    batch.store_loop()
    want = batch.payloads()
    batch.store_many()
    assert batch.payloads() == want, f"{name}: the batched store differs from the loop"
    out = {"matrices": batch.n, "payload_bytes": sum(len(w) for w in want)}
    for what, loop, many, prep in (("store", batch.store_loop, batch.store_many, before), ("load", batch.load_loop, batch.load_many, None)):
        if what == "load" and eval_in:
            continue  # the load does not depend on the form the matrices were stored from
        for _ in range(WARMUP):
            timed(loop, prep), timed(many, prep)
        a, b = [], []
        for _ in range(reps):
            (ta, la), (tb, lb) = timed(loop, prep), timed(many, prep)
            a.append(ta), b.append(tb)
        sa, sb = stats(a), stats(b)
        syncs = (2 * batch.n, 2) if what == "store" else (batch.n, 1)
        row = {"loop": dict(sa, launches=la, synchronises=syncs[0]), "batched": dict(sb, launches=lb, synchronises=syncs[1]),
               "ratio_loop_over_batched": round(sa["median_ms"] / sb["median_ms"], 3),
               "batched_not_slower_than_loop_spread": sb["median_ms"] <= sa["median_ms"] + (sa["p90_ms"] - sa["p10_ms"])}
        out[what] = row
        print(f"{name:34s} {what:5s} loop {sa['median_ms']:9.3f} ms [{sa['p10_ms']:.3f}..{sa['p90_ms']:.3f}] {la:4d} launches | "
              f"batched {sb['median_ms']:9.3f} ms [{sb['p10_ms']:.3f}..{sb['p90_ms']:.3f}] {lb:4d} launches | ratio {row['ratio_loop_over_batched']:.2f}")
    if extra:
        out.update(extra)
    return out


def small_outputs(requests):
    n, limbs, bits, base, d, cols = 256, 12, 51, 17, 2, 4
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, A = sampler.trapdoor(p, d)
    us = mx.GpuDCRTPolyUniformSampler()
    xs, ms = [], []
    for g in range(0, requests, 16):
        targets = [us.sample_uniform(p, d, cols, mx.DistType.FinRingDist()) for _ in range(16)]
        for _ in range(WARMUP):
            sampler.preimage_many_abi(p, td, A, targets)
        for _ in range(20):
            mx.gpu_device_sync()
            t0 = time.perf_counter()
            out = sampler.preimage_many_abi(p, td, A, targets)
            mx.gpu_device_sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        xs += out
    return xs, stats(ms)["median_ms"]


def large_outputs(count):
    n, limbs, bits, base, d, cols = 1 << 14, 10, 24, 12, 1, 50
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, A = sampler.trapdoor(p, d)
    us = mx.GpuDCRTPolyUniformSampler()
    return [sampler.preimage(p, td, A, us.sample_uniform(p, d, cols, mx.DistType.FinRingDist())) for _ in range(count)]


summary = {"reps": REPS, "reps_large": REPS_LARGE}
for requests in (16, 64):
    xs, preimage_ms = small_outputs(requests)
    batch = Batch(xs)
    extra = {"preimage_many_call_ms_per_16": preimage_ms}
    summary[f"{requests} x (76x4, n=256, 12x51) EVAL"] = measure(f"{requests} x 76x4 n=256 EVAL in", batch, REPS, True, extra)
    summary[f"{requests} x (76x4, n=256, 12x51) COEFF"] = measure(f"{requests} x 76x4 n=256 COEFF in", batch, REPS, False, extra)
    print(f"{'':34s} one gpupoly_trapdoor_preimage_many call of 16 requests: {preimage_ms:.3f} ms")
    batch.release()
    del batch, xs
batch = Batch(large_outputs(4))
summary["4 x (22x50, n=2^14, 10x24) EVAL"] = measure("4 x 22x50 n=2^14 EVAL in", batch, REPS_LARGE, True)
summary["4 x (22x50, n=2^14, 10x24) COEFF"] = measure("4 x 22x50 n=2^14 COEFF in", batch, REPS_LARGE, False)
batch.release()
print(json.dumps(summary))
