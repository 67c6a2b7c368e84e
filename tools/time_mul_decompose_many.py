"""gpupoly_matrix_mul_decompose_many (one call) against the per-operand sequence of the existing entry points
(gpupoly_matrix_mul_decompose, gpu_matrix_mul_scalar, gpu_matrix_add per operand), alternated in one process.

hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around calls into preallocated outputs and
temporaries, every shape warmed up, REPS (30) alternated iterations, median and 10th..90th percentile; launches per call
from gpupoly_launch_count; the results of both variants compared with gpu_matrix_equal before anything is timed.
Shapes:
  (a) n = 2^14, 8 limbs of 24 bits, base 2^12 (k = 16), rhs 4 x 64: one 1 x 64 vector with addend and scalar + one 4 x 64
      matrix without - an encoding multiplication at d = 4.                        bar: new <= 0.65 x sequence
  (b) the same ring and rhs: sixteen 1 x 64 vectors with addend and scalar + one 4 x 64 matrix - a 16-slot poly-encoding
      multiplication.                                                              bar: new <= 0.20 x sequence
  (c) n = 256, 12 limbs of 51 bits, base 2^17, rhs 2 x 3 (the M4 chain's mul_decompose): sixteen 1 x 72 operands with
      addends and scalars - launch-bound, milliseconds and launches reported, no bar.
After the table: the library's launch trace of one call of each variant per shape (kernel, launches, ms), which names
the stage that takes the time.  Prints a JSON summary last."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "30")), 3
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


class Case:
    def __init__(self, p, rhs_shape, rows, with_addend):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        self.p, self.ctx, self.n = p, p.ctx(), len(rows)
        k, level = p.modulus_digits(), p.crt_depth() - 1
        r, c = rhs_shape
        self.rhs = us.sample_uniform(p, r, c, dist)
        self.lhss = [us.sample_uniform(p, h, r * k, dist) for h in rows]
        self.adds = [us.sample_uniform(p, h, c, dist) if w else None for h, w in zip(rows, with_addend)]
        self.scs = [us.sample_uniform(p, 1, 1, dist) if w else None for w in with_addend]
        self.outs = [M(p, h, c, level, True) for h in rows]       # the one call's outputs
        self.seq_outs = [M(p, h, c, level, True) for h in rows]   # the sequence's outputs
        self.tmp = [M(p, h, c, level, True) for h in rows]        # its products
        self.tmp2 = [M(p, h, c, level, True) for h in rows]       # its scaled addends
        arr = lambda ms: (C.c_void_p * self.n)(*[None if m is None else m.raw.value for m in ms])  # noqa: E731
        self.a_outs, self.a_lhss, self.a_adds, self.a_scs = arr(self.outs), arr(self.lhss), arr(self.adds), arr(self.scs)

    def many(self):
        _ffi.check_status(lib.gpupoly_matrix_mul_decompose_many(self.a_outs, self.a_lhss, self.a_adds, self.a_scs, self.n, self.rhs.raw,
                                                                self.p.base_bits()), "gpupoly_matrix_mul_decompose_many")

    def sequence(self):
        base = self.p.base_bits()
        for j in range(self.n):
            if self.adds[j] is None:
                _ffi.check_status(lib.gpupoly_matrix_mul_decompose(self.seq_outs[j].raw, self.lhss[j].raw, self.rhs.raw, base), "mul_decompose")
                continue
            _ffi.check_status(lib.gpupoly_matrix_mul_decompose(self.tmp[j].raw, self.lhss[j].raw, self.rhs.raw, base), "mul_decompose")
            _ffi.check_status(lib.gpu_matrix_mul_scalar(self.tmp2[j].raw, self.adds[j].raw, self.scs[j].raw), "mul_scalar")
            _ffi.check_status(lib.gpu_matrix_add(self.seq_outs[j].raw, self.tmp[j].raw, self.tmp2[j].raw), "add")

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0

    def same(self):
        eq = C.c_int(0)
        for a, b in zip(self.outs, self.seq_outs):
            _ffi.check_status(lib.gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
            if not eq.value:
                return False
        return True

    def trace(self, fn):
        _ffi.trace_begin()
        fn()
        rows = _ffi.trace_end()
        agg = {}
        for r_ in rows:
            e = agg.setdefault(r_["kernel"].split("<")[0].split(" ")[0], [0, 0.0])
            e[0] += 1
            e[1] += r_["ms"]
        return sorted(((k_, v[0], round(v[1], 4)) for k_, v in agg.items()), key=lambda t: -t[2])


def measure(name, case, bar):
    for _ in range(WARMUP):
        case.sequence(), case.many()
    mx.gpu_device_sync()
    assert case.same(), f"{name}: the one call differs from the per-operand sequence"
    a, b = [], []
    for _ in range(REPS):
        (ta, la), (tb, lb) = case.timed(case.sequence), case.timed(case.many)
        a.append(ta), b.append(tb)
    sa, sb = stats(a), stats(b)
    ratio = round(sb["median_ms"] / sa["median_ms"], 3)
    verdict = "no bar" if bar is None else ("meets" if ratio <= bar else "MISSES") + f" the bar of {bar:.2f}"
    print(f"{name:44s} sequence {sa['median_ms']:8.3f} ms [{sa['p10_ms']:.3f}..{sa['p90_ms']:.3f}] {la:3d} launches | one call "
          f"{sb['median_ms']:8.3f} ms [{sb['p10_ms']:.3f}..{sb['p90_ms']:.3f}] {lb:3d} launches | new / sequence {ratio:.3f}: {verdict}")
    out = {"sequence": dict(sa, launches=la), "one_call": dict(sb, launches=lb), "new_over_sequence": ratio, "bar": bar,
           "trace_one_call": case.trace(case.many), "trace_sequence": case.trace(case.sequence)}
    for which in ("trace_one_call", "trace_sequence"):
        print(f"    {which}: " + "; ".join(f"{k_} x{cnt} {ms:.3f} ms" for k_, cnt, ms in out[which]))
    return out


summary = {"reps": REPS}
n, limbs, bits, base = 1 << 14, 8, 24, 12
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["a"] = measure("(a) n=2^14 L=8: 1x64 (+addend o scalar), 4x64", Case(p, (4, 64), [1, 4], [True, False]), 0.65)
summary["b"] = measure("(b) n=2^14 L=8: 16 x 1x64 (+addend o scalar), 4x64", Case(p, (4, 64), [1] * 16 + [4], [True] * 16 + [False]), 0.20)
n, limbs, bits, base = 256, 12, 51, 17
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["c"] = measure("(c) n=256 L=12 51-bit: 16 x 1x72 (+addend o scalar)", Case(p, (2, 3), [1] * 16, [True] * 16), None)
print(json.dumps(summary))
