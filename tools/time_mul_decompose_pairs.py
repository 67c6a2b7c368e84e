"""gpupoly_matrix_mul_decompose_pairs (one call) against the per-request sequence of the existing entry points
(gpu_matrix_copy_block of the window, gpupoly_matrix_mul_decompose, gpu_matrix_mul_scalar, gpu_matrix_sub per request), the
legs alternated in one process; then the slot-transfer gate targets built on it (mxx_amd.slot_transfer) against the loops of
the per-request restatements.

hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around each leg, every shape warmed up, REPS (30)
alternated iterations, median and 10th..90th percentile; launches per leg counted from the library's launch trace
(_ffi.trace_begin / trace_end, device copies included); the results of both legs compared with gpu_matrix_equal before
anything is timed.  The primitive's legs write into preallocated outputs and temporaries; the target builders allocate as
their callers would.
Shapes:
  (a) n = 256, 12 limbs of 51 bits, base 2^17 (k = 36), d = 2: 16 requests of 2 x 72 against their own 2 x 72 matrix, a
      four-column chunk, scalar and addend, subtracted.
  (b) the same with 64 requests.
  (c) n = 2^14, 8 limbs of 24 bits, base 2^12 (k = 16), d = 1: 16 requests of 1 x 16 against their own 1 x 18 matrix, an
      18-column chunk.  The one call must not be slower than the sequence beyond the sequence's own spread.
  (d) gate_target_chunks against the loop of build_gate_target_chunk, ring and chunk of (a), 16 requests.
  (e) slot_reduce_gate_target_chunks with 8 slots against the loop of build_slot_reduce_gate_target_chunk, 8 requests.
After each line: the launch trace of one run of each leg (kernel, launches, ms).  Prints a JSON summary last."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402
from mxx_amd import slot_transfer as ST  # noqa: E402

REPS, WARMUP = max(10, int(os.environ.get("REPS", "30"))), 3
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
US, FIN = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def same(xs, ys):
    eq = C.c_int(0)
    for a, b in zip(xs, ys):
        _ffi.check_status(lib.gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
        if not eq.value:
            return False
    return True


def trace(fn):
    """(launches, [(kernel, launches, ms)]) of one run"""
    mx.gpu_device_sync()
    _ffi.trace_begin()
    fn()
    mx.gpu_device_sync()
    rows = _ffi.trace_end()
    agg = {}
    for r_ in rows:
        e = agg.setdefault(r_["kernel"].split("<")[0].split(" (")[0], [0, 0.0])
        e[0] += 1
        e[1] += r_["ms"]
    return len(rows), sorted(((k_, v[0], round(v[1], 4)) for k_, v in agg.items()), key=lambda t: -t[2])


class Pairs:
    """count requests of rows x (r k) against r x m, the chunk [col_start, col_start + c), scalar and addend, subtracted"""

    def __init__(self, p, count, rows, r, m, col_start, c):
        self.p, self.ctx, self.n, self.col_start, self.c, self.r = p, p.ctx(), count, col_start, c, r
        k, level = p.modulus_digits(), p.crt_depth() - 1
        self.rhss = [US.sample_uniform(p, r, m, FIN) for _ in range(count)]
        self.lhss = [US.sample_uniform(p, rows, r * k, FIN) for _ in range(count)]
        self.adds = [US.sample_uniform(p, rows, c, FIN) for _ in range(count)]
        self.scs = [US.sample_uniform(p, 1, 1, FIN) for _ in range(count)]
        new = lambda h, w: [M(p, h, w, level, True) for _ in range(count)]  # noqa: E731
        self.outs, self.seq_outs, self.tmp, self.tmp2, self.win = new(rows, c), new(rows, c), new(rows, c), new(rows, c), new(r, c)
        arr = lambda ms: (C.c_void_p * count)(*[m_.raw.value for m_ in ms])  # noqa: E731
        self.arrs = [arr(x) for x in (self.outs, self.adds, self.lhss, self.rhss, self.scs)]

    def one_call(self):
        _ffi.check_status(lib.gpupoly_matrix_mul_decompose_pairs(*self.arrs, self.n, self.col_start, self.p.base_bits(), 1),
                          "gpupoly_matrix_mul_decompose_pairs")

    def sequence(self):
        base = self.p.base_bits()
        for j in range(self.n):
            _ffi.check_status(lib.gpu_matrix_copy_block(self.win[j].raw, self.rhss[j].raw, 0, 0, 0, self.col_start, self.r, self.c), "copy_block")
            _ffi.check_status(lib.gpupoly_matrix_mul_decompose(self.tmp[j].raw, self.lhss[j].raw, self.win[j].raw, base), "mul_decompose")
            _ffi.check_status(lib.gpu_matrix_mul_scalar(self.tmp2[j].raw, self.tmp[j].raw, self.scs[j].raw), "mul_scalar")
            _ffi.check_status(lib.gpu_matrix_sub(self.seq_outs[j].raw, self.adds[j].raw, self.tmp2[j].raw), "sub")

    legs = property(lambda self: (self.sequence, self.one_call))

    def results(self):
        return self.seq_outs, self.outs


class Targets:
    """the batched slot-transfer targets against the loop of the per-request restatement"""

    def __init__(self, p, d, count, chunk, slots=0):
        self.ctx = p.ctx()
        self.sh = ST.SlotGateShared(p, bytes(range(32)), d)
        m_g = self.sh.m_g
        mat = lambda rows, cols: US.sample_uniform(p, rows, cols, FIN)  # noqa: E731
        seeds = [mx.GpuRngSeed.from_bytes(bytes((t * 29 + i) & 0xFF for i in range(32))) for t in range(count)]
        if slots:
            secrets, slot_as, a_in = [mat(d, d) for _ in range(slots)], [mat(d, m_g) for _ in range(slots)], mat(d, m_g)
            dst = [t % slots for t in range(count)]
            self.batched = lambda: ST.slot_reduce_gate_target_chunks(self.sh, 3, [a_in] * count, dst, secrets, slot_as, seeds, 4.578, chunk)
            self.loop = lambda: [ST.build_slot_reduce_gate_target_chunk(self.sh, 3, a_in, dst[t], secrets, slot_as, seeds[t], 4.578, *chunk)
                                 for t in range(count)]
        else:
            lhs, s_js, a_js, scs = ([mat(d, m_g) for _ in range(count)], [mat(d, d) for _ in range(count)], [mat(d, m_g) for _ in range(count)],
                                    [mat(1, 1) for _ in range(count)])
            self.batched = lambda: ST.gate_target_chunks(self.sh, 3, lhs, s_js, a_js, scs, seeds, 4.578, chunk)
            self.loop = lambda: [ST.build_gate_target_chunk(self.sh, 3, lhs[t], s_js[t], a_js[t], scs[t], seeds[t], 4.578, *chunk) for t in range(count)]

    legs = property(lambda self: (self.loop, self.batched))

    def results(self):
        return self.loop(), self.batched()


def measure(name, case, names=("sequence", "one call")):
    old, new = case.legs
    for _ in range(WARMUP):
        old(), new()
    mx.gpu_device_sync()
    assert same(*case.results()), f"{name}: the two legs differ"
    a, b = [], []
    for _ in range(REPS):
        for fn, into in ((old, a), (new, b)):
            case.ctx.timer_start()
            fn()
            into.append(case.ctx.timer_stop())
    sa, sb = stats(a), stats(b)
    (la, ta), (lb, tb) = trace(old), trace(new)
    ratio = round(sb["median_ms"] / sa["median_ms"], 3)
    print(f"{name:58s} {names[0]} {sa['median_ms']:8.3f} ms [{sa['p10_ms']:.3f}..{sa['p90_ms']:.3f}] {la:4d} launches | {names[1]} "
          f"{sb['median_ms']:8.3f} ms [{sb['p10_ms']:.3f}..{sb['p90_ms']:.3f}] {lb:3d} launches | new / old {ratio:.3f}")
    for which, t in ((names[1], tb), (names[0], ta)):
        print(f"    trace, {which}: " + "; ".join(f"{k_} x{cnt} {ms:.3f} ms" for k_, cnt, ms in t))
    return {names[0]: dict(sa, launches=la), names[1]: dict(sb, launches=lb), "new_over_old": ratio,
            "within_the_old_legs_spread": sb["median_ms"] <= sa["p90_ms"]}


summary = {"reps": REPS}
n, limbs, bits, base = 256, 12, 51, 17
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
k = p.modulus_digits()
summary["a"] = measure("(a) n=256 L=12 51-bit d=2: 16 x (2x72)(72x4) o s, addend -", Pairs(p, 16, 2, 2, 2 * k, 4, 4))
summary["b"] = measure("(b) the same, 64 requests", Pairs(p, 64, 2, 2, 2 * k, 4, 4))
summary["d"] = measure("(d) gate_target_chunks, 16 requests, d=2, chunk (4, 4)", Targets(p, 2, 16, (4, 4)), ("loop", "batched"))
summary["e"] = measure("(e) slot_reduce_gate_target_chunks, 8 slots, 8 requests", Targets(p, 2, 8, (4, 4), slots=8), ("loop", "batched"))
n, limbs, bits, base = 1 << 14, 8, 24, 12
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["c"] = measure("(c) n=2^14 L=8 24-bit d=1: 16 x (1x16)(16x18) o s, addend -", Pairs(p, 16, 1, 1, 18, 0, 18))
print(json.dumps(summary))
