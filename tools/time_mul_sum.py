"""gpupoly_matrix_mul_sum / gpupoly_matrix_mul_acc (fused) against the per-term sequence of the existing entry points
(gpu_matrix_mul into a temporary, then gpu_matrix_add / gpu_matrix_sub in place), alternated in one process.

hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around calls into preallocated outputs and
temporaries, every shape warmed up, REPS alternated iterations (200; REPS_LARGE = 20 for the fat product), median and
10th..90th percentile; launches per call from gpupoly_launch_count; the results of both variants compared with
gpu_matrix_equal before anything is timed.  A shape class counts as SLOWER when the fused p10 exceeds the sequence's p90.
Shapes:
  (1) n = 256, 12 limbs of 51 bits: five terms (1 x 76)(76 x 4) plus an addend, one of them subtracted - the ggh15 chunk
      (src/lookup/ggh15/encoding.rs:205-298).  Fused: one mul_sum for the four added terms + one mul_acc for the subtracted one.
  (2) n = 2^14, 10 limbs of 24 bits: five terms (1 x 22)(22 x 50) plus an addend, one mul_sum.
  (3) the benchmark's M2A shape, (1 x 30)(30 x 120), n = 2^14, 15 limbs of 24 bits, words layout: one term accumulated in
      place (mul_acc) against mul + add_in_place.
  (4) M2B, (64 x 64)(64 x 64), n = 2^14, 8 limbs: one term accumulated in place - through the dispatcher's choice above 8 rows
      and, for the record, through the term-table kernel (MXX_HIP_MUL_SUM_PATH=tile).
Prints a JSON summary last."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS, REPS_LARGE, WARMUP = int(os.environ.get("REPS", "200")), int(os.environ.get("REPS_LARGE", "20")), 3
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
ok = _ffi.check_status


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def words(m):
    """force the words layout (samples of 24-bit rings start as PACKED24)"""
    ptr, size = C.c_void_p(), C.c_size_t()
    ok(lib.gpupoly_matrix_device_ptr(m.raw, C.byref(ptr), C.byref(size)), "gpupoly_matrix_device_ptr")
    return m


class Case:
    """out = base + sum_t sign_t lhss[t] * rhss[t]; base None: the outputs accumulate in place (out is its own addend)"""

    def __init__(self, p, rows, cols, ks, signs, in_place):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        level = p.crt_depth() - 1
        self.ctx, self.signs, self.in_place = p.ctx(), signs, in_place
        self.lhss = [words(us.sample_uniform(p, rows, k, dist)) for k in ks]
        self.rhss = [words(us.sample_uniform(p, k, cols, dist)) for k in ks]
        self.base = words(us.sample_uniform(p, rows, cols, dist))
        self.out, self.seq_out = M(p, rows, cols, level, True), M(p, rows, cols, level, True)
        self.tmp = [M(p, rows, cols, level, True) for _ in ks]
        self.reset()
        plus = [t for t, s in enumerate(signs) if s > 0]
        minus = [t for t, s in enumerate(signs) if s < 0]
        arr = lambda ms, idx: (C.c_void_p * max(len(idx), 1))(*[ms[t].raw.value for t in idx])  # noqa: E731
        self.groups = [(arr(self.lhss, idx), arr(self.rhss, idx), len(idx), neg) for idx, neg in ((plus, 0), (minus, 1)) if idx]

    def reset(self):
        for o in (self.out, self.seq_out):
            ok(lib.gpu_matrix_copy(o.raw, self.base.raw), "gpu_matrix_copy")

    def fused(self):
        if self.in_place and len(self.lhss) == 1:
            ok(lib.gpupoly_matrix_mul_acc(self.out.raw, self.lhss[0].raw, self.rhss[0].raw, 1 if self.signs[0] < 0 else 0), "gpupoly_matrix_mul_acc")
            return
        addend = self.out if self.in_place else self.base
        for la, ra, n, neg in self.groups:
            ok(lib.gpupoly_matrix_mul_sum(self.out.raw, 0, self.out.ncol, addend.raw, la, ra, n, neg), "gpupoly_matrix_mul_sum")
            addend = self.out

    def sequence(self):
        acc = self.seq_out if self.in_place else self.base
        for t, s in enumerate(self.signs):
            ok(lib.gpu_matrix_mul(self.tmp[t].raw, self.lhss[t].raw, self.rhss[t].raw), "gpu_matrix_mul")
            f = lib.gpu_matrix_add if s > 0 else lib.gpu_matrix_sub
            ok(f(self.seq_out.raw, acc.raw, self.tmp[t].raw), "gpu_matrix_add / gpu_matrix_sub")
            acc = self.seq_out

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0

    def same(self):
        eq = C.c_int(0)
        ok(lib.gpu_matrix_equal(self.out.raw, self.seq_out.raw, C.byref(eq)), "gpu_matrix_equal")
        return bool(eq.value)


def measure(name, case, reps, fused_only=False):
    case.reset()
    case.sequence(), case.fused()
    mx.gpu_device_sync()
    assert case.same(), f"{name}: the fused call differs from the per-term sequence"
    for _ in range(WARMUP):
        case.sequence(), case.fused()
    a, b = [], []
    la = lb = 0
    for _ in range(reps):
        if not fused_only:
            ta, la = case.timed(case.sequence)
            a.append(ta)
        tb, lb = case.timed(case.fused)
        b.append(tb)
    sb = stats(b)
    out = {"fused": dict(sb, launches=lb), "reps": reps}
    line = f"{name:58s} fused {sb['median_ms']:8.4f} ms [{sb['p10_ms']:.4f}..{sb['p90_ms']:.4f}] {lb:2d} launches"
    if not fused_only:
        sa = stats(a)
        slower = sb["p10_ms"] > sa["p90_ms"]
        out.update(sequence=dict(sa, launches=la), fused_over_sequence=round(sb["median_ms"] / sa["median_ms"], 3), slower=slower)
        line += (f" | sequence {sa['median_ms']:8.4f} ms [{sa['p10_ms']:.4f}..{sa['p90_ms']:.4f}] {la:2d} launches | fused / sequence "
                 f"{out['fused_over_sequence']:.3f}" + (" SLOWER (fused p10 > sequence p90)" if slower else ""))
    print(line, flush=True)
    return out


summary = {}
n, limbs, bits, base = 256, 12, 51, 17
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["1_ggh15_chunk"] = measure("(1) n=256 L=12 51-bit: 5 x (1x76)(76x4) + addend, one subtracted", Case(p, 1, 4, [76] * 5, [1, 1, 1, 1, -1], False), REPS)
n, limbs, bits, base = 1 << 14, 10, 24, 12
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["2_five_terms"] = measure("(2) n=2^14 L=10 24-bit: 5 x (1x22)(22x50) + addend", Case(p, 1, 50, [22] * 5, [1] * 5, False), REPS)
n, limbs = 1 << 14, 15
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
summary["3_m2a_acc"] = measure("(3) M2A n=2^14 L=15: (1x30)(30x120) accumulated in place", Case(p, 1, 120, [30], [1], True), REPS)
del p
n, limbs = 1 << 14, 8
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
case = Case(p, 64, 64, [64], [1], True)
summary["4_m2b_acc"] = measure("(4) M2B n=2^14 L=8: (64x64)(64x64) accumulated in place", case, REPS_LARGE)
os.environ["MXX_HIP_MUL_SUM_PATH"] = "tile"
_ffi.reload_env()
summary["4_m2b_acc_term_table_kernel"] = measure("(4) the same through the term-table kernel (PATH=tile)", case, max(REPS_LARGE // 2, 5), fused_only=True)
del os.environ["MXX_HIP_MUL_SUM_PATH"]
_ffi.reload_env()
print(json.dumps(summary))
