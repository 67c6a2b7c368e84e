"""gpupoly_matrix_crt_recompose_rounded (one call) against the per-level loop a caller has today, alternated in one process.

Loop leg: GpuDCRTPolyMatrix._crt_recompose_rows_loop - per (slot, limb) decode_centered(level, q_i), mul_scalar by the
constant polynomial of reconst_coeffs[i] (host build, upload, forward transform), add_in_place, then concat_rows; with
T = 4 terms per level it first forms every level as `input + refresh - one - decoder` with the three + / - calls of the
online path (src/noise_refresh/naive_vec.rs:1687).  It uses only entry points older than the fused call.
Fused leg: one GpuDCRTPolyMatrix.crt_recompose_rows_terms.
hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around each leg - host stalls of the loop leg
included: it is what the caller waits for -, every shape warmed up, REPS alternated iterations, median and 10th..90th
percentile, launches per call from gpupoly_launch_count, both results compared with gpu_matrix_equal before timing.
Shapes (EVAL terms, as the online path holds them), each with T = 1 and T = 4:
  (a) n = 2^10, 5 limbs of 51 bits, c = 15, num_slots = 16
  (b) n = 2^16, 8 limbs of 28 bits, c = 16, num_slots = 4
The report goes to --out (profiles/crt_recompose_timing.txt) and to stdout; a JSON summary is its last line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxx_amd import _ffi  # noqa: E402
import mxx_amd as mx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crt_recompose_timing.txt"))
ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "10")))
args = ap.parse_args()
REPS, WARMUP = args.reps, 2
SIGNS = {1: [1], 4: [1, 1, -1, -1]}
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


class Case:
    def __init__(self, p, cols, num_slots, T):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        self.p, self.ctx, self.num_slots, self.signs = p, p.ctx(), num_slots, SIGNS[T]
        self.terms = [[us.sample_uniform(p, 1, cols, dist) for _ in range(T)] for _ in range(num_slots * p.crt_depth())]
        for level in self.terms:
            for m in level:
                m.ntt_all_in_place()
                lib.gpupoly_matrix_device_ptr(m.raw, C.byref(C.c_void_p()), C.byref(C.c_size_t()))  # words layout from here on
        self.loop_out = self.fused_out = None

    def loop(self):
        levels = [lv[0] if len(lv) == 1 else lv[0] + lv[1] - lv[2] - lv[3] for lv in self.terms]
        self.loop_out = M._crt_recompose_rows_loop(self.p, levels, self.num_slots)

    def fused(self):
        self.fused_out = M.crt_recompose_rows_terms(self.p, self.terms, self.signs, self.num_slots)

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0

    def same(self):
        eq = C.c_int(0)
        _ffi.check_status(lib.gpu_matrix_equal(self.loop_out.raw, self.fused_out.raw, C.byref(eq)), "gpu_matrix_equal")
        return bool(eq.value)


def measure(name, case):
    for _ in range(WARMUP):
        case.loop()
        case.fused()
    mx.gpu_device_sync()
    assert case.same(), f"{name}: the one call differs from the per-level loop"
    a, b, la, lb = [], [], 0, 0
    for _ in range(REPS):
        ta, la = case.timed(case.loop)
        a.append(ta)
        tb, lb = case.timed(case.fused)
        b.append(tb)
    sa, sb = stats(a), stats(b)
    out = {"loop": dict(sa, launches=la), "fused": dict(sb, launches=lb), "loop_over_fused": round(sa["median_ms"] / sb["median_ms"], 2)}
    say(f"{name:58s} loop {sa['median_ms']:10.3f} ms [{sa['p10_ms']:.3f}..{sa['p90_ms']:.3f}] {la:5d} launches | fused "
        f"{sb['median_ms']:9.4f} ms [{sb['p10_ms']:.4f}..{sb['p90_ms']:.4f}] {lb:3d} launches | loop / fused {out['loop_over_fused']:.2f}")
    return out


summary = {"reps": REPS}
say(f"{REPS} alternated iterations per shape, median [p10..p90]")
n, limbs, bits = 1 << 10, 5, 51
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 17)
for T in (1, 4):
    summary[f"a_T{T}"] = measure(f"(a) n=2^10 L=5 51-bit c=15 num_slots=16 T={T}", Case(p, 15, 16, T))
n, limbs, bits = 1 << 16, 8, 28
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 14)
for T in (1, 4):
    summary[f"b_T{T}"] = measure(f"(b) n=2^16 L=8 28-bit c=16 num_slots=4 T={T}", Case(p, 16, 4, T))
say(json.dumps(summary))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
