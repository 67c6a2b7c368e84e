"""gpupoly_matrix_monomial_sum (one call) against the per-term loop a caller has today, alternated in one process.

Loop leg: per term a one-hot vector through GpuDCRTPoly.from_u32s (host build, upload, forward transform), mul_scalar and
+ on EVAL operands; COEFF operands are first transformed (clone + ntt) and the sum is transformed back - the existing
entry points offer no other way.  Fused leg: one GpuDCRTPolyMatrix.monomial_sum.
hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around each leg - host stalls of the loop leg
included: it is what the caller waits for -, every shape warmed up, REPS alternated iterations, median and 10th..90th
percentile, launches per call from gpupoly_launch_count, both results compared with gpu_matrix_equal before timing.
Shapes:
  (a) 16 terms of 2 x 64 at n = 2^14, 8 limbs of 24 bits, EVAL            (b) the same in COEFF
  (c) 256 terms of 2 x 4 at n = 256, 12 limbs of 51 bits, EVAL: collapse_slot_matrices at num_slots = n
  (d) 2 terms of 1 x 64 at n = 2^14, 8 limbs of 24 bits, EVAL
For (a), (b), (d): algorithmic bytes (each operand read once, the addend read once, the output written once) over the fused
median.  With --parent-lib PATH the loop leg runs once more in a fresh process against that build of the library
(MXX_GPUPOLY_LIB; a build without the monomial entries runs the loop leg alone).  The report goes to --out
(profiles/monomial_sum_timing.txt) and to stdout; a JSON summary is its last line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxx_amd import _ffi  # noqa: E402

NEW = ("gpupoly_matrix_fill_monomial", "gpupoly_matrix_mul_monomial", "gpupoly_matrix_monomial_sum")
if not all(hasattr(C.CDLL(_ffi.LIB_PATH), s) for s in NEW):  # an older build: the loop leg alone
    for s in NEW:
        _ffi.SIGNATURES.pop(s)
    HAVE_FUSED = False
else:
    HAVE_FUSED = True
import mxx_amd as mx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monomial_sum_timing.txt"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--loop-only", action="store_true")
ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
args = ap.parse_args()
REPS, WARMUP = args.reps, 2
FUSED = HAVE_FUSED and not args.loop_only
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
    def __init__(self, p, shape, terms, ev):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        self.p, self.ctx, self.ev = p, p.ctx(), ev
        n = p.ring_dimension()
        self.mats = [us.sample_uniform(p, shape[0], shape[1], dist) for _ in range(terms)]
        self.addend = us.sample_uniform(p, shape[0], shape[1], dist)
        for m in self.mats + [self.addend]:
            m.ensure_eval() if ev else m.intt_all_in_place()
            lib.gpupoly_matrix_device_ptr(m.raw, C.byref(C.c_void_p()), C.byref(C.c_size_t()))  # words layout from here on
        self.shifts = [(j * (n // terms) + (j % 3)) % n for j in range(terms)]  # below N: from_u32s spells +x^s
        self.bytes = (terms + 2) * shape[0] * shape[1] * p.crt_depth() * n * p.ctx().word_bytes()
        self.loop_out = self.fused_out = None

    def loop(self):
        acc = self.addend if self.ev else self.addend.ensure_eval()
        for m, s in zip(self.mats, self.shifts):
            mono = mx.GpuDCRTPoly.from_u32s(self.p, [0] * s + [1])
            acc = acc + m.ensure_eval().mul_scalar(mono)
        self.loop_out = acc if self.ev else acc.into_coeff_domain()

    def fused(self):
        self.fused_out = M.monomial_sum(self.mats, self.shifts, addend=self.addend)

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


def measure(name, case, with_rate):
    for _ in range(WARMUP):
        case.loop()
        if FUSED:
            case.fused()
    mx.gpu_device_sync()
    if FUSED:
        assert case.same(), f"{name}: the one call differs from the per-term loop"
    a, b, la, lb = [], [], 0, 0
    for _ in range(REPS):
        ta, la = case.timed(case.loop)
        a.append(ta)
        if FUSED:
            tb, lb = case.timed(case.fused)
            b.append(tb)
    sa = stats(a)
    out = {"loop": dict(sa, launches=la)}
    text = f"{name:52s} loop {sa['median_ms']:9.3f} ms [{sa['p10_ms']:.3f}..{sa['p90_ms']:.3f}] {la:4d} launches"
    if FUSED:
        sb = stats(b)
        out["fused"] = dict(sb, launches=lb)
        out["fused_over_loop"] = round(sb["median_ms"] / sa["median_ms"], 4)
        verdict = "no slower" if sb["median_ms"] <= sa["median_ms"] or sb["p10_ms"] <= sa["p90_ms"] else "SLOWER"
        text += (f" | fused {sb['median_ms']:8.4f} ms [{sb['p10_ms']:.4f}..{sb['p90_ms']:.4f}] {lb:2d} launches | fused / loop "
                 f"{out['fused_over_loop']:.4f}: {verdict}")
        if with_rate:
            out["fused_TBps"] = round(case.bytes / (sb["median_ms"] * 1e-3) / 1e12, 3)
            text += f" | {case.bytes / 1e6:.1f} MB algorithmic = {out['fused_TBps']:.2f} TB/s"
    say(text)
    return out


summary = {"reps": REPS, "library": _ffi.LIB_PATH, "fused_leg": FUSED}
say(f"library {_ffi.LIB_PATH}; {REPS} alternated iterations per shape, median [p10..p90]")
n, limbs, bits = 1 << 14, 8, 24
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 12)
summary["a"] = measure("(a) n=2^14 L=8 24-bit: 16 terms of 2x64, EVAL", Case(p, (2, 64), 16, True), True)
summary["b"] = measure("(b) n=2^14 L=8 24-bit: 16 terms of 2x64, COEFF", Case(p, (2, 64), 16, False), True)
summary["d"] = measure("(d) n=2^14 L=8 24-bit: 2 terms of 1x64, EVAL", Case(p, (1, 64), 2, True), True)
n, limbs, bits = 256, 12, 51
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 17)
summary["c"] = measure("(c) n=256 L=12 51-bit: 256 terms of 2x4, EVAL", Case(p, (2, 4), 256, True), False)
if args.parent_lib:
    say(f"--- the loop leg against {os.path.basename(args.parent_lib)} (a fresh process) ---")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--reps", str(REPS), "--out", os.devnull],
                           env=dict(os.environ, MXX_GPUPOLY_LIB=os.path.abspath(args.parent_lib)), capture_output=True, text=True)
    if child.returncode != 0:
        say(f"child failed ({child.returncode}): {child.stderr[-2000:]}")
    else:
        body = child.stdout.strip().splitlines()
        for ln in body[:-1]:
            say("    " + ln)
        summary["parent_loop"] = json.loads(body[-1])
say(json.dumps(summary))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
