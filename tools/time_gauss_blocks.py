"""gpupoly_matrix_sample_gauss_blocks (one call) against the loop of plain sampler calls and against the Gaussian segments in
chunks of 64, and the batched gate-stage targets (mxx_amd.lookup.gate_stage1_targets / gate_stage3_targets) against their
per-gate legs, alternated in one process.

Sampling legs, Gaussian distribution, T seeded blocks of r x c:
  loop      T calls of GpuDCRTPolyMatrix.sample_distribution (sample, scatter, transform per call)
  segments  GpuDCRTPolyMatrix.sample_distribution_segments per 64 blocks (r x 64 c each): the only many-seed Gaussian form
            the library had
  blocks    one GpuDCRTPolyMatrix.sample_gauss_blocks in the columns layout (r x T c)
Target legs, 16 gates, d = 2, a four-column chunk:
  per_gate  the reference's function restated, gate by gate (build_gate_stageN_target_chunk)
  batched   gate_stageN_targets
hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around each leg - host stalls of the loop legs
included: it is what the caller waits for -, every shape warmed up, REPS alternated iterations, median, min..max and 90th percentile,
launches per leg from gpupoly_launch_count, results compared with gpu_matrix_equal before timing.
Shapes:
  (a) 64 blocks of 2 x 4 at n = 2^8, 12 limbs of 51 bits, sigma 4.578
  (b) 130 blocks of the same
  (c) 16 blocks of 1 x 18 at n = 2^14, 8 limbs of 24 bits
  (s1), (s3) the stage-1 and stage-3 targets of 16 gates at n = 2^8, 12 limbs of 51 bits
The report goes to --out (profiles/gauss_blocks_timing.txt) and to stdout; a JSON summary is its last line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxx_amd import _ffi  # noqa: E402
import mxx_amd as mx  # noqa: E402
from mxx_amd import lookup as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_blocks_timing.txt"))
ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "10")))
args = ap.parse_args()
REPS, WARMUP, SIGMA = max(6, args.reps), 2, 4.578
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
GAUSS = mx.DistType.GaussDist(SIGMA).as_ffi()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(ms):
    ms = sorted(ms)
    p90 = ms[min(len(ms) - 1, max(0, round(0.9 * (len(ms) - 1))))]  # nearest rank, as time_lut_targets.py takes it
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "p90_ms": round(p90, 4)}


def seed(tag):
    return mx.GpuRngSeed.from_bytes(bytes((tag * 37 + 11 * i + 5) & 0xFF for i in range(32)))


def timed(ctx, fn):
    c0 = lib.gpupoly_launch_count()
    ctx.timer_start()
    fn()
    ms = ctx.timer_stop()
    return ms, lib.gpupoly_launch_count() - c0


def measure(name, ctx, legs, check, compare):
    """legs: {name: callable}; check() after the warm-up; compare: [(new leg, old leg)] - the new one is 'not slower' when its
    median is at most the old one's maximum"""
    for _ in range(WARMUP):
        for fn in legs.values():
            fn()
    mx.gpu_device_sync()
    check()
    times, launches = {k: [] for k in legs}, {}
    for _ in range(REPS):
        for k, fn in legs.items():
            ms, launches[k] = timed(ctx, fn)
            times[k].append(ms)
    out = {k: dict(stats(v), launches=launches[k]) for k, v in times.items()}
    say(name)
    for k in legs:
        s = out[k]
        say(f"    {k:10s} {s['median_ms']:10.4f} ms [{s['min_ms']:.4f}..{s['max_ms']:.4f}] p90 {s['p90_ms']:.4f} {s['launches']:5d} launches")
    for new, old in compare:
        ratio = out[old]["median_ms"] / out[new]["median_ms"]
        inside = out[new]["median_ms"] <= out[old]["max_ms"]
        out[f"{old}_over_{new}"] = round(ratio, 2)
        out[f"{new}_not_slower_than_{old}"] = inside
        say(f"    {old} / {new} {ratio:.2f}; {new} median {'within or below' if inside else 'ABOVE'} the min..max of {old}")
    return out


class Blocks:
    def __init__(self, p, blocks, rows, cols):
        self.p, self.T, self.rows, self.cols = p, blocks, rows, cols
        self.seeds = [seed(100 + t) for t in range(blocks)]
        self.out = {}

    def loop(self):
        self.out["loop"] = [M.sample_distribution(self.p, self.rows, self.cols, GAUSS, SIGMA, s) for s in self.seeds]

    def segments(self):
        self.out["segments"] = [M.sample_distribution_segments(self.p, self.rows, [self.cols] * len(self.seeds[lo:lo + 64]), GAUSS, SIGMA,
                                                               self.seeds[lo:lo + 64]) for lo in range(0, self.T, 64)]

    def blocks(self):
        self.out["blocks"] = M.sample_gauss_blocks(self.p, self.seeds, SIGMA, nrow=self.rows, seg_cols=[self.cols] * self.T)

    def check(self):
        wide, at = self.out["blocks"], 0
        for part in self.out["segments"]:
            assert wide.slice_columns(at, at + part.ncol) == part, "the blocks differ from the segments"
            at += part.ncol
        for lo in range(0, self.T, 64):
            count = min(64, self.T - lo)
            parts = wide.slice_columns(lo * self.cols, (lo + count) * self.cols).split_columns([self.cols] * count)
            for t, part in enumerate(parts):
                assert part == self.out["loop"][lo + t], f"block {lo + t} differs from the plain call"

    def legs(self):
        return {"loop": self.loop, "segments": self.segments, "blocks": self.blocks}


class Stage:
    def __init__(self, p, stage, gates=16, d=2, chunk=(4, 4)):
        m_g = d * p.modulus_digits()
        fin = mx.DistType.FinRingDist()
        us = mx.GpuDCRTPolyUniformSampler()
        mats = [us.sample_uniform(p, d, m_g, fin) for _ in range(4)]
        self.shared = L.GateShared(p, bytes(range(32)), 0, *mats)
        self.stage, self.chunk = stage, chunk
        self.s_seeds = [seed(200 + t) for t in range(gates)]
        self.e_seeds = [seed(300 + t) for t in range(gates)]
        self.out = {}

    def per_gate(self):
        build = L.build_gate_stage1_target_chunk if self.stage == 1 else L.build_gate_stage3_target_chunk
        self.out["per_gate"] = [build(self.shared, s, e, SIGMA, *self.chunk) for s, e in zip(self.s_seeds, self.e_seeds)]

    def batched(self):
        fn = L.gate_stage1_targets if self.stage == 1 else L.gate_stage3_targets
        self.out["batched"] = fn(self.shared, self.s_seeds, self.e_seeds, SIGMA, self.chunk)

    def check(self):
        for t, (a, b) in enumerate(zip(self.out["per_gate"], self.out["batched"])):
            assert a == b, f"target {t} differs from the per-gate leg"

    def legs(self):
        return {"per_gate": self.per_gate, "batched": self.batched}


summary = {"reps": REPS}
say(f"{REPS} alternated iterations per shape after {WARMUP} warm-up rounds, median [min..max]")
n, limbs, bits = 1 << 8, 12, 51
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 17)
for key, blocks in (("a", 64), ("b", 130)):
    case = Blocks(p, blocks, 2, 4)
    summary[key] = measure(f"({key}) {blocks} blocks of 2 x 4, n=2^8, 12 limbs of 51 bits, sigma {SIGMA}", p.ctx(), case.legs(), case.check,
                           [("blocks", "segments"), ("blocks", "loop")])
for stage in (1, 3):
    case = Stage(p, stage)
    summary[f"s{stage}"] = measure(f"(s{stage}) stage-{stage} targets of 16 gates, d=2, four columns, n=2^8, 12 limbs of 51 bits", p.ctx(),
                                   case.legs(), case.check, [("batched", "per_gate")])
n, limbs, bits = 1 << 14, 8, 24
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 12)
case = Blocks(p, 16, 1, 18)
summary["c"] = measure(f"(c) 16 blocks of 1 x 18, n=2^14, 8 limbs of 24 bits, sigma {SIGMA}", p.ctx(), case.legs(), case.check,
                       [("blocks", "segments"), ("blocks", "loop")])
say(json.dumps(summary))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
