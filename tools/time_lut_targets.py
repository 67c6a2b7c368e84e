"""The preimage targets of T LUT rows of one column chunk (tools/README.md), two ways in one process:
  loop   `build_lut_preimage_target_chunk` row by row: the reference's sequence through the older entries (slice, gadget,
         mul_scalar, decompose, tag hash, decomposed window sample, three products with their adds)
  call   one `gpupoly_matrix_lut_targets` call (`lut_preimage_target_chunks`)
and the same two followed by `preimage_many_abi` over the targets (loop+pre, call+pre), on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, c = 4, T = 16 and T = 64;   n = 2^14, 8 x 24 bits, base 2^12, d = 1, c = 4, T = 16.
The targets of both legs are compared first (`gpu_matrix_equal`) and A x == target is checked.  Then the legs alternate;
every leg is bracketed by device events on the context's stream and by the host clock until the device is idle; median,
minimum, maximum and 90th percentile (nearest rank, as time_lwe_targets.py takes it) of REPS (6) after a warm-up - the
spread is max - min of a leg -, launches per call from
gpupoly_launch_count, and the launch trace of both target legs summed per kernel.  Output goes to stdout and to
profiles/lut_targets_timing.txt (or the path given as the first argument)."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, lookup  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "6")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, chunk columns, rows
    ("m4 (u64), T = 16", 256, 12, 51, 17, 2, 4, 16),
    ("m4 (u64), T = 64", 256, 12, 51, 17, 2, 4, 64),
    ("n16384 (u32), T = 16", 16384, 8, 24, 12, 1, 4, 16),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lut_targets_timing.txt"), "w")
_PARAMS = {}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def run_shape(name, n, limbs, bits, base, d, c, T):
    key = (n, limbs, bits, base, d)
    if key not in _PARAMS:
        p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
        sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
        us = mx.GpuDCRTPolyUniformSampler()
        m = d * p.modulus_digits()
        ws = [us.sample_uniform(p, d, m, mx.DistType.FinRingDist()) for _ in range(4)]
        _PARAMS[key] = (p, sampler, sampler.trapdoor(p, d), lookup.LutShared(p, os.urandom(32), 3, *ws))
    p, sampler, (td, A), sh = _PARAMS[key]
    Q = p.modulus()
    rows = [(t, int.from_bytes(os.urandom(80), "little") % Q) for t in range(T)]
    k, m = p.modulus_digits(), d * p.modulus_digits()
    chunk = (min(k - 1, m - c), c)  # across a tower boundary (d = 2: and a source row)
    draws = [os.urandom(32) for _ in range(3 * T)]
    seeds = [tuple(mx.GpuRngSeed.from_bytes(draws[3 * j + i]) for i in range(3)) for j in range(T)]

    def loop():
        return [lookup.build_lut_preimage_target_chunk(sh, i, y, *chunk) for i, y in rows]

    def call():
        return lookup.lut_preimage_target_chunks(sh, rows, chunk)

    def loop_pre():
        return sampler.preimage_many_abi(p, td, A, loop(), _seeds=seeds)

    def call_pre():
        return [x for _, x in lookup.sample_lut_preimages(sh, sampler, td, A, rows, chunk, _seeds=seeds)]

    legs = [("loop", loop), ("call", call), ("loop+pre", loop_pre), ("call+pre", call_pre)]
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m = {d * p.modulus_digits()}; {T} rows, chunk of {c} columns at {chunk[0]}")
    got = {nm: fn() for nm, fn in legs}
    assert all(x == y for x, y in zip(got["loop"], got["call"])), "the one call differs from the literal loop"
    assert all(x == y for x, y in zip(got["loop+pre"], got["call+pre"])), "the preimages differ"
    assert all(A * x == t for x, t in zip(got["call+pre"], got["call"]))
    say("outputs: call == loop (gpu_matrix_equal), the preimages of both agree for the same seeds; A x == target")
    del got
    ctx = p.ctx()
    for _ in range(WARMUP):
        for _, fn in legs:
            fn()
    dev, wall, launches = collections.defaultdict(list), collections.defaultdict(list), {}
    for _ in range(REPS):
        for nm, fn in legs:  # the legs alternate
            mx.gpu_device_sync()
            c0 = lib.gpupoly_launch_count()
            t0 = time.perf_counter()
            ctx.timer_mark(0)
            out = fn()
            ctx.timer_mark(1)
            mx.gpu_device_sync()
            wall[nm].append((time.perf_counter() - t0) * 1e3)
            dev[nm].append(ctx.timer_elapsed(0, 1))
            launches[nm] = lib.gpupoly_launch_count() - c0
            del out
    for nm, _ in legs:
        say(f"{nm:9s} device events median {statistics.median(dev[nm]):.3f} ms (min {min(dev[nm]):.3f}, max {max(dev[nm]):.3f}, p90 {pct(dev[nm], 0.9):.3f}), "
            f"host until idle median {statistics.median(wall[nm]):.3f} ms (min {min(wall[nm]):.3f}, max {max(wall[nm]):.3f}, p90 {pct(wall[nm], 0.9):.3f}), "
            f"{launches[nm]} launches per call")
    for nm, fn in legs[:2]:
        mx.gpu_device_sync()
        _ffi.trace_begin()
        fn()
        mx.gpu_device_sync()
        per = collections.OrderedDict()
        for rec in _ffi.trace_end():
            e = per.setdefault(rec["kernel"].split("<")[0].strip("( "), [0, 0.0])
            e[0] += 1
            e[1] += rec["ms"]
        say(f"-- launch trace, {nm} leg ({sum(v[0] for v in per.values())} traced launches and copies, "
            f"{sum(v[1] for v in per.values()):.3f} ms summed over streams):")
        for k, (cnt, ms) in per.items():
            say(f"   {cnt:4d} x {k:48s} {ms:8.3f} ms")
    med = {nm: statistics.median(wall[nm]) for nm, _ in legs}
    spread = {nm: max(wall[nm]) - min(wall[nm]) for nm, _ in legs}
    say(f"host until idle: loop / call = {med['loop'] / med['call']:.2f} (spread: loop {spread['loop']:.3f} ms, call {spread['call']:.3f} ms); "
        f"loop+pre / call+pre = {med['loop+pre'] / med['call+pre']:.2f} "
        f"(spread: loop+pre {spread['loop+pre']:.3f} ms, call+pre {spread['call+pre']:.3f} ms)")
    slower = [nm for nm, ref in (("call", "loop"), ("call+pre", "loop+pre")) if med[nm] > med[ref] + max(spread[nm], spread[ref])]
    say("the one call is " + ("SLOWER than the loop beyond the spread in: " + ", ".join(slower) if slower else "not slower than the loop in either pair"))


for shape in SHAPES:
    run_shape(*shape)
OUT.close()
