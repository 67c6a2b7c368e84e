"""The preimage targets of T public-parameter indices x all column parts of the Wee25 commitment (tools/README.md), three ways
in one process:
  loop      `t_top_target_block` target by target: the reference's sequence through the older entries (tag hash, sample, zero
            fills, entry writes, decompositions, concat_rows, gadget product, product, subtraction)
  two-step  the composition the fused kernel replaces, from the instrument's pieces: the stacked block sample, ONE product of
            the stacked W against T_bottom into scratch, ONE negation pass over that scratch.  The pass reads and writes every
            target word once like a negate-and-scatter kernel would, but adds no constant and scatters nothing; the T x P output
            matrices such a pass would fill are made (and left unwritten), as the call makes its own: a LOWER bound on any
            two-step form (the scratch's blocks are compared with the call's where no constant hits)
  call      one `gpupoly_matrix_wee25_targets` call (`t_top_target_blocks`)
and the first and the last followed by `preimage_many_abi` over the targets (loop+pre, call+pre) - for as many of the indices
as keep one leg's preimages (m_b x m_b each, m_b / s times a target) under 24 GB -, on the shapes
  n = 256, 12 x 51 bits, base 2^17, secret size 1 and 2, 16 indices x all 72 parts;
  n = 2^14, 8 x 24 bits, base 2^12, secret size 1, 3 indices x all 32 parts (96 targets of 9.4 MB: 0.9 GB of outputs).
The targets of the legs are compared first (`gpu_matrix_equal`) and B x == target is checked.  Then the legs alternate; every
leg is bracketed by device events on the context's stream and by the host clock until the device is idle; median and the
10th..90th percentile of REPS (11) after a warm-up, launches per call from gpupoly_launch_count, and the launch trace of the
three target legs summed per kernel.  Output goes to stdout and to profiles/wee25_targets_timing.txt (or the path given as the
first argument); a second argument picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402
from mxx_amd.commit import Wee25Commit  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "11")), 2
SHAPES = [
    # name, n, limbs, bits, base, secret size, indices
    ("m4 (u64), s = 1", 256, 12, 51, 17, 1, 16),
    ("m4 (u64), s = 2", 256, 12, 51, 17, 2, 16),
    ("n16384 (u32), s = 1", 16384, 8, 24, 12, 1, 3),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wee25_targets_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def run_shape(name, n, limbs, bits, base, s, T):
    key = (n, limbs, bits, base)
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    w = Wee25Commit(p, s, 2, 4.578)
    w.hash_key = os.urandom(32)
    sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, B = sampler.trapdoor(p, s)
    t_bottom = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, w.m_b, w.j_2m_cols, mx.DistType.GaussDist(4.578))
    parts = [t_bottom.slice_columns(q * w.m_b, (q + 1) * w.m_b) for q in range(w.nparts)]
    first = w.m_g - 1  # a consecutive run across a block group's end
    idxs = list(range(first, first + T))
    count = T * w.nparts
    draws = [os.urandom(32) for _ in range(3 * count)]
    seeds = [tuple(mx.GpuRngSeed.from_bytes(draws[3 * j + i]) for i in range(3)) for j in range(count)]
    hs = w.sampler()
    pre_bytes = w.nparts * w.m_b * w.m_b * limbs * n * p.ctx().word_bytes()  # the preimages of one index
    pre_T = max(1, min(T, int(24e9 // pre_bytes)))
    pre_idxs, seeds = idxs[:pre_T], seeds[:pre_T * w.nparts]

    def loop(which=idxs):
        return [w.t_top_target_block(i, q * w.m_b, parts[q]) for i in which for q in range(w.nparts)]

    def two_step():
        stack = hs.sample_hash_stacked(p, w.hash_key, w.tags(first, T), s, w.m_b, mx.DistType.FinRingDist())
        outs = [mx.GpuDCRTPolyMatrix(p, s, w.m_b, t_bottom.level, True) for _ in range(count)]
        return -(stack.reshape_view(T * s, w.m_b) * t_bottom), outs

    def call():
        return [t for row in w.t_top_target_blocks(t_bottom, idxs) for t in row]

    def loop_pre():
        return sampler.preimage_many_abi(p, td, B, loop(pre_idxs), _seeds=seeds)

    def call_pre():
        return [x for _, x in w.sample_t_top_preimages(sampler, td, B, t_bottom, pre_idxs, _seeds=seeds).values()]

    legs = [("loop", loop), ("two-step", two_step), ("call", call), ("loop+pre", loop_pre), ("call+pre", call_pre)]
    pairs = (("call", "loop"), ("call", "two-step"), ("call+pre", "loop+pre"))
    mb = count * s * w.m_b * limbs * n * p.ctx().word_bytes() / 1e6
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, secret size {s}, k = {w.log_base_q}, m_b = {w.m_b}; {T} indices from "
        f"{first} x {w.nparts} parts = {count} targets, {mb:.0f} MB of outputs; the +pre legs take the first {pre_T} indices ({pre_T * w.nparts} preimages)")
    got = {nm: fn() for nm, fn in legs}
    assert all(a == b for a, b in zip(got["loop"], got["call"])), "the one call differs from the literal loop"
    assert all(a == b for a, b in zip(got["loop+pre"], got["call+pre"])), "the preimages differ"
    assert all(B * x == t for x, t in zip(got["call+pre"][::7], got["call"][::7]))
    last = w.nparts - 1  # no index of the run hits the last part
    assert all(w.j_2m_hit(i)[2] + w.log_base_q <= last * w.m_b for i in idxs)
    for t in range(T):
        assert got["two-step"][0].slice(t * s, (t + 1) * s, last * w.m_b, (last + 1) * w.m_b) == got["call"][t * w.nparts + last]
    say("outputs: call == loop (gpu_matrix_equal), the preimages of both agree for the same seeds; B x == target; the two-step "
        "scratch == the call's targets where no constant hits")
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
        say(f"{nm:9s} device events median {statistics.median(dev[nm]):.3f} ms (p10 {pct(dev[nm], 0.1):.3f}, p90 {pct(dev[nm], 0.9):.3f}), "
            f"host until idle median {statistics.median(wall[nm]):.3f} ms (p10 {pct(wall[nm], 0.1):.3f}, p90 {pct(wall[nm], 0.9):.3f}), "
            f"{launches[nm]} launches per call")
    for nm, fn in legs[:3]:
        mx.gpu_device_sync()
        _ffi.trace_begin()
        out = fn()
        mx.gpu_device_sync()
        del out
        per = collections.OrderedDict()
        for rec in _ffi.trace_end():
            e = per.setdefault(rec["kernel"].split("<")[0].strip("( "), [0, 0.0])
            e[0] += 1
            e[1] += rec["ms"]
        say(f"-- launch trace, {nm} leg ({sum(v[0] for v in per.values())} traced launches and copies, "
            f"{sum(v[1] for v in per.values()):.3f} ms summed over streams):")
        for kn, (cnt, ms) in per.items():
            say(f"   {cnt:5d} x {kn:48s} {ms:9.3f} ms")
    for clock, series in (("device events", dev), ("host until idle", wall)):
        med = {nm: statistics.median(series[nm]) for nm, _ in legs}
        spread = {nm: pct(series[nm], 0.9) - pct(series[nm], 0.1) for nm, _ in legs}
        say(f"{clock}: " + "; ".join(f"{ref} / {nm} = {med[ref] / med[nm]:.2f} (p10..p90 spread: {ref} {spread[ref]:.3f} ms, {nm} {spread[nm]:.3f} ms)"
                                     for nm, ref in pairs))
        slower = [f"{nm} vs {ref}" for nm, ref in pairs if med[nm] > med[ref] + max(spread[nm], spread[ref])]
        faster = med["call"] + max(spread["call"], spread["two-step"]) < med["two-step"]
        say(f"{clock}: the call is " + ("SLOWER beyond the spread in: " + ", ".join(slower) if slower else "not slower in any pair")
            + "; the fused launch is " + ("faster than the two-step lower bound beyond the spread" if faster else "NOT faster than the two-step lower bound beyond the spread"))
    del t_bottom, parts


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
