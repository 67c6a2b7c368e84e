"""The LWE online public lookup for S slots of one gate over the whole output width (tools/README.md), two ways in one
process:
  per-slot  `public_lookup` slot by slot: per chunk one decomposed hash sample and one gpupoly_matrix_mul_sum written in
            place - the reference's slot loop (src/lookup/lwe/poly_encoding_gpu.rs:419-453) through the older entries
  one call  `public_lookup_slots`: the S full-width outputs allocated once, one gpupoly_matrix_lwe_lookup call per chunk
on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, 18 chunks of 4 columns, 16 and 64 slots;
  n = 2^14, 8 x 24 bits, base 2^12, d = 1, 18-column chunks (one chunk: m_g = 16), 16 slots.
The operands are uniform random (the formula needs no real preimages; w = d (digits + 2), the trapdoor's width); the legs'
outputs are compared first (`gpu_matrix_equal`).  Then the legs alternate; every leg is bracketed by device events on the
context's stream and by the host clock until the device is idle; median and the 10th..90th percentile of REPS (9) after a
warm-up, launches per call from gpupoly_launch_count.  The one call is said to be faster only when the loop's p10 exceeds
its p90, and slower only the other way round; anything else is parity within the spread.  One traced call then gives the
main kernel's own time over all chunks against its algorithmic bytes, ((w + m_g) c + r c + the left words r (w + m_g)) x
words per polynomial per slot and chunk.  Output goes to stdout and to profiles/lwe_lookup_timing.txt (or the path given as
the first argument); a second argument picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, lwe_lookup  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "9")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, chunk width, slots
    ("m4 (u64), 16 slots", 256, 12, 51, 17, 2, 4, 16),
    ("m4 (u64), 64 slots", 256, 12, 51, 17, 2, 4, 64),
    ("n16384 (u32), 16 slots", 16384, 8, 24, 12, 1, 18, 16),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lwe_lookup_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def run_shape(name, n, limbs, bits, base, d, width, S):
    key = (n, limbs, bits, base)
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    uni = mx.GpuDCRTPolyUniformSampler()
    rand = lambda rows, cols: uni.sample_uniform(p, rows, cols, mx.DistType.FinRingDist())  # noqa: E731
    m_g, w, r = d * p.modulus_digits(), d * (p.modulus_digits() + 2), 1
    hash_key = os.urandom(32)
    a = rand(d, m_g)
    shareds = [lwe_lookup.LweShared(p, hash_key, 7, 3, s, a, a) for s in range(S)]
    entries = [(5 * s + 1) % 8 for s in range(S)]
    chunks = [(c0, min(width, m_g - c0)) for c0 in range(0, m_g, width)]
    c_bs, c_zs = [rand(r, w) for _ in range(S)], [rand(r, m_g) for _ in range(S)]
    by_slot = [[rand(w, cl) for _, cl in chunks] for _ in range(S)]  # every slot its own stored K_high chunks

    def per_slot():
        return [lwe_lookup.public_lookup(shareds[s], c_bs[s], c_zs[s], by_slot[s], entries[s]) for s in range(S)]

    def one_call():
        return lwe_lookup.public_lookup_slots(shareds, c_bs, c_zs, by_slot, entries)

    legs = [("per-slot", per_slot), ("one call", one_call)]
    poly = limbs * n * p.ctx().word_bytes()
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m_g = {m_g}, w = {w}, r = {r}; {S} slots, {len(chunks)} chunks of "
        f"{chunks[0][1]} columns")
    got = {nm: fn() for nm, fn in legs}
    assert all(x == y for x, y in zip(got["per-slot"], got["one call"])), "the one-call lookup differs from the per-slot loop"
    say("outputs: one call == per-slot loop (gpu_matrix_equal), every slot")
    del got
    algo = sum(S * ((w + m_g) * cl + r * cl + r * (w + m_g)) for _, cl in chunks) * poly
    say(f"byte model: the main kernel's algorithmic bytes over all chunks, S ((w + m_g) c + r c + r (w + m_g)) words per polynomial: {algo / 1e6:.1f} MB")
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
        say(f"{nm:8s} device events median {statistics.median(dev[nm]):.3f} ms (p10 {pct(dev[nm], 0.1):.3f}, p90 {pct(dev[nm], 0.9):.3f}), "
            f"host until idle median {statistics.median(wall[nm]):.3f} ms (p10 {pct(wall[nm], 0.1):.3f}, p90 {pct(wall[nm], 0.9):.3f}), "
            f"{launches[nm]} kernel launches per call")
    for clock, series in (("device events", dev), ("host until idle", wall)):
        ratio = statistics.median(series["per-slot"]) / statistics.median(series["one call"])
        if pct(series["per-slot"], 0.1) > pct(series["one call"], 0.9):
            verdict = "FASTER (the loop's p10 exceeds the one call's p90)"
        elif pct(series["one call"], 0.1) > pct(series["per-slot"], 0.9):
            verdict = "SLOWER (its p10 exceeds the loop's p90)"
        else:
            verdict = "at PARITY within the spread"
        say(f"{clock}: per-slot / one call = {ratio:.2f}; the one call is {verdict}")
    # the main kernel alone: its traced time over the chunks of one call against the algorithmic bytes
    mx.gpu_device_sync()
    _ffi.trace_begin()
    one_call()
    events = _ffi.trace_end()
    main = [e for e in events if "lwe_lookup_kernel" in e["kernel"]]
    ms = sum(e["ms"] for e in main)
    say(f"main kernel: {len(main)} launches of {len([e for e in events if e['threads']])} kernels and {len([e for e in events if not e['threads']])} copies "
        f"in the one call, {ms:.3f} ms in all: {algo / 1e9 / (ms / 1e3):.0f} GB/s of algorithmic bytes "
        f"(grid {main[0]['blocks']} blocks x {main[0]['threads']} threads)")


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
