"""The BGG+ poly-encoding vectors of S slots and P inputs (tools/README.md), two ways in one process:
  per-slot  `sample_poly_encoding_vectors_literal`: the reference's slot loop (src/bgg/sampler_gpu.rs:110-160) through the
            older entries - per slot s S_slot, a Gaussian 1 x P m sample, from_poly_vec_row, t A_all, t G against a filled
            gadget, tensor, sub, add and P slice_columns
  one call  T = (s [S_0 | S_1 | ...]) viewed S x d, then ONE gpupoly_matrix_bgg_encode_slots call
on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, P = 4, 16 and 64 slots;
  n = 2^14, 8 x 24 bits, base 2^12, d = 1, P = 8, 16 slots.
Both legs start from the masks, public keys and plaintexts resident on the device and end with the vectors resident on the
device (the reference's compact-byte hops on either side are left out of BOTH legs), under the same seeds; their outputs are
compared first (`gpu_matrix_equal`).  Then the legs alternate; every leg is bracketed by device events on the context's
stream and by the host clock until the device is idle; median and the 10th..90th percentile of REPS (9) after a warm-up,
kernel launches per call from gpupoly_launch_count, copies from one traced call.  The one call is said to be faster only when
the loop's p10 exceeds its p90, and slower only the other way round; anything else is parity within the spread.  One traced
call then gives the main kernel's own time against its algorithmic bytes - the errors read and the outputs written once,
every public key, the secrets and the plaintexts read once - next to gpupoly_matrix_fill_zero of an S x P m matrix (device
events around 20 fills), the bytes of the outputs written once.  Output goes to stdout and to
profiles/bgg_encode_timing.txt (or the path given as the first argument); a second argument picks shapes by index ("2" or
"0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, bgg  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "9")), 2
SIGMA = 4.578
SHAPES = [
    # name, n, limbs, bits, base, d, inputs P, slots
    ("m4 (u64), 16 slots", 256, 12, 51, 17, 2, 4, 16),
    ("m4 (u64), 64 slots", 256, 12, 51, 17, 2, 4, 64),
    ("n16384 (u32), 16 slots", 16384, 8, 24, 12, 1, 8, 16),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgg_encode_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def traced(fn):
    mx.gpu_device_sync()
    _ffi.trace_begin()
    out = fn()
    events = _ffi.trace_end()
    del out
    return events


def run_shape(name, n, limbs, bits, base, d, P, S):
    key = (n, limbs, bits, base)
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    M = mx.GpuDCRTPolyMatrix
    uni = mx.GpuDCRTPolyUniformSampler()
    rand = lambda rows, cols: uni.sample_uniform(p, rows, cols, mx.DistType.FinRingDist())  # noqa: E731
    m = d * p.modulus_digits()
    keys = [rand(d, m) for _ in range(P)]
    all_keys = keys[0].concat_columns(keys[1:])
    gadget = M.gadget_matrix(p, d)
    sampler = bgg.BGGPolyEncodingSampler(p, [uni.sample_poly(p, mx.DistType.TernaryDist()) for _ in range(d)], SIGMA)
    masks = sampler.sample_slot_secret_mats(p, S)
    mask_list = [masks.slice_columns(s * d, (s + 1) * d) for s in range(S)]
    pt = rand(S, P - 1)
    pt_rows = [[pt.entry(s, i) for s in range(S)] for i in range(P - 1)]
    seeds = [mx.GpuRngSeed.from_bytes(os.urandom(32)) for _ in range(S)]

    def per_slot():
        return bgg.sample_poly_encoding_vectors_literal(p, sampler.secret_vec, all_keys, gadget, pt_rows, mask_list, S, P, m, SIGMA, _seeds=seeds)

    def one_call():
        return M.bgg_encode_slots(sampler.slot_secrets(p, masks, S), keys, pt, SIGMA, seeds)

    legs = [("per-slot", per_slot), ("one call", one_call)]
    poly = limbs * n * p.ctx().word_bytes()
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m = {m}, P = {P}; {S} slots, sigma {SIGMA}")
    loop, one = per_slot(), one_call()
    assert all(one[i].row_view(s, s + 1) == loop[i][s] for i in range(P) for s in range(S)), "the one call differs from the per-slot loop"
    say("outputs: one call == per-slot loop (gpu_matrix_equal), every input and slot")
    del loop, one
    algo = (2 * S * P * m + P * d * m + S * d + S * (P - 1)) * poly
    say(f"byte model: the main kernel's algorithmic bytes, (2 S P m + P d m + S d + S (P - 1)) polynomials: {algo / 1e6:.1f} MB")
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
    copies = {nm: len([e for e in traced(fn) if not e["threads"]]) for nm, fn in legs}
    for nm, _ in legs:
        say(f"{nm:8s} device events median {statistics.median(dev[nm]):.3f} ms (p10 {pct(dev[nm], 0.1):.3f}, p90 {pct(dev[nm], 0.9):.3f}), "
            f"host until idle median {statistics.median(wall[nm]):.3f} ms (p10 {pct(wall[nm], 0.1):.3f}, p90 {pct(wall[nm], 0.9):.3f}), "
            f"{launches[nm]} kernel launches and {copies[nm]} copies per call")
    for clock, series in (("device events", dev), ("host until idle", wall)):
        ratio = statistics.median(series["per-slot"]) / statistics.median(series["one call"])
        if pct(series["per-slot"], 0.1) > pct(series["one call"], 0.9):
            verdict = "FASTER (the loop's p10 exceeds the one call's p90)"
        elif pct(series["one call"], 0.1) > pct(series["per-slot"], 0.9):
            verdict = "SLOWER (its p10 exceeds the loop's p90)"
        else:
            verdict = "at PARITY within the spread"
        say(f"{clock}: per-slot / one call = {ratio:.2f}; the one call is {verdict}")
    # the main kernel alone against its algorithmic bytes, next to a fill_zero of the same output
    events = traced(one_call)
    for e in events:
        say(f"    one call: {e['kernel'][:90]:90s} {e['blocks']:>8d} x {e['threads']:<4d} {e['ms']:.4f} ms")
    main = [e for e in events if "bgg_encode_kernel" in e["kernel"]]
    ms = sum(e["ms"] for e in main)  # one launch per group of slots
    say(f"main kernel: {len(main)} launch(es), {ms:.4f} ms: {algo / 1e9 / (ms / 1e3):.0f} GB/s of algorithmic bytes (grid {main[0]['blocks']} blocks x {main[0]['threads']} threads)")
    sink = M(p, S, P * m, limbs - 1, True)
    fills = []
    for _ in range(1 + 5):  # the first round warms up; 20 fills between two device events
        mx.gpu_device_sync()
        ctx.timer_mark(0)
        for _ in range(20):
            lib.gpupoly_matrix_fill_zero(sink.raw)
        ctx.timer_mark(1)
        mx.gpu_device_sync()
        fills.append(ctx.timer_elapsed(0, 1) / 20)
    fill_ms = statistics.median(fills[1:])
    say(f"fill_zero of the same S x P m output: {fill_ms:.4f} ms: {S * P * m * poly / 1e9 / (fill_ms / 1e3):.0f} GB/s of its {S * P * m * poly / 1e6:.1f} MB")


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
