"""The slot-transfer online evaluation over the whole output width (tools/README.md), two ways in one process:
  per-slot  `output_slot` / `slot_reduce_output_slot` destination by destination: the reference's functions
            (src/slot_transfer/bgg_poly_encoding.rs:119-386) through the older entries, one product per stored chunk, the hash
            sample and its decomposition per destination, c_b0 P0_src per destination and source
  one call  `slot_transfer_slots` / `slot_reduce_slots`: c_b0 P0_src once per distinct source, the full-width outputs allocated
            once, one gpupoly_matrix_slot_transfer_eval call per chunk
on the shapes
  slot_transfer, n = 256, 12 x 51 bits, base 2^17, d = 2, 18 chunks of 4 columns, 16 and 64 destination slots;
  slot_transfer, n = 2^14, 8 x 24 bits, base 2^12, d = 1, one chunk (m_g = 16), 16 destination slots;
  slot_reduce, the first ring, 8 inputs x 8 slots.
The operands are uniform random (the formula needs no real preimages; w0 = d (digits + 2), w1 = 2 d (digits + 2), the
trapdoors' widths); the legs' outputs are compared first (`gpu_matrix_equal`).  Then the legs alternate; every leg is bracketed
by device events on the context's stream and by the host clock until the device is idle; median and the 10th..90th percentile
of REPS (9) after a warm-up, launches per call from gpupoly_launch_count.  The one call is said to be faster only when the
loop's p10 exceeds its p90, and slower only the other way round; anything else is parity within the spread.  One traced call
then gives the launch census and the main kernel's own time over all chunks against its algorithmic bytes (MXX_TRACE_BYTES).
Output goes to stdout and to profiles/slot_transfer_eval_timing.txt (or the path given as the first argument); a second
argument picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, slot_transfer as ST  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "9")), 2
SHAPES = [
    # name, gate, n, limbs, bits, base, d, chunk width, destinations, slots per input (reduce)
    ("slot_transfer m4 (u64), 16 slots", "transfer", 256, 12, 51, 17, 2, 4, 16, 0),
    ("slot_transfer m4 (u64), 64 slots", "transfer", 256, 12, 51, 17, 2, 4, 64, 0),
    ("slot_transfer n16384 (u32), 16 slots", "transfer", 16384, 8, 24, 12, 1, 16, 16, 0),
    ("slot_reduce m4 (u64), 8 inputs x 8 slots", "reduce", 256, 12, 51, 17, 2, 4, 8, 8),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slot_transfer_eval_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def run_shape(name, gate, n, limbs, bits, base, d, width, S, num_slots):
    key = (n, limbs, bits, base)
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    uni = mx.GpuDCRTPolyUniformSampler()
    rand = lambda rows, cols: uni.sample_uniform(p, rows, cols, mx.DistType.FinRingDist())  # noqa: E731
    k = p.modulus_digits()
    m_g, w0, w1, r = d * k, d * (k + 2), 2 * d * (k + 2), 1
    nsrc = num_slots if gate == "reduce" else min(S, 16)
    chunks = [(c0, min(width, m_g - c0)) for c0 in range(0, m_g, width)]
    # the stored preimages as the evaluator reads them: P0 whole, P1 and Pg chunk by chunk
    p0 = [rand(w0, w1) for _ in range(nsrc)]
    p1 = {(s, c0): rand(w1, cl) for s in range(S) for c0, cl in chunks}
    pg = {(s, c0): rand(w0, cl) for s in range(S) for c0, cl in chunks}
    shared = ST.SlotEvalShared(p, os.urandom(32), d, rand(r, w0), lambda slot: [p0[slot]], lambda slot, c0, cl: p1[(slot, c0)],
                               lambda gate_id, slot, c0, cl: pg[(slot, c0)])
    assert shared.column_chunks(width) == chunks
    Q = p.modulus()
    if gate == "transfer":
        src_slots = [((5 * t + 2) % nsrc if t % 4 else (t // 4) % nsrc, None if t % 2 else 3) for t in range(S)]  # sources repeat
        vectors = [rand(r, m_g) for _ in range(nsrc)]
        mus = [(12345 + 7 * s) * (Q // 3) % Q for s in range(nsrc)]
        plaintexts = [mx.GpuDCRTPoly.from_biguint_to_constant(p, mu) for mu in mus]

        def per_slot():
            return [ST.output_slot(shared, 7, vectors, plaintexts, src_slots, t, width)[0] for t in range(S)]

        def one_call():
            return ST.slot_transfer_slots(shared, 7, vectors, mus, src_slots, width)
        terms = 1
    else:
        inputs = [[rand(r, m_g) for _ in range(num_slots)] for _ in range(S)]
        mus = [[(12345 + 7 * s + 31 * t) * (Q // 3) % Q for s in range(num_slots)] for t in range(S)]
        plaintexts = [[mx.GpuDCRTPoly.from_biguint_to_constant(p, mu) for mu in row] for row in mus]

        def per_slot():
            return [ST.slot_reduce_output_slot(shared, 7, inputs, plaintexts, t, num_slots, width)[0] for t in range(S)]

        def one_call():
            return ST.slot_reduce_slots(shared, 7, inputs, mus, num_slots, width)
        terms = num_slots

    legs = [("per-slot", per_slot), ("one call", one_call)]
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m_g = {m_g}, w0 = {w0}, w1 = {w1}, r = {r}; {S} destinations, "
        f"{terms} term(s) each, {len(chunks)} chunks of {chunks[0][1]} columns")
    got = {nm: fn() for nm, fn in legs}
    assert all(x == y for x, y in zip(got["per-slot"], got["one call"])), "the one-call evaluation differs from the per-slot functions"
    say("outputs: one call == per-slot functions (gpu_matrix_equal), every destination")
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
    # the launch census of one call, and the two new kernels alone against their algorithmic bytes
    mx.gpu_device_sync()
    _ffi.trace_begin()
    one_call()
    events = _ffi.trace_end()
    say(f"one call: {len([e for e in events if e['threads']])} kernels and {len([e for e in events if not e['threads']])} copies over "
        f"{len(chunks)} chunks and stage 1")
    for label, pick in (("pre-pass", "slot_eval_lhs_kernel"), ("main kernel", "slot_eval_kernel")):
        mine = [e for e in events if pick in e["kernel"]]
        ms, nbytes = sum(e["ms"] for e in mine), sum(e["bytes"] for e in mine)
        say(f"{label}: {len(mine)} launches, {ms:.3f} ms in all, {nbytes / 1e6:.1f} MB of algorithmic bytes: {nbytes / 1e9 / (ms / 1e3):.0f} GB/s "
            f"(grid {mine[0]['blocks']} blocks x {mine[0]['threads']} threads)")


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
