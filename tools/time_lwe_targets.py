"""The preimage targets of T LUT rows of one column chunk of the LWE public lookup (tools/README.md), two ways in one process:
  loop   `build_adjusted_target_chunk` row by row: the reference's sequence through the older entries (constant upload, gadget
         matrix times x, d x m subtraction, slices, mul_scalar, tag hash, decomposed window sample, product, subtractions)
  call   one `gpupoly_matrix_lwe_targets` call (`lwe_target_chunks`)
the same two followed by `preimage_many_abi` over the targets (loop+pre, call+pre), and the online side for one row over
every chunk: `public_lookup` (one mul_sum per chunk, written in place) against the plain-operator loop (two products, a sum
and a concatenation; "plain"), on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, c = 4, T = 16 and T = 64;   n = 2^14, 8 x 24 bits, base 2^12, d = 1, T = 16 with the
  whole width as one chunk (m = 16 there; a chunk is never wider than m, and its digit scratch makes two row groups).
The targets of both legs are compared first (`gpu_matrix_equal`), A x == target and the lookup relation are checked.  Then
the legs alternate; every leg is bracketed by device events on the context's stream and by the host clock until the device
is idle; median and the 10th..90th percentile of REPS (11) after a warm-up, launches per call from gpupoly_launch_count,
and the launch trace of both target legs summed per kernel.  Output goes to stdout and to profiles/lwe_targets_timing.txt
(or the path given as the first argument); a second argument picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, lwe_lookup  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "11")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, chunk columns, rows
    ("m4 (u64), T = 16", 256, 12, 51, 17, 2, 4, 16),
    ("m4 (u64), T = 64", 256, 12, 51, 17, 2, 4, 64),
    ("n16384 (u32), T = 16", 16384, 8, 24, 12, 1, 16, 16),
]
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lwe_targets_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def run_shape(name, n, limbs, bits, base, d, c, T):
    key = (n, limbs, bits, base, d)
    us = mx.GpuDCRTPolyUniformSampler()
    if key not in _PARAMS:
        p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
        sampler = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578)
        m = d * p.modulus_digits()
        hash_key = os.urandom(32)
        a_z = us.sample_uniform(p, d, m, mx.DistType.FinRingDist())
        a_lt = lwe_lookup.derive_a_lt_matrix(p, d, hash_key, 17, 2)
        _PARAMS[key] = (p, sampler, sampler.trapdoor(p, d), lwe_lookup.LweShared(p, hash_key, 17, 3, 2, a_z, a_lt))
    p, sampler, (td, A), sh = _PARAMS[key]
    Q = p.modulus()
    rows = [(3 * t + 1, t, int.from_bytes(os.urandom(80), "little") % Q) for t in range(T)]
    k, m = p.modulus_digits(), d * p.modulus_digits()
    assert 0 < c <= m, "a chunk is at most the matrix's width"
    chunk = (min(k - 1, m - c), c)  # across a tower boundary (d = 2: and a source row) where the width leaves room
    draws = [os.urandom(32) for _ in range(3 * T)]
    seeds = [tuple(mx.GpuRngSeed.from_bytes(draws[3 * j + i]) for i in range(3)) for j in range(T)]
    # the online side of row 0: K_high for every chunk, noise-free encodings
    chunks = [(c0, min(c, m - c0)) for c0 in range(0, m, c)]
    entry, x, y = rows[0]
    k_high = [lwe_lookup.sample_lwe_preimages(sh, sampler, td, A, rows[:1], ch)[0][1] for ch in chunks]
    G = mx.GpuDCRTPolyMatrix.gadget_matrix(p, d)
    s = us.sample_uniform(p, 1, d, mx.DistType.FinRingDist())
    c_b, c_z = s * A, s * (sh.a_z - G * mx.GpuDCRTPoly.from_usize_to_constant(p, x))

    def loop():
        return [lwe_lookup.build_adjusted_target_chunk(sh, *row, *chunk) for row in rows]

    def call():
        return lwe_lookup.lwe_target_chunks(sh, rows, chunk)

    def loop_pre():
        return sampler.preimage_many_abi(p, td, A, loop(), _seeds=seeds)

    def call_pre():
        return [kh for _, kh in lwe_lookup.sample_lwe_preimages(sh, sampler, td, A, rows, chunk, _seeds=seeds)]

    def plain():
        parts = [c_b * kh + c_z * lwe_lookup.derive_k_low_chunk(sh, entry, *ch) for kh, ch in zip(k_high, chunks)]
        return parts[0].concat_columns(parts[1:]) if len(parts) > 1 else parts[0]

    def lookup():
        return lwe_lookup.public_lookup(sh, c_b, c_z, k_high, entry)

    legs = [("loop", loop), ("call", call), ("loop+pre", loop_pre), ("call+pre", call_pre), ("plain", plain), ("lookup", lookup)]
    pairs = (("call", "loop"), ("call+pre", "loop+pre"), ("lookup", "plain"))
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m = {m}; {T} rows, chunk of {c} columns at {chunk[0]}; "
        f"online side: one row, {len(chunks)} chunks")
    got = {nm: fn() for nm, fn in legs}
    assert all(a == b for a, b in zip(got["loop"], got["call"])), "the one call differs from the literal loop"
    assert all(a == b for a, b in zip(got["loop+pre"], got["call+pre"])), "the preimages differ"
    assert all(A * kh == t for kh, t in zip(got["call+pre"], got["call"]))
    assert got["lookup"] == got["plain"] and got["lookup"] == s * (sh.a_lt - G * mx.GpuDCRTPoly.from_elem_to_constant(p, y))
    say("outputs: call == loop (gpu_matrix_equal), the preimages of both agree for the same seeds; A x == target; "
        "public_lookup == the plain-operator loop == s (A_lt - G o y)")
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
        for kn, (cnt, ms) in per.items():
            say(f"   {cnt:4d} x {kn:48s} {ms:8.3f} ms")
    med = {nm: statistics.median(wall[nm]) for nm, _ in legs}
    spread = {nm: pct(wall[nm], 0.9) - pct(wall[nm], 0.1) for nm, _ in legs}
    say("host until idle: " + "; ".join(f"{ref} / {nm} = {med[ref] / med[nm]:.2f} (p10..p90 spread: {ref} {spread[ref]:.3f} ms, {nm} {spread[nm]:.3f} ms)"
                                        for nm, ref in pairs))
    slower = [nm for nm, ref in pairs if med[nm] > med[ref] + max(spread[nm], spread[ref])]
    say("the new path is " + ("SLOWER than the old one beyond the spread in: " + ", ".join(slower) if slower else "not slower than the old one in any pair"))


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
