"""The message blocks of T LUT rows of the commitment-based public lookup (tools/README.md), two ways in one process:
  loop   `message_block_literal` row by row: the reference's sequence through the older entries (two tag hashes and samples, a
         gadget fill with its mul_scalar, a zero fill and a concatenation, the d x m_b * m_b x m_b product, a constant upload
         with its mul_scalar, the decomposition, the d x m_g * m_g x m_b product, three additions or subtractions)
  call   one `gpupoly_matrix_commit_lut_messages` call (`CommitMsgStream.message_blocks`)
on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, T = 16 and T = 64;   n = 2^14, 8 x 24 bits, base 2^12, d = 1, T = 16.
One gate whose LUT names row (x + 1) mod T, a uniform random matrix for the verifier (the formula needs no public parameters).
The blocks of both legs are compared first (`gpu_matrix_equal`).  Then the legs alternate; every leg is bracketed by device
events on the context's stream and by the host clock until the device is idle; median and the 10th..90th percentile of REPS
(11) after a warm-up, launches per call from gpupoly_launch_count, and the launch trace of both legs summed per kernel.  The
combine kernel's algorithmic bytes (what its launch states: the digits once per row tile, P_g once per column tile, R_t,
A_out's block and the outputs once) over its traced time stand next to `fill_zero` of the same T outputs, the plain write
rate of that many bytes in T launches.  Output goes to stdout and to profiles/commit_lut_timing.txt (or the path given as the
first argument); a second argument picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, commit_lookup  # noqa: E402
from mxx_amd.bgg import BggPublicKey  # noqa: E402
from mxx_amd.commit import Wee25Commit  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "11")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, rows
    ("m4 (u64), T = 16", 256, 12, 51, 17, 2, 16),
    ("m4 (u64), T = 64", 256, 12, 51, 17, 2, 64),
    ("n16384 (u32), T = 16", 16384, 8, 24, 12, 1, 16),
]
KERNEL = "commit_lut_combine_kernel"
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "commit_lut_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def run_shape(name, n, limbs, bits, base, d, T):
    key = (n, limbs, bits, base)
    us = mx.GpuDCRTPolyUniformSampler()
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    M = mx.GpuDCRTPolyMatrix
    commit = Wee25Commit(p, d, 2, 4.578)
    m_g, m_b = commit.m_g, commit.m_b
    hash_key = os.urandom(32)
    Q = p.modulus()
    uniform = lambda rows, cols: us.sample_uniform(p, rows, cols, mx.DistType.FinRingDist()).ensure_eval()  # noqa: E731
    lut = {x: ((x + 1) % T, int.from_bytes(os.urandom(80), "little") % Q) for x in range(T)}
    gate_states = [(7, 0, BggPublicKey(uniform(d, m_g), True), BggPublicKey(uniform(d, m_g), True))]
    b_1 = commit_lookup.derive_b_1_matrix(p, d, m_b, hash_key)
    padded = commit_lookup.compute_padded_len(2, T)
    slices = [uniform(m_b, m_b) for _ in range(padded)]
    whole = slices[0].concat_columns(slices[1:])  # the verifier of every position, made once: both legs take slices of it

    def verifier_of(positions):
        positions = list(positions)
        if positions == list(range(padded)):
            return whole
        return slices[positions[0]] if len(positions) == 1 else slices[positions[0]].concat_columns([slices[i] for i in positions[1:]])

    stream = commit_lookup.CommitMsgStream(p, commit, None, b_1, hash_key, {0: lut}, gate_states, verifier_of=verifier_of)
    assert stream.lut_vector_len == T and stream.padded_len == padded
    rows = range(padded) if padded == T else range(T)
    stream.gate_operands(0)  # A_out and the key sum are made once per stream, outside both legs' rows

    def loop():
        return stream.message_blocks_literal(rows)

    def call():
        return stream.message_blocks(rows)

    def zeros():
        return [M.zero(p, d, m_b) for _ in range(T)]

    legs = [("loop", loop), ("call", call), ("fill_zero", zeros)]
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m_g = {m_g}, m_b = {m_b}; {T} rows of one gate, "
        f"verifier of {padded} blocks")
    got = {nm: fn() for nm, fn in legs[:2]}
    assert len(got["call"]) == T and all(a == b for a, b in zip(got["loop"], got["call"])), "the one call differs from the literal loop"
    say("outputs: call == loop (gpu_matrix_equal) for every row")
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
    combine = []
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
            if KERNEL in rec["kernel"]:
                combine.append((rec["bytes"], rec["ms"]))
        say(f"-- launch trace, {nm} leg ({sum(v[0] for v in per.values())} traced launches and copies, "
            f"{sum(v[1] for v in per.values()):.3f} ms summed over streams):")
        for kn, (cnt, ms) in per.items():
            say(f"   {cnt:4d} x {kn:48s} {ms:8.3f} ms")
    nbytes, ms = sum(b for b, _ in combine), sum(t for _, t in combine)
    out_bytes = T * d * m_b * limbs * n * p.ctx().word_bytes()
    zero_ms = statistics.median(dev["fill_zero"])
    say(f"combine kernel: {len(combine)} launches (row groups), {nbytes / 1e9:.3f} GB algorithmic in {ms:.3f} ms = {nbytes / ms / 1e9:.2f} TB/s; "
        f"fill_zero of the same {T} outputs: {out_bytes / 1e9:.3f} GB in {zero_ms:.3f} ms = {out_bytes / zero_ms / 1e9:.2f} TB/s ({T} launches)")
    med = {nm: statistics.median(wall[nm]) for nm, _ in legs}
    spread = {nm: pct(wall[nm], 0.9) - pct(wall[nm], 0.1) for nm, _ in legs}
    say(f"host until idle: loop / call = {med['loop'] / med['call']:.2f} (p10..p90 spread: loop {spread['loop']:.3f} ms, call {spread['call']:.3f} ms)")
    slower = med["call"] > med["loop"] + max(spread["call"], spread["loop"])
    say("the new path is " + ("SLOWER than the old one beyond the spread" if slower else "not slower than the old one"))
    del stream, slices, whole


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
