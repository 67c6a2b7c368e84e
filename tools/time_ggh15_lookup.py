"""The GGH15 online public lookup for S slots of one gate over the whole output width (tools/README.md), four ways in one
process:
  literal   `build_public_lookup_output_chunk` slot by slot and chunk by chunk, then concat_columns: the reference's sequence
            (src/lookup/ggh15/encoding.rs:172-300) through the older entries
  mul_sum   the same per-slot, per-chunk sequence with the five adds of a chunk fused: the products
            P rhs as the reference forms them, then two gpupoly_matrix_mul_sum calls written into the slot's output in place
  batched   `public_lookup_slots`: stage 1 (six stacked products) once, then one gpupoly_matrix_ggh15_lookup call per chunk
  stage 2   the per-chunk calls of `batched` alone, the stage-1 products given
on the shapes
  n = 256, 12 x 51 bits, base 2^17, d = 2, chunk width 4, 16 and 64 slots;
  n = 2^14, 8 x 24 bits, base 2^12, d = 1, chunk width 18 (one chunk: m_g = 16), 16 slots.
The operands are uniform random (the formula needs no real preimages); the legs' outputs are compared first
(`gpu_matrix_equal`).  Then the legs alternate; every leg is bracketed by device events on the context's stream and by the
host clock until the device is idle; median and the 10th..90th percentile of REPS (9) after a warm-up, launches per call
from gpupoly_launch_count.  A per-slot leg is called slower only when its p10 exceeds the batched call's p90 (section 5j's
rule).  Next to the timings the byte model: stage 1 reads each of the five preimages and G^-1(U_g) once per call where the
per-slot sequence reads them once per slot and chunk; stage 2's floor is the bytes of [V_s; K_s] plus the outputs.
Output goes to stdout and to profiles/ggh15_lookup_timing.txt (or the path given as the first argument); a second argument
picks shapes by index ("2" or "0,1")."""
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi, ggh15_eval  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "9")), 2
SHAPES = [
    # name, n, limbs, bits, base, d, chunk width, slots
    ("m4 (u64), 16 slots", 256, 12, 51, 17, 2, 4, 16),
    ("m4 (u64), 64 slots", 256, 12, 51, 17, 2, 4, 64),
    ("n16384 (u32), 16 slots", 16384, 8, 24, 12, 1, 18, 16),
]
LUT_ROWS = 8
lib = _ffi.lib()
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ggh15_lookup_timing.txt"), "w")
_PARAMS = {}


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def mul_sum_slot(sh, c_b0, c_in, x, chunks):
    """the literal sequence of one slot with the adds of every chunk fused, each chunk written into its columns of the output"""
    M, p, d, m_g = mx.GpuDCRTPolyMatrix, sh.params, sh.d, sh.m_g
    k, y = sh.get(x.const_coeff_u64())
    gy = M.gadget_matrix(p, d) * mx.GpuDCRTPoly.from_elem_to_constant(p, y)
    out = M(p, c_b0.nrow, m_g, c_b0.level, True)
    for c0, cl in chunks:
        gy_mid = sh.preimage_gate2_gy * gy.slice_columns(c0, c0 + cl).decompose()
        v = sh.sampler().sample_hash_decomposed_columns(p, sh.hash_key, sh.v_tag(k), d, m_g, c0, cl, mx.DistType.FinRingDist())
        v_mid, vx_mid = sh.preimage_gate2_v * v, sh.preimage_gate2_vx * (v * x)
        in_b0 = sh.preimage_gate1 * sh.lut_preimage_chunk(k, c0, cl)
        lhss, rhss = [c_b0, c_b0, c_b0, c_b0], [sh.preimage_gate2_identity.slice_columns(c0, c0 + cl), gy_mid, v_mid, vx_mid]
        for i0, il in sh.column_chunks():
            u_dec = sh.sampler().sample_hash_decomposed_columns(p, sh.hash_key, sh.u_g_tag(), d, m_g, i0, il, mx.DistType.FinRingDist())
            lhss.append(c_in * u_dec)
            rhss.append(v.slice(i0, i0 + il, 0, cl))
        M.mul_sum(lhss, rhss, out=out, dst_col=c0)
        M.mul_sum([c_b0], [in_b0], addend=out, negate=True, out=out, dst_col=c0)
    return out


def run_shape(name, n, limbs, bits, base, d, width, S):
    key = (n, limbs, bits, base)
    if key not in _PARAMS:
        _PARAMS[key] = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    p = _PARAMS[key]
    uni = mx.GpuDCRTPolyUniformSampler()
    rand = lambda rows, cols: uni.sample_uniform(p, rows, cols, mx.DistType.FinRingDist())  # noqa: E731
    m_g, w = d * p.modulus_digits(), d * (p.modulus_digits() + 2)
    lut = {x: (x, 1000003 * x + 17) for x in range(LUT_ROWS)}
    sh = ggh15_eval.PublicLookupShared(p, os.urandom(32), 7, 3, d, rand(w, w), *[rand(w, m_g) for _ in range(4)], lut,
                                       {x: rand(w, m_g) for x in range(LUT_ROWS)}, chunk_width=min(width, m_g))
    xs = [mx.GpuDCRTPoly.from_usize_to_constant(p, (5 * s + 1) % LUT_ROWS) for s in range(S)]
    b0s, cins = [rand(1, w) for _ in range(S)], [rand(1, m_g) for _ in range(S)]
    rows = [sh.get(x.const_coeff_u64()) for x in xs]
    chunks = sh.column_chunks()
    mids = ggh15_eval.public_lookup_stage1(sh, b0s, cins)

    def literal():
        return [ggh15_eval._literal_slot(sh, b0s[s], cins[s], xs[s], chunks) for s in range(S)]

    def mul_sum():
        return [mul_sum_slot(sh, b0s[s], cins[s], xs[s], chunks) for s in range(S)]

    def batched():
        return [vec for vec, _ in ggh15_eval.public_lookup_slots(sh, b0s, cins, xs)]

    def stage2():
        return [ggh15_eval.public_lookup_stage2(sh, mids, rows, xs, chunk) for chunk in chunks]

    legs = [("literal", literal), ("mul_sum", mul_sum), ("batched", batched), ("stage 2", stage2)]
    wb = p.ctx().word_bytes()
    poly = limbs * n * wb
    say(f"== {name}: n = {n}, {limbs} x {bits} bits, base 2^{base}, d = {d}, m_g = {m_g}, w = {w}; {S} slots, {len(chunks)} chunks of {chunks[0][1]} columns")
    got = {nm: fn() for nm, fn in legs[:3]}
    assert all(a == b for a, b in zip(got["literal"], got["batched"])), "the batched lookup differs from the literal loop"
    assert all(a == b for a, b in zip(got["literal"], got["mul_sum"])), "the mul_sum form differs from the literal loop"
    say("outputs: batched == literal == mul_sum form (gpu_matrix_equal), every slot")
    del got
    p_bytes = (4 * w * m_g + w * w + m_g * m_g) * poly
    say(f"byte model: the five preimages and G^-1(U_g) are {p_bytes / 1e6:.1f} MB; stage 1 reads them once per call, the per-slot sequence "
        f"once per slot and chunk ({S * len(chunks)} times: {S * len(chunks) * p_bytes / 1e9:.2f} GB); stage 2's floor, [V_s; K_s] plus the "
        f"outputs over all chunks: {S * (m_g * (m_g + w) + m_g) * poly / 1e6:.1f} MB")
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
        for ref in ("literal", "mul_sum"):
            ratio = statistics.median(series[ref]) / statistics.median(series["batched"])
            faster = pct(series[ref], 0.1) > pct(series["batched"], 0.9)
            say(f"{clock}: {ref} / batched = {ratio:.2f}; batched is " + ("FASTER (the sequence's p10 exceeds the batched call's p90)" if faster
                                                                          else "NOT faster beyond the spread"))


for index in ([int(i) for i in sys.argv[2].split(",")] if len(sys.argv) > 2 else range(len(SHAPES))):
    run_shape(*SHAPES[index])
OUT.close()
