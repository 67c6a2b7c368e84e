"""gpupoly_matrix_nested_rns_decompose (one call) against the host sequence a caller has today, and its main kernel's
store rate against gpupoly_matrix_fill_zero of the same output, in one process.

Host leg: the mirror of nested_rns_gadget_decomposed (src/gadgets/arith/nested_rns/encoding.rs:273-338) over the entry
points older than the call - coeffs() of the source, Python integers per coefficient, window level and digit, from_coeffs
of the rows.  It is kinder than the reference's loop: slot(a, s) is computed once per (a, s) and looked up afterwards,
where the reference recomputes it per coefficient.  It is timed on ONE entry (wall clock, the device synchronised) and
scaled by the number of entries for the 2 x 16 shapes: the loop is serial per entry, as map_nested_rns_values is.
Device leg: NestedRnsContext.gadget_decomposed of an EVAL source into an EVAL result (inverse transform of a copy, table
look-up kernel, forward transform), hipEvent timing on the context's stream, warmed up, REPS iterations, median
[p10..p90]; its result is compared with the host leg's on the timed entry.
Store rate: the launch trace's time of nrns_decompose_kernel in a call with a COEFF result - the form of the kernel that
stores every word of the output; the EVAL call over the full window stores one limb per row into scratch, transforms
that and spreads it with the zeros - over the bytes of the output, next to the
time of gpupoly_matrix_fill_zero on the same matrix (one memset between two events on the stream, as the trace brackets a
kernel), median of REPS each.
Shapes: 1 x 1 and 2 x 16 at n = 2^10 (1 x 24 bits) and n = 2^14 (8 x 24 bits, 12 x 51 bits); p bits 7, two unreduced
multiplications, scale 2^8, the full window.
The report goes to --out (profiles/nested_rns_timing.txt) and to stdout; a JSON summary is its last line."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxx_amd import _ffi  # noqa: E402
import mxx_amd as mx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_rns_timing.txt"))
ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "10")))
args = ap.parse_args()
REPS, WARMUP = args.reps, 2
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


def rdiv(a, b):
    return (a + b // 2) // b


def host_sequence(ctx, src):
    """nested_rns_gadget_decomposed of `src` over coeffs() / from_coeffs, the full window"""
    p, ps, scale, qs = ctx.params, ctx.p_moduli, ctx.scale, ctx.q_moduli
    Q, Pfull = math.prod(qs), math.prod(ps)
    p_hat = [Pfull // pj for pj in ps]
    inv = [pow(h % pj, -1, pj) for h, pj in zip(p_hat, ps)]
    rc = [(Q // q) * pow((Q // q) % q, -1, q) for q in qs]
    memo = {}

    def terms(xs):
        ys = [x * i % pj for x, i, pj in zip(xs, inv, ps)]
        return ys, rdiv(sum(rdiv(y * scale, pj) for y, pj in zip(ys, ps)), scale)

    def slot(a, s):
        v = memo.get((a, s))
        if v is None:
            ys, w = terms([s % pj for pj in ps])
            v = memo[(a, s)] = ((sum(y * h for y, h in zip(ys, p_hat)) - w * Pfull) * rc[a]) % Q
        return v

    cw, A = len(ps) + 1, len(qs)
    coeffs = src.coeffs()
    rows = [[None] * src.ncol for _ in range(src.nrow * A * cw)]
    for r in range(src.nrow):
        for c in range(src.ncol):
            outs = [[0] * len(coeffs[r][c]) for _ in range(A * cw)]
            for k, value in enumerate(coeffs[r][c]):
                for a, q in enumerate(qs):
                    res = value % q
                    ys, w = terms([res % pj for pj in ps])
                    for d, s in enumerate(ys):
                        outs[a * cw + d][k] = slot(a, s)
                    outs[a * cw + cw - 1][k] = slot(a, w)
            for t, poly in enumerate(outs):
                rows[r * A * cw + t][c] = poly
    return M.from_coeffs(p, rows)


def kernel_ms(records, name):
    return sum(r["ms"] for r in records if name in r["kernel"])


def measure(label, ctx, rows, cols, host_ms_entry, check_entry):
    p = ctx.params
    us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
    src = us.sample_uniform(p, rows, cols, dist)
    src.ntt_all_in_place()
    for _ in range(WARMUP):
        out = ctx.gadget_decomposed(src)
    mx.gpu_device_sync()
    call = []
    for _ in range(REPS):
        out = None  # the block goes back to the context's cache before the next call asks for it
        p.ctx().timer_start()
        out = ctx.gadget_decomposed(src)
        call.append(p.ctx().timer_stop())
    kern, fill = [], []
    for _ in range(REPS):
        out = None
        _ffi.trace_begin()
        out = ctx.gadget_decomposed(src, eval_format=False)
        kern.append(kernel_ms(_ffi.trace_end(), "nrns_decompose_kernel"))
        p.ctx().timer_start()
        _ffi.check_status(lib.gpupoly_matrix_fill_zero(out.raw), "gpupoly_matrix_fill_zero")
        fill.append(p.ctx().timer_stop())
    out_bytes = out.nrow * out.ncol * (out.level + 1) * p.ring_dimension() * p.ctx().word_bytes()
    sc, sk, sf = stats(call), stats(kern), stats(fill)
    entries = rows * cols
    host_ms = host_ms_entry * entries
    kern_rate, fill_rate = out_bytes / sk["median_ms"] / 1e6, out_bytes / sf["median_ms"] / 1e6  # GB/s
    res = {"entries": entries, "out_MiB": round(out_bytes / 2**20, 1), "host_ms": round(host_ms, 1), "host_scaled_from_one_entry": entries > 1,
           "call": sc, "host_over_call": round(host_ms / sc["median_ms"], 1), "kernel": sk, "fill_zero": sf,
           "kernel_GBps": round(kern_rate, 1), "fill_GBps": round(fill_rate, 1), "kernel_over_fill_rate": round(kern_rate / fill_rate, 3)}
    say(f"{label:44s} out {res['out_MiB']:9.1f} MiB | host {host_ms:11.1f} ms{' (one entry x %d)' % entries if entries > 1 else '':18s} | call "
        f"{sc['median_ms']:9.4f} ms [{sc['p10_ms']:.4f}..{sc['p90_ms']:.4f}] | host / call {res['host_over_call']:9.1f}")
    say(f"{'':44s} main kernel {sk['median_ms']:9.4f} ms [{sk['p10_ms']:.4f}..{sk['p90_ms']:.4f}] = {kern_rate:7.1f} GB/s | fill_zero "
        f"{sf['median_ms']:9.4f} ms [{sf['p10_ms']:.4f}..{sf['p90_ms']:.4f}] = {fill_rate:7.1f} GB/s | kernel / fill rate {res['kernel_over_fill_rate']:.3f}")
    return res


summary = {"reps": REPS}
say(f"{REPS} iterations per shape, median [p10..p90]; p bits 7, 2 unreduced multiplications, scale 2^8, full window")
for key, n, limbs, bits in (("n10_1x24", 1 << 10, 1, 24), ("n14_8x24", 1 << 14, 8, 24), ("n14_12x51", 1 << 14, 12, 51)):
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 12)
    ctx = mx.NestedRnsContext(p, 7, 2, 1 << 8)
    say(f"n = {n}, {limbs} x {bits} bits: p moduli {ctx.p_moduli} (D = {len(ctx.p_moduli)})")
    us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
    one = us.sample_uniform(p, 1, 1, dist)
    one.ntt_all_in_place()
    dev = ctx.gadget_decomposed(one)  # builds the tables
    mx.gpu_device_sync()
    t0 = time.perf_counter()
    host = host_sequence(ctx, one)
    mx.gpu_device_sync()
    host_ms_entry = (time.perf_counter() - t0) * 1e3
    assert host == dev, f"{key}: the one call differs from the host sequence"
    del host, dev
    for rows, cols in ((1, 1), (2, 16)):
        summary[f"{key}_{rows}x{cols}"] = measure(f"n=2^{n.bit_length() - 1} {limbs}x{bits}-bit {rows}x{cols}", ctx, rows, cols, host_ms_entry, one)
say(json.dumps(summary))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
