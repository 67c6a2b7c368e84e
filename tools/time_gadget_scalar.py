"""gpupoly_matrix_mul_decompose_gadget_const_many / _scalar_many (the LargeScalarMul gate, lhs * G^-1(G_d o c)) against the
sequence of the existing entry points - gpu_matrix_fill_gadget, gpu_matrix_mul_scalar, gpupoly_matrix_mul_decompose_many -
alternated in one process.

hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around calls into preallocated outputs and temporaries,
every shape warmed up, REPS alternated iterations (200; REPS_LARGE = 10 at n = 2^16), median and 10th..90th percentile;
launches per call from gpupoly_launch_count; the results of both variants compared with gpu_matrix_equal before anything is
timed.  The operands of a call are the pair of a BGG+ encoding: the 1 x dk vector and the d x dk key matrix
(src/bgg/encoding.rs:191-200).  The sequence fills G and scales it on every call, as the reference's Evaluables do; its
scalar - also for the constant - is a resident EVAL polynomial made beforehand (the reference builds it with from_biguints per
gate; that upload and transform are not charged to the sequence).  A form counts as SLOWER when the new entry's median
exceeds the sequence's by more than the two runs' p10..p90 spreads together; the launch trace of one call of each new entry
is printed for every shape.  For the constant entry the achieved bytes/s is 2 x operand bytes / median.
Shapes: n = 2^16, 8 limbs of 28 bits, base 14 (the reference's end-to-end ring), d = 1 and d = 4; n = 256, 12 limbs of 51
bits, base 17, d = 2.  Prints a JSON summary last."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS, REPS_LARGE, WARMUP = int(os.environ.get("REPS", "200")), int(os.environ.get("REPS_LARGE", "10")), 2
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
ok = _ffi.check_status
CONST = (1 << 100) + 12345  # a two-word constant (a `shift` or `p_full` of the arithmetic gadgets)


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def words(m):
    """force the words layout (samples of 24-bit rings start as PACKED24)"""
    ptr, size = C.c_void_p(), C.c_size_t()
    ok(lib.gpupoly_matrix_device_ptr(m.raw, C.byref(ptr), C.byref(size)), "gpupoly_matrix_device_ptr")
    return m


def arr(ms):
    return (C.c_void_p * len(ms))(*[None if m is None else m.raw.value for m in ms])


def same(a, b):
    eq = C.c_int(0)
    ok(lib.gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value)


class Shape:
    def __init__(self, p, d):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        fresh = lambda r, c: M(p, r, c, p.crt_depth() - 1, True)  # noqa: E731
        self.p, self.ctx, self.d, self.base = p, p.ctx(), d, p.base_bits()
        dk = d * p.modulus_digits()
        self.lhss = [words(us.sample_uniform(p, 1, dk, dist)), words(us.sample_uniform(p, d, dk, dist))]
        self.x = words(us.sample_uniform(p, 1, 1, dist))
        self.c = mx.GpuDCRTPoly.from_biguints(p, [CONST]).inner
        self.g, self.gs = fresh(d, dk), fresh(d, dk)
        self.new = [fresh(1, dk), fresh(d, dk)]
        self.seq = [fresh(1, dk), fresh(d, dk)]
        self.cw = (C.c_uint64 * 2)(CONST & (2**64 - 1), CONST >> 64)
        self.operand_bytes = sum(m.nrow * m.ncol for m in self.lhss) * p.crt_depth() * p.ring_dimension() * (8 if max(p.moduli()) >= 1 << 31 else 4)

    def new_const(self):
        ok(lib.gpupoly_matrix_mul_decompose_gadget_const_many(arr(self.new), arr(self.lhss), None, 2, self.cw, 2, 0, self.base), "const_many")

    def new_ring(self):
        ok(lib.gpupoly_matrix_mul_decompose_gadget_scalar_many(arr(self.new), arr(self.lhss), None, 2, self.x.raw, 0, self.base), "scalar_many")

    def _seq(self, scalar):
        ok(lib.gpu_matrix_fill_gadget(self.g.raw, self.base), "gpu_matrix_fill_gadget")
        ok(lib.gpu_matrix_mul_scalar(self.gs.raw, self.g.raw, scalar.raw), "gpu_matrix_mul_scalar")
        ok(lib.gpupoly_matrix_mul_decompose_many(arr(self.seq), arr(self.lhss), None, None, 2, self.gs.raw, self.base), "mul_decompose_many")

    def seq_const(self):
        self._seq(self.c)

    def seq_ring(self):
        self._seq(self.x)

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0


def measure(name, sh, form, reps):
    new, seq = getattr(sh, "new_" + form), getattr(sh, "seq_" + form)
    seq(), new()
    mx.gpu_device_sync()
    assert all(same(a, b) for a, b in zip(sh.new, sh.seq)), f"{name}: the new entry differs from the sequence"
    for _ in range(WARMUP):
        seq(), new()
    a, b = [], []
    la = lb = 0
    for _ in range(reps):
        ta, la = sh.timed(seq)
        tb, lb = sh.timed(new)
        a.append(ta), b.append(tb)
    sa, sb = stats(a), stats(b)
    spread = (sa["p90_ms"] - sa["p10_ms"]) + (sb["p90_ms"] - sb["p10_ms"])
    slower = sb["median_ms"] - sa["median_ms"] > spread
    out = {"new": dict(sb, launches=lb), "sequence": dict(sa, launches=la), "reps": reps, "sequence_over_new": round(sa["median_ms"] / sb["median_ms"], 2),
           "slower": slower}
    line = (f"{name:40s} new {sb['median_ms']:10.4f} ms [{sb['p10_ms']:.4f}..{sb['p90_ms']:.4f}] {lb} launches | sequence {sa['median_ms']:10.4f} ms "
            f"[{sa['p10_ms']:.4f}..{sa['p90_ms']:.4f}] {la} launches | sequence / new {out['sequence_over_new']:.2f}")
    if form == "const":
        out["new"]["achieved_GBps"] = round(2 * sh.operand_bytes / (sb["median_ms"] * 1e-3) / 1e9, 1)
        line += f" | constant path: 2 x {sh.operand_bytes} B / median = {out['new']['achieved_GBps']} GB/s"
    print(line + (" SLOWER (beyond both p10..p90 spreads)" if slower else ""), flush=True)
    mx.gpu_device_sync()
    _ffi.trace_begin()
    new()
    for r in _ffi.trace_end():
        print(f"    trace {r['kernel'][:60]:60s} blocks {r['blocks']:8d} threads {r['threads']:4d} bytes {r['bytes']:14.0f} {r['ms']:9.4f} ms", flush=True)
    return out


def run(label, n, limbs, bits, base, d, reps):
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sh = Shape(p, d)
    return {form: measure(f"{label} d={d} {form}", sh, form, reps) for form in ("const", "ring")}


summary = {}
summary["n65536_L8_28bit_d1"] = run("n=2^16 L=8 28-bit", 1 << 16, 8, 28, 14, 1, REPS_LARGE)
summary["n65536_L8_28bit_d4"] = run("n=2^16 L=8 28-bit", 1 << 16, 8, 28, 14, 4, REPS_LARGE)
summary["n256_L12_51bit_d2"] = run("n=256 L=12 51-bit", 256, 12, 51, 17, 2, REPS)
print(json.dumps(summary))
