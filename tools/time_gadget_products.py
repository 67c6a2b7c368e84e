"""gpupoly_matrix_mul_gadget / gpupoly_matrix_gadget_mul against the sequence of the existing entry points that builds the
gadget matrix (gpu_matrix_fill_gadget, gpu_matrix_copy_block for a window, gpu_matrix_mul_scalar / gpu_matrix_mul,
gpu_matrix_sub), alternated in one process.

hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around calls into preallocated outputs and
temporaries, every shape warmed up, REPS alternated iterations (200; REPS_LARGE = 20 at n = 2^16), median and 10th..90th
percentile; launches per call from gpupoly_launch_count; the results of both variants compared with gpu_matrix_equal before
anything is timed.  `sequence` fills G on every call, as the reference's callers do (src/lookup/lwe/pubkey_gpu.rs:193-222
builds, scales, subtracts and frees it per lookup-table entry); `cached` is the same sequence with G filled beforehand, for
callers that keep it.  A form counts as SLOWER when the new entry's median exceeds the sequence's median by more than the two
runs' p10..p90 spreads together.
Forms, G = I_d (x) g, k = digits per entry:
  in_place   A -= G x                       one mul_gadget (addend = out)   | fill_gadget, mul_scalar, sub
  chunk      O = A_chunk - G[:, chunk] y    one mul_gadget                  | fill_gadget, copy_block, mul_scalar, sub
  s_g        O = s G, s 1 x d               one mul_gadget                  | fill_gadget, mul
  g_d        O = G D, D (d k) x (d k)       one gadget_mul                  | fill_gadget, mul
Shapes: n = 256, 12 limbs of 51 bits, base 17, d = 2 (launch-bound); n = 2^14, 10 limbs of 24 bits, base 12, d = 1; n = 2^16,
8 limbs of 28 bits, base 14, d = 1 and d = 4.  Prints a JSON summary last."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx  # noqa: E402
from mxx_amd import _ffi  # noqa: E402

REPS, REPS_LARGE, WARMUP = int(os.environ.get("REPS", "200")), int(os.environ.get("REPS_LARGE", "20")), 3
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
ok = _ffi.check_status


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def words(m):
    """force the words layout (samples of 24-bit rings start as PACKED24)"""
    ptr, size = C.c_void_p(), C.c_size_t()
    ok(lib.gpupoly_matrix_device_ptr(m.raw, C.byref(ptr), C.byref(size)), "gpupoly_matrix_device_ptr")
    return m


class Shape:
    """operands, outputs and temporaries of all four forms on one ring and one d, made once"""

    def __init__(self, p, d, with_g_d=True):
        us, dist = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
        sample = lambda r, c: words(us.sample_uniform(p, r, c, dist))  # noqa: E731
        fresh = lambda r, c: M(p, r, c, p.crt_depth() - 1, True)  # noqa: E731
        self.p, self.ctx, self.d, self.base = p, p.ctx(), d, p.base_bits()
        k = self.k = p.modulus_digits()
        dk = d * k
        self.cw, self.c0 = max(dk // 2, 1), dk - max(dk // 2, 1)  # the chunk: the last half of G's columns
        self.a, self.x, self.s = sample(d, dk), sample(1, 1), sample(1, d)
        self.a_chunk = sample(d, self.cw)
        self.g, self.g_cached, self.t = fresh(d, dk), fresh(d, dk), fresh(d, dk)
        self.gc, self.tc = fresh(d, self.cw), fresh(d, self.cw)
        self.new_a, self.seq_a = fresh(d, dk), fresh(d, dk)
        self.new_c, self.seq_c = fresh(d, self.cw), fresh(d, self.cw)
        self.new_s, self.seq_s = fresh(1, dk), fresh(1, dk)
        ok(lib.gpu_matrix_fill_gadget(self.g_cached.raw, self.base), "gpu_matrix_fill_gadget")
        if with_g_d:
            self.dm = sample(dk, dk)
            self.new_d, self.seq_d = fresh(d, dk), fresh(d, dk)

    def reset(self):
        for o in (self.new_a, self.seq_a):
            ok(lib.gpu_matrix_copy(o.raw, self.a.raw), "gpu_matrix_copy")

    def _g(self, cached):
        if cached:
            return self.g_cached
        ok(lib.gpu_matrix_fill_gadget(self.g.raw, self.base), "gpu_matrix_fill_gadget")
        return self.g

    # ---- A -= G x ----
    def in_place_new(self):
        ok(lib.gpupoly_matrix_mul_gadget(self.new_a.raw, 0, None, self.x.raw, 0, self.new_a.ncol, self.new_a.raw, 1, self.base, 0), "mul_gadget")

    def in_place_seq(self, cached=False):
        g = self._g(cached)
        ok(lib.gpu_matrix_mul_scalar(self.t.raw, g.raw, self.x.raw), "gpu_matrix_mul_scalar")
        ok(lib.gpu_matrix_sub(self.seq_a.raw, self.seq_a.raw, self.t.raw), "gpu_matrix_sub")

    # ---- O = A_chunk - G[:, chunk] y ----
    def chunk_new(self):
        ok(lib.gpupoly_matrix_mul_gadget(self.new_c.raw, 0, None, self.x.raw, self.c0, self.cw, self.a_chunk.raw, 1, self.base, 0), "mul_gadget")

    def chunk_seq(self, cached=False):
        g = self._g(cached)
        ok(lib.gpu_matrix_copy_block(self.gc.raw, g.raw, 0, 0, 0, self.c0, self.d, self.cw), "gpu_matrix_copy_block")
        ok(lib.gpu_matrix_mul_scalar(self.tc.raw, self.gc.raw, self.x.raw), "gpu_matrix_mul_scalar")
        ok(lib.gpu_matrix_sub(self.seq_c.raw, self.a_chunk.raw, self.tc.raw), "gpu_matrix_sub")

    # ---- O = s G ----
    def s_g_new(self):
        ok(lib.gpupoly_matrix_mul_gadget(self.new_s.raw, 0, self.s.raw, None, 0, self.new_s.ncol, None, 0, self.base, 0), "mul_gadget")

    def s_g_seq(self, cached=False):
        ok(lib.gpu_matrix_mul(self.seq_s.raw, self.s.raw, self._g(cached).raw), "gpu_matrix_mul")

    # ---- O = G D ----
    def g_d_new(self):
        ok(lib.gpupoly_matrix_gadget_mul(self.new_d.raw, self.dm.raw, None, 0, self.base, 0), "gadget_mul")

    def g_d_seq(self, cached=False):
        ok(lib.gpu_matrix_mul(self.seq_d.raw, self._g(cached).raw, self.dm.raw), "gpu_matrix_mul")

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0


def same(a, b):
    eq = C.c_int(0)
    ok(lib.gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value)


def measure(name, shape, form, outs, reps):
    new, seq = getattr(shape, form + "_new"), getattr(shape, form + "_seq")
    cached = lambda: seq(True)  # noqa: E731
    shape.reset()
    seq(), new()
    mx.gpu_device_sync()
    assert same(*outs), f"{name}: the new entry differs from the sequence"
    for _ in range(WARMUP):
        seq(), cached(), new()
    a, b, c = [], [], []
    la = lb = lc = 0
    for _ in range(reps):
        ta, la = shape.timed(seq)
        tc, lc = shape.timed(cached)
        tb, lb = shape.timed(new)
        a.append(ta), b.append(tb), c.append(tc)
    sa, sb, sc = stats(a), stats(b), stats(c)
    spread = (sa["p90_ms"] - sa["p10_ms"]) + (sb["p90_ms"] - sb["p10_ms"])
    slower = sb["median_ms"] - sa["median_ms"] > spread
    out = {"new": dict(sb, launches=lb), "sequence": dict(sa, launches=la), "cached": dict(sc, launches=lc), "reps": reps,
           "sequence_over_new": round(sa["median_ms"] / sb["median_ms"], 2), "cached_over_new": round(sc["median_ms"] / sb["median_ms"], 2),
           "slower": slower}
    print(f"{name:46s} new {sb['median_ms']:9.4f} ms [{sb['p10_ms']:.4f}..{sb['p90_ms']:.4f}] {lb} launch | sequence {sa['median_ms']:9.4f} ms "
          f"[{sa['p10_ms']:.4f}..{sa['p90_ms']:.4f}] {la} launches | cached G {sc['median_ms']:9.4f} ms [{sc['p10_ms']:.4f}..{sc['p90_ms']:.4f}] "
          f"{lc} launches | sequence / new {out['sequence_over_new']:.2f}, cached / new {out['cached_over_new']:.2f}"
          + (" SLOWER (beyond both p10..p90 spreads)" if slower else ""), flush=True)
    return out


def run(label, n, limbs, bits, base, d, reps):
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sh = Shape(p, d)
    res = {}
    for form, outs in (("in_place", (sh.new_a, sh.seq_a)), ("chunk", (sh.new_c, sh.seq_c)), ("s_g", (sh.new_s, sh.seq_s)), ("g_d", (sh.new_d, sh.seq_d))):
        res[form] = measure(f"{label} d={d} {form}", sh, form, outs, reps)
    return res


summary = {}
summary["n256_L12_51bit_d2"] = run("n=256 L=12 51-bit", 256, 12, 51, 17, 2, REPS)
summary["n16384_L10_24bit_d1"] = run("n=2^14 L=10 24-bit (M3A)", 1 << 14, 10, 24, 12, 1, REPS)
summary["n65536_L8_28bit_d1"] = run("n=2^16 L=8 28-bit", 1 << 16, 8, 28, 14, 1, REPS_LARGE)
summary["n65536_L8_28bit_d4"] = run("n=2^16 L=8 28-bit", 1 << 16, 8, 28, 14, 4, REPS_LARGE)
print(json.dumps(summary))
