"""gpupoly_matrix_sample_distribution_blocks (one call) against the loop of plain sampler calls, and
GpuDCRTPolyHashSampler.sample_hash_weighted_sum against the literal per-term loop of commit_base
(src/commit/wee25.rs:858-883), alternated in one process.

Sampling legs, uniform distribution, T seeded blocks of 1 x c:
  loop   T calls of GpuDCRTPolyMatrix.sample_distribution (key derivation, sampling, transform or pack per call)
  blocks one GpuDCRTPolyMatrix.sample_distribution_blocks in the stacked layout (T x c)
  many   the same in the columns layout plus split_columns: what sample_hash_many does per 64 tags
  hash_table    one GpuDCRTPolyMatrix.sample_hash_blocks, stacked, the T literal tags uploaded as a table and hashed on the
                device (gpupoly_matrix_sample_hash_blocks): the hashing is INSIDE the clock
  hash_indexed  the same with IndexedTags: the tags generated on the device, nothing uploaded
  host_hash     what the public interface cost before the device hash: T hash_seed_for_matrix calls of the mirror (host
                Python Keccak) INSIDE the clock, then `blocks`
Sum legs, sum_t W_t o a_t with W_t the t-th block and a_t entry t of a 1 x T EVAL row:
  loop   acc = acc + sample(seed_t) * a_t, the a_t taken out of the row beforehand
  fused  sample_hash_weighted_sum: one stacked sample, one one-row product, no accumulation for a single chunk
The seeds are hashed before the clock starts in every leg but hash_table, hash_indexed and host_hash (the mirror's Keccak is
host Python and would drown both sides); the host hashing time those legs hide is reported per shape (wall clock, once), and
the hash kernel alone for 64 and for 2^16 indexed tags (launch trace).
hipEvent timing on the context's stream (gpupoly_timer_start / _stop) around each leg - host stalls of the loop legs
included: it is what the caller waits for -, every shape warmed up, REPS alternated iterations, median and 10th..90th
percentile, launches per leg from gpupoly_launch_count, results compared with gpu_matrix_equal before timing.
Shapes:
  (a) 64 blocks of 1 x 4 at n = 2^8, 12 limbs of 51 bits
  (b) 64 blocks of 1 x 18 at n = 2^14, 8 limbs of 24 bits
The report goes to --out (profiles/hash_seeds_timing.txt; profiles/sample_blocks_timing.txt is the run of section 5p) and to stdout; a JSON summary is its last line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxx_amd import _ffi  # noqa: E402
import mxx_amd as mx  # noqa: E402
from mxx_amd.sampler import sample_gpu_matrix_with_seed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_seeds_timing.txt"))
ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "10")))
args = ap.parse_args()
REPS, WARMUP = args.reps, 2
lib = _ffi.lib()
M = mx.GpuDCRTPolyMatrix
FIN = mx.DistType.FinRingDist()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(ms):
    ms = sorted(ms)
    pick = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
    return {"median_ms": round(pick(0.5), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


class PreHashed(mx.GpuDCRTPolyHashSampler):
    """the hash sampler with its seeds looked up instead of hashed: the tags are positions in a list made beforehand"""

    def __init__(self, seeds):
        super().__init__()
        self.seeds = seeds

    def _on_device(self):
        return False

    def _seeds(self, key, tags, params=None):
        return [self.seeds[t] for t in tags]


class Case:
    def __init__(self, p, blocks, cols):
        key = self.key = bytes(range(32))
        self.p, self.ctx, self.T, self.cols = p, p.ctx(), blocks, cols
        self.indexed = mx.IndexedTags(b"wee25_w_block_", 0, blocks)
        self.literal = list(self.indexed)
        t0 = time.perf_counter()
        self.seeds = [mx.hash_seed_for_matrix(key, tag) for tag in self.literal]
        self.host_hash_ms = (time.perf_counter() - t0) * 1e3
        self.sampler = PreHashed(self.seeds)
        self.weights = mx.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, blocks, FIN).reshape_view(1, blocks)  # in words from here on
        self.entries = [self.weights.entry(0, t) for t in range(blocks)]
        self.out = {}

    def sample_loop(self):
        self.out["sample_loop"] = [M.sample_distribution(self.p, 1, self.cols, FIN.as_ffi(), 0.0, s) for s in self.seeds]

    def sample_blocks(self):
        self.out["sample_blocks"] = M.sample_distribution_blocks(self.p, self.seeds, FIN.as_ffi(), block_polys=self.cols)

    def hash_table(self):
        self.out["hash_table"] = M.sample_hash_blocks(self.p, self.key, self.literal, FIN.as_ffi(), block_polys=self.cols)

    def hash_indexed(self):
        self.out["hash_indexed"] = M.sample_hash_blocks(self.p, self.key, self.indexed, FIN.as_ffi(), block_polys=self.cols)

    def host_hash(self):
        seeds = [mx.hash_seed_for_matrix(self.key, tag) for tag in self.literal]
        self.out["host_hash"] = M.sample_distribution_blocks(self.p, seeds, FIN.as_ffi(), block_polys=self.cols)

    def sample_many(self):
        self.out["sample_many"] = self.sampler.sample_hash_many(self.p, b"", range(self.T), 1, self.cols, FIN)

    def sum_loop(self):
        acc = M.zero(self.p, 1, self.cols)
        for s, a in zip(self.seeds, self.entries):
            acc = acc + sample_gpu_matrix_with_seed(self.p, 1, self.cols, FIN, s) * a
        self.out["sum_loop"] = acc

    def sum_fused(self):
        self.out["sum_fused"] = self.sampler.sample_hash_weighted_sum(self.p, b"", range(self.T), self.weights, 1, self.cols)

    def timed(self, fn):
        c0 = lib.gpupoly_launch_count()
        self.ctx.timer_start()
        fn()
        ms = self.ctx.timer_stop()
        return ms, lib.gpupoly_launch_count() - c0

    def check(self):
        stack, loop, many = self.out["sample_blocks"], self.out["sample_loop"], self.out["sample_many"]
        for t in range(self.T):
            assert stack.row_view(t, t + 1) == loop[t] and many[t] == loop[t], f"block {t} differs from the plain call"
        for leg in ("hash_table", "hash_indexed", "host_hash"):
            assert self.out[leg] == stack and self.out[leg].layout == stack.layout, f"{leg} differs from the seeds-given call"
        assert self.out["sum_fused"] == self.out["sum_loop"], "the weighted sum differs from the per-term loop"


def measure(name, case):
    legs = {"sample_loop": case.sample_loop, "sample_blocks": case.sample_blocks, "hash_table": case.hash_table,
            "hash_indexed": case.hash_indexed, "host_hash": case.host_hash, "sample_many": case.sample_many,
            "sum_loop": case.sum_loop, "sum_fused": case.sum_fused}
    for _ in range(WARMUP):
        for fn in legs.values():
            fn()
    mx.gpu_device_sync()
    case.check()
    times, launches = {k: [] for k in legs}, {}
    for _ in range(REPS):
        for k, fn in legs.items():
            ms, launches[k] = case.timed(fn)
            times[k].append(ms)
    out = {k: dict(stats(v), launches=launches[k]) for k, v in times.items()}
    out["sample_loop_over_blocks"] = round(out["sample_loop"]["median_ms"] / out["sample_blocks"]["median_ms"], 2)
    out["sample_loop_over_many"] = round(out["sample_loop"]["median_ms"] / out["sample_many"]["median_ms"], 2)
    out["sum_loop_over_fused"] = round(out["sum_loop"]["median_ms"] / out["sum_fused"]["median_ms"], 2)
    out["host_hashing_hidden_ms"] = round(case.host_hash_ms, 3)
    out["hash_indexed_minus_blocks_ms"] = round(out["hash_indexed"]["median_ms"] - out["sample_blocks"]["median_ms"], 4)
    out["hash_table_minus_blocks_ms"] = round(out["hash_table"]["median_ms"] - out["sample_blocks"]["median_ms"], 4)
    say(name)
    for k in legs:
        s = out[k]
        say(f"    {k:14s} {s['median_ms']:10.4f} ms [{s['p10_ms']:.4f}..{s['p90_ms']:.4f}] {s['launches']:5d} launches")
    say(f"    sampling: loop / blocks {out['sample_loop_over_blocks']:.2f}, loop / many {out['sample_loop_over_many']:.2f};"
        f" weighted sum: loop / fused {out['sum_loop_over_fused']:.2f}")
    say(f"    host hashing hidden by sample_loop / sample_blocks / sample_many / sum_*: {case.host_hash_ms:.1f} ms for {case.T} tags;"
        f" hash_indexed - sample_blocks {out['hash_indexed_minus_blocks_ms']:+.4f} ms, hash_table - sample_blocks"
        f" {out['hash_table_minus_blocks_ms']:+.4f} ms")
    return out


summary = {"reps": REPS}
say(f"{REPS} alternated iterations per shape, median [p10..p90]")
n, limbs, bits = 1 << 8, 12, 51
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 17)
summary["a"] = measure("(a) 64 blocks of 1 x 4, n=2^8, 12 limbs of 51 bits", Case(p, 64, 4))
n, limbs, bits = 1 << 14, 8, 24
p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), 12)
summary["b"] = measure("(b) 64 blocks of 1 x 18, n=2^14, 8 limbs of 24 bits", Case(p, 64, 18))
# the hash kernel alone: 64 indexed tags of 22 bytes (one wave, one rate block per tag - the launch in front of the shapes
# above) and 2^16 of them
from mxx_amd.matrix import device_hash_seeds  # noqa: E402

for count in (64, 1 << 16):
    tags = mx.IndexedTags(b"wee25_w_block_", 0, count)
    kernel_ms = []
    for i in range(WARMUP + REPS):
        _ffi.trace_begin()
        device_hash_seeds(p, bytes(range(32)), tags)
        ms = [e["ms"] for e in _ffi.trace_end() if e["kernel"] == "hash_seeds_kernel"]
        assert len(ms) == 1
        if i >= WARMUP:
            kernel_ms.append(ms[0])
    s = summary[f"hash_seeds_kernel_{count}_tags"] = stats(kernel_ms)
    say(f"hash_seeds_kernel alone, {count} indexed tags: {s['median_ms']:.4f} ms [{s['p10_ms']:.4f}..{s['p90_ms']:.4f}]"
        f" = {s['median_ms'] * 1e6 / count:.1f} ns per tag")
say(json.dumps(summary))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
