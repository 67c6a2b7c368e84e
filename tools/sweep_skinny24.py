"""The one-row packed product at the M2A shape (n = 2^14, L = 15, (1 x 30)(30 x 120)): every variant of the kernel, alternated.

    python tools/sweep_skinny24.py                 # every variant, ROUNDS rounds of REPS products each, one table
    python tools/sweep_skinny24.py run VARIANT...  # 3 products of each named variant and nothing else (for rocprofv3 --pmc)

Variants: `words` (B in 4-byte words), `tile:184` / `tile:184p` / `tile:144` / `tile:144p` (matmul_kernel on packed B with
that MXX_HIP_MATMUL_TILE, MXX_HIP_SKINNY24=0), `TC,G,WPE,MAP` (MXX_HIP_SKINNY24=force:...), `auto` (no switch set).
Under `rocprofv3 --kernel-trace --stats` every variant is a kernel name of its own.  Times here are device events around
REPS back-to-back products; bytes are B packed (or in words) + A + C, from shapes.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx
from mxx_amd import _ffi

N, L, SHAPE = 16384, 15, (1, 30, 120)
ROUNDS, REPS = 5, 5
SHAPES = ["8,1,5,12", "8,2,5,12", "8,4,5,12", "8,8,5,12", "8,8,4,12", "8,1,5,16", "8,2,5,16", "8,4,5,16",
          "4,1,8,12", "4,2,8,12", "4,4,8,12", "4,1,8,16", "4,2,8,16", "4,4,8,16"]
SWITCHES = ("MXX_HIP_SKINNY24", "MXX_HIP_MATMUL_TILE")


def select(variant):
    for s in SWITCHES:
        os.environ.pop(s, None)
    if variant.startswith("tile:"):
        os.environ["MXX_HIP_SKINNY24"] = "0"
        os.environ["MXX_HIP_MATMUL_TILE"] = variant[5:]
    elif variant not in ("words", "auto"):
        os.environ["MXX_HIP_SKINNY24"] = "force:" + variant
    _ffi.reload_env()


def main():
    only = sys.argv[2:] if len(sys.argv) > 2 and sys.argv[1] == "run" else None
    variants = only or (["words", "tile:184", "tile:184p", "tile:144", "tile:144p"] + SHAPES + ["auto"])
    p = mx.GpuDCRTPolyParams(N, mx.gen_crt_basis(N, L, 24), 12)
    ctx = p.ctx()
    us, d = mx.GpuDCRTPolyUniformSampler(), mx.DistType.FinRingDist()
    r, k, c = SHAPE
    a = us.sample_uniform(p, r, k, d)
    a.row_view(0, 1)  # A in words, as after bench.py's warm-up
    b_packed = us.sample_uniform(p, k, c, d)
    b_words = None
    if "words" in variants:
        os.environ["MXX_HIP_PACK24"] = "0"
        _ffi.reload_env()
        b_words = us.sample_uniform(p, k, c, d)
        os.environ.pop("MXX_HIP_PACK24")
        _ffi.reload_env()
    assert b_packed.layout == "packed24" and a.layout == "words"
    res = {v: [] for v in variants}
    labels = {}
    for rnd in range(1 if only else ROUNDS + 1):  # round 0 warms every variant up
        for v in variants:
            select(v)
            b = b_words if v == "words" else b_packed
            if only:
                for _ in range(3):
                    out = a * b
                mx.gpu_device_sync()
                labels[v] = ctx.last_kernel()
                continue
            ctx.timer_start()
            for _ in range(REPS):
                out = a * b
            t = ctx.timer_stop() / REPS
            labels[v] = ctx.last_kernel()
            if rnd:
                res[v].append(t * 1e3)
            del out
    select("auto")
    assert b_packed.layout == "packed24"
    for v in variants:
        if only:
            print(f"{v:10s} {labels[v][:70]}", flush=True)
            continue
        gb = ((3 if v != "words" else 4) * k * c + 4 * r * k + 4 * r * c) * L * N / 1e9
        ts = res[v]
        print(f"{v:10s} min {min(ts):7.1f} med {statistics.median(ts):7.1f} max {max(ts):7.1f} us  {gb / min(ts) * 1e3:5.2f} TB/s at min  "
              f"{labels[v][:60]}", flush=True)


if __name__ == "__main__":
    main()
