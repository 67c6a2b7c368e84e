"""The batched preimage at trapdoor dimensions d = 3 and d = 4 (tools/README.md).  Three measurements:
  (a) the plain p1 entry (`gpu_matrix_sample_p1_full_cached`) at m = 2d = 6 and 8 rows from either kernel - the eight-row
      persistent-lane kernel (the default) and the one-thread-per-element kernel (MXX_HIP_P1=simple, the parent commit's
      default at these m); shapes n = 256, 12 x 51 bits, 16 columns and n = 2^14, 8 x 24 bits, 48 columns
  (b) sixteen 4-column requests against one key (n = 256, 12 x 51 bits, base 2^17): one `gpupoly_trapdoor_preimage_many`
      call (`preimage_many_abi`) against the loop of `preimage` calls
  (c) 8 keys x 2 such requests: one `gpupoly_trapdoor_preimage_keyed` call (`preimage_many_keys`) against one
      `gpupoly_trapdoor_preimage_many` call per key
The measuring is done by worker processes (`--worker`), one library each: this build's and, with --parent-lib, the parent
commit's (MXX_GPUPOLY_LIB; there the batched entries answer "unsupported" at d > 2 and the wrappers run the loop, which is
the baseline).  The workers of the two libraries alternate for --rounds rounds; inside a worker the legs of a measurement
alternate, every sample is bracketed by device events on the context's stream and ends in a device synchronise, and the
outputs of the legs are compared first (same seeds, `gpu_matrix_equal`).  Reported: the median over a worker's samples,
then per leg the median and the range of those medians over the rounds - the run-to-run spread a difference has to exceed.
The launch trace of the batched d = 4 call, summed per kernel, comes from the first worker of this build.  The report goes
to --out (default profiles/preimage_dim_timing.txt)."""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P1_SHAPES = [  # name, n, limbs, bits, base, columns, calls per sample
    ("n256", 256, 12, 51, 17, 16, 20),
    ("n16384", 1 << 14, 8, 24, 12, 48, 4),
]
RING = (256, 12, 51, 17)  # (b), (c)


def worker(reps, trace):
    sys.path.insert(0, ROOT)
    import mxx_amd as mx
    from mxx_amd import _ffi
    from mxx_amd.trapdoor import GpuDCRTTrapdoor, p1_covariance_parameters

    lib, M = _ffi.lib(), mx.GpuDCRTPolyMatrix
    os.environ.pop("MXX_HIP_P1", None)
    os.environ.pop("MXX_HIP_SAMPLER_PER_LANE", None)
    _ffi.reload_env()
    res = {"library": _ffi.LIB_PATH}

    def sample(ctx, fn):
        """(device ms, launches) of fn(), device idle before and after"""
        mx.gpu_device_sync()
        c0 = lib.gpupoly_launch_count()
        ctx.timer_mark(0)
        out = fn()
        ctx.timer_mark(1)
        mx.gpu_device_sync()
        del out
        return ctx.timer_elapsed(0, 1), lib.gpupoly_launch_count() - c0

    def alternate(ctx, legs, before=None):
        for _ in range(2):  # warm-up
            for nm, fn in legs:
                if before:
                    before(nm)
                fn()
        ms, launches = collections.defaultdict(list), {}
        for _ in range(reps):
            for nm, fn in legs:
                if before:
                    before(nm)
                t, launches[nm] = sample(ctx, fn)
                ms[nm].append(t)
        p90 = lambda xs: sorted(xs)[min(len(xs) - 1, max(0, round(0.9 * (len(xs) - 1))))]  # noqa: E731 - nearest rank, as time_lut_targets.py
        return {nm: {"median_ms": statistics.median(ms[nm]), "min_ms": min(ms[nm]), "max_ms": max(ms[nm]), "p90_ms": p90(ms[nm]),
                     "launches": launches[nm]} for nm, _ in legs}

    # ---- (a) the plain p1 entry
    def p1_mode(nm):
        if nm == "simple":
            os.environ["MXX_HIP_P1"] = "simple"
        else:
            os.environ.pop("MXX_HIP_P1", None)
        _ffi.reload_env()

    for name, n, limbs, bits, base, cols, calls in P1_SHAPES:
        p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
        for d in (3, 4):
            td = GpuDCRTTrapdoor.new(p, d, 4.578)
            cache = td.p1_covariance_cache(*p1_covariance_parameters(p, d, 4.578))
            tp2 = M.sample_distribution(p, 2 * d, cols, mx.DistType.GaussDist(3.0e5).as_ffi(), 3.0e5,
                                        mx.GpuRngSeed.from_bytes(bytes(range(32)))).into_coeff_domain()
            seed = mx.GpuRngSeed.from_bytes(bytes(range(1, 33)))
            outs = {nm: M.new_empty(p, 2 * d, cols) for nm in ("default", "simple")}

            def call(nm, k=1):
                for _ in range(k):
                    _ffi.check_status(lib.gpu_matrix_sample_p1_full_cached(cache.raw, tp2.raw, seed, outs[nm].raw), "p1")

            for nm in outs:
                p1_mode(nm)
                call(nm)
            assert outs["default"] == outs["simple"], "the two p1 kernels differ"
            legs = [(nm, (lambda nm=nm: call(nm, calls))) for nm in ("default", "simple")]
            r = alternate(p.ctx(), legs, before=p1_mode)
            p1_mode("default")
            for v in r.values():  # per call
                for key in ("median_ms", "min_ms", "max_ms", "p90_ms"):
                    v[key] /= calls
                v["launches"] //= calls
            res[f"a/{name}/m{2 * d}"] = r

    # ---- (b), (c)
    n, limbs, bits, base = RING
    p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, limbs, bits), base)
    sampler, us = mx.GpuDCRTPolyTrapdoorSampler(p, 4.578), mx.GpuDCRTPolyUniformSampler()
    for d in (3, 4):
        keys = [sampler.trapdoor(p, d) for _ in range(8)]
        key_of = [k for k in range(8) for _ in range(2)]
        targets = [us.sample_uniform(p, d, 4, mx.DistType.FinRingDist()) for _ in range(16)]
        seeds = [tuple(mx.GpuRngSeed.from_bytes(os.urandom(32)) for _ in range(3)) for _ in targets]
        td, a = keys[0]

        def many():
            return sampler.preimage_many_abi(p, td, a, targets, _seeds=seeds)

        def loop():
            return [sampler.preimage(p, td, a, t, _seeds=sd) for t, sd in zip(targets, seeds)]

        def keyed():
            return sampler.preimage_many_keys(p, keys, key_of, targets, _seeds=seeds)

        def per_key():
            out = []
            for k, (tdk, ak) in enumerate(keys):
                mine = [j for j, kk in enumerate(key_of) if kk == k]
                out += sampler.preimage_many_abi(p, tdk, ak, [targets[j] for j in mine], _seeds=[seeds[j] for j in mine])
            return out

        x, y = many(), loop()
        assert all(u == v for u, v in zip(x, y)) and all(a * u == t for u, t in zip(x, targets)), "many differs from the loop"
        x, y = keyed(), per_key()
        assert all(u == v for u, v in zip(x, y)) and all(keys[k][1] * u == t for k, u, t in zip(key_of, x, targets)), "keyed differs"
        del x, y
        res[f"b/d{d}"] = alternate(p.ctx(), [("many", many), ("loop", loop)])
        res[f"c/d{d}"] = alternate(p.ctx(), [("keyed", keyed), ("per_key", per_key)])
        if trace and d == 4:
            mx.gpu_device_sync()
            _ffi.trace_begin()
            many()
            mx.gpu_device_sync()
            per = collections.OrderedDict()
            for rec in _ffi.trace_end():
                e = per.setdefault(rec["kernel"].split("<")[0].strip("( "), [0, 0.0])
                e[0] += 1
                e[1] += rec["ms"]
            res["trace/b/d4/many"] = [[k, cnt, ms] for k, (cnt, ms) in per.items()]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "6")))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--commit", default="", help="this build's commit (read from git when not given)")
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preimage_dim_timing.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.reps, args.trace)

    def git(rev):
        try:
            return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            return "unknown"

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    libs = [("this", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    say(f"this build: {args.commit or git('HEAD')} + working tree; parent library: "
        f"{(args.parent_commit or git('HEAD')) if args.parent_lib else 'not measured'}")
    say(f"{args.rounds} rounds, the libraries alternate (a fresh process each); {args.reps} alternated samples per leg and process; device events, ms")
    runs = collections.defaultdict(list)
    for rnd in range(args.rounds):
        for which, path in libs:
            env = dict(os.environ)
            env.pop("MXX_GPUPOLY_LIB", None)
            if path:
                env["MXX_GPUPOLY_LIB"] = path
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(args.reps)]
            if rnd == 0 and which == "this":
                cmd.append("--trace")
            t0 = time.time()
            child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
            if child.returncode != 0:  # nothing more is started on the device after a failure
                say(f"worker ({which}, round {rnd}) failed with status {child.returncode}:\n{child.stderr[-3000:]}")
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
                return 1
            runs[which].append(json.loads(child.stdout.strip().splitlines()[-1]))
            print(f"   worker ({which}, round {rnd}): {time.time() - t0:.1f} s", flush=True)

    def over_rounds(which, key, leg):
        meds = [r[key][leg]["median_ms"] for r in runs[which]]
        return statistics.median(meds), min(meds), max(meds), runs[which][0][key][leg]["launches"]

    def row(label, which, key, leg):
        med, lo, hi, launches = over_rounds(which, key, leg)
        say(f"   {label:44s} {med:9.4f} ms  (rounds {lo:.4f} .. {hi:.4f})  {launches:4d} launches")
        return med, lo, hi

    say()
    say("(a) gpu_matrix_sample_p1_full_cached, per call")
    for name, n, limbs, bits, base, cols, calls in P1_SHAPES:
        for m in (6, 8):
            key = f"a/{name}/m{m}"
            say(f"== n = {n}, {limbs} x {bits} bits, {cols} columns, m = {m} ({calls} calls per sample)")
            lanes = row("lane kernel (this build's default)", "this", key, "default")
            simple = row("one thread per element (MXX_HIP_P1=simple)", "this", key, "simple")
            if args.parent_lib:
                parent = row("parent library (its default)", "parent", key, "default")
                verdict = "no slower than the parent" if lanes[1] <= parent[2] else "SLOWER than the parent"
                say(f"   lanes / simple = {lanes[0] / simple[0]:.3f}, lanes / parent = {lanes[0] / parent[0]:.3f}: lane kernel {verdict} "
                    f"(ranges over the rounds {'overlap or lanes below' if lanes[1] <= parent[2] else 'apart'})")
    for part, title, batched, base_leg in (("b", "(b) sixteen 4-column requests, one key", "many", "loop"),
                                           ("c", "(c) 8 keys x 2 requests of 4 columns", "keyed", "per_key")):
        say()
        say(f"{title}; n = {RING[0]}, {RING[1]} x {RING[2]} bits, base 2^{RING[3]}")
        for d in (3, 4):
            key = f"{part}/d{d}"
            say(f"== d = {d}")
            one = row({"many": "one gpupoly_trapdoor_preimage_many call", "keyed": "one gpupoly_trapdoor_preimage_keyed call"}[batched],
                      "this", key, batched)
            other = row({"loop": "loop of preimage calls", "per_key": "one gpupoly_trapdoor_preimage_many per key"}[base_leg],
                        "this", key, base_leg)
            say(f"   {base_leg} / {batched} = {other[0] / one[0]:.2f}")
            if args.parent_lib:
                row(f"parent library: {base_leg} (the baseline)", "parent", key, base_leg)
                row(f"parent library: the wrapper ('{batched}', falls back)", "parent", key, batched)
    tr = runs["this"][0].get("trace/b/d4/many")
    if tr:
        say()
        say(f"-- launch trace of the one gpupoly_trapdoor_preimage_many call at d = 4 ({sum(c for _, c, _ in tr)} launches and copies, "
            f"{sum(ms for _, _, ms in tr):.3f} ms summed):")
        for k, cnt, ms in tr:
            say(f"   {cnt:4d} x {k:48s} {ms:8.3f} ms")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
