"""Times the windowed decompositions against the sequences they replace, for the same window, on one MI355X.

Rings: the reference's end-to-end ring (n = 2^16, 8 x 28 bits, base 2^14: k = 16) and n = 256 with 12 x 51 bits (base 2^17:
k = 36).  Cases, on a conceptual d x (d k) hash-sampled matrix with d = 2:
  columns        sample_hash_decomposed_columns of a 16-column chunk: sample_distribution_columns + intt + decompose_base
                 against gpupoly_matrix_sample_decomposed_window over every row;
  columns, 1/4   the same, keeping rows [d k / 4, d k / 2): the sequence above + a row slice against the windowed call;
  chunk          decompose_chunk(1, k) of a resident EVAL d x 16 matrix: decompose_base + a row slice against
                 gpupoly_matrix_decompose_rows.
Both sides of a case are timed in turn inside one loop (device events around the calls, after a warm-up of each); the
minimum and the median of the repetitions are printed, and written to the file given as the first argument."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mxx_amd as mx

REPS = 9


def seed(tag):
    return mx.GpuRngSeed.from_bytes(bytes([(tag * 37 + i * 11 + 5) & 0xFF for i in range(32)]))


def timed_pair(ctx, old, new, reps=REPS):
    old(), new()
    t = {"old": [], "new": []}
    for _ in range(reps):
        for name, fn in (("old", old), ("new", new)):
            ctx.timer_start()
            fn()
            t[name].append(ctx.timer_stop())
    return {name: (min(v), sorted(v)[len(v) // 2]) for name, v in t.items()}


def main():
    M = mx.GpuDCRTPolyMatrix
    lines = ["ring\tcase\tparent sequence min / median ms\twindowed call min / median ms\tratio of minima"]
    for name, n, depth, bits, base in (("n=2^16, 8 x 28 bits, base 2^14", 1 << 16, 8, 28, 14), ("n=256, 12 x 51 bits, base 2^17", 256, 12, 51, 17)):
        p = mx.GpuDCRTPolyParams(n, mx.gen_crt_basis(n, depth, bits), base)
        ctx = p.ctx()
        k = p.modulus_digits()
        d, cols = 2, 16
        total, col0 = d * k, 16
        uni = mx.DistType.FinRingDist().as_ffi()
        s = seed(1)
        rs, re = d * k // 4, d * k // 2
        resident = M.sample_distribution(p, d, cols, uni, 0.0, seed(2))
        _ = resident.to_rns()[0, 0, 0, 0]  # words layout from here on, as after any first use

        def old_columns():
            return M.sample_distribution_columns(p, d, total, col0, cols, uni, 0.0, s).decompose_owned()

        cases = [
            ("columns", old_columns, lambda: M.sample_distribution_decomposed_window(p, d, total, col0, cols, uni, 0.0, s)),
            ("columns, 1/4 of the rows", lambda: old_columns().slice_rows(rs, re),
             lambda: M.sample_distribution_decomposed_window(p, d, total, col0, cols, uni, 0.0, s, False, rs, re)),
            ("decompose_chunk", lambda: resident.decompose().slice_rows(d, 2 * d), lambda: resident.decompose_rows(d, 2 * d)),
        ]
        for cname, old, new in cases:
            assert old() == new(), (name, cname)
            r = timed_pair(ctx, old, new)
            lines.append(f"{name}\t{cname}\t{r['old'][0]:.3f} / {r['old'][1]:.3f}\t{r['new'][0]:.3f} / {r['new'][1]:.3f}\t{r['old'][0] / r['new'][0]:.2f}")
            print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
