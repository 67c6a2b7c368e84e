"""CPU-only: the launch-grid arithmetic of the library (mxx_amd/csrc/grid_plan.h) as a stand-alone program.

A small C++ program with its own `main` includes the header - it has no HIP dependency - and prints the grid each rule gives
for the counts on its command line.  It is built with the address and undefined-behaviour sanitizers and run as a program;
nothing is loaded into Python.  The properties are checked here in Python's unbounded integers, against the hardware limits
(x <= 2^31 - 1 blocks and x * threads < 2^32, y and z <= 65535) and against the index formulas the kernels use:

  item_grid    item  = (blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x, guarded by item >= items
  fold_yz      entry = blockIdx.z * gridDim.y + blockIdx.y, guarded by entry >= entries (transpose, column blocks, tensor,
               the preimage's gather / scatter, the target builders' combine)
  vector_grid  the same in 32 bits (limb_vector_index, gadget_products.hip), guarded by v >= vectors
  ntt14_grid   poly  = blockIdx.z * gridDim.y + blockIdx.y with NO guard: the grid must be exact, y * z == polys

Both formulas map the grid one-to-one onto [0, x*y*threads) resp. [0, y*z) (mixed-radix digits), so "covers every item"
is extent >= count, "each exactly once" is extent == count, and "over-covers by less than one row of y" is that the grid
without its last row falls short of the count.  The small counts are enumerated outright as well.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y_MAX = 65535
X_MAX = (1 << 31) - 1

PROGRAM = r"""
#include "grid_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long long num(const char *s) { return std::strtoull(s, nullptr, 10); }

// argv: groups of five, (rule a b c d); one line per group
int main(int argc, char **argv) {
    if (argc < 6 || (argc - 1) % 5) return 2;
    for (int a = 1; a < argc; a += 5) {
        const char *rule = argv[a];
        const unsigned long long p = num(argv[a + 1]), q = num(argv[a + 2]), r = num(argv[a + 3]), s = num(argv[a + 4]);
        if (!std::strcmp(rule, "item")) {  // items threads
            const dim3 g = item_grid(static_cast<size_t>(p), static_cast<unsigned>(q));
            std::printf("1 %u %u %u\n", g.x, g.y, g.z);
        } else if (!std::strcmp(rule, "fold")) {  // entries
            size_t gy = 0, gz = 0;
            const bool ok = fold_yz(static_cast<size_t>(p), gy, gz);
            std::printf("%d 1 %zu %zu\n", ok ? 1 : 0, gy, gz);
        } else if (!std::strcmp(rule, "ntt14")) {  // vectors L
            dim3 g(0, 0, 0);
            const bool ok = ntt14_grid(static_cast<size_t>(p), static_cast<uint32_t>(q), g);
            std::printf("%d %u %u %u\n", ok ? 1 : 0, g.x, g.y, g.z);
        } else if (!std::strcmp(rule, "tile")) {  // rows cols tr tc
            std::printf("%d 0 0 0\n", tile_grid_fits(p, q, static_cast<uint32_t>(r), static_cast<uint32_t>(s)) ? 1 : 0);
        } else if (!std::strcmp(rule, "vec")) {  // vectors N vn
            if (p == 0 || p > kMaxVectors) return 4;  // the entries return or refuse before the rule
            const VectorGrid g = vector_grid(static_cast<uint32_t>(p), static_cast<uint32_t>(q), static_cast<uint32_t>(r));
            std::printf("%u %u %u %u\n", g.block.x, g.grid.x, g.grid.y, g.grid.z);
        } else {
            return 3;
        }
    }
    return 0;
}
"""


def is_prime(v):
    if v < 2:
        return False
    f = 2
    while f * f <= v:
        if v % f == 0:
            return False
        f += 1
    return True


def prime_near(v, step):
    while not is_prime(v):
        v += step
    return v


def _counts():
    edges = [0, 1, Y_MAX - 1, Y_MAX, Y_MAX + 1, Y_MAX + 2, 2 * Y_MAX - 1, 2 * Y_MAX, 2 * Y_MAX + 1, Y_MAX * Y_MAX - 1, Y_MAX * Y_MAX,
             Y_MAX * Y_MAX + 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1]
    primes = [prime_near(Y_MAX, -1), prime_near(Y_MAX + 1, 1), prime_near(2 * Y_MAX, -1), prime_near(2 * Y_MAX, 1),
              prime_near(Y_MAX * Y_MAX, -1), prime_near(Y_MAX * Y_MAX, 1), prime_near(1 << 31, -1), prime_near(1 << 31, 1)]
    squares = [prime_near(Y_MAX, -1) ** 2, prime_near(Y_MAX + 1, 1) ** 2, prime_near(46341, -1) ** 2, prime_near(46341, 1) ** 2,
               prime_near(362, -1) ** 2, prime_near(362, 1) ** 2]  # at 65535, at sqrt(2^31), at sqrt(2 * 65535)
    return sorted(set(edges + primes + squares))


COUNTS = _counts()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_plan")
    src = d / "grid_plan_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "grid_plan_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # no dependence on where the dynamic runtime falls in the link order
           "-I", os.path.join(ROOT, "mxx_amd", "csrc"), str(src), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return str(exe)


def _run(program, cases):
    """cases: (rule, a, b, c, d) -> one tuple of four integers each"""
    argv = [str(x) for c in cases for x in (tuple(c) + (0, 0, 0))[:5]]
    run = subprocess.run([program] + argv, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    return [tuple(int(x) for x in ln.split()) for ln in lines]


def test_the_header_is_what_the_library_compiles():
    """the rules are not restated for the test: the library's sources take them from this header and hold no second copy"""
    csrc = os.path.join(ROOT, "mxx_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".h", ".hip", ".inc"))}
    assert '#include "grid_plan.h"' in text["common.h"]
    for name in ("item_grid(size_t items", "ntt14_grid(size_t vectors", "tile_grid_fits(uint64_t rows", "vector_grid(uint32_t vectors",
                 "fold_yz(size_t entries"):
        assert [f for f, t in text.items() if name in t] == ["grid_plan.h"], name
    assert "hip_runtime" not in text["grid_plan.h"].split("#else")[1]
    for f in ("matrix.hip", "arith.hip", "preimage.hip", "row_targets.h", "lwe_lookup.hip", "ggh15_lookup.hip", "slot_transfer_eval.hip",
              "gadget_scalar.hip"):
        assert "fold_yz(" in text[f], f
    # no launcher spells the fold by hand any more (vector_grid, in the header, keeps its own 32-bit form)
    by_hand = [f for f, t in text.items() if f != "grid_plan.h" and ("+ gy - 1) / gy" in t or ", 65535), gz" in t)]
    assert by_hand == [], by_hand
    assert "grid_plan.h" in open(os.path.join(csrc, "Makefile")).read()


@pytest.mark.parametrize("threads", [128, 256])
def test_item_grid(program, threads):
    got = _run(program, [("item", n, threads) for n in COUNTS])
    for n, (_, x, y, z) in zip(COUNTS, got):
        blocks = -(-n // threads)
        assert 1 <= x <= X_MAX and x * threads <= 1 << 31 and 1 <= y <= Y_MAX and z == 1, (n, x, y)
        assert x * y >= blocks, (n, "not covered")  # item_index() reaches x * y * threads items, each once
        assert x * (y - 1) < max(blocks, 1), (n, "a whole row of y beyond the items")
        if y == 1:
            assert x == max(blocks, 1)  # no spare block in one row
        assert (y > 1) == (blocks > (1 << 31) // threads), n
    folded = [n for n, g in zip(COUNTS, got) if g[2] > 1]
    assert folded and min(folded) == (1 << 31) + 1 and Y_MAX * Y_MAX in folded


def test_fold_yz(program):
    got = _run(program, [("fold", n) for n in COUNTS])
    for n, (ok, _, gy, gz) in zip(COUNTS, got):
        assert ok == (n <= Y_MAX * Y_MAX), n
        assert 1 <= gy <= Y_MAX and gz >= 1, (n, gy, gz)
        assert gy * gz >= n and gy * (gz - 1) < max(n, 1), (n, gy, gz)
        if ok:
            assert gz <= Y_MAX
            assert gy == min(max(n, 1), Y_MAX) and gz == max(1, -(-n // gy))  # the rule as the launch sites spelled it
    assert dict(zip(COUNTS, got))[Y_MAX + 1][2:] == (Y_MAX, 2) and dict(zip(COUNTS, got))[2 * Y_MAX + 1][2:] == (Y_MAX, 3)
    # the kernels' formula, enumerated: every entry below the count exactly once, the rest at or beyond it
    for n, (ok, _, gy, gz) in zip(COUNTS, got):
        if n <= 2 * Y_MAX + 1:
            entry = (np.arange(gz, dtype=np.int64)[:, None] * gy + np.arange(gy, dtype=np.int64)[None, :]).ravel()
            assert np.array_equal(np.sort(entry[entry < n]), np.arange(n))


@pytest.mark.parametrize("L", [1, 3])
def test_ntt14_grid_is_exact_or_refused(program, L):
    """no tail guard in the grouped 2^14 kernels: y * z == polys, and false exactly when no z <= 65535 divides polys with
    polys / z <= 65535 (a prime above 65535, the square of one, anything above 65535^2)"""
    got = _run(program, [("ntt14", n * L, L) for n in COUNTS])
    for n, (ok, x, y, z) in zip(COUNTS, got):
        lo = max(1, -(-n // Y_MAX))
        exact = n == 0 or any(n % c == 0 for c in range(lo, min(Y_MAX, n) + 1))
        assert ok == exact, n
        if ok:
            assert x == L and y * z == n and y <= Y_MAX and 1 <= z <= Y_MAX, (n, x, y, z)
            if n:
                assert y >= 1
    by = dict(zip(COUNTS, (g[0] for g in got)))
    assert by[prime_near(Y_MAX, -1) ** 2] == 1 and by[prime_near(Y_MAX + 1, 1) ** 2] == 0 and by[prime_near(Y_MAX + 1, 1)] == 0
    assert by[Y_MAX * Y_MAX] == 1 and by[Y_MAX * Y_MAX + 1] == 0 and by[Y_MAX + 1] == 1 and by[(1 << 31) - 1] == 0  # 2^31 - 1 is prime
    if L > 1:  # vectors that are no whole polynomials
        assert [g[0] for g in _run(program, [("ntt14", n * L + 1, L) for n in COUNTS])] == [0] * len(COUNTS)
    assert _run(program, [("ntt14", 5, 0)])[0][0] == 0


def test_tile_grid_fits_flips_between_65535_and_65536_tiles(program):
    tiles = [(1, 1), (1, 4), (2, 4), (4, 4), (2, 2), (1, 8), (2, 8), (4, 8), (8, 8)]  # dispatch_stacked_tile's, matmul_tile.h
    cases, want = [], []
    for tr, tc in tiles:
        for rows, cols, fits in [(1, Y_MAX * tc, 1), (1, Y_MAX * tc + 1, 0), (1, Y_MAX * tc - tc + 1, 1), (tr, Y_MAX * tc, 1),
                                 (tr + 1, Y_MAX * tc, 0), (Y_MAX * tr, 1, 1), (Y_MAX * tr + 1, 1, 0), (Y_MAX * tr, tc + 1, 0),
                                 (255 * tr, 257 * tc, 1), (256 * tr, 256 * tc, 0), (254 * tr + 1, 256 * tc + 1, 1), (0, 1 << 40, 1),
                                 (3 * tr, 21845 * tc, 1), (3 * tr, 21845 * tc + 1, 0), (1 << 31, 1 << 31, 0)]:
            cases.append(("tile", rows, cols, tr, tc))
            want.append(fits)
            assert fits == int((-(-rows // tr)) * (-(-cols // tc)) <= Y_MAX)
    assert [g[0] for g in _run(program, cases)] == want


@pytest.mark.parametrize("N,vn", [(4, 4), (2, 2), (2, 1), (1, 1), (256, 4), (1024, 2), (4096, 4), (16384, 4), (65536, 2)])
def test_vector_grid(program, N, vn):
    counts = [n for n in COUNTS if 1 <= n <= Y_MAX * Y_MAX]
    got = _run(program, [("vec", n, N, vn) for n in counts])
    lanes = -(-N // vn)
    for n, (threads, gx, gy, gz) in zip(counts, got):
        assert threads % 64 == 0 and 64 <= threads <= 256 and threads == min(256, -(-lanes // 64) * 64)
        assert gx == -(-lanes // (4 * threads)) and 1 <= gx <= X_MAX  # four passes of the kernels' strided loop at the most
        assert 1 <= gy <= Y_MAX and 1 <= gz <= Y_MAX and gy * gz >= n and gy * (gz - 1) < n, (n, gy, gz)
        assert gy * gz - 1 < 1 << 32  # limb_vector_index() is 32 bits wide
    # what the entries refuse never reaches the rule (the program returns 4 as they would refuse)
    run = subprocess.run([program, "vec", str(Y_MAX * Y_MAX + 1), str(N), str(vn), "0"], capture_output=True, text=True)
    assert run.returncode == 4
