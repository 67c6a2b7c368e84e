"""CPU-only: the host side of the bit / integer read-out (mxx_amd/csrc/readout_bounds.h) as a stand-alone program.

A small C++ program with its own `main` includes the header and prints, for a basis and bounds given on the command line,
each bound's mixed-radix digits and its "is Q" flag, or that it is refused.  It is built with the address and
undefined-behaviour sanitizers and run as a program; nothing is loaded into Python.  Expected values are Python's
`B // (q_0 .. q_{k-1}) % q_k`.
"""
import math
import os
import random
import subprocess

import pytest

import plainref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "readout_bounds.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<uint64_t> parse_words(const char *s) {  // comma-separated hexadecimal words, little-endian
    std::vector<uint64_t> out;
    const char *p = s;
    while (*p) {
        char *end = nullptr;
        out.push_back(std::strtoull(p, &end, 16));
        p = *end == ',' ? end + 1 : end;
    }
    return out;
}

static void print_bound(const readout::BoundDigits &b, int L) {
    std::printf("ok %d", b.is_q);
    for (int k = 0; k < L; ++k) std::printf(" %" PRIx64, b.d[k]);
    for (int k = L; k < readout::kMaxLimbs; ++k)
        if (b.d[k] != 0) std::printf(" dirty");
    std::printf("\n");
}

// argv[1]: the moduli; every further argument: a bound's words, or pow:E, qmpow:E, half1, low
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::vector<uint64_t> q = parse_words(argv[1]);
    const int L = static_cast<int>(q.size());
    for (int a = 2; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg.rfind("pow:", 0) == 0) {
            print_bound(readout::power_of_two_bound(static_cast<unsigned>(std::atoi(arg.c_str() + 4)), q.data(), L), L);
        } else if (arg.rfind("qmpow:", 0) == 0) {
            print_bound(readout::q_minus_power_of_two_bound(static_cast<unsigned>(std::atoi(arg.c_str() + 6)), q.data(), L), L);
        } else if (arg == "half1") {
            print_bound(readout::half_plus_one_bound(q.data(), L), L);
        } else if (arg == "low") {
            std::vector<uint64_t> pw(q.size());
            uint64_t q_low = 0;
            readout::wrapping_prefix_products(q.data(), L, pw.data(), &q_low);
            std::printf("low %" PRIx64, q_low);
            for (int k = 0; k < L; ++k) std::printf(" %" PRIx64, pw[k]);
            std::printf("\n");
        } else {
            const std::vector<uint64_t> w = parse_words(argv[a]);
            readout::BoundDigits b;
            std::memset(&b, 0x5a, sizeof(b));
            if (readout::bound_digits(w.data(), w.size(), q.data(), L, &b)) {
                const unsigned char *raw = reinterpret_cast<const unsigned char *>(&b);
                bool untouched = true;
                for (size_t i = 0; i < sizeof(b); ++i) untouched = untouched && raw[i] == 0x5a;
                std::printf("refused %d\n", untouched ? 1 : 0);
            } else {
                print_bound(b, L);
            }
        }
    }
    return 0;
}
"""

# the (bits, limbs) of the device test's cells
BASES = [(10, 2), (24, 1), (24, 3), (24, 8), (24, 9), (28, 16), (28, 17), (31, 3), (51, 2), (51, 9), (62, 17), (60, 64)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("readout_bounds")
    src = d / "readout_bounds_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "readout_bounds_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # no dependence on where the dynamic runtime falls in the link order
           "-I", os.path.join(ROOT, "mxx_amd", "csrc"), str(src), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return str(exe)


def _words(v, n=None):
    n = max(1, -(-v.bit_length() // 64)) if n is None else n
    return ",".join(format((v >> (64 * w)) & ((1 << 64) - 1), "x") for w in range(n))


def _run(exe, moduli, args):
    run = subprocess.run([exe, ",".join(format(q, "x") for q in moduli)] + args, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    return run.stdout.splitlines()


def _digits_line(B, moduli):
    Q = math.prod(moduli)
    if B == Q:
        return "ok 1" + " 0" * len(moduli)
    digits, prefix = [], 1
    for q in moduli:
        digits.append(B // prefix % q)
        prefix *= q
    return "ok 0 " + " ".join(format(d, "x") for d in digits)


@pytest.mark.parametrize("bits,L", BASES)
def test_digits_flags_and_refusals_match_python(program, bits, L):
    moduli = P.primes(64, bits, L)
    Q = math.prod(moduli)
    rnd = random.Random(1000 * bits + L)
    wq = -(-Q.bit_length() // 64)
    bounds = [0, 1, Q - 1, Q, Q // 2, (Q // 2) >> 1, 3 * ((Q // 2) >> 1), moduli[0], Q // moduli[-1], Q - moduli[0]]
    bounds += [rnd.randrange(Q) for _ in range(8)]
    bounds = [b for b in bounds if 0 <= b <= Q]
    args = [_words(b) for b in bounds] + [_words(b, wq + 2) for b in bounds]  # with zero words above Q's words too
    lines = _run(program, moduli, args)
    assert lines == [_digits_line(b, moduli) for b in bounds] * 2
    # above Q: Q + 1, the next power of two of the word count, non-zero words above Q's words
    refused = [_words(Q + 1), _words(Q + moduli[0]), _words((1 << (64 * wq)) - 1) if (1 << (64 * wq)) - 1 > Q else _words(Q + 2),
               _words(1 << (64 * wq)), _words((1 << (64 * (wq + 1))) + 5, wq + 3)]
    assert _run(program, moduli, refused) == ["refused 1"] * len(refused)


@pytest.mark.parametrize("bits,L", BASES)
def test_fit_bounds_and_wrapping_products_match_python(program, bits, L):
    moduli = P.primes(64, bits, L)
    Q = math.prod(moduli)
    lines = _run(program, moduli, ["pow:32", "pow:64", "pow:31", "pow:63", "qmpow:31", "qmpow:63", "half1", "low"])
    want = [_digits_line(min(1 << e, Q), moduli) for e in (32, 64, 31, 63)]
    want += [_digits_line(max(Q - (1 << e), 0), moduli) for e in (31, 63)]
    want += [_digits_line(Q // 2 + 1, moduli)]
    mask = (1 << 64) - 1
    prefixes = [math.prod(moduli[:k]) & mask for k in range(L)]
    want += ["low " + " ".join(format(v, "x") for v in [Q & mask] + prefixes)]
    assert lines == want


def test_random_bases_through_the_program(program):
    """random bases of 1 to 6 odd moduli of 7 to 51 bits (not primes: the header asks for none): the program's digits of
    random bounds, of the values next to them and of the fit bounds against Python's"""
    rnd = random.Random(11)
    mask = (1 << 64) - 1
    for _ in range(25):
        L = rnd.randint(1, 6)
        moduli = [rnd.randrange(1 << 6, 1 << rnd.randint(7, 51)) | 1 for _ in range(L)]
        Q = math.prod(moduli)
        bounds = []
        for _ in range(6):
            B = rnd.randrange(Q)
            bounds += [v for v in (B, B - 1, B + 1, B - B % moduli[0], B + moduli[0], B - moduli[0]) if 0 <= v <= Q]
        lines = _run(program, moduli, [_words(b) for b in bounds] + ["pow:32", "pow:63", "qmpow:31", "qmpow:63", "half1", "low"])
        want = [_digits_line(b, moduli) for b in bounds]
        want += [_digits_line(min(1 << 32, Q), moduli), _digits_line(min(1 << 63, Q), moduli)]
        want += [_digits_line(max(Q - (1 << 31), 0), moduli), _digits_line(max(Q - (1 << 63), 0), moduli), _digits_line(Q // 2 + 1, moduli)]
        want += ["low " + " ".join(format(v, "x") for v in [Q & mask] + [math.prod(moduli[:k]) & mask for k in range(L)])]
        assert lines == want, moduli
        assert _run(program, moduli, [_words(Q + 1), _words(Q + rnd.randrange(1, Q))]) == ["refused 1"] * 2


def test_bad_bases_are_refused(program):
    assert _run(program, [5, 0, 7], ["1"]) == ["refused 1"]
    assert _run(program, [3] * 65, ["1"]) == ["refused 1"]


def test_comparator_and_wrapping_sum_identities():
    """The mathematics only - no project code runs here, and this passes whatever the header or the kernels do: the two
    identities the kernels rest on, c < B as the lexicographic comparison of the mixed-radix digits, top digit first, and
    c mod 2^64 as the wrapping sum of digit times prefix product.  The header's digits for random bases are checked by
    test_random_bases_through_the_program."""
    rnd = random.Random(7)
    mask = (1 << 64) - 1
    for _ in range(200):
        L = rnd.randint(1, 6)
        moduli = [rnd.randrange(1 << 6, 1 << rnd.randint(7, 51)) | 1 for _ in range(L)]
        Q = math.prod(moduli)

        def digits(x):
            out, prefix = [], 1
            for q in moduli:
                out.append(x // prefix % q)
                prefix *= q
            return out

        for _ in range(20):
            c, B = rnd.randrange(Q), rnd.randrange(Q)
            if rnd.random() < 0.3:
                B = min(Q - 1, max(0, c + rnd.choice([-1, 0, 1, moduli[0], -moduli[0]])))
            dc, dB = digits(c), digits(B)
            assert (dc[::-1] < dB[::-1]) == (c < B)
            assert sum(d * (math.prod(moduli[:k]) & mask) for k, d in enumerate(dc)) & mask == c & mask
