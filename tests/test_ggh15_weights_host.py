"""CPU-only: the host side of the GGH15 public lookup (mxx_amd/csrc/ggh15_weights.h) as a stand-alone program.

A small C++ program with its own `main` includes the header and prints, for a basis, a base and a tower given on the command
line, the weights of the gy term for every digit position e and each value v: digit e' of v B^e mod q_tw, reduced into every
limb.  It is built with the address and undefined-behaviour sanitizers and run as a program; nothing is loaded into Python.
Expected values are Python's `((v << (e b)) % q >> (e' b)) % 2^b % q_l`, and `plainref.gadget_scalar_digits` for whole
constants.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import plainref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "ggh15_weights.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv: base_bits dpt tower moduli(comma-separated hex) values(comma-separated hex): one line per (value, e)
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const uint32_t base = static_cast<uint32_t>(std::atoi(argv[1])), dpt = static_cast<uint32_t>(std::atoi(argv[2]));
    const size_t tw = static_cast<size_t>(std::atoi(argv[3]));
    std::vector<uint64_t> lists[2];
    for (int a = 0; a < 2; ++a)
        for (const char *p = argv[4 + a]; *p;) {
            char *end = nullptr;
            lists[a].push_back(std::strtoull(p, &end, 16));
            p = *end == ',' ? end + 1 : end;
        }
    const std::vector<uint64_t> &q = lists[0];
    for (uint64_t v : lists[1])
        for (uint32_t e = 0; e < dpt; ++e) {
            std::vector<uint64_t> out(q.size() * dpt);  // exactly L dpt words: a write past them is the sanitizer's to report
            ggh15::gy_weights(v, q[tw], base, dpt, e, q.data(), q.size(), out.data());
            for (uint64_t w : out) std::printf("%" PRIx64 " ", w);
            std::printf("\n");
        }
    return 0;
}
"""

# (n for the primes' congruence, bits of each tower, base_bits): the device test's width classes, short last digits (13 of 15,
# 20 of 57 and 61), dpt 6 and 11, and mixed widths whose digits - and 2^base itself - exceed the narrow modulus
CELLS = [(64, (10, 10), 5), (256, (15, 15), 13), (256, (24, 24, 24), 12), (256, (31, 31), 16), (256, (31, 31), 6), (256, (51, 51, 51), 17),
         (256, (57, 57), 20), (256, (61, 61), 20), (256, (62, 62), 31), (256, (62, 62), 6), (64, (51, 12), 17), (256, (41, 31), 31),
         (256, (51, 33), 34), (2, (17,), 17)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("ggh15_weights")
    src = d / "ggh15_weights_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "ggh15_weights_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # no dependence on where the dynamic runtime falls in the link order
           "-I", os.path.join(ROOT, "mxx_amd", "csrc"), str(src), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return str(exe)


def _moduli(n, bits):
    out = []
    for b in bits:
        out.append(next(q for q in P.primes(n, b, len(bits)) if q not in out))
    return out


@pytest.mark.parametrize("n,bits,base", CELLS)
def test_weights_equal_the_digits_of_the_scaled_residue(program, n, bits, base):
    moduli = _moduli(n, bits)
    dpt = P.digits_per_tower(moduli, base)
    rng = random.Random(17 * base + sum(bits))
    for tw, q in enumerate(moduli):
        values = [0, 1, q - 1, q // 2, (1 << (q.bit_length() - 1)) - 1] + [rng.randrange(q) for _ in range(3)]
        run = subprocess.run([program, str(base), str(dpt), str(tw), ",".join(format(m, "x") for m in moduli),
                              ",".join(format(v, "x") for v in values)], capture_output=True, text=True)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
        lines = run.stdout.splitlines()
        assert len(lines) == len(values) * dpt
        for i, v in enumerate(values):
            # plainref: column (tw, e) of G^-1(g o v) holds the digits of the element that is v 2^(e b) mod q_tw in tower tw
            const = np.zeros((len(moduli), 1), dtype=np.uint64)
            const[tw, 0] = v
            block = P.gadget_scalar_digits(const, moduli, base, dpt)  # (k, k, L, 1)
            for e in range(dpt):
                got = [int(w, 16) for w in lines[i * dpt + e].split()]
                scaled = (v << (e * base)) % q
                want = [(scaled >> (ep * base)) % (1 << base) % ql for ql in moduli for ep in range(dpt)]
                assert got == want, (moduli, base, tw, v, e)
                rows = block[tw * dpt:(tw + 1) * dpt, tw * dpt + e, :, 0]  # (dpt, L)
                assert got == [int(rows[ep, l]) for l in range(len(moduli)) for ep in range(dpt)], (moduli, base, tw, v, e)
