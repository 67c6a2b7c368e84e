"""CPU-only: the host side of the slot-transfer evaluation (mxx_amd/csrc/slot_weights.h) as a stand-alone program.

A small C++ program with its own `main` includes the header and prints, for a basis given on the command line, the two weights
of a term in every limb - kappa mod q_l and kappa * mu mod q_l - for each (kappa, mu) pair, mu a big integer of several
little-endian 64-bit words.  It is built with the address and undefined-behaviour sanitizers and run as a program; nothing is
loaded into Python.  Expected values are Python's `kappa % q` and `kappa * mu % q`.
"""
import os
import random
import subprocess

import pytest

from test_ggh15_weights_host import CELLS, _moduli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "slot_weights.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<uint64_t> hex_list(const char *p) {
    std::vector<uint64_t> out;
    while (*p) {
        char *end = nullptr;
        out.push_back(std::strtoull(p, &end, 16));
        p = *end == ',' ? end + 1 : end;
    }
    return out;
}

// argv: words_per_mu moduli(comma-separated hex) kappas(comma-separated hex) mu words(comma-separated hex, words_per_mu per kappa):
// one line per kappa with 2 L words
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const size_t wpm = static_cast<size_t>(std::atoi(argv[1]));
    const std::vector<uint64_t> q = hex_list(argv[2]), kappas = hex_list(argv[3]), words = hex_list(argv[4]);
    if (words.size() != kappas.size() * wpm) return 3;
    for (size_t j = 0; j < kappas.size(); ++j) {
        const std::vector<uint64_t> mu(words.begin() + j * wpm, words.begin() + (j + 1) * wpm);  // exactly wpm words: a read past them is the sanitizer's to report
        std::vector<uint64_t> out(2 * q.size());                                                // exactly 2 L words, likewise for a write
        slot_eval::term_weights(kappas[j], mu.data(), wpm, q.data(), q.size(), out.data());
        for (uint64_t w : out) std::printf("%" PRIx64 " ", w);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("slot_weights")
    src = d / "slot_weights_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "slot_weights_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # no dependence on where the dynamic runtime falls in the link order
           "-I", os.path.join(ROOT, "mxx_amd", "csrc"), str(src), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return str(exe)


def _words(value, count):
    return [(value >> (64 * i)) & ((1 << 64) - 1) for i in range(count)]


@pytest.mark.parametrize("n,bits,base", CELLS)
def test_weights_equal_pythons_residues(program, n, bits, base):
    moduli = _moduli(n, bits)
    big_q = 1
    for q in moduli:
        big_q *= q
    rng = random.Random(23 * base + sum(bits))
    for wpm in (1, 3):
        top = 1 << (64 * wpm)
        # mu: 0, 1, Q - 1 (cut to the words where Q is longer), all-ones words (past every q_l: q_l < 2^62), random words;
        # kappa: 3, 0 (a legal weight), 1, 2^32 - 1, a full 64-bit word, 0 again, random
        mus = [0, 1, min(big_q, top) - 1, top - 1] + [rng.randrange(top) for _ in range(4)]
        kappas = [3, 0, 1, (1 << 32) - 1, (1 << 64) - 1, 0] + [rng.randrange(1 << 64) for _ in range(2)]
        assert len(mus) == len(kappas)
        assert all(mus[3] >= q for q in moduli) and (wpm == 1 or mus[3] >= 1 << 128)  # several words, past every modulus
        run = subprocess.run([program, str(wpm), ",".join(format(q, "x") for q in moduli), ",".join(format(k, "x") for k in kappas),
                              ",".join(format(w, "x") for mu in mus for w in _words(mu, wpm))], capture_output=True, text=True)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
        lines = run.stdout.splitlines()
        assert len(lines) == len(kappas)
        for kappa, mu, line in zip(kappas, mus, lines):
            got = [int(w, 16) for w in line.split()]
            want = [v for q in moduli for v in (kappa % q, kappa * mu % q)]
            assert got == want, (moduli, wpm, kappa, mu)
