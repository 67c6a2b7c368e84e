"""CPU-only: the launch plan of the Gaussian lane samplers (mxx_amd/csrc/lane_plan.h) as a stand-alone program.

A small C++ program with its own `main` includes the header and prints the plan for every group of seven arguments on its
command line.  It is built with the address and undefined-behaviour sanitizers and run as a program; nothing is loaded into
Python.  The expected values are the rules the five launch sites spelled out by hand before they shared the header,
restated here in Python (`site_rules`): the lane count cut to a divisor of a span's wave-chunks, the rounded-up grid, the
three families' cadences, the forced cadence, the one-service choice and the UNI test.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64

PROGRAM = r"""
#include "lane_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// argv: groups of (total span raw_per_lane cut forced_fill family uni_form); one line per group
int main(int argc, char **argv) {
    if (argc < 8 || (argc - 1) % 7) return 2;
    for (int a = 1; a < argc; a += 7) {
        const size_t total = std::strtoull(argv[a], nullptr, 10), span = std::strtoull(argv[a + 1], nullptr, 10);
        const uint32_t raw = static_cast<uint32_t>(std::strtoul(argv[a + 2], nullptr, 10));
        const bool cut = std::atoi(argv[a + 3]) != 0, uni_form = std::atoi(argv[a + 6]) != 0;
        const int forced = std::atoi(argv[a + 4]);
        const char *family = argv[a + 5];
        const LaneCadence *cadence = !std::strcmp(family, "matrix") ? &kCadenceGaussMatrix
                                     : !std::strcmp(family, "gadget") ? &kCadenceGadget
                                     : !std::strcmp(family, "p1")     ? &kCadenceP1
                                                                      : nullptr;
        if (!cadence) return 3;
        const LanePlan p = lane_plan(total, span, raw, cut, forced, *cadence, uni_form);
        std::printf("%u %u %u %d %d %d\n", p.per_lane, p.blocks, p.fill_every, p.starve_limit, p.single ? 1 : 0, p.uni ? 1 : 0);
    }
    return 0;
}
"""


def site_rules(total, span, raw, cut, forced, family, uni_form):
    """what the launch sites computed by hand: (per_lane, blocks, fill_every, starve_limit, single, uni)"""
    per_lane = raw
    if cut:  # the segments entry, the blocks leg, the G-sampler and p1 with segments
        while (span // WAVE) % per_lane:
            per_lane -= 1
    blocks = (total + WAVE * per_lane - 1) // (WAVE * per_lane)
    if family == "matrix":  # plain, segments, blocks
        fill, starve = (1, 1) if per_lane == 1 else (3, 65)
    elif family == "gadget":  # G-sampler lanes: always 3; the kernel runs with the checkpoint's own starve limit of 16
        fill, starve = 3, 16
    else:  # p1: always 2
        fill, starve = 2, 16
    if forced:
        fill = forced
    uni = bool(uni_form) and span % (WAVE * per_lane) == 0
    return per_lane, blocks, fill, starve, int(per_lane == 1), int(uni)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_plan")
    src = d / "lane_plan_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "lane_plan_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # no dependence on where the dynamic runtime falls in the link order
           "-I", os.path.join(ROOT, "mxx_amd", "csrc"), str(src), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return str(exe)


def _check(program, cases):
    argv = [str(int(x)) if not isinstance(x, str) else x for c in cases for x in c]
    run = subprocess.run([program] + argv, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        assert tuple(int(x) for x in ln.split()) == site_rules(*c), c


RAW = (1, 2, 3, 8)
SPANS = tuple(WAVE * chunks for chunks in (1, 2, 4, 128))


def _totals(span):
    # whole spans (what the cut forms launch), and totals that end inside a wave, a lane's share and a span
    return sorted({span, 3 * span, 6 * span, 1, WAVE - 1, WAVE + 1, span + 1, 3 * span - 1, 5 * span + WAVE // 2, 6 * span + 3 * WAVE + 7})


@pytest.mark.parametrize("family", ["matrix", "gadget", "p1"])
def test_plan_equals_the_launch_sites_rules(program, family):
    """the family's default cadence and forced cadences 1..8; raw lane counts 1, 2, 3, 8 with and without the divisor cut at spans
    of 1, 2, 4 and 128 wave-chunks; totals that are no multiple of a wave; with and without a UNI form"""
    cases = [(total, span, raw, cut, forced, family, uni_form)
             for span in SPANS for total in _totals(span) for raw in RAW for cut in (0, 1) for forced in range(0, 9) for uni_form in (0, 1)]
    _check(program, cases)


def test_cut_lane_counts(program):
    """the divisor cut by hand: 8 -> 4 at four wave-chunks, 3 -> 2 at two and at 128, 3 -> 1 at one; uncut counts stay"""
    want = {(64, 8): 1, (128, 8): 2, (256, 8): 8 // 2, (8192, 8): 8, (64, 3): 1, (128, 3): 2, (256, 3): 2, (8192, 3): 2, (256, 2): 2, (64, 2): 1}
    for (span, raw), per_lane in want.items():
        assert site_rules(6 * span, span, raw, 1, 0, "matrix", 1)[0] == per_lane
        assert site_rules(6 * span, span, raw, 0, 0, "matrix", 1)[0] == raw
    _check(program, [(6 * span, span, raw, cut, 0, "matrix", 1) for (span, raw) in want for cut in (0, 1)])


def test_cadence_defaults(program):
    """the three families' figures, written out: (fill_every, starve_limit) at one element per lane and at more"""
    want = {"matrix": ((1, 1), (3, 65)), "gadget": ((3, 16), (3, 16)), "p1": ((2, 16), (2, 16))}
    for family, (single, many) in want.items():
        assert site_rules(640, 128, 1, 0, 0, family, 0)[2:4] == single
        assert site_rules(640, 128, 2, 0, 0, family, 0)[2:4] == many
        assert site_rules(640, 128, 2, 0, 5, family, 0)[2:4] == (5, many[1])  # forced: the refill figure alone
    _check(program, [(640, 128, raw, 0, forced, family, 0) for family in want for raw in (1, 2) for forced in (0, 5)])


def test_uni_rule_at_its_boundaries(program):
    """UNI holds exactly when a wave's chunk (64 * per_lane) divides the span: at the chunk itself and its multiples, not one
    wave to either side, never for a span below a wave (n = 64 in pairs) and never without a UNI form"""
    cases = []
    for raw, cut in itertools.product(RAW, (0, 1)):
        chunk = WAVE * raw
        for span in (chunk, 2 * chunk, 3 * chunk, chunk - WAVE, chunk + WAVE, 2 * chunk + WAVE, chunk // 2, 32, 96, 8192):
            if span <= 0:
                continue
            for uni_form in (0, 1):
                cases.append((5 * span, span, raw, cut, 0, "gadget", uni_form))
    assert site_rules(640, 128, 2, 0, 0, "matrix", 1)[5] == 1 and site_rules(960, 192, 2, 0, 0, "matrix", 1)[5] == 0
    assert site_rules(320, 64, 2, 0, 0, "matrix", 1)[5] == 0 and site_rules(320, 64, 2, 1, 0, "matrix", 1)[5] == 1  # the cut restores it
    assert site_rules(160, 32, 1, 0, 0, "matrix", 1)[5] == 0 and site_rules(640, 128, 2, 0, 0, "gadget", 0)[5] == 0
    _check(program, cases)
