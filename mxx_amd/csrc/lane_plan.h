// lane_plan.h - the launch plan of the persistent-lane Gaussian samplers (rng.h).  Plain C++, no
// HIP: tests/test_lane_plan_host.py builds it into a program of its own.
#pragma once

#include <stddef.h>
#include <stdint.h>

// threads per workgroup of the persistent-lane kernels (a lane's ring is 128 bytes of LDS: 8 KB per wave)
#ifndef SAMPLER_THREADS
#define SAMPLER_THREADS 64
#endif

// Keystream cadence of a kernel family: refills at every fill-th checkpoint, and the number of starving lanes that forces
// a pass in between, for launches of at most one element per lane (`single`) and for longer ones (`many`).
// MXX_HIP_SAMPLER_FILL_EVERY overrides the refill figure of every family.
struct LaneCadence {
    uint32_t fill_single, fill_many;
    int starve_single, starve_many;
};
// Gaussian matrix (plain entry, segments, blocks): a pair of coefficients per stream lasts ~42 steps, so refills are held
// to every third checkpoint and never forced - 64 lanes cannot reach 65 (sampling.hip has the counts).  With one group per
// lane the call lasts as long as its unluckiest lane's chain, which must not wait for keystream: every checkpoint.
constexpr LaneCadence kCadenceGaussMatrix{1, 3, 1, 65};
// G-sampler lanes: an element starts with block 0's leftover draws - every third checkpoint (trapdoor.hip has the A/B:
// every checkpoint 3.33 ms, every second 2.78, every third 2.63 on M3A).  This family's kernel and p1's take no starve
// limit: they run with rng_fill_wave's own 16.
constexpr LaneCadence kCadenceGadget{3, 3, 16, 16};
// p1 lanes: every second checkpoint (M3A: 0.47 -> 0.445 ms, every third 0.447)
constexpr LaneCadence kCadenceP1{2, 2, 16, 16};

struct LanePlan {
    uint32_t per_lane;    // elements per lane: a wave owns SAMPLER_THREADS * per_lane consecutive elements
    unsigned blocks;      // one-wave workgroups
    uint32_t fill_every;
    int starve_limit;
    bool single;          // per_lane == 1: the kernels' one-service superstep (rng.h, karney_urgent)
    bool uni;             // every wave's chunk lies inside one span: the kernels' UNI form
};

// total: elements of the launch.  span: elements a wave's chunk should stay inside (the groups of a polynomial, or N).
// raw_per_lane: sampler_per_lane's answer.  cut: lower it to a divisor of the span's wave-chunks, so that every chunk does
// stay inside one span (the segment and block forms need that; the caller has checked that span is a multiple of a wave).
// forced_fill: MXX_HIP_SAMPLER_FILL_EVERY, 0 = the family's own.  uni_form: the family has a UNI form and no switch turns
// it off.
inline LanePlan lane_plan(size_t total, size_t span, uint32_t raw_per_lane, bool cut, int forced_fill, const LaneCadence &cadence,
                          bool uni_form) {
    LanePlan p;
    p.per_lane = raw_per_lane;
    if (cut)
        while ((span / SAMPLER_THREADS) % p.per_lane) --p.per_lane;
    const size_t chunk = static_cast<size_t>(SAMPLER_THREADS) * p.per_lane;
    p.blocks = static_cast<unsigned>((total + chunk - 1) / chunk);
    p.single = p.per_lane == 1;
    p.fill_every = forced_fill ? static_cast<uint32_t>(forced_fill) : (p.single ? cadence.fill_single : cadence.fill_many);
    p.starve_limit = p.single ? cadence.starve_single : cadence.starve_many;
    p.uni = uni_form && span % chunk == 0;
    return p;
}
