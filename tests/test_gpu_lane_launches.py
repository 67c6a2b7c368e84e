"""GPU: grid and trace label of the Gaussian lane kernels at every launch site, for forced lane counts 1, 2, 3 and 8.

The five sites - the plain sampler, the segments entry, the blocks leg, the G-sampler's lanes and p1's lanes, the latter two
with their segment forms and p1 with its keyed form - take elements per lane, grid, cadence and the choice of instance from
one plan (mxx_amd/csrc/lane_plan.h).  Each case runs one call with the launch trace on and compares the recorded
(label, workgroups, threads) of the lane kernel with the rules the sites spelled out by hand before
(`test_lane_plan_host.site_rules`).  The labels are the strings the library recorded before the sites shared the plan; a
profile or a roofline keyed on them (bench.py composes its rooflines from the trace) keeps reading the same names.
The default lane count is not pinned: it follows the occupancy the runtime reports.
"""
import pytest

from conftest import make_params, rand_matrix
from test_gpu_preimage_abi import SIGMA, eval_targets, explicit_seeds
from test_gpu_preimage_batch import gseed
from test_gpu_preimage_dim import _cache, _keyed
from test_lane_plan_host import site_rules

pytestmark = pytest.mark.gpu

N = 256
PER_LANE = pytest.mark.parametrize("per_lane", [1, 2, 3, 8])
WORDS = {"u32": (24, 12), "u64": (51, 17)}  # two limbs of (bits, base): 32-bit and 64-bit words
WORD = pytest.mark.parametrize("word", list(WORDS))

# keyed by (single, uni) / by single: one service point per superstep at one element per lane, else two
PLAIN = {(1, 1): "sample_gauss_kernel<1, true>", (1, 0): "sample_gauss_kernel<1, false>",
         (0, 1): "sample_gauss_kernel<2, true>", (0, 0): "sample_gauss_kernel<2, false>"}
SEGMENTS = {1: "sample_gauss_kernel<1, true, true>", 0: "sample_gauss_kernel<2, true, true>"}
BLOCKS = {1: "sample_gauss_blocks_kernel<1>", 0: "sample_gauss_blocks_kernel<2>"}
GSAMP = {(1, 1): "gauss_samp_lanes_kernel<W, MAXD, 1, true>", (1, 0): "gauss_samp_lanes_kernel<W, MAXD, 1, false>",
         (0, 1): "gauss_samp_lanes_kernel<W, MAXD, 2, true>", (0, 0): "gauss_samp_lanes_kernel<W, MAXD, 2, false>"}
GSAMP_SEGMENTS = {1: "gauss_samp_lanes_kernel<W, MAXD, 1, true, true>", 0: "gauss_samp_lanes_kernel<W, MAXD, 2, true, true>"}
# keyed by (word, m, form, single)
P1 = {
    ("u32", 2, "plain", 1): "p1_sample_lanes_kernel<uint32_t, 2, 1, false>",
    ("u32", 2, "plain", 0): "p1_sample_lanes_kernel<uint32_t, 2, 2, false>",
    ("u32", 2, "segments", 1): "p1_sample_lanes_kernel<uint32_t, 2, 1, true>",
    ("u32", 2, "segments", 0): "p1_sample_lanes_kernel<uint32_t, 2, 2, true>",
    ("u32", 2, "keyed", 1): "p1_sample_lanes_kernel<uint32_t, 2, 1, true, true>",
    ("u32", 2, "keyed", 0): "p1_sample_lanes_kernel<uint32_t, 2, 2, true, true>",
    ("u32", 6, "plain", 1): "p1_sample_lanes_kernel<uint32_t, 8, 1, false>",
    ("u32", 6, "plain", 0): "p1_sample_lanes_kernel<uint32_t, 8, 2, false>",
    ("u32", 6, "segments", 1): "p1_sample_lanes_kernel<uint32_t, 8, 1, true>",
    ("u32", 6, "segments", 0): "p1_sample_lanes_kernel<uint32_t, 8, 2, true>",
    ("u32", 6, "keyed", 1): "p1_sample_lanes_kernel<uint32_t, 8, 1, true, true>",
    ("u32", 6, "keyed", 0): "p1_sample_lanes_kernel<uint32_t, 8, 2, true, true>",
    ("u64", 2, "plain", 1): "p1_sample_lanes_kernel<uint64_t, 2, 1, false>",
    ("u64", 2, "plain", 0): "p1_sample_lanes_kernel<uint64_t, 2, 2, false>",
    ("u64", 2, "segments", 1): "p1_sample_lanes_kernel<uint64_t, 2, 1, true>",
    ("u64", 2, "segments", 0): "p1_sample_lanes_kernel<uint64_t, 2, 2, true>",
    ("u64", 2, "keyed", 1): "p1_sample_lanes_kernel<uint64_t, 2, 1, true, true>",
    ("u64", 2, "keyed", 0): "p1_sample_lanes_kernel<uint64_t, 2, 2, true, true>",
    ("u64", 6, "plain", 1): "p1_sample_lanes_kernel<uint64_t, 8, 1, false>",
    ("u64", 6, "plain", 0): "p1_sample_lanes_kernel<uint64_t, 8, 2, false>",
    ("u64", 6, "segments", 1): "p1_sample_lanes_kernel<uint64_t, 8, 1, true>",
    ("u64", 6, "segments", 0): "p1_sample_lanes_kernel<uint64_t, 8, 2, true>",
    ("u64", 6, "keyed", 1): "p1_sample_lanes_kernel<uint64_t, 8, 1, true, true>",
    ("u64", 6, "keyed", 0): "p1_sample_lanes_kernel<uint64_t, 8, 2, true, true>",
}


def lane_launch(gpu, hip_env, per_lane, kernel, call):
    """(label, workgroups, threads) of the one launch of `kernel` that `call` makes with `per_lane` elements per lane forced"""
    from mxx_amd import _ffi

    hip_env.set("MXX_HIP_SAMPLER_PER_LANE", str(per_lane))
    gpu.gpu_device_sync()
    _ffi.trace_begin()
    try:
        call()
        gpu.gpu_device_sync()
    finally:
        tr = _ffi.trace_end()
    hits = [(t["kernel"], t["blocks"], t["threads"]) for t in tr if t["kernel"].split("<")[0] == kernel]
    assert len(hits) == 1, [t["kernel"] for t in tr]
    return hits[0]


def params(gpu, oracle, word, n=N, base=None):
    bits, own_base = WORDS[word]
    return make_params(gpu, oracle, n, 2, bits, base or own_base)


def gauss(gpu):
    return gpu.DistType.GaussDist(SIGMA).as_ffi()


# ---------------------------------------------------------------------------------------------------
# the Gaussian matrix: plain, segments, blocks (a stream per pair of coefficients: 128 pairs per polynomial at n = 256)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N, 64], ids=["n256", "n64_never_uni"])
@WORD
@PER_LANE
def test_plain_sampler(gpu, oracle, hip_env, per_lane, word, n):
    p = params(gpu, oracle, word, n)
    M = gpu.GpuDCRTPolyMatrix
    got = lane_launch(gpu, hip_env, per_lane, "sample_gauss_kernel", lambda: M.sample_distribution(p, 2, 3, gauss(gpu), SIGMA, gseed(gpu, 1)))
    plan = site_rules(6 * n // 2, n // 2, per_lane, 0, 0, "matrix", 1)
    assert got == (PLAIN[plan[4], plan[5]], plan[1], 64)
    assert plan[5] == int(n == N and per_lane <= 2)  # half a wave of pairs at n = 64; 128 pairs hold a chunk of 64 or 128


@WORD
@PER_LANE
def test_segments_entry(gpu, oracle, hip_env, per_lane, word):
    p = params(gpu, oracle, word)
    M = gpu.GpuDCRTPolyMatrix
    seeds = [gseed(gpu, 10 + j) for j in range(3)]
    got = lane_launch(gpu, hip_env, per_lane, "sample_gauss_kernel", lambda: M.sample_distribution_segments(p, 2, [1, 1, 1], gauss(gpu), SIGMA, seeds))
    plan = site_rules(6 * N // 2, N // 2, per_lane, 1, 0, "matrix", 1)
    assert plan[0] == min(per_lane, 2)  # two wave-chunks per polynomial
    assert got == (SEGMENTS[plan[4]], plan[1], 64)


@WORD
@PER_LANE
def test_blocks_leg(gpu, oracle, hip_env, per_lane, word):
    p = params(gpu, oracle, word)
    M = gpu.GpuDCRTPolyMatrix
    seeds = [gseed(gpu, 20 + j) for j in range(3)]
    got = lane_launch(gpu, hip_env, per_lane, "sample_gauss_blocks_kernel", lambda: M.sample_gauss_blocks(p, seeds, SIGMA, nrow=2, seg_cols=[1, 1, 1]))
    plan = site_rules(6 * N // 2, N // 2, per_lane, 1, 0, "matrix", 1)
    assert got == (BLOCKS[plan[4]], plan[1], 64)


# ---------------------------------------------------------------------------------------------------
# the G-sampler's lanes: an element per (polynomial, tower, coefficient), one and three digits per tower
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("digits", [1, 3])
@WORD
@PER_LANE
def test_g_sampler_lanes(gpu, oracle, hip_env, per_lane, word, digits, segments):
    bits = WORDS[word][0]
    base = bits // digits
    p = params(gpu, oracle, word, base=base)
    assert p.modulus_digits() == 2 * digits
    M = gpu.GpuDCRTPolyMatrix
    src = M.from_rns(p, rand_matrix(oracle, 31, 2, 3, p.moduli(), N), False)
    c = ((1 << base) + 1) * SIGMA
    if segments:
        seeds = [gseed(gpu, 30 + j) for j in range(3)]
        call = lambda: src.gauss_samp_gq_arb_base_segments(c, SIGMA, seeds, [1, 1, 1])
    else:
        call = lambda: src.gauss_samp_gq_arb_base(c, SIGMA, gseed(gpu, 3))
    got = lane_launch(gpu, hip_env, per_lane, "gauss_samp_lanes_kernel", call)
    plan = site_rules(6 * 2 * N, N, per_lane, int(segments), 0, "gadget", 1)
    label = GSAMP_SEGMENTS[plan[4]] if segments else GSAMP[plan[4], plan[5]]
    assert got == (label, plan[1], 64)


# ---------------------------------------------------------------------------------------------------
# p1's lanes: an element per (column, coefficient); m = 2 and m = 6 rows (the two- and the eight-row instances)
# ---------------------------------------------------------------------------------------------------
_WORLDS = {}


def world(gpu, oracle, word, d):
    """parameters, sampler, two trapdoors of dimension d and the first one's covariance cache: made once, left unchanged"""
    if (word, d) not in _WORLDS:
        p = params(gpu, oracle, word)
        sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, SIGMA)
        keys = [sampler.trapdoor(p, d) for _ in range(2)]
        _WORLDS[word, d] = (p, sampler, keys, _cache(sampler, p, keys[0][0], d))
    return _WORLDS[word, d]


@pytest.mark.parametrize("form", ["plain", "segments", "keyed"])
@pytest.mark.parametrize("d", [1, 3], ids=["m2", "m6"])
@WORD
@PER_LANE
def test_p1_lanes(gpu, oracle, hip_env, per_lane, word, d, form):
    p, sampler, keys, cache = world(gpu, oracle, word, d)
    M = gpu.GpuDCRTPolyMatrix
    cols = 3
    if form == "keyed":  # a request of one column per key: every request's perturbation is padded to d columns
        _, targets = eval_targets(gpu, oracle, p, d, [1, 1, 1], 9100)
        seeds = explicit_seeds(gpu, 3, 1500)
        call = lambda: _keyed(gpu, sampler, p, keys, [0, 1, 0], targets, seeds)
        cols = 3 * d
    else:
        tp2 = M.sample_distribution(p, 2 * d, cols, gauss(gpu), 3.0e5, gseed(gpu, 9))
        if form == "segments":
            seeds = [gseed(gpu, 40 + j) for j in range(3)]
            call = lambda: M.sample_p1_full_cached_segments(cache, tp2, seeds, [1, 1, 1])
        else:
            call = lambda: M.sample_p1_full_cached(cache, tp2, gseed(gpu, 4))
    got = lane_launch(gpu, hip_env, per_lane, "p1_sample_lanes_kernel", call)
    plan = site_rules(cols * N, N, per_lane, int(form != "plain"), 0, "p1", 0)
    assert got == (P1[word, 2 * d, form, plan[4]], plan[1], 64)
