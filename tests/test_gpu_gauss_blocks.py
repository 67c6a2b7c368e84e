"""GPU: many independently seeded Gaussian blocks in one call (`gpupoly_matrix_sample_gauss_blocks`,
`gpupoly_matrix_sample_hash_gauss_blocks`) and the samplers that ride on them.

The bar is the one of the seeded blocks: a block must be the matrix the plain sampler writes for it ALONE under its seed and
sigma, bit for bit, and that matrix is checked against the CPU restatement (oracle.sample_distribution)."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

SEEDED = "gpupoly_matrix_sample_gauss_blocks"
HASHED = "gpupoly_matrix_sample_hash_gauss_blocks"
GAUSS = 1
# (n, depth, bits, base_bits)
CONTEXTS = {
    "one_wave_per_poly": (128, 2, 28, 14),  # smallest ring served: 64 pairs per polynomial, per_lane forced to 1; 32-bit words
    "ggh15_ring": (256, 3, 51, 17),         # the GGH15 ring; 64-bit words
    "packable": (256, 2, 24, 12),           # a context whose uniform samples are stored packed: a Gaussian one must not be
    "eight_chunks": (1024, 2, 24, 12),      # 8 wave-chunks per polynomial
}
SIGMAS = (3.5, 4.578, 1e-9)  # 1e-9: the reference's own error_sigma (src/lookup/ggh15/gpu_tests.rs:119), the degenerate divisor
KEY = bytes((7 * i + 1) & 0xFF for i in range(32))


def params_of(gpu, oracle, name):
    return make_params(gpu, oracle, *CONTEXTS[name])


def seed_bytes(tag):
    return bytes((tag * 37 + 11 * i + 5) & 0xFF for i in range(32))


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(seed_bytes(tag))


def block_shape(t, polys):
    """an r x c with r * c == polys, varied with the block index: the stacked row must not depend on it"""
    shapes = [(r, polys // r) for r in range(1, polys + 1) if polys % r == 0]
    return shapes[t % len(shapes)]


def launches(lib, fn):
    c0 = lib.gpupoly_launch_count()
    fn()
    return lib.gpupoly_launch_count() - c0


# ---------------------------------------------------------------------------------------------------
# 1. both layouts against the plain sampler and the CPU restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_blocks_equal_the_plain_sampler_block_by_block(gpu, oracle, ctx, sigma):
    p = params_of(gpu, oracle, ctx)
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    for nblk in (1, 3, 65, 130):  # 65 and 130: past the 64 entries of the Gaussian segments' table
        seeds = [gseed(gpu, 1000 + t) for t in range(nblk)]
        for polys in (1, 6):
            stack = M.sample_gauss_blocks(p, seeds, sigma, block_polys=polys)
            assert stack.is_ntt and stack.size() == (nblk, polys) and stack.layout == "words"
            for t in range(nblk):
                r, c = block_shape(t, polys)
                alone = M.sample_distribution(p, r, c, GAUSS, sigma, seeds[t])
                assert stack.row_view(t, t + 1).reshape_view(r, c) == alone, f"stacked: block {t} of {nblk} as {r} x {c}"
                if t < 3 and (nblk, polys) == (3, 6):
                    want = oracle.matrix_ntt(oracle.sample_distribution(r, c, moduli, n, "gauss", sigma, seed_bytes(1000 + t)), moduli)
                    assert np.array_equal(alone.to_rns(), want)
                    assert np.array_equal(stack.to_rns()[t].reshape(want.shape), want)
    for rows in (1, 2):
        for widths in ([1, 3, 2], [1] * 130):
            seeds = [gseed(gpu, 2000 + j) for j in range(len(widths))]
            wide = M.sample_gauss_blocks(p, seeds, sigma, nrow=rows, seg_cols=widths)
            assert wide.is_ntt and wide.size() == (rows, sum(widths)) and wide.layout == "words"
            res = wide.to_rns()
            parts = []
            for lo in range(0, len(widths), 64):
                parts += wide.slice_columns(sum(widths[:lo]), sum(widths[:lo + 64])).split_columns(widths[lo:lo + 64])
            at = 0
            for j, (w, part) in enumerate(zip(widths, parts)):
                assert part == M.sample_distribution(p, rows, w, GAUSS, sigma, seeds[j]), f"columns: block {j} of {len(widths)}, {rows} rows"
                if j < 3 and len(widths) == 3:
                    want = oracle.matrix_ntt(oracle.sample_distribution(rows, w, moduli, n, "gauss", sigma, seed_bytes(2000 + j)), moduli)
                    assert np.array_equal(res[:, at:at + w], want)
                at += w


# ---------------------------------------------------------------------------------------------------
# 2. lane counts: 3 does not divide the 8 wave-chunks of a polynomial and is cut down to a divisor
# ---------------------------------------------------------------------------------------------------
def test_the_stack_does_not_depend_on_the_lane_count(gpu, oracle, hip_env):
    p = params_of(gpu, oracle, "eight_chunks")
    M = gpu.GpuDCRTPolyMatrix
    seeds = [gseed(gpu, 2500 + t) for t in range(5)]
    stacks = []
    for per_lane in ("1", "2", "3", "8"):
        hip_env.set("MXX_HIP_SAMPLER_PER_LANE", per_lane)
        stacks.append(M.sample_gauss_blocks(p, seeds, 4.578, block_polys=3))
        assert stacks[-1] == stacks[0], per_lane
        wide = M.sample_gauss_blocks(p, seeds, 4.578, nrow=1, seg_cols=[3] * 5)
        assert wide.reshape_view(5, 3) == stacks[0], per_lane  # one row: the columns layout is the same order of polynomials
    hip_env.unset("MXX_HIP_SAMPLER_PER_LANE")
    for t in range(5):
        assert stacks[0].row_view(t, t + 1) == M.sample_distribution(p, 1, 3, GAUSS, 4.578, seeds[t]), t


# ---------------------------------------------------------------------------------------------------
# 3. a block boundary between consecutive waves, first and last wave of the launch included
# ---------------------------------------------------------------------------------------------------
def test_blocks_change_on_consecutive_waves(gpu, oracle):
    p = params_of(gpu, oracle, "one_wave_per_poly")  # a wave is a polynomial
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    widths = [1, 2, 1]
    seeds = [gseed(gpu, 2700 + j) for j in range(3)]
    res = M.sample_gauss_blocks(p, seeds, 3.5, nrow=1, seg_cols=widths).to_rns()
    at = 0
    for j, w in enumerate(widths):
        alone = M.sample_distribution(p, 1, w, GAUSS, 3.5, seeds[j]).to_rns()
        assert np.array_equal(res[:, at:at + w], alone), j
        assert np.array_equal(alone, oracle.matrix_ntt(oracle.sample_distribution(1, w, moduli, n, "gauss", 3.5, seed_bytes(2700 + j)), moduli))
        at += w


# ---------------------------------------------------------------------------------------------------
# 4. the hashed entry and the hash sampler
# ---------------------------------------------------------------------------------------------------
def test_the_hashed_entry_equals_the_seeded_entry_under_device_hash_seeds(gpu, oracle):
    from mxx_amd.matrix import IndexedTags, device_hash_seeds

    p = params_of(gpu, oracle, "ggh15_ring")
    M = gpu.GpuDCRTPolyMatrix
    forms = {
        "table": [b"tag_" + t.to_bytes(8, "little") + b"x" * (t % 5) for t in range(70)],
        "decimal": IndexedTags(b"ggh15_gate_err_", 95, 70, decimal=True),
        "le64": IndexedTags(b"wee25_w_block_", 250, 70),
    }
    for name, tags in forms.items():
        seeds = device_hash_seeds(p, KEY, tags)
        assert len(seeds) == 70
        assert M.sample_hash_gauss_blocks(p, KEY, tags, 3.5, block_polys=2) == M.sample_gauss_blocks(p, seeds, 3.5, block_polys=2), name
        widths = [1 + t % 3 for t in range(70)]
        assert M.sample_hash_gauss_blocks(p, KEY, tags, 3.5, nrow=2, seg_cols=widths) == \
            M.sample_gauss_blocks(p, seeds, 3.5, nrow=2, seg_cols=widths), name


@pytest.mark.parametrize("n,expect_blocks", [(256, True), (16, False)])
def test_sample_hash_many_and_stacked_equal_the_loop(gpu, oracle, n, expect_blocks):
    """n = 256: the hashed Gaussian blocks; n = 16: they answer "unsupported" and the fallback must give the loop's matrices"""
    from mxx_amd import _ffi

    p = make_params(gpu, oracle, n, 2, 28, 14)
    M, sampler, dist = gpu.GpuDCRTPolyMatrix, gpu.GpuDCRTPolyHashSampler(), gpu.DistType.GaussDist(3.5)
    tags = [b"tag_" + t.to_bytes(8, "little") for t in range(70)]
    if not expect_blocks:
        with pytest.raises(_ffi.GpuPolyError, match="unsupported"):
            M.sample_hash_gauss_blocks(p, KEY, tags, 3.5, block_polys=2)
    loop = [sampler.sample_hash(p, KEY, tag, 2, 1, dist) for tag in tags]
    count = launches(_ffi.lib(), lambda: sampler.sample_hash_stacked(p, KEY, tags, 2, 1, dist))
    assert (count == 5) == expect_blocks, count
    many = sampler.sample_hash_many(p, KEY, tags, 2, 1, dist)
    stacked = sampler.sample_hash_stacked(p, KEY, tags, 2, 1, dist)
    assert len(many) == 70 and stacked.size() == (70, 2) and stacked.is_ntt
    for t in range(70):
        assert many[t].size() == (2, 1) and many[t] == loop[t], t
        assert stacked.row_view(t, t + 1).reshape_view(2, 1) == loop[t], t


def test_sample_uniform_many_equals_the_loop_under_the_same_seeds(gpu, oracle):
    from mxx_amd.sampler import seed_source

    p = params_of(gpu, oracle, "ggh15_ring")
    M, us = gpu.GpuDCRTPolyMatrix, gpu.GpuDCRTPolyUniformSampler()
    raw = [seed_bytes(2900 + t) for t in range(5)]
    for dist in (gpu.DistType.GaussDist(4.578), gpu.DistType.TernaryDist(), gpu.DistType.FinRingDist()):
        stack = us.sample_uniform_many(p, 2, 3, dist, 5, _seeds=[gpu.GpuRngSeed.from_bytes(b) for b in raw])
        with seed_source(raw):
            drawn = us.sample_uniform_many(p, 2, 3, dist, 5)
        assert stack.size() == (5, 6) and drawn == stack
        for t in range(5):
            alone = M.sample_distribution(p, 2, 3, dist.as_ffi(), dist.sigma, gpu.GpuRngSeed.from_bytes(raw[t]))
            assert stack.row_view(t, t + 1).reshape_view(2, 3) == alone, (dist, t)
    assert us.sample_uniform_many(p, 2, 3, gpu.DistType.GaussDist(4.578), 0).size() == (0, 6)


# ---------------------------------------------------------------------------------------------------
# 5. an output below the top level
# ---------------------------------------------------------------------------------------------------
def test_an_output_below_the_top_level_through_the_raw_entries(gpu, oracle):
    """`out` created at level 1 of the three-limb context and tagged COEFF: the entry samples limbs 0..1 only, as the plain entry
    does for such a matrix, and tags the result EVAL (an EVAL read-out of a matrix still tagged COEFF would transform it)."""
    from mxx_amd import _ffi

    p = params_of(gpu, oracle, "ggh15_ring")
    M, n, lib = gpu.GpuDCRTPolyMatrix, p.ring_dimension(), _ffi.lib()
    low = p.moduli()[:2]
    seeds = (gpu.GpuRngSeed * 3)(*[gseed(gpu, 3000 + t) for t in range(3)])
    stack = M(p, 3, 2, 1, False)
    _ffi.check_status(lib.gpupoly_matrix_sample_gauss_blocks(stack.raw, 3.5, seeds, 3, _ffi.GPUPOLY_BLOCKS_STACKED, None), SEEDED)
    wide = M(p, 2, 3, 1, False)
    cols = (C.c_size_t * 3)(1, 1, 1)
    _ffi.check_status(lib.gpupoly_matrix_sample_gauss_blocks(wide.raw, 3.5, seeds, 3, _ffi.GPUPOLY_BLOCKS_COLUMNS, cols), SEEDED)
    stack.is_ntt = wide.is_ntt = True
    got_stack, got_wide = stack.to_rns(), wide.to_rns()
    assert got_stack.shape == (3, 2, 2, n)
    for t in range(3):
        for shape, got in (((1, 2), got_stack[t].reshape(1, 2, 2, n)), ((2, 1), got_wide[:, t:t + 1])):
            want = oracle.matrix_ntt(oracle.sample_distribution(shape[0], shape[1], low, n, "gauss", 3.5, seed_bytes(3000 + t)), low)
            assert np.array_equal(got, want), (t, shape)


# ---------------------------------------------------------------------------------------------------
# 6. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_block_count(gpu, oracle):
    from mxx_amd import _ffi
    from mxx_amd.matrix import IndexedTags

    p = params_of(gpu, oracle, "ggh15_ring")
    M, lib = gpu.GpuDCRTPolyMatrix, _ffi.lib()
    seeds = [gseed(gpu, 4000 + j) for j in range(130)]
    many = launches(lib, lambda: M.sample_gauss_blocks(p, seeds, 3.5, nrow=1, seg_cols=[1] * 130))
    two = launches(lib, lambda: M.sample_gauss_blocks(p, seeds[:2], 3.5, nrow=1, seg_cols=[65, 65]))
    stacked = launches(lib, lambda: M.sample_gauss_blocks(p, seeds, 3.5, block_polys=1))
    hashed = launches(lib, lambda: M.sample_hash_gauss_blocks(p, KEY, IndexedTags(b"t_", 0, 130, decimal=True), 3.5, block_polys=1))
    hashed_two = launches(lib, lambda: M.sample_hash_gauss_blocks(p, KEY, [b"a", b"bc"], 3.5, nrow=1, seg_cols=[65, 65]))
    loop = launches(lib, lambda: [M.sample_distribution(p, 1, 1, GAUSS, 3.5, s) for s in seeds])
    print(f"launches: 130 blocks {many}, 2 blocks {two}, stacked {stacked}, hashed {hashed} / {hashed_two}, 130 plain calls {loop}")
    assert many == two == stacked == 4  # derive, sample, scatter, transform
    assert hashed == hashed_two == 5    # the hash in front
    assert hashed < loop


# ---------------------------------------------------------------------------------------------------
# 7. refusals: nothing launched, `out` (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_output_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    p = params_of(gpu, oracle, "packable")
    small = make_params(gpu, oracle, 16, 2, 24, 12)
    M, lib = gpu.GpuDCRTPolyMatrix, _ffi.lib()
    seeds = (gpu.GpuRngSeed * 3)(*[gseed(gpu, 5000 + t) for t in range(3)])
    tags, keep, _ = hash_tags_arg(KEY, [b"a", b"bc", b"def"])
    STACKED, COLUMNS = _ffi.GPUPOLY_BLOCKS_STACKED, _ffi.GPUPOLY_BLOCKS_COLUMNS
    sentinels = {id(q): oracle.random_matrix(91, 2, 3, q.moduli(), q.ring_dimension()) for q in (p, small)}

    def widths(*w):
        return (C.c_size_t * len(w))(*w)

    def seeded(out, sigma=3.5, src=seeds, nblk=2, layout=STACKED, seg_cols=None):
        return lib.gpupoly_matrix_sample_gauss_blocks(None if out is None else out.raw, sigma, src, nblk, layout, seg_cols)

    def hashed(out, sigma=3.5, src=tags, nblk=2, layout=STACKED, seg_cols=None):
        return lib.gpupoly_matrix_sample_hash_gauss_blocks(None if out is None else out.raw, sigma, None if src is None else C.byref(src),
                                                           nblk, layout, seg_cols)

    def check(entry, name, fn, word, params=p):
        sentinel = sentinels[id(params)]
        out = M.from_rns(params, sentinel, False)  # COEFF-tagged: a tag flipped to EVAL would change the COEFF read-out
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert entry in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name

    for entry, call in ((SEEDED, seeded), (HASHED, hashed)):
        cases = {
            "null out": (lambda out: call(None), ""),
            "null seeds or tags": (lambda out: call(out, src=None), "null"),
            "no blocks": (lambda out: call(out, nblk=0), ""),
            "more than 2^20 blocks": (lambda out: call(out, nblk=(1 << 20) + 1), ""),
            "unknown layout": (lambda out: call(out, layout=2), "layout"),
            "stacked with seg_cols": (lambda out: call(out, seg_cols=widths(1, 2)), "seg_cols"),
            "stacked rows": (lambda out: call(out, nblk=3), "row"),
            "columns without seg_cols": (lambda out: call(out, layout=COLUMNS), "seg_cols"),
            "zero width": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(3, 0)), "zero"),
            "widths short of the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 1)), "sum"),
            "widths past the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(2, 2)), "sum"),
            "sigma 0": (lambda out: call(out, sigma=0.0), "sigma must be positive"),
            "negative sigma": (lambda out: call(out, sigma=-3.5), "sigma must be positive"),
            "sigma NaN": (lambda out: call(out, sigma=float("nan"), layout=COLUMNS, seg_cols=widths(1, 2)), "sigma must be positive"),
        }
        for name, (fn, word) in cases.items():
            check(entry, name, fn, word)
        check(entry, "n = 16", lambda out: call(out), "unsupported", small)
        check(entry, "n = 16, columns", lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported", small)
        # the same calls succeed once the fault is gone, and an output without polynomials launches nothing and is tagged EVAL
        out = M.from_rns(p, sentinels[id(p)], False)
        assert call(out) == 0 and call(out, layout=COLUMNS, seg_cols=widths(1, 2)) == 0
        for empty, kw in ((M(p, 2, 0, 1, False), {}), (M(p, 0, 3, 1, False), dict(layout=COLUMNS, seg_cols=widths(1, 2)))):
            c0 = lib.gpupoly_launch_count()
            assert call(empty, **kw) == 0 and lib.gpupoly_launch_count() == c0
        hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
        check(entry, "reference keying", lambda out: call(out), "unsupported")
        check(entry, "reference keying, columns", lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported")
        hip_env.unset("MXX_HIP_RNG_COMPAT")
    # the older block entries still send the Gaussian distribution away
    out = M.from_rns(p, sentinels[id(p)], False)
    assert lib.gpupoly_matrix_sample_distribution_blocks(out.raw, GAUSS, seeds, 2, STACKED, None) != 0
    assert "unsupported" in _ffi.last_error_string()
    del keep


# ---------------------------------------------------------------------------------------------------
# 8. several callers at once: the table is per call
# ---------------------------------------------------------------------------------------------------
def test_two_threads_get_their_own_blocks(gpu, oracle):
    p = params_of(gpu, oracle, "ggh15_ring")
    M = gpu.GpuDCRTPolyMatrix
    sets = [[gseed(gpu, 6000 + 100 * k + t) for t in range(9)] for k in range(2)]
    want = [M.sample_gauss_blocks(p, s, 4.578, block_polys=4) for s in sets]
    got, errors = [[], []], []
    barrier = threading.Barrier(2)

    def worker(k):
        try:
            barrier.wait()
            for _ in range(8):
                got[k].append(M.sample_gauss_blocks(p, sets[k], 4.578, block_polys=4))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not (want[0] == want[1])
    for k in range(2):
        assert len(got[k]) == 8 and all(m == want[k] for m in got[k]), k
        for t in range(9):
            assert want[k].row_view(t, t + 1) == M.sample_distribution(p, 1, 4, GAUSS, 4.578, sets[k][t]), (k, t)
