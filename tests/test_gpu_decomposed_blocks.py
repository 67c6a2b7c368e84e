"""GPU: G^-1 of many independently seeded samples in one call (`gpupoly_matrix_sample_decomposed_blocks`,
`gpupoly_matrix_sample_hash_decomposed_blocks`).

The bar: block t of the wide result is, bit for bit (gpu_matrix_equal), what `gpupoly_matrix_sample_decomposed_window`
writes ALONE under block t's seed for the same window, in the format the output was created with; for three blocks that
matrix is also held to the CPU restatement (oracle.sample_distribution + oracle.decompose).  The window call of a seed is
made once per (distribution, small, rows, window, format) and shared by the four block counts."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_sample_decomposed_blocks"
HASH_ENTRY = "gpupoly_matrix_sample_hash_decomposed_blocks"
DISTS = ("uniform", "bit", "ternary")
# word class -> (n, depth, bits, base_bits): the tuples of tests/test_gpu_sample_blocks.py
CONTEXTS = {
    "u32_packed24": (16, 2, 24, 12),
    "u32_words": (16, 2, 28, 14),
    "u64": (16, 2, 51, 17),
    "partial_group": (4, 1, 24, 12),       # fewer than eight coefficients per polynomial
    "ggh15_small_ring": (256, 3, 51, 17),  # the GGH15 chain's ring
}
NBLK = (1, 3, 65, 130)  # 65 and 130: past one workgroup's polynomials and the 64 entries of the segment tables
WINDOWS = ((6, 0, 6), (6, 2, 3), (7, 6, 1))  # (full_ncol, col_offset, c): the whole matrix, an inner window, the ragged last column
KEY = bytes((13 * i + 7) & 0xFF for i in range(32))


def seed_bytes(tag):
    return bytes((tag * 37 + 11 * i + 5) & 0xFF for i in range(32))


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(seed_bytes(tag))


def blocks_of(wide, nblk, c):
    """the nblk column blocks of `wide`, 64 per split_columns call"""
    out = []
    for lo in range(0, nblk, 64):
        hi = min(lo + 64, nblk)
        piece = wide if (lo, hi) == (0, nblk) else wide.slice_columns(lo * c, hi * c)
        out += piece.split_columns([c] * (hi - lo))
    return out


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_every_block_equals_the_window_entry_alone(gpu, oracle, ctx, dist):
    p = make_params(gpu, oracle, *CONTEXTS[ctx])
    M, moduli, n, code, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), oracle.DIST[dist], p.base_bits()
    seeds = [gseed(gpu, 7000 + t) for t in range(max(NBLK))]
    for small in (False, True):
        k = -(-p.crt_bits() // base) * (1 if small else len(moduli))
        for rows in (1, 2):
            for full, off, c in WINDOWS:
                for is_ntt in (True, False):
                    alone = [M.sample_distribution_decomposed_window(p, rows, full, off, c, code, 0.0, s, small, is_ntt=is_ntt) for s in seeds]
                    for nblk in NBLK:
                        wide = M.sample_decomposed_blocks(p, seeds[:nblk], rows, full, off, c, code, small=small, is_ntt=is_ntt)
                        assert wide.size() == (rows * k, nblk * c) and wide.is_ntt == is_ntt
                        for t, block in enumerate(blocks_of(wide, nblk, c)):
                            assert block.is_ntt == alone[t].is_ntt == is_ntt
                            assert block == alone[t], f"block {t} of {nblk}: small={small} rows={rows} window={(full, off, c)} ntt={is_ntt}"
                        if nblk == 3:
                            got = wide.to_coeff_rns()
                            for t in range(3):
                                src = oracle.sample_distribution(rows, c, moduli, n, dist, 0.0, seed_bytes(7000 + t), full_ncol=full, col_offset=off)
                                want = oracle.decompose(src, moduli, base, small)
                                assert np.array_equal(got[:, t * c:(t + 1) * c], want), (t, small, rows, (full, off, c), is_ntt)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("dist", DISTS)
def test_an_output_below_the_top_level(gpu, oracle, dist, level):
    """`out` at level 0 / 1 of the three-limb ring: k = dpt * (level + 1) digit rows per source row with dpt from the CONTEXT's
    crt_bits (the same number, in this same-width basis, as oracle.decompose derives from the truncated basis it is handed);
    every block against the CPU restatement at that basis and against the window entry alone, seeded and hashed forms."""
    from mxx_amd.matrix import device_hash_seeds

    p = make_params(gpu, oracle, *CONTEXTS["ggh15_small_ring"])
    M, n, code, base = gpu.GpuDCRTPolyMatrix, p.ring_dimension(), oracle.DIST[dist], p.base_bits()
    moduli = p.moduli()[: level + 1]
    dpt = -(-p.crt_bits() // base)
    assert level < p.crt_depth() - 1 and oracle.digits_per_tower(moduli, base) == dpt
    seeds = [gseed(gpu, 7500 + t) for t in range(3)]
    tags = [b"low_" + bytes([t]) for t in range(3)]
    rows, (full, off, c) = 2, WINDOWS[1]
    for small in (False, True):
        k = dpt * (1 if small else level + 1)
        for is_ntt in (True, False):
            wide = M.sample_decomposed_blocks(p, seeds, rows, full, off, c, code, small=small, is_ntt=is_ntt, level=level)
            assert wide.level == level and wide.size() == (rows * k, 3 * c) and wide.is_ntt == is_ntt
            got = wide.to_rns()
            for t, block in enumerate(blocks_of(wide, 3, c)):
                src = oracle.sample_distribution(rows, c, moduli, n, dist, 0.0, seed_bytes(7500 + t), full_ncol=full, col_offset=off)
                want = oracle.decompose(src, moduli, base, small)
                assert np.array_equal(got[:, t * c:(t + 1) * c], oracle.matrix_ntt(want, moduli) if is_ntt else want), (t, small, is_ntt)
                alone = M.sample_distribution_decomposed_window(p, rows, full, off, c, code, 0.0, seeds[t], small, is_ntt=is_ntt, level=level)
                assert block == alone, (t, small, is_ntt)
            hashed = M.sample_hash_decomposed_blocks(p, KEY, tags, rows, full, off, c, code, small=small, is_ntt=is_ntt, level=level)
            assert hashed == M.sample_decomposed_blocks(p, device_hash_seeds(p, KEY, tags), rows, full, off, c, code, small=small,
                                                        is_ntt=is_ntt, level=level), (small, is_ntt)


def test_hashed_form_equals_the_seeds_given_form_for_every_tag_form(gpu, oracle):
    from mxx_amd.matrix import device_hash_seeds

    p = make_params(gpu, oracle, *CONTEXTS["ggh15_small_ring"])
    M, code = gpu.GpuDCRTPolyMatrix, oracle.DIST["uniform"]
    forms = {
        "table": [b"", b"a", b"ggh15_lut_v_idx_3_17", bytes(range(200)), b"a"],
        "le64": gpu.IndexedTags(b"wee25_w_block_", (1 << 32) - 2, 5),
        "decimal": gpu.IndexedTags(b"ggh15_lut_v_idx_3_", 98, 5, decimal=True),
    }
    for name, tags in forms.items():
        seeds = device_hash_seeds(p, KEY, tags)  # gpupoly_hash_seeds
        for small, is_ntt in ((False, True), (True, False)):
            want = M.sample_decomposed_blocks(p, seeds, 2, 7, 2, 3, code, small=small, is_ntt=is_ntt)
            got = M.sample_hash_decomposed_blocks(p, KEY, tags, 2, 7, 2, 3, code, small=small, is_ntt=is_ntt)
            assert got.is_ntt == is_ntt and got == want, (name, small)
    # the mirror's many-tags call: the loop's matrices
    sampler, fin = gpu.GpuDCRTPolyHashSampler(), gpu.DistType.FinRingDist()
    tags = [b"tag_" + bytes([t]) for t in range(70)]
    many = sampler.sample_hash_decomposed_columns_many(p, KEY, tags, 2, 7, 2, 3, fin)
    assert len(many) == 70
    for t in (0, 1, 63, 64, 69):
        assert many[t] == sampler.sample_hash_decomposed_columns(p, KEY, tags[t], 2, 7, 2, 3, fin), t
    assert sampler.sample_hash_decomposed_columns_many(p, KEY, [], 2, 7, 2, 3, fin) == []


def test_the_launches_do_not_depend_on_the_block_count(gpu, oracle):
    from mxx_amd import _ffi

    p = make_params(gpu, oracle, *CONTEXTS["ggh15_small_ring"])
    M, code = gpu.GpuDCRTPolyMatrix, oracle.DIST["uniform"]
    seeds = [gseed(gpu, 8000 + t) for t in range(130)]
    tags = gpu.IndexedTags(b"ggh15_lut_v_idx_3_", 0, 130, decimal=True)

    def kernels(fn):
        _ffi.trace_begin()
        fn()
        return [e["kernel"] for e in _ffi.trace_end() if e["threads"]]  # copies are traced with no threads

    many = kernels(lambda: M.sample_decomposed_blocks(p, seeds, 2, 7, 2, 3, code))
    two = kernels(lambda: M.sample_decomposed_blocks(p, seeds[:2], 2, 7, 2, 3, code))
    hashed = kernels(lambda: M.sample_hash_decomposed_blocks(p, KEY, tags, 2, 7, 2, 3, code))
    hashed_two = kernels(lambda: M.sample_hash_decomposed_blocks(p, KEY, tags[:2], 2, 7, 2, 3, code))
    loop = kernels(lambda: [M.sample_distribution_decomposed_window(p, 2, 7, 2, 3, code, 0.0, s) for s in seeds[:2]])
    print(f"launches: 130 blocks {many}, 2 blocks {two}, hashed {hashed}, 2 window calls {len(loop)}")
    assert many == two and 0 < len(many) < len(loop)
    assert hashed == hashed_two and len(hashed) == len(many) + 1 and hashed[0] == "hash_seeds_kernel" and hashed[1:] == many


def test_refusals_launch_nothing_and_leave_the_output_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    p = make_params(gpu, oracle, *CONTEXTS["u32_packed24"])
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    k = p.modulus_digits()  # 4
    sentinel = oracle.random_matrix(92, 2 * k, 6, moduli, n)
    seeds = (gpu.GpuRngSeed * 3)(*[gseed(gpu, 9000 + t) for t in range(3)])
    arg, keep, _ = hash_tags_arg(KEY, [b"x", b"yy", b"zzz"])

    def call(out, dist=0, seeds_=seeds, nblk=3, base_bits=base, small=0, src_rows=2, full=7, off=2):
        return lib.gpupoly_matrix_sample_decomposed_blocks(None if out is None else out.raw, dist, seeds_, nblk, base_bits, small, src_rows, full, off)

    def hcall(out, tags_=arg, nblk=3, dist=0, base_bits=base, src_rows=2, full=7, off=2):
        return lib.gpupoly_matrix_sample_hash_decomposed_blocks(None if out is None else out.raw, dist, None if tags_ is None else C.byref(tags_),
                                                                nblk, base_bits, 0, src_rows, full, off)

    bad_hash, _k1, _ = hash_tags_arg(KEY, [b"x", b"yy", b"zzz"])
    bad_hash.hash = 7
    bad_offsets, _k2, _ = hash_tags_arg(KEY, [b"x", b"yy", b"zzz"])
    bad_offsets.tag_offsets[2] = 0  # decreasing
    cases = {
        "null out": (lambda out: call(None), "", ENTRY),
        "null seeds": (lambda out: call(out, seeds_=None), "", ENTRY),
        "no blocks": (lambda out: call(out, nblk=0), "", ENTRY),
        "more than 2^20 blocks": (lambda out: call(out, nblk=(1 << 20) + 1), "", ENTRY),
        "gaussian": (lambda out: call(out, dist=1), "unsupported", ENTRY),
        "dist_type 4": (lambda out: call(out, dist=4), "dist_type", ENTRY),
        "dist_type -1": (lambda out: call(out, dist=-1), "dist_type", ENTRY),
        "columns not a multiple of the blocks": (lambda out: call(out, nblk=4), "multiple", ENTRY),
        "window past full_ncol": (lambda out: call(out, full=3), "full_ncol", ENTRY),
        "offset past full_ncol": (lambda out: call(out, off=8), "full_ncol", ENTRY),
        "rows": (lambda out: call(out, src_rows=1), "rows", ENTRY),
        "rows, small": (lambda out: call(out, small=1), "rows", ENTRY),
        "base_bits 0": (lambda out: call(out, base_bits=0), "base_bits", ENTRY),
        "base_bits 63": (lambda out: call(out, base_bits=63), "base_bits", ENTRY),
        "48-bit stream ids": (lambda out: call(out, full=1 << 47), "48-bit", ENTRY),
        "hashed: null out": (lambda out: hcall(None), "", HASH_ENTRY),
        "hashed: null tags": (lambda out: hcall(out, tags_=None), "", HASH_ENTRY),
        "hashed: gaussian": (lambda out: hcall(out, dist=1), "unsupported", HASH_ENTRY),
        "hashed: window": (lambda out: hcall(out, full=3), "full_ncol", HASH_ENTRY),
        "hashed: rows": (lambda out: hcall(out, src_rows=3), "rows", HASH_ENTRY),
        "hashed: base_bits": (lambda out: hcall(out, base_bits=64), "base_bits", HASH_ENTRY),
        "hashed: unknown hash": (lambda out: hcall(out, tags_=bad_hash), "", HASH_ENTRY),
        "hashed: decreasing offsets": (lambda out: hcall(out, tags_=bad_offsets), "", HASH_ENTRY),
    }

    def check(name, fn, word, entry):
        out = M.from_rns(p, sentinel, False)  # COEFF-tagged: a tag flipped to EVAL would change the COEFF read-out
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert entry in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name

    for name, (fn, word, entry) in cases.items():
        check(name, fn, word, entry)
    # the same calls succeed once the fault is gone; an output without polynomials launches nothing and is tagged EVAL
    out = M.from_rns(p, sentinel, False)
    assert call(out) == 0 and hcall(out) == 0
    for empty, kw in ((M(p, 2 * k, 0, 1, False), {}), (M(p, 0, 6, 1, False), dict(src_rows=0))):
        c0 = lib.gpupoly_launch_count()
        assert call(empty, **kw) == 0 and lib.gpupoly_launch_count() == c0
        assert hcall(empty, **kw) == 0 and lib.gpupoly_launch_count() == c0
    # the reference's own keying has no block form: refused, and the mirror's many-tags call gives the loop's matrices
    sampler, fin = gpu.GpuDCRTPolyHashSampler(), gpu.DistType.FinRingDist()
    tags = [b"blk" + bytes([t]) for t in range(3)]
    default = sampler.sample_hash_decomposed_columns_many(p, KEY, tags, 2, 7, 2, 2, fin)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda out: call(out), "unsupported", ENTRY)
    check("reference keying, hashed", lambda out: hcall(out), "unsupported", HASH_ENTRY)
    many = sampler.sample_hash_decomposed_columns_many(p, KEY, tags, 2, 7, 2, 2, fin)
    for t, tag in enumerate(tags):
        assert many[t] == sampler.sample_hash_decomposed_columns(p, KEY, tag, 2, 7, 2, 2, fin)
        assert not (many[t] == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert sampler.sample_hash_decomposed_columns_many(p, KEY, tags, 2, 7, 2, 2, fin)[2] == default[2]
    del keep, _k1, _k2
