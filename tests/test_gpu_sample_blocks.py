"""GPU: many independently seeded uniform / bit / ternary blocks in one call (`gpupoly_matrix_sample_distribution_blocks`,
DESIGN.md section 5p), the reshape view (`gpupoly_matrix_reshape_view`) and the hash sampler's `sample_hash_many`,
`sample_hash_stacked` and `sample_hash_weighted_sum` that ride on them.

The bar is the one of the Gaussian segments: a block must be the matrix the plain sampler writes for it ALONE under its seed,
bit for bit, and that matrix is checked against the CPU restatement (oracle.sample_distribution).

One item of the entry's refusal list cannot be built through a real matrix: a stacked `out` of 2^48 columns (no device holds
it).  The 48-bit refusal is reached through the columns layout, whose widths are judged one by one before their sum."""
import ctypes as C

import numpy as np
import pytest

import plainref
from conftest import high_rejection_moduli, make_params

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_sample_distribution_blocks"
DISTS = ("uniform", "bit", "ternary")
# word class -> (n, depth, bits, base_bits); None: the moduli of conftest.high_rejection_moduli(16, 2)
CONTEXTS = {
    "u32_packed24": (16, 2, 24, 12),       # the uniform sample finishes PACKED24
    "u32_words": (16, 2, 28, 14),          # the tight transform
    "u64": (16, 2, 51, 17),                # the double-precision transform
    "u64_high_rejection": None,            # one draw in nine is rejected: the overflow stream runs
    "partial_group": (4, 1, 24, 12),       # fewer than eight coefficients per polynomial
    "ggh15_small_ring": (256, 3, 51, 17),  # the GGH15 chain's ring
}
_HIGH = {}


def params_of(gpu, oracle, name):
    if CONTEXTS[name] is not None:
        return make_params(gpu, oracle, *CONTEXTS[name])
    if "p" not in _HIGH:
        _HIGH["p"] = gpu.GpuDCRTPolyParams(16, high_rejection_moduli(16, 2), 20)
    return _HIGH["p"]


def seed_bytes(tag):
    return bytes((tag * 37 + 11 * i + 5) & 0xFF for i in range(32))


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(seed_bytes(tag))


def block_shape(t, polys):
    """an r x c with r * c == polys, varied with the block index: the stacked row must not depend on it"""
    shapes = [(r, polys // r) for r in range(1, polys + 1) if polys % r == 0]
    return shapes[t % len(shapes)]


# ---------------------------------------------------------------------------------------------------
# both layouts against the plain sampler and the CPU restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_blocks_equal_the_plain_sampler_block_by_block(gpu, oracle, ctx, dist):
    p = params_of(gpu, oracle, ctx)
    M, moduli, n, code = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), oracle.DIST[dist]
    for nblk in (1, 3, 65, 130):  # 65 and 130: past the 64 entries of the Gaussian segments' table
        seeds = [gseed(gpu, 1000 + t) for t in range(nblk)]
        for polys in (1, 6):
            stack = M.sample_distribution_blocks(p, seeds, code, block_polys=polys)
            assert stack.is_ntt and stack.size() == (nblk, polys)
            assert stack.layout == M.sample_distribution(p, nblk, polys, code, 0.0, seeds[0]).layout, (nblk, polys)
            for t in range(nblk):
                r, c = block_shape(t, polys)
                alone = M.sample_distribution(p, r, c, code, 0.0, seeds[t])
                assert stack.row_view(t, t + 1).reshape_view(r, c) == alone, f"stacked: block {t} of {nblk} as {r} x {c}"
                if t < 3 and (nblk, polys) == (3, 6):
                    want = oracle.matrix_ntt(oracle.sample_distribution(r, c, moduli, n, dist, 0.0, seed_bytes(1000 + t)), moduli)
                    assert np.array_equal(alone.to_rns(), want)
                    assert np.array_equal(stack.to_rns()[t].reshape(want.shape), want)
    for rows in (1, 2):
        for widths in ([1, 3, 2], [1] * 130):
            seeds = [gseed(gpu, 2000 + j) for j in range(len(widths))]
            wide = M.sample_distribution_blocks(p, seeds, code, nrow=rows, seg_cols=widths)
            assert wide.is_ntt and wide.size() == (rows, sum(widths))
            assert wide.layout == M.sample_distribution(p, rows, sum(widths), code, 0.0, seeds[0]).layout, (rows, len(widths))
            res = wide.to_rns()
            parts = []
            for lo in range(0, len(widths), 64):
                parts += wide.slice_columns(sum(widths[:lo]), sum(widths[:lo + 64])).split_columns(widths[lo:lo + 64])
            at = 0
            for j, (w, part) in enumerate(zip(widths, parts)):
                assert part == M.sample_distribution(p, rows, w, code, 0.0, seeds[j]), f"columns: block {j} of {len(widths)}, {rows} rows"
                if j < 3 and len(widths) == 3:
                    want = oracle.matrix_ntt(oracle.sample_distribution(rows, w, moduli, n, dist, 0.0, seed_bytes(2000 + j)), moduli)
                    assert np.array_equal(res[:, at:at + w], want)
                at += w


@pytest.mark.parametrize("dist", DISTS)
def test_an_output_below_the_top_level_through_the_raw_entries(gpu, oracle, dist):
    """`out` created at level 1 of a three-limb context and tagged COEFF: the entry samples limbs 0..1 only, as the plain entry
    does for such a matrix, and tags the result EVAL (an EVAL read-out of a matrix still tagged COEFF would transform it)."""
    from mxx_amd import _ffi

    p = params_of(gpu, oracle, "ggh15_small_ring")
    M, n, code, lib = gpu.GpuDCRTPolyMatrix, p.ring_dimension(), oracle.DIST[dist], _ffi.lib()
    low = p.moduli()[:2]
    seeds = (gpu.GpuRngSeed * 3)(*[gseed(gpu, 3000 + t) for t in range(3)])
    stack = M(p, 3, 2, 1, False)
    _ffi.check_status(lib.gpupoly_matrix_sample_distribution_blocks(stack.raw, code, seeds, 3, _ffi.GPUPOLY_BLOCKS_STACKED, None), ENTRY)
    wide = M(p, 2, 3, 1, False)
    cols = (C.c_size_t * 3)(1, 1, 1)
    _ffi.check_status(lib.gpupoly_matrix_sample_distribution_blocks(wide.raw, code, seeds, 3, _ffi.GPUPOLY_BLOCKS_COLUMNS, cols), ENTRY)
    stack.is_ntt = wide.is_ntt = True
    got_stack, got_wide = stack.to_rns(), wide.to_rns()
    assert got_stack.shape == (3, 2, 2, n)
    for t in range(3):
        for shape, got in (((1, 2), got_stack[t].reshape(1, 2, 2, n)), ((2, 1), got_wide[:, t:t + 1])):
            alone = M(p, shape[0], shape[1], 1, False)
            _ffi.check_status(lib.gpu_matrix_sample_distribution(alone.raw, code, 0.0, seeds[t]), "gpu_matrix_sample_distribution")
            alone.is_ntt = True
            want = oracle.matrix_ntt(oracle.sample_distribution(shape[0], shape[1], low, n, dist, 0.0, seed_bytes(3000 + t)), low)
            assert np.array_equal(alone.to_rns(), want) and np.array_equal(got, want), (t, shape)


def test_the_launches_do_not_depend_on_the_block_count(gpu, oracle):
    from mxx_amd import _ffi

    p = params_of(gpu, oracle, "ggh15_small_ring")
    M, code, lib = gpu.GpuDCRTPolyMatrix, oracle.DIST["uniform"], _ffi.lib()
    seeds = [gseed(gpu, 4000 + j) for j in range(130)]

    def launches(fn):
        c0 = lib.gpupoly_launch_count()
        fn()
        return lib.gpupoly_launch_count() - c0

    many = launches(lambda: M.sample_distribution_blocks(p, seeds, code, nrow=1, seg_cols=[1] * 130))
    two = launches(lambda: M.sample_distribution_blocks(p, seeds[:2], code, nrow=1, seg_cols=[65, 65]))
    loop = launches(lambda: [M.sample_distribution(p, 1, 1, code, 0.0, s) for s in seeds])
    print(f"launches: 130 blocks of 1 column {many}, 2 blocks of 65 columns {two}, 130 plain calls {loop}")
    assert many == two and 0 < many < loop


# ---------------------------------------------------------------------------------------------------
# refusals: nothing launched, `out` (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_output_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi

    p = params_of(gpu, oracle, "u32_packed24")
    M, moduli, n, lib = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib()
    sentinel = oracle.random_matrix(91, 2, 3, moduli, n)
    seeds = (gpu.GpuRngSeed * 3)(*[gseed(gpu, 5000 + t) for t in range(3)])
    STACKED, COLUMNS = _ffi.GPUPOLY_BLOCKS_STACKED, _ffi.GPUPOLY_BLOCKS_COLUMNS

    def widths(*w):
        return (C.c_size_t * len(w))(*w)

    def call(out, dist=0, seeds_=seeds, nblk=2, layout=STACKED, seg_cols=None):
        return lib.gpupoly_matrix_sample_distribution_blocks(None if out is None else out.raw, dist, seeds_, nblk, layout, seg_cols)

    cases = {
        "null out": (lambda out: call(None), ""),
        "null seeds": (lambda out: call(out, seeds_=None), ""),
        "no blocks": (lambda out: call(out, nblk=0), ""),
        "more than 2^20 blocks": (lambda out: call(out, nblk=(1 << 20) + 1), ""),
        "unknown layout": (lambda out: call(out, layout=2), "layout"),
        "negative layout": (lambda out: call(out, layout=-1), "layout"),
        "stacked with seg_cols": (lambda out: call(out, seg_cols=widths(1, 2)), "seg_cols"),
        "stacked rows": (lambda out: call(out, nblk=3), "row"),
        "columns without seg_cols": (lambda out: call(out, layout=COLUMNS), "seg_cols"),
        "zero width": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(3, 0)), "zero"),
        "widths short of the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 1)), "sum"),
        "widths past the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(2, 2)), "sum"),
        "gaussian": (lambda out: call(out, dist=1), "unsupported"),
        "gaussian, columns": (lambda out: call(out, dist=1, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported"),
        "dist_type 4": (lambda out: call(out, dist=4), "dist_type"),
        "dist_type -1": (lambda out: call(out, dist=-1), "dist_type"),
        "a block of 2^48 polynomials": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(1 << 47, 3)), "48-bit"),
    }

    def check(name, fn, word):
        out = M.from_rns(p, sentinel, False)  # COEFF-tagged: a tag flipped to EVAL would change the COEFF read-out
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert ENTRY in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # the same calls succeed once the fault is gone, and an output without polynomials launches nothing and is tagged EVAL
    out = M.from_rns(p, sentinel, False)
    assert call(out) == 0 and call(out, layout=COLUMNS, seg_cols=widths(1, 2)) == 0
    for empty, kw in ((M(p, 2, 0, 1, False), {}), (M(p, 0, 3, 1, False), dict(layout=COLUMNS, seg_cols=widths(1, 2)))):
        c0 = lib.gpupoly_launch_count()
        assert call(empty, **kw) == 0 and lib.gpupoly_launch_count() == c0
    sampler = gpu.GpuDCRTPolyHashSampler()
    key, tags = bytes(range(32)), [b"blk" + bytes([t]) for t in range(5)]
    fin = gpu.DistType.FinRingDist()
    default = sampler.sample_hash_many(p, key, tags, 1, 2, fin)
    # the reference's own keying has no block form: refused, and the mirror falls back to the loop with the loop's matrices
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda out: call(out), "unsupported")
    check("reference keying, columns", lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported")
    many = sampler.sample_hash_many(p, key, tags, 1, 2, fin)
    stacked = sampler.sample_hash_stacked(p, key, tags, 1, 2, fin)
    for t, tag in enumerate(tags):
        alone = sampler.sample_hash(p, key, tag, 1, 2, fin)
        assert many[t] == alone and stacked.row_view(t, t + 1) == alone
        assert not (alone == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert sampler.sample_hash_many(p, key, tags, 1, 2, fin)[4] == default[4]


# ---------------------------------------------------------------------------------------------------
# reshape_view
# ---------------------------------------------------------------------------------------------------
def test_reshape_view_shares_the_words_under_another_shape(gpu, oracle):
    from mxx_amd import _ffi
    from mxx_amd._ffi import GpuPolyError

    p = params_of(gpu, oracle, "u32_packed24")
    M, moduli, n, lib = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib()
    res = oracle.random_matrix(17, 2, 6, moduli, n)
    parent = M.from_rns(p, res, True)
    v34, v112 = parent.reshape_view(3, 4), parent.reshape_view(1, 12)
    assert v34.size() == (3, 4) and v112.size() == (1, 12) and v34.is_ntt
    assert np.array_equal(v34.to_rns(), res.reshape(3, 4, len(moduli), n))
    assert np.array_equal(v112.to_rns(), res.reshape(1, 12, len(moduli), n))
    assert np.array_equal(v34.reshape_view(2, 6).to_rns(), res)  # a view of a view
    # writes through the view show in the parent
    add = oracle.random_matrix(18, 3, 4, moduli, n)
    v34.add_in_place(M.from_rns(p, add, True))
    total = oracle.pointwise("add", res, add.reshape(res.shape), moduli)
    assert np.array_equal(parent.to_rns(), total) and np.array_equal(v112.to_rns(), total.reshape(1, 12, len(moduli), n))
    # the overlap rule sees the view through its bytes: a product into a view of one of its operands is refused
    rhs = M.from_rns(p, oracle.random_matrix(19, 4, 4, moduli, n), True)
    c0 = lib.gpupoly_launch_count()
    with pytest.raises(GpuPolyError, match="overlaps"):
        M.mul_sum([v34], [rhs], out=parent.reshape_view(3, 4))
    assert lib.gpu_matrix_mul(parent.reshape_view(3, 4).raw, v34.raw, rhs.raw) != 0  # the plain product words it "alias"
    assert "alias" in _ffi.last_error_string() and lib.gpupoly_launch_count() == c0
    assert np.array_equal(parent.to_rns(), total)
    assert np.array_equal((v34 * rhs).to_rns(), oracle.matmul(total.reshape(3, 4, len(moduli), n), rhs.to_rns(), moduli))
    # another polynomial count
    for shape in ((3, 5), (0, 0), (12, 0), (5, 2)):
        with pytest.raises(GpuPolyError, match="gpupoly_matrix_reshape_view"):
            parent.reshape_view(*shape)
    empty = M(p, 0, 5, 1, True)
    assert empty.reshape_view(7, 0).size() == (7, 0)
    # a PACKED24 parent is unpacked by the view and stays usable: the same residues
    s = gseed(gpu, 6000)
    packed = M.sample_distribution(p, 2, 6, 0, 0.0, s)
    want = M.sample_distribution(p, 2, 6, 0, 0.0, s).to_rns()
    assert packed.layout == "packed24"
    view = packed.reshape_view(4, 3)
    assert packed.layout == "words" and view.layout == "words"
    assert np.array_equal(view.to_rns(), want.reshape(4, 3, len(moduli), n)) and np.array_equal(packed.to_rns(), want)
    assert (rhs.slice_rows(0, 3) * view).size() == (3, 3)


# ---------------------------------------------------------------------------------------------------
# the hash sampler
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,dist,nrow,ncol", [("u32_packed24", "fin_ring", 2, 3), ("u64", "bit", 1, 2), ("u32_words", "ternary", 3, 1),
                                                ("ggh15_small_ring", "gauss", 1, 2), ("u32_words", "gauss", 2, 1)])
def test_sample_hash_many_and_stacked_equal_the_loop(gpu, oracle, ctx, dist, nrow, ncol):
    """70 tags: two chunks of the mirror.  The Gaussian cases go through the Gaussian segments (n = 256) and, where those
    answer `unsupported` (n = 16), through the loop."""
    p = params_of(gpu, oracle, ctx)
    sampler = gpu.GpuDCRTPolyHashSampler()
    d = gpu.DistType(dist, 3.5 if dist == "gauss" else 0.0)
    key = bytes((7 * i + 1) & 0xFF for i in range(32))
    tags = [b"tag_" + t.to_bytes(8, "little") for t in range(70)]
    loop = [sampler.sample_hash(p, key, tag, nrow, ncol, d) for tag in tags]
    many = sampler.sample_hash_many(p, key, tags, nrow, ncol, d)
    assert len(many) == 70
    for t in range(70):
        assert many[t].size() == (nrow, ncol) and many[t] == loop[t], t
    stacked = sampler.sample_hash_stacked(p, key, tags, nrow, ncol, d)
    assert stacked.size() == (70, nrow * ncol) and stacked.is_ntt
    for t in range(70):
        assert stacked.row_view(t, t + 1).reshape_view(nrow, ncol) == loop[t], t
    assert sampler.sample_hash_many(p, key, [], nrow, ncol, d) == []
    assert [m.size() for m in sampler.sample_hash_many(p, key, tags[:2], 0, ncol, d)] == [(0, ncol)] * 2


# ---------------------------------------------------------------------------------------------------
# the weighted sum in the shape of commit_base (src/commit/wee25.rs:858-883)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ["u32_packed24", "u64"])
def test_weighted_sum_equals_the_commit_base_loop(gpu, oracle, ctx):
    p = params_of(gpu, oracle, ctx)
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    sampler = gpu.GpuDCRTPolyHashSampler()
    fin = gpu.DistType.FinRingDist()
    secret_size, m_b, cols = 1, 3, 2
    m_g = p.modulus_digits()
    T = cols * m_g
    key = bytes((5 * i + 9) & 0xFF for i in range(32))
    msg = M.from_rns(p, oracle.random_matrix(23, 1, cols, moduli, n), True)
    D = msg.decompose()
    assert D.size() == (m_g, cols)
    tags = [b"wee25_w_block_" + (j * m_g + r).to_bytes(8, "little") for j in range(cols) for r in range(m_g)]
    acc = M.zero(p, secret_size, m_b)
    for j in range(cols):
        for r in range(m_g):
            acc = acc + sampler.sample_hash(p, key, tags[j * m_g + r], secret_size, m_b, fin) * D.entry(r, j)
    weights = D.transpose().reshape_view(1, T)
    got = sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b)
    assert got.size() == (secret_size, m_b) and got.is_ntt and got == acc
    addend = M.from_rns(p, oracle.random_matrix(24, secret_size, m_b, moduli, n), True)
    addend_res = addend.to_rns()
    assert sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b, addend=addend) == addend + acc
    assert sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b, addend=addend, negate=True) == addend - acc
    assert sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b, negate=True) == -acc
    assert np.array_equal(addend.to_rns(), addend_res)  # the addend is an input
    assert sampler.sample_hash_weighted_sum(p, key, [], M(p, 1, 0, len(moduli) - 1, True), secret_size, m_b, addend=addend) == addend
    # three uneven chunks: T = 8 -> 3 + 3 + 2 (24 bits), T = 12 -> 5 + 5 + 2 (51 bits)
    step = {8: 3, 12: 5}[T]
    assert len(range(0, T, step)) == 3 and T % step not in (0, step)
    poly_bytes = len(moduli) * n * p.ctx().word_bytes()
    chunks, real = [], sampler.sample_hash_stacked
    sampler.sample_hash_stacked = lambda params, k, tg, *a: chunks.append(len(tg)) or real(params, k, tg, *a)
    for kw in ({}, dict(addend=addend, negate=True)):
        del chunks[:]
        chunked = sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b, max_stack_bytes=step * m_b * poly_bytes + 1, **kw)
        assert chunks == [step, step, T - 2 * step]
        assert chunked == (addend - acc if kw else acc)
    del sampler.sample_hash_stacked
    if ctx == "u32_packed24":  # and against the plain reference fed with the CPU restatement's samples
        stack = np.stack([oracle.matrix_ntt(oracle.sample_distribution(secret_size, m_b, moduli, n, "uniform", 0.0,
                                                                       gpu.hash_seed_for_matrix(key, tag)), moduli).reshape(m_b, len(moduli), n)
                          for tag in tags])
        w = D.transpose().to_rns().reshape(1, T, len(moduli), n)
        want = plainref.slot_mul_sum(addend_res.reshape(1, m_b, len(moduli), n), [w], [stack], moduli, True)
        got = sampler.sample_hash_weighted_sum(p, key, tags, weights, secret_size, m_b, addend=addend, negate=True)
        assert np.array_equal(got.to_rns(), want.reshape(secret_size, m_b, len(moduli), n))
