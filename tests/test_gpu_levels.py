"""GPU: every kernel family on matrices BELOW the top level of their context.

A matrix at level l uses limbs 0..=l (gpu_matrix_create), so every launcher works with two limb counts that agree only at
the top level: the matrix's L = l + 1 (word strides, grid extents, k = dpt * L) and the context's limb_count (the tables,
the width-class switches, crt_bits and so dpt).  A kernel that confuses them is right at the top level - where the rest
of the suite runs - and wrong here.  Each cell runs at level 0 and at level D - 2 of the contexts of tests/levels.py,
against the plain references handed the truncated basis moduli[: l + 1]; every comparison is bit for bit.  Cells that
force a kernel family assert from the launch trace (tests/ran.py) that the family ran, under the acceptance predicates
of the top-level tests they borrow their shapes from.  tests/levels.py holds the table of what covers which entry.
"""
import ctypes as C

import numpy as np
import pytest

import levels as lv
import plainref
import ran
import test_gpu_core as core
from mxx_amd import _ffi

pytestmark = pytest.mark.gpu

EVAL, COEFF = _ffi.GPU_POLY_FORMAT_EVAL, _ffi.GPU_POLY_FORMAT_COEFF


def _bits(ctx):
    kind, *rest = lv.CONTEXTS[ctx]
    return rest[1] if kind == "gen" else max(rest[0])


def _at(cells, big_from=15):
    """(cell..., level) for level 0 and D - 2 of the cell's context; rings of 2^big_from points and more keep L <= 2"""
    out = []
    for cell in cells:
        ctx, logn = cell[0], cell[1]
        lvls = lv.levels_of(ctx)
        if logn >= big_from and ctx not in lv.MIXED:
            lvls = (0, 1)
        out += [cell + (l,) for l in lvls]
    return out


def _up(gpu, p, x, eval_format):
    return gpu.GpuDCRTPolyMatrix.from_rns(p, x, eval_format)


def _words(m, is_ntt):
    """the words of a matrix written by a raw entry, read under the tag the entry must have left"""
    m.is_ntt = is_ntt
    return m.to_rns()


# ---------------------------------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------------------------------
def _transform_cells():
    cells = []
    for ctx in lv.GEN + lv.MIXED:  # the generic path: n = 2, 16, 512
        for logn in (1, 4, 9):
            cells += [(ctx, logn, None, None), (ctx, logn, "MXX_HIP_NTT_PATH", "generic")]
    for ctx in lv.GEN:  # the LDS kernels
        cells += [(ctx, 10, None, None), (ctx, 12, None, None)]
    cells += [("24", 11, None, None), ("24", 13, None, None), ("28", 13, None, None), ("24_24_31", 10, None, None), ("28_28_51", 10, None, None)]
    for ctx in ("24", "51", "58"):
        cells += [(ctx, 10, "MXX_HIP_NTT_PATH", "generic"), (ctx, 10, "MXX_HIP_NTT_PATH", "global")]
    for design in (None, "unsigned", "whole"):  # 3 polynomials at L = 1 and L = 3: ntt14_grid sees vectors % L on both
        cells.append(("24", 14, "MXX_HIP_NTT14", design))
    cells += [("28", 14, None, None), ("28", 14, "MXX_HIP_NTT14", "whole"), ("51", 14, None, None), ("28_28_51", 14, None, None)]
    for ctx in ("24", "28", "51"):  # whole at 2^15 in 32-bit words, split beyond
        for logn in (15, 16, 17):
            cells += [(ctx, logn, None, None), (ctx, logn, "MXX_HIP_NTT_PATH", "global")]
    for ctx, logn in (("51", 10), ("51", 15), ("28_28_51", 10)):
        cells.append((ctx, logn, "MXX_HIP_NTT64", "int"))
    return cells


def _transform_expect(ctx, logn, switch, value, moduli):
    """the (switch, value) of tests/ran.py's table whose family this cell must show, or None where the predicates of
    tests/test_gpu_core.py say that the forced kernel declines (or nothing is forced and the default has no table row)"""
    bits, cls = _bits(ctx), ran.Launched.word_class(moduli)
    if switch == "MXX_HIP_NTT_PATH":
        ok = core._generic_accepts(logn, bits) if value == "generic" else True
        return (switch, value) if ok else None
    if switch == "MXX_HIP_NTT14":
        # _ntt14_accepts of tests/test_gpu_surface.py: grouped signed to 24 bits, unsigned to 25, whole to 28
        ok = {None: bits <= 24, "unsigned": bits <= 25, "whole": bits <= 28}[value]
        return (switch, value) if ok and cls == "u32" else None
    if switch == "MXX_HIP_NTT64":
        return (switch, value) if core._f64_accepts(bits) else None
    if cls == "u64f" and core._f64_accepts(bits) and logn >= 1:
        return ("MXX_HIP_NTT64", None)
    return None


@pytest.mark.parametrize("ctx,logn,switch,value,level", _at(_transform_cells()))
def test_transforms_forward_inverse_and_tag(gpu, oracle, hip_env, ctx, logn, switch, value, level):
    n = 1 << logn
    p = lv.params(gpu, oracle, ctx, n)
    moduli = p.moduli()[: level + 1]
    polys = 3 if logn <= 14 else 1
    x = lv.host(oracle, 500 + logn + level, 1, polys, moduli, n)
    want, want_inv = oracle.matrix_ntt(x, moduli), oracle.matrix_ntt(x, moduli, inverse=True)
    if switch and value:
        hip_env.set(switch, value)
    m, e = _up(gpu, p, x, False), _up(gpu, p, x, True)
    assert m.level == level
    with ran.launches() as k:
        m.ntt_all_in_place()
        fwd = m.to_rns()
        m.ntt_all_in_place()  # idempotent on the tag
        again = m.to_rns()
        m.intt_all_in_place()
        back = m.to_rns()
        m.intt_all_in_place()
        e.intt_all_in_place()
    assert np.array_equal(fwd, want), "forward"
    assert np.array_equal(again, want), "a second forward call must do nothing"
    assert np.array_equal(back, x) and np.array_equal(m.to_rns(), x), "inverse"
    assert np.array_equal(e.to_rns(), want_inv), "inverse of evaluation-domain inputs"
    pair = _transform_expect(ctx, logn, switch, value, p.moduli())
    if pair:
        k.assert_ran(pair[0], pair[1], p.moduli(), forward=True, inverse=True)
    if logn >= 16:  # the same call at the top level of the context over the prefix basis: identical words
        q = lv.params(gpu, oracle, ctx, n, prefix=level)
        t = _up(gpu, q, x, False)
        t.ntt_all_in_place()
        assert np.array_equal(t.to_rns(), fwd)
        # polynomial 0 (= the last one) in every limb against the plain definition, at slots of both halves and the ends
        slots = [0, 1, n // 2 - 1, n // 2, n - 2, n - 1]
        assert np.array_equal(fwd[0, 0][:, slots], plainref.ntt_slots(x[0, 0], moduli, slots))


FUSED_CELLS = [("24", 10), ("24", 14), ("28", 14), ("31", 10), ("51", 10), ("58", 9), ("24_24_31", 10), ("28_28_51", 10)]


@pytest.mark.parametrize("ctx,logn,level", _at(FUSED_CELLS))
def test_fused_transform_variants(gpu, oracle, ctx, logn, level):
    """mul_scalar_intt, add_rows, ntt_add_rows (kept and consumed source) into a row block of a taller matrix"""
    n = 1 << logn
    p = lv.params(gpu, oracle, ctx, n)
    moduli = p.moduli()[: level + 1]
    a, b = lv.host(oracle, 601, 2, 2, moduli, n), lv.host(oracle, 602, 2, 2, moduli, n, edges=False)
    s = lv.host(oracle, 603, 1, 1, moduli, n, edges=False)
    ga, gb, gs = _up(gpu, p, a, True), _up(gpu, p, b, True), _up(gpu, p, s, True)
    got = ga.mul_scalar_intt(gs)
    assert got.level == level and not got.is_ntt
    assert np.array_equal(got.to_rns(), oracle.matrix_ntt(oracle.pointwise("mul", a, s, moduli), moduli, inverse=True))
    frame = lv.host(oracle, 604, 5, 2, moduli, n, edges=False)
    tall = _up(gpu, p, frame, True)
    tall.add_rows_from(2, ga, gb)
    want = frame.copy()
    want[2:4] = oracle.pointwise("add", a, b, moduli)
    assert np.array_equal(tall.to_rns(), want)
    for consume in (False, True):
        coeff = _up(gpu, p, a, False)
        tall = _up(gpu, p, frame, True)
        tall.ntt_add_rows_from(3, coeff, gb, consume=consume)
        want = frame.copy()
        want[3:5] = oracle.pointwise("add", oracle.matrix_ntt(a, moduli), b, moduli)
        assert np.array_equal(tall.to_rns(), want), consume
        if not consume:
            assert np.array_equal(coeff.to_rns(), a), "the source must be left as it was"


@pytest.mark.parametrize("level", lv.levels_of("24"))
def test_uniform_sample_at_2_14_is_packed_below_the_top(gpu, oracle, level):
    """pack24_eligible looks at the context (pack24_ok) and the shape, not the level: the uniform sample of a 24-bit context
    stays PACKED24 at every level, and its words after unpacking are the oracle's sample transformed"""
    n = 1 << 14
    p = lv.params(gpu, oracle, "24", n)
    moduli = p.moduli()[: level + 1]
    out = lv.new(gpu, p, 1, 3, level, True)
    lv.call("gpu_matrix_sample_distribution", out.raw, oracle.DIST["uniform"], 0.0, gpu.GpuRngSeed.from_bytes(lv.seed_bytes(1)))
    top = gpu.GpuDCRTPolyMatrix.sample_distribution(p, 1, 3, oracle.DIST["uniform"], 0.0, gpu.GpuRngSeed.from_bytes(lv.seed_bytes(1)))
    assert out.layout == top.layout == "packed24"
    want = oracle.matrix_ntt(oracle.sample_distribution(1, 3, moduli, n, "uniform", 0.0, lv.seed_bytes(1)), moduli)
    assert np.array_equal(_words(out, True), want)


# ---------------------------------------------------------------------------------------------------------------------
# point-wise entries and structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,logn,level", _at([(c, 4) for c in lv.GEN + lv.MIXED] + [("24", 10), ("51", 10)]))
def test_pointwise_and_structure(gpu, oracle, ctx, logn, level):
    n = 1 << logn
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    a, b = lv.host(oracle, 701, 3, 4, moduli, n), lv.host(oracle, 702, 3, 4, moduli, n, edges=False)
    c, d, s = (lv.host(oracle, 703 + i, *shape, moduli, n, edges=False) for i, shape in enumerate(((3, 2), (2, 4), (1, 1))))
    ga, gb, gc, gd, gs = (_up(gpu, p, x, True) for x in (a, b, c, d, s))
    assert np.array_equal((ga + gb).to_rns(), oracle.pointwise("add", a, b, moduli))
    assert np.array_equal((ga - gb).to_rns(), oracle.pointwise("sub", a, b, moduli))
    assert np.array_equal((-ga).to_rns(), oracle.pointwise("sub", np.zeros_like(a), a, moduli))
    assert np.array_equal(ga.mul_scalar(gs).to_rns(), oracle.pointwise("mul", a, s, moduli))
    acc = ga.clone()
    acc.add_in_place(gb)
    assert np.array_equal(acc.to_rns(), oracle.pointwise("add", a, b, moduli))
    assert ga == ga.clone() and not (ga == gb)
    assert np.array_equal(ga.transpose().to_rns(), a.transpose(1, 0, 2, 3))
    cat = ga.concat_columns([gc])
    assert np.array_equal(cat.to_rns(), np.concatenate([a, c], axis=1))
    left, right = cat.split_columns([4, 2])
    assert np.array_equal(left.to_rns(), a) and np.array_equal(right.to_rns(), c)
    out = ga.clone()
    out.add_block_from(gd, 1, 0, 0, 0, 2, 4)
    want = a.copy()
    want[1:3] = oracle.pointwise("add", a[1:3], d, moduli)
    assert np.array_equal(out.to_rns(), want)
    out.copy_block_from(gc, 0, 2, 1, 0, 2, 2)
    want[0:2, 2:4] = c[1:3]
    assert np.array_equal(out.to_rns(), want)
    assert np.array_equal(ga.slice(1, 3, 1, 4).to_rns(), a[1:3, 1:4])
    # identity (the constant 1, and a scalar on the diagonal) and the Kronecker product, through the raw entries
    eye = lv.new(gpu, p, 3, 3, level, True)
    lv.call("gpupoly_matrix_fill_identity", eye.raw, None)
    one = oracle.matrix_ntt(np.concatenate([np.ones((1, 1, level + 1, 1), dtype=np.uint64), np.zeros((1, 1, level + 1, n - 1), dtype=np.uint64)], axis=3), moduli)
    got = _words(eye, True)
    for i in range(3):
        for j in range(3):
            assert np.array_equal(got[i, j], one[0, 0] if i == j else np.zeros_like(one[0, 0])), (i, j)
    assert eye * ga == ga
    lv.call("gpupoly_matrix_fill_identity", eye.raw, gs.raw)
    assert np.array_equal((eye * ga).to_rns(), oracle.pointwise("mul", a, s, moduli))
    t = ga.tensor(gc).to_rns()
    for i in range(3):
        for j in range(4):
            blk = oracle.pointwise("mul", c, a[i:i + 1, j:j + 1], moduli)
            assert np.array_equal(t[3 * i:3 * i + 3, 2 * j:2 * j + 2], blk), (i, j)
    z = lv.new(gpu, p, 2, 2, level, False)
    lv.call("gpupoly_matrix_fill_zero", z.raw)
    assert not z.to_rns().any()


# ---------------------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------------------
def _worst_b(oracle, seed, k, c, moduli, n):
    b = np.broadcast_to((np.asarray(moduli, dtype=np.uint64) - np.uint64(1)).reshape(1, 1, -1, 1), (k, c, len(moduli), n)).copy()
    b[::2] = oracle.random_matrix(seed, k, c, moduli, n)[::2]
    return b


# family -> (context, n, shape); the shapes of test_matmul_kernel_families / test_matmul_dma_kernel (tests/test_gpu_core.py)
PRODUCT_FAMILIES = {"reg": ("24", 128, (9, 5, 17)), "lds": ("24", 128, (20, 7, 33)), "dma": ("24", 128, (33, 12, 17)),
                    "wide": ("31", 128, (33, 12, 17)), "dma31": ("31", 128, (32, 8, 16))}


@pytest.mark.parametrize("family,level", [(f, l) for f, (ctx, _, _) in PRODUCT_FAMILIES.items() for l in lv.levels_of(ctx)])
def test_product_families(gpu, oracle, hip_env, family, level):
    ctx, n, (r, k, c) = PRODUCT_FAMILIES[family]
    path = "dma" if family == "dma31" else family
    p = lv.params(gpu, oracle, ctx, n)
    moduli = p.moduli()[: level + 1]
    a, b = oracle.random_matrix(801, r, k, moduli, n), _worst_b(oracle, 802, k, c, moduli, n)
    ga, gb = _up(gpu, p, a, True), _up(gpu, p, b, True)
    hip_env.set("MXX_HIP_MATMUL_PATH", path)
    got = ga * gb
    assert got.level == level
    assert np.array_equal(got.to_rns(), oracle.matmul(a, b, moduli))
    accepts = {"reg": True, "lds": n >= 64 and n % 64 == 0,
               "dma": core._streamed_accepts(dict(shape=(r, k, c), bits=_bits(ctx), n=n), 64),
               "wide": core._streamed_accepts(dict(shape=(r, k, c), bits=_bits(ctx), n=n), 32)}[path]
    assert accepts, "the cell must select the family it names"
    assert p.ctx().last_kernel().startswith(ran.TABLE[("MXX_HIP_MATMUL_PATH", path)]["u32"].last), (path, p.ctx().last_kernel())


@pytest.mark.parametrize("level", (0, 1))
def test_product_matrix_cores(gpu, oracle, hip_env, level):
    """the "below MAX_Q" rule of test_matmul_mfma_kernel with three limbs"""
    from test_gpu_surface import _mfma_accepts

    n, (r, k, c) = 128, (33, 12, 40)
    moduli_all = lv.mfma_basis(n)
    p = gpu.GpuDCRTPolyParams(n, moduli_all, 8)
    moduli = moduli_all[: level + 1]
    a, b = oracle.random_matrix(811, r, k, moduli, n), oracle.random_matrix(812, k, c, moduli, n)
    qs = np.asarray(moduli, dtype=np.uint64).reshape(-1, 1)
    edge = np.concatenate([np.zeros_like(qs), (qs - 1) // 2, (qs + 1) // 2, qs - 1], axis=1)
    a[0, :, :, :4] = edge
    b[:, 0, :, :4] = edge[:, ::-1]
    hip_env.set("MXX_HIP_MATMUL_PATH", "mfma")
    got = _up(gpu, p, a, True) * _up(gpu, p, b, True)
    assert np.array_equal(got.to_rns(), oracle.matmul(a, b, moduli))
    assert _mfma_accepts(moduli_all, n, k)
    assert p.ctx().last_kernel().startswith(ran.TABLE[("MXX_HIP_MATMUL_PATH", "mfma")]["u32"].last), p.ctx().last_kernel()


@pytest.mark.parametrize("tile", ["184", "444p", "881", "482p"])
@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "31") for l in lv.levels_of(c)])
def test_product_register_tiles(gpu, oracle, hip_env, tile, ctx, level):
    n = 64
    p = lv.params(gpu, oracle, ctx, n)
    moduli = p.moduli()[: level + 1]
    hip_env.set("MXX_HIP_MATMUL_PATH", "reg")
    hip_env.set("MXX_HIP_MATMUL_TILE", tile)
    for (r, k, c) in ((int(tile[0]) + 1, 6, 2 * int(tile[1]) + 1), (5, 37, 9)):
        a, b = oracle.random_matrix(821, r, k, moduli, n), _worst_b(oracle, 822, k, c, moduli, n)
        got = _up(gpu, p, a, True) * _up(gpu, p, b, True)
        assert np.array_equal(got.to_rns(), oracle.matmul(a, b, moduli)), (tile, r, k, c)
        label = p.ctx().last_kernel()  # n >= 4: launch_matmul reads the tile switch
        head = ran.TABLE[("MXX_HIP_MATMUL_TILE", "RCS[p]")]["u32"].last + f",{tile[0]},{tile[1]},{tile[2]}"
        assert label.startswith(head), (tile, label)
        assert label[len(head):].startswith(",loads-ahead") == tile.endswith("p"), (tile, label)


@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "51", "58", "24_24_31", "28_28_51") for l in lv.levels_of(c)])
def test_product_default_dispatch_and_batch(gpu, oracle, ctx, level):
    """the small-grid shapes of test_matmul_small_grid_dispatch under the automatic choice, and mul_batch with mixed shapes"""
    n = 256
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    shapes = [(3, 5, 9), (4, 7, 8), (2, 33, 16), (1, 31, 15)]
    hosts = [(oracle.random_matrix(830 + i, r, k, moduli, n), _worst_b(oracle, 840 + i, k, c, moduli, n)) for i, (r, k, c) in enumerate(shapes)]
    devs = [(_up(gpu, p, a, True), _up(gpu, p, b, True)) for a, b in hosts]
    wants = [oracle.matmul(a, b, moduli) for a, b in hosts]
    for (ga, gb), want in zip(devs, wants):
        assert np.array_equal((ga * gb).to_rns(), want)
    outs = M.mul_batch([d[0] for d in devs], [d[1] for d in devs])
    for out, want in zip(outs, wants):
        assert out.level == level and np.array_equal(out.to_rns(), want)
    # the same gates with point-wise ones through gpupoly_batch
    (a0, _), (a1, _) = hosts[0], hosts[1]
    gates = [("mul", devs[0][0], devs[0][1]), ("add", devs[0][0], devs[0][0]), ("neg", devs[1][0], None), ("mul", devs[2][0], devs[2][1])]
    got = M.eval_gates(gates)
    assert np.array_equal(got[0].to_rns(), wants[0]) and np.array_equal(got[3].to_rns(), wants[2])
    assert np.array_equal(got[1].to_rns(), oracle.pointwise("add", a0, a0, moduli))
    assert np.array_equal(got[2].to_rns(), oracle.pointwise("sub", np.zeros_like(a1), a1, moduli))


# ---------------------------------------------------------------------------------------------------------------------
# decomposition and gadgets
# ---------------------------------------------------------------------------------------------------------------------
DECOMPOSE_CELLS = ([(c, 7) for c in lv.GEN + lv.MIXED] + [("24", 10), ("28", 10), ("51", 10), ("58", 10), ("24_24_31", 10), ("28_28_51", 10),
                                                          ("24", 14), ("28", 14), ("51", 14), ("24", 16), ("28", 16), ("51", 16)])


def _decompose_raw(gpu, p, src, level, small, k):
    out = lv.new(gpu, p, src.nrow * k, src.ncol, level, True)
    lv.call("gpu_matrix_decompose_base_small" if small else "gpu_matrix_decompose_base", src.raw, p.base_bits(), out.raw)
    return out


@pytest.mark.parametrize("fused", [None, "0"])
@pytest.mark.parametrize("ctx,logn,level", _at(DECOMPOSE_CELLS, big_from=16))
def test_decompose_and_gadgets(gpu, oracle, hip_env, ctx, logn, level, fused):
    """G^-1 with dpt from the CONTEXT's widest modulus (in the mixed-width contexts the matrix's own limbs are narrower:
    plainref.digits takes dpt explicitly): digits word for word, COEFF and EVAL sources, the small variant, a row window,
    and G_l * G_l^-1(M) == M at the level"""
    n = 1 << logn
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli, base, dpt = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1], p.base_bits(), lv.dpt_of(p)
    L = level + 1
    k = dpt * L
    rows, cols = (2, 2) if logn <= 10 else (1, 1)
    x = lv.host(oracle, 900 + logn, rows, cols, moduli, n)
    want_coeff = lv.ref_digits(x, moduli, base, dpt)
    want = oracle.matrix_ntt(want_coeff, moduli)
    if fused is not None:
        hip_env.set("MXX_HIP_DECOMPOSE_FUSED", fused)
    src = _up(gpu, p, x, False)
    with ran.launches() as tr:
        dec = _decompose_raw(gpu, p, src, level, False, k)
    assert np.array_equal(_words(dec, True), want)
    accepts = core._fused_digits_accepts(logn, _bits(ctx)) if fused is None else True
    if accepts:
        tr.assert_ran("MXX_HIP_DECOMPOSE_FUSED", fused, p.moduli())
    src_eval = _up(gpu, p, oracle.matrix_ntt(x, moduli), True)  # an EVAL source: the out-of-place inverse feeds the digits
    assert np.array_equal(_words(_decompose_raw(gpu, p, src_eval, level, False, k), True), want)
    assert np.array_equal(src_eval.to_rns(), oracle.matrix_ntt(x, moduli)), "the source is left untouched"
    small = _decompose_raw(gpu, p, src, level, True, dpt)
    assert np.array_equal(_words(small, True), oracle.matrix_ntt(lv.ref_digits(x, moduli, base, dpt, small=True), moduli))
    # a row window that starts inside tower 0's digits and ends inside the last tower's
    lo, hi = 1, rows * k - 1
    if hi > lo:
        win = lv.new(gpu, p, hi - lo, cols, level, False)
        lv.call("gpupoly_matrix_decompose_rows", src.raw, base, 0, lo, win.raw)
        assert np.array_equal(_words(win, False), want_coeff[lo:hi])
    # the gadget matrices at the level, and the relation
    G = lv.new(gpu, p, rows, rows * k, level, True)
    lv.call("gpu_matrix_fill_gadget", G.raw, base)
    assert np.array_equal(_words(G, True), oracle.matrix_ntt(lv.ref_gadget(rows, moduli, base, dpt, n), moduli))
    assert np.array_equal((G * dec).to_rns(), oracle.matrix_ntt(x, moduli)), "G * G^-1(M) != M"
    Gs = lv.new(gpu, p, rows, rows * dpt, level, True)
    lv.call("gpu_matrix_fill_small_gadget", Gs.raw, base)
    assert np.array_equal(_words(Gs, True), oracle.matrix_ntt(lv.ref_gadget(rows, moduli, base, dpt, n, small=True), moduli))
    if logn >= 16 and ctx not in lv.MIXED:  # the same call at the top level of the prefix context
        q = lv.params(gpu, oracle, ctx, n, prefix=level)
        assert lv.dpt_of(q) == dpt
        top = _decompose_raw(gpu, q, _up(gpu, q, x, False), level, False, k)
        assert np.array_equal(_words(top, True), _words(dec, True))


@pytest.mark.parametrize("ctx,logn,level", _at([(c, 7) for c in lv.GEN + lv.MIXED] + [("24", 10), ("51", 10)]))
def test_decomposed_products_and_identity_chunk(gpu, oracle, ctx, logn, level):
    """mul_decompose, mul_decompose_small, mul_tensor_identity(_decompose), sample_decomposed and
    fill_small_decomposed_identity_chunk, through the raw entries at the level"""
    n = 1 << logn
    p = lv.params(gpu, oracle, ctx, n)
    moduli, base, dpt = p.moduli()[: level + 1], p.base_bits(), lv.dpt_of(p)
    k = dpt * (level + 1)
    B = lv.host(oracle, 950, 3, 2, moduli, n)
    B_eval = oracle.matrix_ntt(B, moduli)
    D = oracle.matrix_ntt(lv.ref_digits(B, moduli, base, dpt), moduli)
    Ds = oracle.matrix_ntt(lv.ref_digits(B, moduli, base, dpt, small=True), moduli)
    S, Ss = oracle.random_matrix(951, 2, 3 * k, moduli, n), oracle.random_matrix(952, 2, 3 * dpt, moduli, n)
    gB = _up(gpu, p, B_eval, True)
    for entry, lhs, want in (("gpupoly_matrix_mul_decompose", S, oracle.matmul(S, D, moduli)),
                             ("gpupoly_matrix_mul_decompose_small", Ss, oracle.matmul(Ss, Ds, moduli))):
        out = lv.new(gpu, p, 2, 2, level, True)
        g_lhs = _up(gpu, p, lhs, True)  # held: a handle outlives the call only while its matrix object does
        lv.call(entry, out.raw, g_lhs.raw, gB.raw, base)
        assert np.array_equal(_words(out, True), want), entry
    S2 = oracle.random_matrix(953, 2, 6, moduli, n)
    out = lv.new(gpu, p, 2, 4, level, True)
    g_lhs = _up(gpu, p, S2, True)
    lv.call("gpupoly_matrix_mul_tensor_identity", out.raw, g_lhs.raw, gB.raw, 2)
    want = np.concatenate([oracle.matmul(S2[:, :3], B_eval, moduli), oracle.matmul(S2[:, 3:], B_eval, moduli)], axis=1)
    assert np.array_equal(_words(out, True), want)
    S3 = oracle.random_matrix(954, 2, 6 * k, moduli, n)
    out = lv.new(gpu, p, 2, 4, level, True)
    g_lhs = _up(gpu, p, S3, True)
    lv.call("gpupoly_matrix_mul_tensor_identity_decompose", out.raw, g_lhs.raw, gB.raw, 2, base)
    want = np.concatenate([oracle.matmul(S3[:, :3 * k], D, moduli), oracle.matmul(S3[:, 3 * k:], D, moduli)], axis=1)
    assert np.array_equal(_words(out, True), want)
    # G^-1 of a fresh sample == the digits of the oracle's sample
    seed = lv.seed_bytes(40 + level)
    for dist in ("uniform", "ternary"):
        smp = oracle.sample_distribution(2, 2, moduli, n, dist, 0.0, seed)
        for small, kk in ((0, k), (1, dpt)):
            out = lv.new(gpu, p, 2 * kk, 2, level, True)
            lv.call("gpupoly_matrix_sample_decomposed", out.raw, oracle.DIST[dist], 0.0, gpu.GpuRngSeed.from_bytes(seed), base, small)
            assert np.array_equal(_words(out, True), oracle.matrix_ntt(lv.ref_digits(smp, moduli, base, dpt, small=bool(small)), moduli)), (dist, small)
    # rows [3 c, 3 c + 3) of the small decomposition of scalar * I_3, a (3 dpt) x 3 matrix whose row j * dpt + e holds digit e of
    # the scalar in column j and zeros elsewhere
    digits = oracle.matrix_ntt(lv.ref_digits(B[:1, :1], moduli, base, dpt, small=True), moduli)  # (dpt, 1, L, n)
    row = _up(gpu, p, np.ascontiguousarray(digits.transpose(1, 0, 2, 3)), True)
    full = np.zeros((3 * dpt, 3, level + 1, n), dtype=np.uint64)
    for j in range(3):
        full[j * dpt:(j + 1) * dpt, j] = digits[:, 0]
    for chunk in range(dpt):
        out = lv.new(gpu, p, 3, 3, level, True)
        lv.call("gpu_matrix_fill_small_decomposed_identity_chunk", out.raw, row.raw, chunk)
        assert np.array_equal(_words(out, True), full[3 * chunk:3 * chunk + 3]), chunk


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
def _gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(lv.seed_bytes(tag))


@pytest.mark.parametrize("dist,sigma", [("uniform", 0.0), ("gauss", 4.578), ("bit", 0.0), ("ternary", 0.0)])
@pytest.mark.parametrize("ctx,level", [(c, l) for c in lv.GEN + lv.MIXED for l in lv.levels_of(c)])
def test_plain_samplers(gpu, oracle, ctx, level, dist, sigma):
    """sample_distribution, and _columns with an offset window of a wider conceptual matrix"""
    n = 128
    p = lv.params(gpu, oracle, ctx, n)
    moduli, code = p.moduli()[: level + 1], oracle.DIST[dist]
    out = lv.new(gpu, p, 2, 3, level, False)
    lv.call("gpu_matrix_sample_distribution", out.raw, code, sigma, _gseed(gpu, 21))
    want = oracle.matrix_ntt(oracle.sample_distribution(2, 3, moduli, n, dist, sigma, lv.seed_bytes(21)), moduli)
    assert np.array_equal(_words(out, True), want)
    win = lv.new(gpu, p, 2, 3, level, False)
    lv.call("gpu_matrix_sample_distribution_columns", win.raw, code, sigma, _gseed(gpu, 22), 7, 2)
    want = oracle.matrix_ntt(oracle.sample_distribution(2, 3, moduli, n, dist, sigma, lv.seed_bytes(22), full_ncol=7, col_offset=2), moduli)
    assert np.array_equal(_words(win, True), want)


@pytest.mark.parametrize("form", ["lanes", "simple"])
@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "28", "51", "58") + lv.MIXED for l in lv.levels_of(c)])
def test_gauss_samp_gq(gpu, oracle, hip_env, ctx, level, form):
    """z = gauss_samp_gq_arb_base(M) at the level: G_l * z == M, one integer per coefficient in every limb, and in the
    same-width bases (where the oracle's own dpt is the context's) every digit equals the CPU restatement's"""
    n = 128
    p = lv.params(gpu, oracle, ctx, n)
    moduli, base, dpt = p.moduli()[: level + 1], p.base_bits(), lv.dpt_of(p)
    k = dpt * (level + 1)
    if form == "simple":
        hip_env.set("MXX_HIP_GSAMP", "simple")
    x = lv.host(oracle, 1100, 2, 2, moduli, n)
    c = ((1 << base) + 1) * 4.578
    src, z = _up(gpu, p, x, False), lv.new(gpu, p, 2 * k, 2, level, False)
    lv.call("gpu_matrix_gauss_samp_gq_arb_base", src.raw, base, c, 4.578, _gseed(gpu, 31), z.raw)
    got = _words(z, False)
    if ctx not in lv.MIXED:
        assert np.array_equal(got, oracle.gauss_samp_gq(x, moduli, base, c, lv.seed_bytes(31)))
    zc = oracle.centered(got[:, :, 0], moduli[0])
    assert np.abs(zc).max() < 8 * c
    for l, q in enumerate(moduli):
        assert np.array_equal(oracle.centered(got[:, :, l], q), zc), l
    G = oracle.matrix_ntt(lv.ref_gadget(2, moduli, base, dpt, n), moduli)
    assert np.array_equal(oracle.matmul(G, oracle.matrix_ntt(got, moduli), moduli), oracle.matrix_ntt(x, moduli)), "G * z != target"


def _small(rng, rows, cols, bound, moduli, n):
    v = rng.integers(-bound, bound + 1, size=(rows, cols, n))
    return np.stack([np.mod(v, q).astype(np.uint64) for q in moduli], axis=-2)


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "51") for l in lv.levels_of(c)])
def test_p1_sampler_full_and_cached(gpu, oracle, ctx, level, d):
    n, cols = 128, 3
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    rng = np.random.default_rng(1200 + d)
    a, b, dm = (_small(rng, d, d, bound, moduli, n) for bound in (60, 25, 60))
    tp2 = _small(rng, 2 * d, cols, 5000, moduli, n)
    sigma, s_par, dgg = 12.0, 900.0, 4.578
    ga, gb, gd = (_up(gpu, p, x, False) for x in (a, b, dm))
    sv, up = oracle.p1_covariance(a, b, dm, moduli, sigma, s_par, dgg)
    want = oracle.sample_p1(tp2, moduli, sv, up, -(sigma * sigma) / (s_par * s_par - sigma * sigma), lv.seed_bytes(41))
    cache = M.create_p1_covariance_cache(ga, gb, gd, sigma, s_par, dgg)
    out = lv.new(gpu, p, 2 * d, cols, level, True)
    g_tp2 = _up(gpu, p, tp2, False)  # held: a handle outlives the call only while its matrix object does
    lv.call("gpu_matrix_sample_p1_full_cached", cache.raw, g_tp2.raw, _gseed(gpu, 41), out.raw)
    out.is_ntt = True
    assert np.array_equal(out.to_coeff_rns(), want)
    full = lv.new(gpu, p, 2 * d, cols, level, True)
    g_tp2 = _up(gpu, p, tp2, False)
    lv.call("gpu_matrix_sample_p1_full", ga.raw, gb.raw, gd.raw, g_tp2.raw, sigma, s_par, dgg, _gseed(gpu, 41), full.raw)
    full.is_ntt = True
    assert full == out


# ---------------------------------------------------------------------------------------------------------------------
# preimage: key material created at the level, through the C entries
# ---------------------------------------------------------------------------------------------------------------------
SIGMA = 4.578


class _Key:
    """a trapdoor at `level`: the CPU restatement's R, E, A at the truncated basis, uploaded as level-l matrices"""

    def __init__(self, gpu, oracle, p, level, d, master):
        from mxx_amd.trapdoor import GpuDCRTTrapdoor

        self.moduli, n, base = p.moduli()[: level + 1], p.ring_dimension(), p.base_bits()
        self.host = oracle.trapdoor_gen(self.moduli, n, base, SIGMA, d, master)  # r, e, a
        r, e, a = (_up(gpu, p, x, True) for x in self.host)
        self.td, self.A = GpuDCRTTrapdoor(r, e), a
        self.k, c, s = oracle.preimage_params(self.moduli, n, base, SIGMA, d)
        self.cache = self.td.p1_covariance_cache(c, s, SIGMA)
        assert self.td.re.level == level and self.A.level == level and self.A.size() == (d, 2 * d + d * self.k)


def _request_seeds(gpu, oracle, masters):
    flat = [gpu.GpuRngSeed.from_bytes(oracle._seed_from(m, i).tobytes()) for m in masters for i in (3, 4, 5)]  # p2, p1, z
    return (gpu.GpuRngSeed * len(flat))(*flat)


def _preimage_many(gpu, p, key, targets, seeds, level, d):
    outs = [lv.new(gpu, p, 2 * d + d * key.k, t.ncol, level, False) for t in targets]
    lv.call("gpupoly_trapdoor_preimage_many", key.td.re.raw, key.cache.raw, key.A.raw, p.base_bits(), lv.arr(targets), len(targets),
            seeds, lv.arr(outs))
    for o in outs:
        o.is_ntt = True
    return outs


def _preimage_keyed(gpu, p, keys, key_of, targets, seeds, level, d):
    outs = [lv.new(gpu, p, 2 * d + d * keys[0].k, t.ncol, level, False) for t in targets]
    lv.call("gpupoly_trapdoor_preimage_keyed", lv.arr([k.td.re for k in keys]), lv.arr([k.cache for k in keys]), lv.arr([k.A for k in keys]),
            len(keys), p.base_bits(), (C.c_uint32 * len(key_of))(*key_of), lv.arr(targets), len(targets), seeds, lv.arr(outs))
    for o in outs:
        o.is_ntt = True
    return outs


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "51") for l in lv.levels_of(c)])
def test_preimage_many_and_keyed(gpu, oracle, ctx, level, d):
    """Both entries accept a level below the top (preimage.hip takes the level from re->level): A x == target at the
    level, the CPU restatement at the truncated basis word for word, the norm bound of the top-level tests, and the same
    call in the context over the prefix basis under the same seeds."""
    from mxx_amd.trapdoor import compute_preimage_norm

    n, cols = 128, [3, 0, 2]
    p, q = lv.params(gpu, oracle, ctx, n), lv.params(gpu, oracle, ctx, n, prefix=level)
    moduli, base = p.moduli()[: level + 1], p.base_bits()
    assert lv.dpt_of(p) == lv.dpt_of(q) == oracle.digits_per_tower(moduli, base)
    keys = [_Key(gpu, oracle, p, level, d, lv.seed_bytes(50 + i)) for i in range(2)]
    tops = [_Key(gpu, oracle, q, level, d, lv.seed_bytes(50 + i)) for i in range(2)]
    t_np = [oracle.matrix_ntt(oracle.random_matrix(1300 + j, d, max(c, 1), moduli, n), moduli)[:, :c] for j, c in enumerate(cols)]
    masters = [lv.seed_bytes(60 + j) for j in range(len(cols))]
    seeds = _request_seeds(gpu, oracle, masters)
    bound = compute_preimage_norm(np.sqrt(n), d * keys[0].k, float(1 << base))

    def targets_in(params):
        return [_up(gpu, params, np.ascontiguousarray(t), True) if t.shape[1] else lv.new(gpu, params, d, 0, level, True) for t in t_np]

    def check(outs, key_of, what):
        for j, (x, c) in enumerate(zip(outs, cols)):
            key = keys[key_of[j]]
            assert x.level == level and x.size() == (2 * d + d * key.k, c), (what, j)
            if c == 0:
                continue
            r, e, a = key.host
            assert np.array_equal(x.to_rns(), oracle.preimage(moduli, n, base, SIGMA, r, e, a, t_np[j], masters[j])), (what, j)
            assert np.array_equal(oracle.matmul(a, x.to_rns(), moduli), t_np[j]), (what, j, "A x != target")
            assert key.A * x == targets_in(p)[j], (what, j)
            assert 0 < x.centered_max_abs() < bound, (what, j)

    many = _preimage_many(gpu, p, keys[0], targets_in(p), seeds, level, d)
    check(many, [0, 0, 0], "many")
    key_of = [1, 0, 1]
    keyed = _preimage_keyed(gpu, p, keys, key_of, targets_in(p), seeds, level, d)
    check(keyed, key_of, "keyed")
    top_many = _preimage_many(gpu, q, tops[0], targets_in(q), seeds, level, d)
    top_keyed = _preimage_keyed(gpu, q, tops, key_of, targets_in(q), seeds, level, d)
    for a, b in zip(many + keyed, top_many + top_keyed):
        assert np.array_equal(a.to_rns(), b.to_rns()), "the prefix context gives other words under the same seeds"


# ---------------------------------------------------------------------------------------------------------------------
# movement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "51", "24_24_31") for l in lv.levels_of(c)])
def test_movement(gpu, oracle, ctx, level):
    """copy_to_context into contexts sharing the device (the same basis, and the prefix basis whose top level this is),
    all_gather_columns over two contexts on one device, store_const_coeff_batch, load / store with a padded stride"""
    from mxx_amd.parallel import GpuComm

    n = 1024
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli, L = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1], level + 1
    twin = gpu.GpuDCRTPolyParams(n, p.moduli(), p.base_bits(), gpu_ids=p.gpu_ids(), dnum=170 + level)
    prefix = gpu.GpuDCRTPolyParams(n, moduli, p.base_bits(), gpu_ids=p.gpu_ids(), dnum=180 + level)
    assert len({x.ctx_raw().value for x in (p, twin, prefix)}) == 3
    x = lv.host(oracle, 1400, 2, 3, moduli, n)
    for eval_format in (True, False):
        src = _up(gpu, p, x, eval_format)
        for dst in (twin, prefix):
            rep = src.to_params(dst)
            assert rep.params is dst and rep.level == level and rep.is_ntt == eval_format
            assert np.array_equal(rep.to_rns(), x)
            assert rep == _up(gpu, dst, x, eval_format)  # the tag travelled: a format-checked entry agrees
    comm = GpuComm([p, twin])
    blocks = [_up(gpu, p, np.ascontiguousarray(x[:, :2]), True), _up(gpu, twin, np.ascontiguousarray(x[:, 2:]), True)]
    fulls = comm.all_gather_columns(blocks)
    for f in fulls:
        assert f.level == level and np.array_equal(f.to_rns(), x)
    comm.close()
    coeff = _up(gpu, p, x, False)
    assert np.array_equal(coeff.store_const_coeff_words(), x[..., 0])
    # polynomials 8 * (L n + 5) bytes apart on the host: the gaps stay as they were on the way out
    bpp = 8 * (L * n + 5)
    wire = np.full((6, L * n + 5), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    wire[:, : L * n] = x.reshape(6, L * n)
    m = lv.new(gpu, p, 2, 3, level, False)
    m.load_rns_bytes(wire.view(np.uint8).reshape(-1), bpp, COEFF)
    assert np.array_equal(m.to_rns(), x)
    back = np.full_like(wire, 0x5A5A5A5A5A5A5A5A)
    m.store_rns_bytes(back.view(np.uint8).reshape(-1), bpp, COEFF)
    assert np.array_equal(back[:, : L * n].reshape(x.shape), x) and (back[:, L * n:] == 0x5A5A5A5A5A5A5A5A).all()
    m.ntt_all_in_place()
    assert np.array_equal(m.to_rns(), oracle.matrix_ntt(x, moduli))


@pytest.mark.parametrize("ctx,level", [(c, l) for c in ("24", "51") for l in lv.levels_of(c)])
def test_views_pointers_wire_aliases_hashed_blocks_and_mul_acc(gpu, oracle, ctx, level):
    """the entries that no other cell here reaches: row and reshape views, the device pointer's byte count, the 1x1 aliases of
    the compact wire format, the hashed forms of the block samplers, and the accumulating product"""
    from mxx_amd.matrix import device_hash_seeds, hash_tags_arg

    n = 128
    p = lv.params(gpu, oracle, ctx, n)
    M, moduli, L, lib = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1], level + 1, _ffi.lib()
    a = lv.host(oracle, 1450, 4, 3, moduli, n)
    ga = _up(gpu, p, a, True)
    view = ga.row_view(1, 3)
    assert view.level == level and np.array_equal(view.to_rns(), a[1:3])
    assert np.array_equal(ga.reshape_view(2, 6).to_rns(), a.reshape(2, 6, L, n))
    view.add_in_place(view)  # a write through the view lands in the parent's rows, and only there
    want = a.copy()
    want[1:3] = oracle.pointwise("add", a[1:3], a[1:3], moduli)
    assert np.array_equal(ga.to_rns(), want)
    ptr, size = C.c_void_p(), C.c_size_t()
    lv.call("gpupoly_matrix_device_ptr", ga.raw, C.byref(ptr), C.byref(size))
    assert ptr.value and size.value == 12 * L * n * p.ctx().word_bytes()
    # the compact wire format of one polynomial through both names, against the oracle at the truncated basis
    coeff = lv.host(oracle, 1451, 1, 1, moduli, n, edges=False)

    def store(entry, m):
        cap = n * 8 * L + 16
        buf, bits, bpc, ln = (C.c_uint8 * cap)(), C.c_uint16(0), C.c_uint16(0), C.c_size_t(0)
        lv.call(entry, m.raw, buf, cap, C.byref(bits), C.byref(bpc), C.byref(ln))
        return bytes(buf[: ln.value]), bits.value, bpc.value

    got = store("gpu_poly_store_compact_bytes", _up(gpu, p, coeff, False))
    assert got == store("gpu_matrix_store_compact_bytes", _up(gpu, p, coeff, False)) == oracle.compact_payload(coeff, moduli)
    payload = (C.c_uint8 * max(len(got[0]), 1)).from_buffer_copy(got[0].ljust(1, b"\0"))
    for entry in ("gpu_poly_load_compact_bytes", "gpu_matrix_load_compact_bytes"):
        back = lv.new(gpu, p, 1, 1, level, True)
        lv.call(entry, back.raw, payload, len(got[0]), got[1])
        assert np.array_equal(_words(back, False), coeff), entry
    # hashed block samplers: the seeded entries' words under the device's own seeds, and the oracle's samples
    tags = [b"level_blk_" + bytes([48 + t]) for t in range(3)]
    seeds = device_hash_seeds(p, lv.seed_bytes(9), tags)
    seed_arr = (gpu.GpuRngSeed * 3)(*seeds)
    arg, keep, _ = hash_tags_arg(lv.seed_bytes(9), tags)
    for name, gauss in (("uniform", False), ("gauss", True)):
        seeded, hashed = lv.new(gpu, p, 3, 2, level, False), lv.new(gpu, p, 3, 2, level, False)
        if gauss:
            lv.call("gpupoly_matrix_sample_gauss_blocks", seeded.raw, 3.5, seed_arr, 3, _ffi.GPUPOLY_BLOCKS_STACKED, None)
            lv.call("gpupoly_matrix_sample_hash_gauss_blocks", hashed.raw, 3.5, C.byref(arg), 3, _ffi.GPUPOLY_BLOCKS_STACKED, None)
        else:
            lv.call("gpupoly_matrix_sample_distribution_blocks", seeded.raw, 0, seed_arr, 3, _ffi.GPUPOLY_BLOCKS_STACKED, None)
            lv.call("gpupoly_matrix_sample_hash_blocks", hashed.raw, 0, C.byref(arg), 3, _ffi.GPUPOLY_BLOCKS_STACKED, None)
        got_s, got_h = _words(seeded, True), _words(hashed, True)
        assert np.array_equal(got_s, got_h), name
        for t in range(3):
            smp = oracle.sample_distribution(1, 2, moduli, n, name, 3.5 if gauss else 0.0, seeds[t].to_bytes())
            assert np.array_equal(got_h[t].reshape(1, 2, L, n), oracle.matrix_ntt(smp, moduli)), (name, t)
    del keep
    # out += lhs * rhs and out -= lhs * rhs
    x, y, acc = oracle.random_matrix(1452, 2, 3, moduli, n), oracle.random_matrix(1453, 3, 2, moduli, n), oracle.random_matrix(1454, 2, 2, moduli, n)
    gx, gy, gacc = _up(gpu, p, x, True), _up(gpu, p, y, True), _up(gpu, p, acc, True)
    prod = oracle.matmul(x, y, moduli)
    gacc.mul_add_in_place(gx, gy)
    assert np.array_equal(gacc.to_rns(), oracle.pointwise("add", acc, prod, moduli))
    gacc.mul_sub_in_place(gx, gy)
    gacc.mul_sub_in_place(gx, gy)
    assert np.array_equal(gacc.to_rns(), oracle.pointwise("sub", acc, prod, moduli))


# ---------------------------------------------------------------------------------------------------------------------
# mixed levels are refused: non-zero, a message naming the entry with "level" or "mismatch", nothing launched, and the
# words and format tag of every matrix passed as they were
# ---------------------------------------------------------------------------------------------------------------------
class _Pool:
    """matrices of the 24-bit context (D = 4) at level 1 ("hi") and level 0 ("lo"), n = 16"""

    def __init__(self, gpu, oracle, n=16):
        self.gpu, self.oracle, self.n = gpu, oracle, n
        self.p = lv.params(gpu, oracle, "24", n)
        self.base, self.dpt = self.p.base_bits(), lv.dpt_of(self.p)
        self.made = []
        self.count = 0

    def m(self, rows, cols, level, is_ntt=True):
        self.count += 1
        x = self.oracle.random_matrix(1500 + self.count, rows, cols, self.p.moduli()[: level + 1], self.n)
        out = _up(self.gpu, self.p, x, is_ntt)
        self.made.append((out, is_ntt, x))
        return out

    def k(self, level):
        return self.dpt * (level + 1)


def _refuse(pool, entry, fn, names=None):
    lib = _ffi.lib()
    _ffi.gpu_device_sync()
    c0 = lib.gpupoly_launch_count()
    rc = fn()
    msg = _ffi.last_error_string() if rc else ""
    c1 = lib.gpupoly_launch_count()
    assert rc != 0, f"{entry}: accepted operands of different levels"
    assert c1 == c0, f"{entry}: launched {c1 - c0} kernels before refusing"
    assert any(nm in msg for nm in (names or (entry,))) and ("level" in msg or "mismatch" in msg), (entry, msg)
    for mat, tag, words in pool.made:
        mat.is_ntt = tag  # the store refuses any other tag than the device's
        assert np.array_equal(mat.to_rns(), words), f"{entry}: a refused call changed a matrix"


def _cases():
    """name -> (entry, builder(pool) -> thunk returning the status)"""
    lib = _ffi.lib
    E, Cf = True, False
    cases = {}

    def add(name, entry, build, names=None):
        cases[name] = (entry, build, names)

    for op in ("gpu_matrix_add", "gpu_matrix_sub"):
        add(f"{op} rhs", op, lambda P, op=op: (lambda o=P.m(2, 2, 1), a=P.m(2, 2, 1), b=P.m(2, 2, 0): getattr(lib(), op)(o.raw, a.raw, b.raw)))
        add(f"{op} out", op, lambda P, op=op: (lambda o=P.m(2, 2, 0), a=P.m(2, 2, 1), b=P.m(2, 2, 1): getattr(lib(), op)(o.raw, a.raw, b.raw)))
    add("mul rhs", "gpu_matrix_mul", lambda P: (lambda o=P.m(2, 2, 1), a=P.m(2, 3, 1), b=P.m(3, 2, 0): lib().gpu_matrix_mul(o.raw, a.raw, b.raw)))
    add("mul lhs", "gpu_matrix_mul", lambda P: (lambda o=P.m(2, 2, 1), a=P.m(2, 3, 0), b=P.m(3, 2, 1): lib().gpu_matrix_mul(o.raw, a.raw, b.raw)))
    add("mul out", "gpu_matrix_mul", lambda P: (lambda o=P.m(2, 2, 0), a=P.m(2, 3, 1), b=P.m(3, 2, 1): lib().gpu_matrix_mul(o.raw, a.raw, b.raw)))
    for op in ("gpu_matrix_mul_scalar", "gpupoly_matrix_mul_scalar_intt"):
        add(f"{op} scalar", op, lambda P, op=op: (lambda o=P.m(2, 2, 1), a=P.m(2, 2, 1), s=P.m(1, 1, 0): getattr(lib(), op)(o.raw, a.raw, s.raw)))
        add(f"{op} out", op, lambda P, op=op: (lambda o=P.m(2, 2, 0), a=P.m(2, 2, 1), s=P.m(1, 1, 1): getattr(lib(), op)(o.raw, a.raw, s.raw)))
    add("neg", "gpupoly_matrix_neg", lambda P: (lambda o=P.m(2, 2, 0), a=P.m(2, 2, 1): lib().gpupoly_matrix_neg(o.raw, a.raw)))
    add("copy", "gpu_matrix_copy", lambda P: (lambda o=P.m(2, 2, 0), a=P.m(2, 2, 1): lib().gpu_matrix_copy(o.raw, a.raw)))
    for op in ("gpu_matrix_copy_block", "gpu_matrix_add_block"):
        add(op, op, lambda P, op=op: (lambda o=P.m(3, 3, 0), a=P.m(2, 2, 1): getattr(lib(), op)(o.raw, a.raw, 1, 1, 0, 0, 2, 2)))
    add("tensor rhs", "gpupoly_matrix_tensor", lambda P: (lambda o=P.m(4, 2, 1), a=P.m(2, 1, 1), b=P.m(2, 2, 0): lib().gpupoly_matrix_tensor(o.raw, a.raw, b.raw)))
    add("tensor out", "gpupoly_matrix_tensor", lambda P: (lambda o=P.m(4, 2, 0), a=P.m(2, 1, 1), b=P.m(2, 2, 1): lib().gpupoly_matrix_tensor(o.raw, a.raw, b.raw)))
    add("transpose", "gpupoly_matrix_transpose", lambda P: (lambda o=P.m(3, 2, 0), a=P.m(2, 3, 1): lib().gpupoly_matrix_transpose(o.raw, a.raw)))
    add("concat", "gpupoly_matrix_concat_columns",
        lambda P: (lambda o=P.m(2, 3, 1), bs=[P.m(2, 2, 1), P.m(2, 1, 0)]: lib().gpupoly_matrix_concat_columns(o.raw, lv.arr(bs), 2)))
    add("split", "gpupoly_matrix_split_columns",
        lambda P: (lambda s=P.m(2, 3, 1), bs=[P.m(2, 2, 1), P.m(2, 1, 0)]: lib().gpupoly_matrix_split_columns(s.raw, lv.arr(bs), 2)))
    add("add_rows out", "gpupoly_matrix_add_rows", lambda P: (lambda o=P.m(4, 2, 0), a=P.m(2, 2, 1), b=P.m(2, 2, 1): lib().gpupoly_matrix_add_rows(o.raw, 1, a.raw, b.raw)))
    add("add_rows rhs", "gpupoly_matrix_add_rows", lambda P: (lambda o=P.m(4, 2, 1), a=P.m(2, 2, 1), b=P.m(2, 2, 0): lib().gpupoly_matrix_add_rows(o.raw, 1, a.raw, b.raw)))
    add("ntt_add_rows out", "gpupoly_matrix_ntt_add_rows",
        lambda P: (lambda o=P.m(4, 2, 0), a=P.m(2, 2, 1, Cf), b=P.m(2, 2, 1): lib().gpupoly_matrix_ntt_add_rows(o.raw, 1, a.raw, b.raw, 0)))
    add("ntt_add_rows addend", "gpupoly_matrix_ntt_add_rows",
        lambda P: (lambda o=P.m(4, 2, 1), a=P.m(2, 2, 1, Cf), b=P.m(2, 2, 0): lib().gpupoly_matrix_ntt_add_rows(o.raw, 1, a.raw, b.raw, 1)))
    add("mul_batch one product", "gpupoly_matrix_mul_batch",
        lambda P: (lambda o=[P.m(2, 2, 1), P.m(1, 1, 1)], a=[P.m(2, 3, 1), P.m(1, 2, 1)], b=[P.m(3, 2, 1), P.m(2, 1, 0)]:
                   lib().gpupoly_matrix_mul_batch(lv.arr(o), lv.arr(a), lv.arr(b), 2)))
    add("mul_batch two levels", "gpupoly_matrix_mul_batch",
        lambda P: (lambda o=[P.m(2, 2, 1), P.m(1, 1, 0)], a=[P.m(2, 3, 1), P.m(1, 2, 0)], b=[P.m(3, 2, 1), P.m(2, 1, 0)]:
                   lib().gpupoly_matrix_mul_batch(lv.arr(o), lv.arr(a), lv.arr(b), 2)))

    def batch(P, gates):
        ops = (_ffi.GpuBatchOp * len(gates))()
        for i, (kind, o, a, b) in enumerate(gates):
            ops[i].kind, ops[i].out, ops[i].lhs, ops[i].rhs = kind, o.raw, a.raw, (b.raw if b is not None else None)
        return lambda: lib().gpupoly_batch(ops, len(gates), P.base)

    # a valid product FIRST: the products of a batch are launched before its point-wise gates are looked at
    add("batch add after a product", "gpupoly_batch", lambda P: batch(P, [(_ffi.GPUPOLY_OP_MUL, P.m(2, 2, 1), P.m(2, 3, 1), P.m(3, 2, 1)),
                                                                           (_ffi.GPUPOLY_OP_ADD, P.m(2, 2, 1), P.m(2, 2, 1), P.m(2, 2, 0))]))
    add("batch mul_scalar after a product", "gpupoly_batch", lambda P: batch(P, [(_ffi.GPUPOLY_OP_MUL, P.m(2, 2, 1), P.m(2, 3, 1), P.m(3, 2, 1)),
                                                                                  (_ffi.GPUPOLY_OP_MUL_SCALAR, P.m(2, 2, 1), P.m(2, 2, 1), P.m(1, 1, 0))]))
    add("batch decompose after a product", "gpupoly_batch", lambda P: batch(P, [(_ffi.GPUPOLY_OP_MUL, P.m(2, 2, 1), P.m(2, 3, 1), P.m(3, 2, 1)),
                                                                                 (_ffi.GPUPOLY_OP_DECOMPOSE, P.m(P.k(1), 2, 0), P.m(1, 2, 1), None)]))
    add("batch mul_decompose after a neg", "gpupoly_batch", lambda P: batch(P, [(_ffi.GPUPOLY_OP_NEG, P.m(2, 2, 1), P.m(2, 2, 1), None),
                                                                                 (_ffi.GPUPOLY_OP_MUL_DECOMPOSE, P.m(2, 2, 1), P.m(2, P.k(1), 1), P.m(1, 2, 0))]))
    for op, small in (("gpupoly_matrix_mul_decompose", False), ("gpupoly_matrix_mul_decompose_small", True)):
        kk = (lambda P, small=small: P.dpt if small else P.k(1))
        add(f"{op} rhs", op, lambda P, op=op, kk=kk: (lambda o=P.m(2, 2, 1), a=P.m(2, kk(P), 1), b=P.m(1, 2, 0): getattr(lib(), op)(o.raw, a.raw, b.raw, P.base)))
        add(f"{op} out", op, lambda P, op=op, kk=kk: (lambda o=P.m(2, 2, 0), a=P.m(2, kk(P), 1), b=P.m(1, 2, 1): getattr(lib(), op)(o.raw, a.raw, b.raw, P.base)))
    add("mul_tensor_identity rhs", "gpupoly_matrix_mul_tensor_identity",
        lambda P: (lambda o=P.m(2, 4, 1), a=P.m(2, 2, 1), b=P.m(1, 2, 0): lib().gpupoly_matrix_mul_tensor_identity(o.raw, a.raw, b.raw, 2)))
    add("mul_tensor_identity_decompose out", "gpupoly_matrix_mul_tensor_identity_decompose",
        lambda P: (lambda o=P.m(2, 4, 0), a=P.m(2, 2 * P.k(1), 1), b=P.m(1, 2, 1): lib().gpupoly_matrix_mul_tensor_identity_decompose(o.raw, a.raw, b.raw, 2, P.base)))
    add("decompose_base", "gpu_matrix_decompose_base",
        lambda P: (lambda s=P.m(1, 2, 1, Cf), o=P.m(P.k(1), 2, 0): lib().gpu_matrix_decompose_base(s.raw, P.base, o.raw)))
    add("decompose_base_small", "gpu_matrix_decompose_base",
        lambda P: (lambda s=P.m(1, 2, 0, Cf), o=P.m(P.dpt, 2, 1): lib().gpu_matrix_decompose_base_small(s.raw, P.base, o.raw)))
    add("decompose_rows", "gpupoly_matrix_decompose_rows",
        lambda P: (lambda s=P.m(1, 2, 1, Cf), o=P.m(2, 2, 0): lib().gpupoly_matrix_decompose_rows(s.raw, P.base, 0, 1, o.raw)))
    add("identity chunk", "gpu_matrix_fill_small_decomposed_identity_chunk",
        lambda P: (lambda o=P.m(3, 3, 1), s=P.m(1, P.dpt, 0): lib().gpu_matrix_fill_small_decomposed_identity_chunk(o.raw, s.raw, 1)))
    add("fill_identity", "gpupoly_matrix_fill_identity", lambda P: (lambda o=P.m(3, 3, 1), s=P.m(1, 1, 0): lib().gpupoly_matrix_fill_identity(o.raw, s.raw)))
    add("gauss_samp_gq", "gpu_matrix_gauss_samp_gq_arb_base",
        lambda P: (lambda s=P.m(1, 2, 1, Cf), o=P.m(P.k(1), 2, 0): lib().gpu_matrix_gauss_samp_gq_arb_base(s.raw, P.base, 18756.0, 4.578, _gseed(P.gpu, 71), o.raw)))

    def p1(P, levels, cached):
        """levels of a, b, d, tp2, out; the cached form builds its cache from a, b, d at level 1"""
        a, b, d = (P.m(1, 1, l, Cf) for l in levels[:3])
        tp2, out = P.m(2, 2, levels[3], Cf), P.m(2, 2, levels[4])
        if not cached:
            return lambda: lib().gpu_matrix_sample_p1_full(a.raw, b.raw, d.raw, tp2.raw, 12.0, 900.0, 4.578, _gseed(P.gpu, 72), out.raw)
        rng = np.random.default_rng(7)
        mats = [_up(P.gpu, P.p, _small(rng, 1, 1, 40, P.p.moduli()[:2], P.n), False) for _ in range(3)]
        cache = P.gpu.GpuDCRTPolyMatrix.create_p1_covariance_cache(*mats, 12.0, 900.0, 4.578)
        return lambda keep=(mats, cache): lib().gpu_matrix_sample_p1_full_cached(cache.raw, tp2.raw, _gseed(P.gpu, 72), out.raw)

    add("p1_full tp2", "gpu_matrix_sample_p1_full", lambda P: p1(P, (1, 1, 1, 0, 1), False))
    add("p1_full out", "gpu_matrix_sample_p1_full", lambda P: p1(P, (1, 1, 1, 1, 0), False))
    add("p1_full d_mat", "gpu_matrix_sample_p1_full", lambda P: p1(P, (1, 1, 0, 1, 1), False))
    add("p1_cached tp2", "gpu_matrix_sample_p1_full_cached", lambda P: p1(P, (1, 1, 1, 0, 1), True))
    add("p1_cached out", "gpu_matrix_sample_p1_full_cached", lambda P: p1(P, (1, 1, 1, 1, 0), True))
    return cases


_CASES = _cases()


@pytest.mark.parametrize("name", sorted(_CASES))
def test_mixed_levels_are_refused(gpu, oracle, name):
    entry, build, names = _CASES[name]
    pool = _Pool(gpu, oracle)
    _refuse(pool, entry, build(pool), names)


@pytest.mark.parametrize("what", ["many target", "many out", "many public matrix", "keyed key", "keyed target"])
def test_mixed_levels_are_refused_by_the_preimage_entries(gpu, oracle, what):
    n, d = 128, 1
    pool = _Pool(gpu, oracle, n)
    p = pool.p
    keys = [_Key(gpu, oracle, p, 1, d, lv.seed_bytes(80)), _Key(gpu, oracle, p, 1, d, lv.seed_bytes(81)), _Key(gpu, oracle, p, 0, d, lv.seed_bytes(82))]
    for key in keys:
        pool.made += [(key.td.re, True, key.td.re.to_rns()), (key.A, True, key.A.to_rns())]
    rows = 2 * d + d * keys[0].k
    seeds = _request_seeds(gpu, oracle, [lv.seed_bytes(90), lv.seed_bytes(91)])
    t = [pool.m(d, 2, 0 if what.endswith("target") else 1), pool.m(d, 1, 1)]
    o = [pool.m(rows, 2, 0 if what == "many out" else 1), pool.m(rows, 1, 1)]
    lib = _ffi.lib()
    if what.startswith("many"):
        A = keys[2].A if what == "many public matrix" else keys[0].A
        fn = lambda: lib.gpupoly_trapdoor_preimage_many(keys[0].td.re.raw, keys[0].cache.raw, A.raw, p.base_bits(), lv.arr(t), 2, seeds, lv.arr(o))  # noqa: E731
        _refuse(pool, "gpupoly_trapdoor_preimage_many", fn)
    else:
        ks = [keys[0], keys[2]] if what == "keyed key" else keys[:2]
        fn = lambda: lib.gpupoly_trapdoor_preimage_keyed(lv.arr([k.td.re for k in ks]), lv.arr([k.cache for k in ks]), lv.arr([k.A for k in ks]), 2,  # noqa: E731
                                                         p.base_bits(), (C.c_uint32 * 2)(0, 1), lv.arr(t), 2, seeds, lv.arr(o))
        _refuse(pool, "gpupoly_trapdoor_preimage_keyed", fn)


def test_mixed_levels_are_refused_by_the_movement_entries(gpu, oracle):
    from mxx_amd.parallel import GpuComm

    pool = _Pool(gpu, oracle, 1024)
    p, lib = pool.p, _ffi.lib()
    twin = gpu.GpuDCRTPolyParams(1024, p.moduli(), p.base_bits(), gpu_ids=p.gpu_ids(), dnum=190)
    comm = GpuComm([p, twin])
    x = oracle.random_matrix(1600, 2, 2, p.moduli()[:2], 1024)
    other = [(_up(gpu, twin, x, True), x), (_up(gpu, twin, np.ascontiguousarray(x[:, :, :1]), True), np.ascontiguousarray(x[:, :, :1]))]
    for blocks, fulls in (([pool.m(2, 2, 1), other[1][0]], [pool.m(2, 4, 1), _up(gpu, twin, np.concatenate([x, x], axis=1), True)]),
                          ([pool.m(2, 2, 1), other[0][0]], [pool.m(2, 4, 0), _up(gpu, twin, np.concatenate([x, x], axis=1), True)])):
        _refuse(pool, "gpupoly_matrix_all_gather_columns", lambda: lib.gpupoly_matrix_all_gather_columns(comm.raw, lv.arr(blocks), lv.arr(fulls)))
    for m, words in other:
        assert np.array_equal(m.to_rns(), words)
    comm.close()
    # a source whose level lies beyond the destination context's limbs
    one_limb = gpu.GpuDCRTPolyParams(1024, p.moduli()[:1], p.base_bits(), gpu_ids=p.gpu_ids(), dnum=191)
    src, raw = pool.m(1, 2, 1), C.c_void_p()
    _refuse(pool, "gpupoly_matrix_copy_to_context", lambda: lib.gpupoly_matrix_copy_to_context(one_limb.ctx_raw(), src.raw, C.byref(raw)))
    assert not raw.value


def test_equal_answers_not_equal_across_levels_without_an_error(gpu, oracle):
    pool = _Pool(gpu, oracle)
    a = pool.m(2, 2, 1)
    words = a.to_rns()
    b = _up(gpu, pool.p, np.ascontiguousarray(words[:, :, :1]), True)  # the same limb-0 words at level 0
    eq = C.c_int(7)
    assert _ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)) == 0 and eq.value == 0
    assert _ffi.lib().gpu_matrix_equal(a.raw, a.clone().raw, C.byref(eq)) == 0 and eq.value == 1
