"""Every launch grid that folds past 65535 entries, and every block window, run past its edge.

Many launchers put one output polynomial (or tile, or limb vector) per workgroup on blockIdx.y; past 65535 of them the index
is folded over blockIdx.z, the kernel rebuilds it as blockIdx.z * gridDim.y + blockIdx.y and guards the ragged last layer, or
the work is cut into several launches.  Each case here

  * runs the smallest ring that takes the kernel path under test: a polynomial of exactly 16 bytes - n = 4 with one 31-bit limb
    ("u32": 32-bit words) or n = 2 with one 51-bit limb ("u64": 64-bit words) - plus n = 4 with three 24-bit limbs ("u32x3": a
    48-byte polynomial stride, no power of two, and L > 1 for the index decodes that divide by L) and n = 2 in 32-bit words
    ("u32s": a limb vector of 8 bytes, the one-word-per-lane instances).  64-bit words have no such instance to reach: it
    needs an odd n and a context starts at n = 2;
  * asserts FROM THE TRACE that the launch was folded or chunked: the named kernel's block count is what the launcher's rule
    gives for the shape, computed here by `fold` / written next to the case, with gz >= 2 or the expected launches.  A case
    whose launch was not folded fails;
  * compares every word with plain numpy on the uploaded residues (Python integers where a product passes 64 bits).

The grid arithmetic itself, over counts no device run can afford, is checked on the host in test_grid_plan_host.py.
"""
import ctypes as C
import re

import numpy as np
import pytest

import gadget_scalar_model as GSM
import plainref as PR
import ran
from conftest import make_params

pytestmark = pytest.mark.gpu

Y_MAX = 65535
SIZE_MAX = (1 << 64) - 1
# name -> (n, limbs, limb bits, base bits); the base gives two digits per tower
RINGS = {"u32": (4, 1, 31, 16), "u64": (2, 1, 51, 26), "u32x3": (4, 3, 24, 12), "u32s": (2, 1, 31, 16), "u32x2": (4, 2, 24, 12),
         "u64x2": (2, 2, 51, 26)}
POLY16 = ["u32", "u64", "u32x3"]  # the 16-byte-per-lane movers: one instance, three polynomial strides


def fold(entries):
    """fold_yz of grid_plan.h as every launch site spelled it: (gy, gz) for `entries` workgroups, one per entry"""
    gy = min(entries, Y_MAX)
    return gy, -(-entries // gy)


def folded_blocks(entries, gx=1):
    """the block count of one folded launch over `entries`; a count that needs no fold is a mistake in the case"""
    gy, gz = fold(entries)
    assert gz >= 2, "the shape does not pass 65535 entries"
    return gx * gy * gz


def ring(gpu, oracle, name):
    n, depth, bits, base = RINGS[name]
    p = make_params(gpu, oracle, n, depth, bits, base)
    assert p.ctx().word_bytes() == (8 if bits > 31 else 4)
    return p


def qcol(p):
    return np.array([int(q) for q in p.moduli()], dtype=np.uint64).reshape(1, 1, -1, 1)


def rand(p, rows, cols, seed):
    """uniform residues (rows, cols, L, n), below each limb's modulus"""
    rng = np.random.default_rng(seed)
    n = p.ring_dimension()
    return np.stack([rng.integers(0, int(q), size=(rows, cols, n), dtype=np.uint64) for q in p.moduli()], axis=2)


def mulmod(a, b, q):
    """a * b mod q, elementwise with broadcasting: in 64 bits below 2^32, in Python integers above"""
    if int(q.max()) < 1 << 32:
        return (a * b) % q
    return ((a.astype(object) * b.astype(object)) % q.astype(object)).astype(np.uint64)


def addmod(a, b, q):
    return (a + b) % q  # both below q < 2^63


def submod(a, b, q):
    return (a + (q - b)) % q


def lib():
    from mxx_amd import _ffi

    return _ffi.lib()


def last_error():
    from mxx_amd import _ffi

    return _ffi.last_error_string()


# ---------------------------------------------------------------------------------------------------
# 1. gpupoly_matrix_transpose: one destination polynomial per (y, z)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POLY16)
def test_transpose_folds_past_65535_polynomials(gpu, oracle, name):
    """257 x 256 = 65792 polynomials: gx = 1 (a polynomial is at most three 16-byte vectors), gy = 65535, gz = 2.  Both tags,
    and the transpose of the transpose, which folds the other way round (256 x 257)."""
    p = ring(gpu, oracle, name)
    M = gpu.GpuDCRTPolyMatrix
    a = rand(p, 257, 256, 11)
    for fmt in (False, True):
        ga = M.from_rns(p, a, fmt)
        with ran.launches() as seen:
            t = ga.transpose()
            back = t.transpose()
        assert seen.blocks_of("transpose_kernel") == [folded_blocks(257 * 256)] * 2 and len(seen) == 2, seen.records
        assert t.size() == (256, 257) and t.is_ntt == fmt
        assert np.array_equal(t.to_rns(), a.transpose(1, 0, 2, 3))
        assert np.array_equal(back.to_rns(), a) and back == ga


# ---------------------------------------------------------------------------------------------------
# 2. concat_columns / split_columns: one polynomial of the launch's column span per (y, z), 64 blocks per launch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths,spans", [([100, 0, 1, 155], [256]), ([4] * 70, [256, 24])], ids=["empty_block_inside", "two_launches"])
@pytest.mark.parametrize("name", POLY16)
def test_column_blocks_fold_past_65535_polynomials(gpu, oracle, name, widths, spans):
    """257 rows.  [100, 0, 1, 155]: one launch over 257 * 256 = 65792 entries, folded, with an empty block inside (it takes no
    slot in the table).  Seventy blocks of width 4: the first launch takes 64 blocks (256 columns, 65792 entries, folded), the
    second the other 6 (24 columns, 6168 entries, one layer) and starts at column 256 of the wide matrix."""
    p = ring(gpu, oracle, name)
    M = gpu.GpuDCRTPolyMatrix
    rows, level = 257, p.crt_depth() - 1
    want_blocks = [folded_blocks(rows * spans[0])] + [rows * s for s in spans[1:]]
    assert all(rows * s <= Y_MAX for s in spans[1:])
    whole = rand(p, rows, sum(widths), 21)
    cuts = np.cumsum([0] + widths)
    parts_np = [whole[:, cuts[j]:cuts[j + 1]] for j in range(len(widths))]
    # concat, EVAL
    parts = [M.from_rns(p, b, True) if b.shape[1] else M(p, rows, 0, level, True) for b in parts_np]
    with ran.launches() as seen:
        wide = M.concat_columns_of(parts)
    assert seen.blocks_of("column_blocks_kernel<false>") == want_blocks and len(seen) == len(spans), seen.records
    assert wide.is_ntt and np.array_equal(wide.to_rns(), whole)
    # split, COEFF
    src = M.from_rns(p, whole, False)
    with ran.launches() as seen:
        back = src.split_columns(widths)
    assert seen.blocks_of("column_blocks_kernel<true>") == want_blocks and len(seen) == len(spans), seen.records
    for b, want in zip(back, parts_np):
        assert not b.is_ntt and b.size() == want.shape[:2]
        if want.shape[1]:
            assert np.array_equal(b.to_rns(), want)
    assert np.array_equal(src.to_rns(), whole)


# ---------------------------------------------------------------------------------------------------
# 3. gpu_matrix_add_block: chunks of whole block rows, 65535 / cols rows per launch; copy_block beside it
# ---------------------------------------------------------------------------------------------------
COPY_2D = "copy_block (2-D runtime copy"  # the trace's reader strips the parentheses around a kernel expression, this label's last one too
BLOCK = dict(rows=300, cols=257, src=(3, 5), dst=(7, 11), src_shape=(305, 280), dst_shape=(310, 300))
ADD_CHUNKS = [255 * 257, 45 * 257]  # rows_per_launch = 65535 // 257 = 255: launches of 255 and 45 rows, gx = 1


@pytest.mark.parametrize("name", ["u32", "u64", "u32x3"])
def test_add_block_chunks_by_rows(gpu, oracle, name):
    """a 300 x 257 block from (3, 5) of a 305 x 280 source onto (7, 11) of a 310 x 300 destination: two launches, the second
    starting at block row 255.  Every word of the destination is compared, outside the block included."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    assert BLOCK["rows"] * BLOCK["cols"] > Y_MAX and Y_MAX // BLOCK["cols"] == 255
    (sr, sc), (dr, dc), R, Cc = BLOCK["src"], BLOCK["dst"], BLOCK["rows"], BLOCK["cols"]
    s_np, d_np = rand(p, *BLOCK["src_shape"], 31), rand(p, *BLOCK["dst_shape"], 32)
    src, dst = M.from_rns(p, s_np, True), M.from_rns(p, d_np, True)
    with ran.launches() as seen:
        dst.add_block_from(src, dr, dc, sr, sc, R, Cc)
    kernel = "block_rect_kernel<uint64_t, true>" if name == "u64" else "block_rect_kernel<uint32_t, true>"
    assert seen.blocks_of(kernel) == ADD_CHUNKS and len(seen) == 2, seen.records
    want = d_np.copy()
    want[dr:dr + R, dc:dc + Cc] = addmod(d_np[dr:dr + R, dc:dc + Cc], s_np[sr:sr + R, sc:sc + Cc], q)
    assert np.array_equal(dst.to_rns(), want)
    assert np.array_equal(src.to_rns(), s_np)
    # the 2-D runtime copy over the same windows
    dst2 = M.from_rns(p, d_np, True)
    with ran.launches() as seen:
        dst2.copy_block_from(src, dr, dc, sr, sc, R, Cc)
    assert list(seen) == [COPY_2D], seen.records
    want = d_np.copy()
    want[dr:dr + R, dc:dc + Cc] = s_np[sr:sr + R, sc:sc + Cc]
    assert np.array_equal(dst2.to_rns(), want)


@pytest.mark.parametrize("name", ["u32", "u64", "u32x3"])
def test_add_block_chunks_by_rows_between_overlapping_views(gpu, oracle, name):
    """the same block between two row views of one 315 x 300 parent, rows [0, 305) and [5, 315): source rows 3..302 and
    destination rows 12..311 of the parent overlap, so the source block is staged first (one 2-D copy) and both launches read
    the staged copy, the second from its row 255.  Every word of the parent is compared with the block taken from the parent as
    it was.  copy_block over the same views goes through its shared temp: two 2-D copies."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    (sr, sc), (dr, dc), R, Cc = BLOCK["src"], BLOCK["dst"], BLOCK["rows"], BLOCK["cols"]
    p_np = rand(p, 315, 300, 33)
    kernel = "block_rect_kernel<uint64_t, true>" if name == "u64" else "block_rect_kernel<uint32_t, true>"
    for add in (True, False):
        parent = M.from_rns(p, p_np, True)
        src, dst = parent.row_view(0, 305), parent.row_view(5, 315)
        with ran.launches() as seen:
            (dst.add_block_from if add else dst.copy_block_from)(src, dr, dc, sr, sc, R, Cc)
        want = p_np.copy()
        block = p_np[sr:sr + R, sc:sc + Cc]
        if add:
            assert list(seen) == [COPY_2D, kernel, kernel] and seen.blocks_of(kernel) == ADD_CHUNKS, seen.records
            want[5 + dr:5 + dr + R, dc:dc + Cc] = addmod(p_np[5 + dr:5 + dr + R, dc:dc + Cc], block, q)
        else:
            assert list(seen) == [COPY_2D] * 2, seen.records
            want[5 + dr:5 + dr + R, dc:dc + Cc] = block
        assert np.array_equal(parent.to_rns(), want)


# ---------------------------------------------------------------------------------------------------
# 4. gpupoly_matrix_tensor: one output polynomial per (y, z)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u32", "u64", "u32x3", "u32s"])
def test_tensor_folds_past_65535_polynomials(gpu, oracle, name):
    """(16 x 16) (x) (17 x 16) = 272 x 256 = 69632 outputs, gx = 1: out[i * 17 + r, j * 16 + c] = a[i, j] o b[r, c], the modular
    pointwise product in numpy.  "u32s" takes the one-word-per-lane instance."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    a, b = rand(p, 16, 16, 41), rand(p, 17, 16, 42)
    ga, gb = M.from_rns(p, a, True), M.from_rns(p, b, True)
    with ran.launches() as seen:
        out = ga.tensor(gb)
    assert seen.blocks_of("tensor_kernel<W, ") == [folded_blocks(272 * 256)] and len(seen) == 1, seen.records
    L, n = a.shape[2:]
    want = mulmod(a[:, None, :, None], b[None, :, None, :], q.reshape(1, 1, 1, 1, L, 1)).reshape(272, 256, L, n)
    assert out.size() == (272, 256) and out.is_ntt
    assert np.array_equal(out.to_rns(), want)


# ---------------------------------------------------------------------------------------------------
# 5. mul_gadget / gadget_mul: one limb vector per (y, z), the index in 32 bits
# ---------------------------------------------------------------------------------------------------
def gadget_weights(p):
    """w[l][e] = (2^base)^e mod q_l: the non-zero constants of g (plainref.gadget's entries, asserted below)"""
    base, dpt = p.base_bits(), PR.digits_per_tower(p.moduli(), p.base_bits())
    return np.array([[pow(2, e * base, int(q)) for e in range(dpt)] for q in p.moduli()], dtype=np.uint64), dpt


# lhs rows x d: vectors = rows * d * k * L with k = 2 L
GADGET_SHAPES = {"u32": (257, 128), "u64": (257, 128), "u32x3": (61, 60), "u32s": (257, 128)}


@pytest.mark.parametrize("name", ["u32", "u64", "u32x3", "u32s"])
def test_mul_gadget_folds_past_65535_limb_vectors(gpu, oracle, name):
    """out = addend - lhs * G_d with the addend apart (every limb vector visited: rows * d k * L of them, above 65535) and then
    out -= lhs * G_d with the addend aliasing out (only the vectors G makes non-zero: rows * d k, still above 65535 on the
    one-limb rings).  Entry (i, (j, t, e)) is lhs[i, j] * 2^(e base) in limb t and 0 elsewhere.  "u32s": N % 4 != 0, the
    one-word-per-lane instance; the others the 16-byte one."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    w, dpt = gadget_weights(p)
    L, n = p.crt_depth(), p.ring_dimension()
    rows, d = GADGET_SHAPES[name]
    k = dpt * L
    g = PR.gadget(2, p.moduli(), p.base_bits(), n)
    assert g.shape[1] == 2 * k and all(int(g[1, k + t * dpt + e, t, 0]) == int(w[t, e]) for t in range(L) for e in range(dpt))
    lhs, ad = rand(p, rows, d, 51), rand(p, rows, d * k, 52)
    prod = np.zeros((rows, d, L, dpt, L, n), dtype=np.uint64)  # [i, j, t, e, l, :]
    for t in range(L):
        for e in range(dpt):
            prod[:, :, t, e, t, :] = mulmod(lhs[:, :, t, :], w[t, e].reshape(1, 1, 1), q[:, :, t, :])
    prod = prod.reshape(rows, d * k, L, n)
    glhs, gad = M.from_rns(p, lhs, True), M.from_rns(p, ad, True)
    vn = "1" if name == "u32s" else "VN"
    with ran.launches() as seen:
        out = glhs.mul_gadget(addend=gad, negate=True)
    assert seen.blocks_of(f"mul_gadget_kernel<W, {vn}>") == [folded_blocks(rows * d * k * L)] and len(seen) == 1, seen.records
    assert np.array_equal(out.to_rns(), submod(ad, prod, q))
    if L == 1:
        with ran.launches() as seen:
            glhs.mul_gadget(addend=gad, negate=True, out=gad)
        assert seen.blocks_of(f"mul_gadget_kernel<W, {vn}>") == [folded_blocks(rows * d * k)] and len(seen) == 1, seen.records
        assert np.array_equal(gad.to_rns(), submod(ad, prod, q))
    assert np.array_equal(glhs.to_rns(), lhs)


@pytest.mark.parametrize("name", ["u32", "u64", "u32x3", "u32s"])
def test_gadget_mul_folds_past_65535_limb_vectors(gpu, oracle, name):
    """out = addend + G_d * rhs for rhs (d k) x c: limb l of entry (j, col) is sum_e 2^(e base) * limb l of row j k + l dpt + e.
    d * c * L limb vectors, above 65535; then the same into an addend that aliases nothing but is negated, in COEFF."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    w, dpt = gadget_weights(p)
    L, n = p.crt_depth(), p.ring_dimension()
    d, c = (257, 256) if L == 1 else (150, 150)
    k = dpt * L
    rhs, ad = rand(p, d * k, c, 61), rand(p, d, c, 62)
    want = np.zeros((d, c, L, n), dtype=np.uint64)
    r4 = rhs.reshape(d, L, dpt, c, L, n)  # [j, t, e, col, l, :]
    for l in range(L):
        for e in range(dpt):
            want[:, :, l, :] = addmod(want[:, :, l, :], mulmod(r4[:, l, e, :, l, :], w[l, e].reshape(1, 1, 1), q[:, :, l, :]), q[:, :, l, :])
    vn = "1" if name == "u32s" else "VN"
    for fmt, negate in ((True, False), (False, True)):
        grhs, gad = M.from_rns(p, rhs, fmt), M.from_rns(p, ad, fmt)
        with ran.launches() as seen:
            out = M.gadget_mul(grhs, addend=gad, negate=negate)
        assert seen.blocks_of(f"gadget_mul_kernel<W, {vn}>") == [folded_blocks(d * c * L)] and len(seen) == 1, seen.records
        assert out.is_ntt == fmt
        assert np.array_equal(out.to_rns(), (submod if negate else addmod)(ad, want, q))


# ---------------------------------------------------------------------------------------------------
# 6. the LargeScalarMul gate: the constant kernel's units over (y, z), the product kernel's row groups over z
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u32x2", "u64x2"])
def test_gadget_const_folds_past_65535_units(gpu, oracle, name):
    """lhs * G^-1(G o C) for a constant: one workgroup per (block row, tower, limb), the index decoded by L * L in 32 bits, so
    two limbs.  129 x (128 k) with k = 2 * 2: 16512 block rows, 66048 units.  The reference is gadget_scalar_model.mul_const in
    Python integers; the addend aliases nothing here, the second call accumulates into its own output."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    L, dpt = 2, 2
    k, rows, d = dpt * L, 129, 128
    units = rows * d * L * L
    const = (1 << 40) + 12345
    lhs, ad = rand(p, rows, d * k, 71), rand(p, rows, d * k, 72)
    want = GSM.mul_const(lhs, const, p.moduli(), p.base_bits(), dpt)
    glhs, gad = M.from_rns(p, lhs, True), M.from_rns(p, ad, True)
    with ran.launches() as seen:
        out = M.large_scalar_mul_many([glhs], const)[0]
        got = M.large_scalar_mul_many([glhs], const, addends=[gad], negate=True)[0]
    kernel = "gadget_const_kernel<W, VN, 2>"
    assert seen.blocks_of(kernel) == [folded_blocks(units)] * 2, seen.records
    assert np.array_equal(out.to_rns(), want)
    assert np.array_equal(got.to_rns(), submod(ad, want, q))


@pytest.mark.parametrize("name", ["u32x2", "u64x2"])
def test_gadget_scalar_row_groups_with_a_ragged_last_group(gpu, oracle, name):
    """lhs * G^-1(G o c) for a ring element: grid (1, towers * L, groups) with groups = min(block rows, 4096 / (gx gy)) = 1024 at
    first, rows_per_group = ceil(2500 / 1024) = 3, then groups = ceil(2500 / 3) = 834: the last group holds one row.  Every word
    against the reference's own sequence restated on the CPU, and the entries of the first row, of row 2499 - the ragged group -
    and of one inside against gadget_scalar_model in Python integers."""
    p = ring(gpu, oracle, name)
    M = gpu.GpuDCRTPolyMatrix
    L, dpt, n = 2, 2, p.ring_dimension()
    k, rows, d = dpt * L, 50, 50
    block_rows = rows * d
    groups = min(block_rows, max(1, 4096 // (1 * L * L)))
    rpg = -(-block_rows // groups)
    groups = -(-block_rows // rpg)
    assert (rpg, groups, block_rows - (groups - 1) * rpg) == (3, 834, 1)
    moduli = p.moduli()
    lhs, c_coeff = rand(p, rows, d * k, 81), rand(p, 1, 1, 82)
    c_eval = oracle.matrix_ntt(c_coeff, moduli)
    glhs, gc = M.from_rns(p, lhs, True), M.from_rns(p, c_eval, True)
    with ran.launches() as seen:
        out = M.large_scalar_mul_many([glhs], gc)[0]
    assert seen.blocks_of("gadget_scalar_kernel<W, VN, 2>") == [L * L * groups], seen.records
    got = out.to_rns()
    assert np.array_equal(got, GSM.restatement(oracle, lhs, c_eval, moduli, p.base_bits())[0])
    entries = [(0, 0), (rows - 1, d * k - 1), (rows - 1, d * k - k), (rows // 2, 7)]
    plain = GSM.mul_scalar_entries(lhs, c_coeff[0, 0], moduli, p.base_bits(), dpt, entries, list(range(n)))
    for (i, col, l), vals in plain.items():
        assert [int(v) for v in got[i, col, l]] == [int(v) for v in vals], (i, col, l)


# ---------------------------------------------------------------------------------------------------
# 10. the product's refusal edge: row tiles x column tiles <= 65535 in one grid extent
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u32", "u64"])
def test_product_grid_at_its_last_tile_and_one_past_it(gpu, oracle, name):
    """(1 x 1) * (1 x cols).  32-bit words, n = 4: one row and 8 or more columns take matmul_kernel<u32,1,8,4> (launch_matmul,
    arith.hip; the operand is in words, so the packed skinny kernel declines).  64-bit words, n = 2, L = 1: stacked_tile
    (matmul_tile.h) wants 131072 lanes of tiled work for the 1 x 4 and 2 x 2 tiles and 65535..65536 columns give at most 65536,
    so the tile is 1 x 1.  cols = 65535 * tc is accepted and right at every column; one more column - one more tile - is
    refused with "matrix too large", nothing is launched and `out` keeps its words and its tag."""
    p = ring(gpu, oracle, name)
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    tc = 8 if name == "u32" else 1
    cols = Y_MAX * tc
    a, b = rand(p, 1, 1, 91), rand(p, 1, cols + 1, 92)
    ga, gb = M.from_rns(p, a, True), M.from_rns(p, b[:, :cols], True)
    with ran.launches() as seen:
        out = ga * gb
    label = p.ctx().last_kernel()
    m = re.match(r"matmul_kernel<u(32|64),(\d+),(\d+),(\d+)", label)
    assert m and (int(m.group(2)), int(m.group(3))) == (1, tc), label
    assert -(-cols // tc) == Y_MAX
    # tile_grid (matmul_tile.h): x = slot chunks (n / SV lanes in one workgroup here), y = row tiles x column tiles, z = limbs
    assert seen.blocks_of("matmul_kernel<W, TR, TC, SV") == [1 * Y_MAX * 1] and len(seen) == 1, seen.records
    assert np.array_equal(out.to_rns(), mulmod(a, b[:, :cols], q))
    # one more tile
    gb1 = M.from_rns(p, b, True)
    sentinel = rand(p, 1, cols + 1, 93)
    keep = M.from_rns(p, sentinel, False)  # COEFF: an accepted product would tag it EVAL
    with ran.launches() as seen:
        rc = lib().gpu_matrix_mul(keep.raw, ga.raw, gb1.raw)
    assert rc != 0 and "matrix too large" in last_error()
    assert list(seen) == [], seen.records
    assert np.array_equal(keep.to_rns(), sentinel)  # read as COEFF: the tag is what it was


# ---------------------------------------------------------------------------------------------------
# window refusals: gpu_matrix_copy_block / gpu_matrix_add_block / gpu_matrix_sample_distribution_columns
# ---------------------------------------------------------------------------------------------------
def _window_cases():
    """(dst_row, dst_col, src_row, src_col, rows, cols, needle) on a 5 x 6 COEFF destination and a 4 x 7 EVAL source: each of the
    four offsets at SIZE_MAX, at SIZE_MAX - count + 1 (offset + count wraps to exactly 0) and one past its extent with an empty
    block"""
    rows, cols = 2, 3
    extent = {"dst_row": 5, "dst_col": 6, "src_row": 4, "src_col": 7}
    out = []
    for pos, name in enumerate(extent):
        count = rows if name.endswith("row") else cols
        for off, r, c in ((SIZE_MAX, rows, cols), (SIZE_MAX - count + 1, rows, cols), (extent[name] + 1, 0 if name.endswith("row") else rows,
                                                                                   cols if name.endswith("row") else 0)):
            args = [0, 0, 0, 0, r, c]
            args[pos] = off
            out.append(tuple(args) + ("destination block out of bounds" if name.startswith("dst") else "source block out of bounds",))
    return out


@pytest.mark.parametrize("entry", ["gpu_matrix_copy_block", "gpu_matrix_add_block"])
def test_block_windows_that_wrap_are_refused(gpu, oracle, entry):
    """every refused call returns non-zero with the entry's message, launches nothing and leaves `out` as it was: its words, and
    its COEFF tag (the source is EVAL; to_rns reads in COEFF and would come back transformed or be refused after a retag)"""
    p = ring(gpu, oracle, "u32")
    M = gpu.GpuDCRTPolyMatrix
    fn = getattr(lib(), entry)
    d_np, s_np = rand(p, 5, 6, 101), rand(p, 4, 7, 102)
    out, src = M.from_rns(p, d_np, False), M.from_rns(p, s_np, True)
    cases = _window_cases()
    assert len(cases) == 12
    for dr, dc, sr, sc, r, c, needle in cases:
        with ran.launches() as seen:
            rc = fn(out.raw, src.raw, dr, dc, sr, sc, r, c)
        assert rc != 0, (entry, dr, dc, sr, sc, r, c)
        assert last_error() == f"{entry}: {needle}", (last_error(), dr, dc, sr, sc, r, c)
        assert list(seen) == [], seen.records
        assert np.array_equal(out.to_rns(), d_np)  # read as COEFF: a retagged matrix would come back transformed
    assert np.array_equal(src.to_rns(), s_np)


def test_add_block_too_wide_is_refused_before_the_retag(gpu, oracle):
    """cols = 65536 inside both windows: blockIdx.y cannot hold one block row.  Refused with "block too wide", before the
    destination's tag is touched; copy_block takes the same window (a runtime copy has no such limit)."""
    p = ring(gpu, oracle, "u32")
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    d_np, s_np = rand(p, 1, Y_MAX + 1, 111), rand(p, 1, Y_MAX + 1, 112)
    out, src = M.from_rns(p, d_np, False), M.from_rns(p, s_np, True)
    with ran.launches() as seen:
        rc = lib().gpu_matrix_add_block(out.raw, src.raw, 0, 0, 0, 0, 1, Y_MAX + 1)
    assert rc != 0 and last_error() == "gpu_matrix_add_block: block too wide"
    assert list(seen) == [], seen.records
    assert np.array_equal(out.to_rns(), d_np)
    # the widest block that fits, one column short, is added: one launch of 65535 entries
    out2 = M.from_rns(p, d_np, True)
    with ran.launches() as seen:
        out2.add_block_from(src, 0, 1, 0, 0, 1, Y_MAX)
    assert seen.blocks_of("block_rect_kernel<uint32_t, true>") == [Y_MAX], seen.records
    want = d_np.copy()
    want[:, 1:] = addmod(d_np[:, 1:], s_np[:, :Y_MAX], q)
    assert np.array_equal(out2.to_rns(), want)
    out.copy_block_from(src, 0, 0, 0, 0, 1, Y_MAX + 1)
    out.is_ntt = True  # the reference's quirk: a successful copy retags the destination with the source's format
    assert np.array_equal(out.to_rns(), s_np)


@pytest.mark.parametrize("entry", ["gpu_matrix_copy_block", "gpu_matrix_add_block"])
def test_block_windows_at_their_accepted_extremes(gpu, oracle, entry):
    """offset = extent with an empty block in every position, and the full window"""
    p = ring(gpu, oracle, "u32")
    M, q = gpu.GpuDCRTPolyMatrix, qcol(p)
    fn = getattr(lib(), entry)
    d_np, s_np = rand(p, 5, 6, 121), rand(p, 4, 7, 122)
    out, src = M.from_rns(p, d_np, True), M.from_rns(p, s_np, True)
    for args in ((5, 0, 0, 0, 0, 3), (0, 6, 0, 0, 2, 0), (0, 0, 4, 0, 0, 3), (0, 0, 0, 7, 2, 0), (5, 6, 4, 7, 0, 0)):
        with ran.launches() as seen:
            assert fn(out.raw, src.raw, *args) == 0, (args, last_error())
        assert list(seen) == [], seen.records
    assert np.array_equal(out.to_rns(), d_np)
    assert fn(out.raw, src.raw, 1, 0, 0, 1, 4, 6) == 0, last_error()  # all of the source's rows, all of the destination's columns
    want = d_np.copy()
    want[1:5] = addmod(d_np[1:5], s_np[:, 1:7], q) if entry.endswith("add_block") else s_np[:, 1:7]
    assert np.array_equal(out.to_rns(), want)


def test_sample_columns_window_that_wraps_is_refused(gpu, oracle):
    """col_offset = SIZE_MAX and SIZE_MAX - cols + 1 against a 10-column conceptual matrix: col_offset + cols wraps below 10"""
    p = ring(gpu, oracle, "u32")
    M = gpu.GpuDCRTPolyMatrix
    d_np = rand(p, 2, 3, 131)
    out = M.from_rns(p, d_np, False)
    seed = gpu.GpuRngSeed.from_bytes(bytes(range(32)))
    uni = gpu.DistType.FinRingDist().as_ffi()
    for off in (SIZE_MAX, SIZE_MAX - 3 + 1, 8, 11):
        with ran.launches() as seen:
            rc = lib().gpu_matrix_sample_distribution_columns(out.raw, uni, 0.0, seed, 10, off)
        assert rc != 0 and last_error() == "gpu_matrix_sample_distribution_columns: column window out of range", (off, last_error())
        assert list(seen) == [], seen.records
        assert np.array_equal(out.to_rns(), d_np)
    # the last window that fits is the plain sampler's columns 7..9
    got = M.sample_distribution_columns(p, 2, 10, 7, 3, uni, 0.0, seed)
    whole = M.sample_distribution(p, 2, 10, uni, 0.0, seed)
    assert np.array_equal(got.to_rns(), whole.to_rns()[:, 7:])


# ---------------------------------------------------------------------------------------------------
# 7 and 9. the heavy entries: the target builders' combine (row_targets.h) and the online lookups, one output polynomial
# or tile per (y, z).  Two references together: the same entry over two halves of the rows or slots, each under the fold,
# written through row views into a second parent and compared on the device; and the feature's own plain reference - the
# oracle's samples of U, Python integers - for the outputs at entry 0, 65534, 65535, 65536 and the last one.
# ---------------------------------------------------------------------------------------------------
KEY = bytes((11 * i + 6) & 0xFF for i in range(32))
# 64-bit words at n = 16 here: the builders multiply 2d (or d) rows by T * c columns first, and at n = 2 with one limb the
# product's own tile rule (stacked_tile, matmul_tile.h) stays at 1 x 1 tiles, more than 65535 of them for any T d c > 65535
TARGET_RINGS = {"u32x2": (4, 2, 24, 12), "u64n16": (16, 2, 51, 26)}
ROW_GROUP_CAP = 1 << 30  # kRowGroupBytes, row_targets.h


def rows_per_group(T, row_bytes, cap=ROW_GROUP_CAP):
    """row_targets.h's rule: the rows (or slots) of one group"""
    return min(T, 1 << 20, max(1, cap // row_bytes))


def target_ring(gpu, oracle, name):
    n, depth, bits, base = TARGET_RINGS.get(name) or RINGS[name]
    return make_params(gpu, oracle, n, depth, bits, base)


def edge_entries(entries):
    """entry 0, the last one, and the three on either side of every fold: 65534, 65535, 65536 and likewise at every further
    multiple of 65535 below the count (a grid of three and more layers)"""
    assert entries > Y_MAX + 1
    out = {0, entries - 1}
    for m in range(Y_MAX, entries, Y_MAX):
        out |= {m - 1, m, min(m + 1, entries - 1)}
    return sorted(out)


def tile_of(entry, per_slot, col_tiles):
    """the lookup kernels' decode of an entry: (slot, row tile)"""
    s, rest = divmod(entry, per_slot)
    return s, rest // col_tiles


def digit_rows(gpu, oracle, p, tag, d, m, chunk, slots):
    """V = G^-1(U[:, chunk]) at `slots`, (m, c, L, len(slots)): U the d x m uniform matrix under hash_seed_for_matrix(KEY, tag)"""
    from test_gpu_ggh15_lookup import digits_eval

    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tag), full_ncol=m, col_offset=chunk[0])
    return digits_eval(u, moduli, base, PR.digits_per_tower(moduli, base), slots)


def combine_blocks(seen, kernel, entries):
    """one launch of the combine kernel over all `entries`, folded - not one per row group"""
    assert seen.blocks_of(kernel) == [folded_blocks(entries)], seen.records


@pytest.mark.parametrize("name", list(TARGET_RINGS))
def test_lut_targets_combine_folds_past_65535_polynomials(gpu, oracle, name):
    """T = 150 rows of d x c = 11 x 40 targets at column 3 of m = 44: 66000 output polynomials in one row group (the digit
    scratch is m c polynomials per row, far below the 1 GiB cap)."""
    from mxx_amd.matrix import IndexedTags
    from test_gpu_lut_targets import gy_block

    p = target_ring(gpu, oracle, name)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), PR.digits_per_tower(moduli, base)
    k, d, T, chunk = L * dpt, 11, 150, (3, 40)
    m, c, level = d * k, chunk[1], L - 1
    entries = T * d * c
    poly_bytes = L * n * p.ctx().word_bytes()
    assert rows_per_group(T, m * c * poly_bytes) == T
    ws_np = [rand(p, d, m, 201 + i) for i in range(4)]
    ws = [M.from_rns(p, w, True) for w in ws_np]
    Q = 1
    for q in moduli:
        Q *= int(q)
    ys = [(t * 0x9E3779B97F4A7C15 + 5) % (Q + 7) for t in range(T)]
    idxs = [(t * 0xD1B54A32D192ED03 + 1) % (1 << 64) for t in range(T)]
    tags = IndexedTags(b"fold_lut_", 40, T, decimal=True)
    raw = lib().gpupoly_matrix_lut_targets
    u64p = C.POINTER(C.c_uint64)

    def run(parent, t0, t1):
        from mxx_amd import _ffi
        from mxx_amd.matrix import hash_tags_arg

        views = [parent.row_view(t * d, (t + 1) * d) for t in range(t0, t1)]
        arg, keep, count = hash_tags_arg(KEY, tags[t0:t1])
        y_arr, wpy = M._int_rows(ys[t0:t1])
        i_arr = np.array(idxs[t0:t1], dtype=np.uint64)
        with ran.launches() as seen:
            rc = raw(M._raw_array(views), count, *[w.raw for w in ws], chunk[0], base, y_arr.ctypes.data_as(u64p), wpy, i_arr.ctypes.data_as(u64p),
                     C.byref(arg))
        _ffi.check_status(rc, "gpupoly_matrix_lut_targets")
        del keep
        return seen

    whole, halves = M(p, T * d, c, level, True), M(p, T * d, c, level, True)
    combine_blocks(run(whole, 0, T), "lut_combine_kernel<W, VN, 2>", entries)
    for t0, t1 in ((0, T // 2), (T // 2, T)):
        assert run(halves, t0, t1).blocks_of("lut_combine_kernel<W, VN, 2>") == [(t1 - t0) * d * c]
    assert whole == halves
    slots = list(range(n)) if n <= 4 else [0, n // 2 - 1, n - 1]
    got = whole.to_rns()
    for t, i in sorted({(e // (d * c), e % (d * c) // c) for e in edge_entries(entries)}):  # whole rows of c polynomials
        v = digit_rows(gpu, oracle, p, tags[t], d, m, chunk, slots)
        idx_col = np.asarray([idxs[t] % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
        q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
        v_idx = ((v.astype(object) * idx_col) % q_col).astype(np.uint64)
        gy = gy_block(moduli, n, base, dpt, ys[t], d, chunk)[..., slots]
        want = PR.slot_mul_sum(ws_np[0][i:i + 1, chunk[0]:chunk[0] + c][..., slots], [w[i:i + 1][..., slots] for w in ws_np[1:]], [gy, v, v_idx],
                               moduli, False)
        assert np.array_equal(got[t * d + i:t * d + i + 1][..., slots], want), (t, i)


@pytest.mark.parametrize("name", list(TARGET_RINGS))
def test_lwe_targets_combine_folds_past_65535_polynomials(gpu, oracle, name):
    """the same shape through gpupoly_matrix_lwe_targets: A_lt[:, chunk] - G[:, chunk] o y_t - (A_z - G o x_t) G^-1(U_t[:, chunk])"""
    from mxx_amd.matrix import IndexedTags
    from test_gpu_lwe_targets import gadget_slots, minus, times_constant

    p = target_ring(gpu, oracle, name)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), PR.digits_per_tower(moduli, base)
    k, d, T, chunk = L * dpt, 11, 150, (3, 40)
    m, c, level = d * k, chunk[1], L - 1
    entries = T * d * c
    assert rows_per_group(T, m * c * L * n * p.ctx().word_bytes()) == T
    az_np, alt_np = rand(p, d, m, 211), rand(p, d, m, 212)
    a_z, a_lt = M.from_rns(p, az_np, True), M.from_rns(p, alt_np, True)
    Q = 1
    for q in moduli:
        Q *= int(q)
    ys = [(t * 0x9E3779B97F4A7C15 + 9) % (Q + 7) for t in range(T)]
    xs = [(t * 0xD1B54A32D192ED03 + 3) % (1 << 64) for t in range(T)]
    tags = IndexedTags(b"fold_lwe_", 7, T)
    raw = lib().gpupoly_matrix_lwe_targets
    u64p = C.POINTER(C.c_uint64)

    def run(parent, t0, t1):
        from mxx_amd import _ffi
        from mxx_amd.matrix import hash_tags_arg

        views = [parent.row_view(t * d, (t + 1) * d) for t in range(t0, t1)]
        arg, keep, count = hash_tags_arg(KEY, tags[t0:t1])
        y_arr, wpy = M._int_rows(ys[t0:t1])
        x_arr = np.array(xs[t0:t1], dtype=np.uint64)
        with ran.launches() as seen:
            rc = raw(M._raw_array(views), count, a_z.raw, a_lt.raw, chunk[0], base, y_arr.ctypes.data_as(u64p), wpy, x_arr.ctypes.data_as(u64p),
                     C.byref(arg))
        _ffi.check_status(rc, "gpupoly_matrix_lwe_targets")
        del keep
        return seen

    whole, halves = M(p, T * d, c, level, True), M(p, T * d, c, level, True)
    combine_blocks(run(whole, 0, T), "lwe_combine_kernel<W, VN, 2>", entries)
    for t0, t1 in ((0, T // 2), (T // 2, T)):
        assert run(halves, t0, t1).blocks_of("lwe_combine_kernel<W, VN, 2>") == [(t1 - t0) * d * c]
    assert whole == halves
    slots = list(range(n)) if n <= 4 else [0, n // 2 - 1, n - 1]
    got = whole.to_rns()
    G = gadget_slots(moduli, base, n, d)
    cols = slice(chunk[0], chunk[0] + c)
    for t, i in sorted({(e // (d * c), e % (d * c) // c) for e in edge_entries(entries)}):
        v = digit_rows(gpu, oracle, p, tags[t], d, m, chunk, slots)
        ext = minus(az_np[i:i + 1], times_constant(G[i:i + 1], xs[t], moduli), moduli)[..., slots]  # A_z - G o x
        addend = minus(alt_np[i:i + 1, cols], times_constant(G[i:i + 1, cols], ys[t], moduli), moduli)[..., slots]
        want = PR.slot_mul_sum(addend, [ext], [v], moduli, True)
        assert np.array_equal(got[t * d + i:t * d + i + 1][..., slots], want), (t, i)


@pytest.mark.parametrize("name", ["u32x2", "u64"])
def test_lwe_lookup_folds_past_65535_tiles(gpu, oracle, name):
    """S = 656 slots of r x c = 20 x 40 outputs at column 3 of m_g = 44, w = 2: row tiles of 2 and column tiles of 4 give 100
    tiles per slot, 65600 in one group (a slot's digit scratch is m_g c polynomials; the budget switch is unset).  Tiles
    65534 .. 65536 and the last one lie in the last slot; slot 0 and that one are held to the plain reference whole."""
    from mxx_amd.matrix import IndexedTags

    p = target_ring(gpu, oracle, name)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), PR.digits_per_tower(moduli, base)
    k = L * dpt
    S, r, w, chunk = 656, 20, 2, (3, 40)
    d = 44 // k
    m_g, c, level = d * k, chunk[1], L - 1
    assert m_g == 44
    per_slot = -(-r // 2) * -(-c // 4)
    entries = S * per_slot
    import os

    assert "MXX_HIP_LWE_LOOKUP_BUDGET" not in os.environ
    assert rows_per_group(S, m_g * c * L * n * p.ctx().word_bytes()) == S
    cb_np, kh_np, cz_np = rand(p, S * r, w, 221), rand(p, S * w, c, 222), rand(p, S * r, m_g, 223)
    cb_all, kh_all, cz_all = M.from_rns(p, cb_np, True), M.from_rns(p, kh_np, True), M.from_rns(p, cz_np, True)
    cbs = [cb_all.row_view(s * r, (s + 1) * r) for s in range(S)]
    khs = [kh_all.row_view(s * w, (s + 1) * w) for s in range(S)]
    czs = [cz_all.row_view(s * r, (s + 1) * r) for s in range(S)]
    tags = IndexedTags(b"fold_slot_", 1000, S, decimal=True)
    kernel = "lwe_lookup_kernel<W, VN, 2, 4>"

    def run(parent, s0, s1):
        outs = [parent.row_view(s * r, (s + 1) * r) for s in range(s0, s1)]
        with ran.launches() as seen:
            M.lwe_lookup(outs, cbs[s0:s1], khs[s0:s1], czs[s0:s1], chunk[0], KEY, tags[s0:s1])
        return seen

    whole, halves = M(p, S * r, c, level, True), M(p, S * r, c, level, True)
    combine_blocks(run(whole, 0, S), kernel, entries)
    for s0, s1 in ((0, S // 2), (S // 2, S)):
        assert run(halves, s0, s1).blocks_of(kernel) == [(s1 - s0) * per_slot]
    assert whole == halves
    got = whole.to_rns()
    slots = list(range(n))
    for s in sorted({e // per_slot for e in edge_entries(entries)}):
        v = digit_rows(gpu, oracle, p, tags[s], d, m_g, chunk, slots)
        want = PR.slot_mul_sum(None, [cb_np[s * r:(s + 1) * r], cz_np[s * r:(s + 1) * r]], [kh_np[s * w:(s + 1) * w], v], moduli, False)
        assert np.array_equal(got[s * r:(s + 1) * r], want), s


@pytest.mark.parametrize("name", ["u32x2", "u64"])
def test_ggh15_lookup_folds_past_65535_tiles(gpu, oracle, name):
    """the same slots through gpupoly_matrix_ggh15_lookup: S = 656, r x c = 20 x 40 at column 3 of m_g = 44, w = m_g + 2 d, 100
    tiles per slot, one group (a slot's scratch is its digits and its rows of the left factor).  The plain reference
    (test_gpu_ggh15_lookup.combine_want on the oracle's digits) is taken for the row tiles that hold tiles 0, 65534 .. 65536
    and the last one by the kernel's decode (slot = entry / 100, row tile = entry % 100 / 10): rows 0..1 of slot 0, rows
    6..7 and 18..19 of slot 655, every column."""
    import os

    from mxx_amd import _ffi
    from mxx_amd.matrix import IndexedTags, hash_tags_arg
    from test_gpu_ggh15_lookup import combine_want

    p = target_ring(gpu, oracle, name)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), PR.digits_per_tower(moduli, base)
    k = L * dpt
    S, r, chunk = 656, 20, (3, 40)
    d = 44 // k
    m_g, c, level = d * k, chunk[1], L - 1
    w = m_g + 2 * d
    per_slot = -(-r // 2) * -(-c // 4)
    entries = S * per_slot
    poly_bytes = L * n * p.ctx().word_bytes()
    assert "MXX_HIP_GGH15_LOOKUP_BUDGET" not in os.environ
    assert rows_per_group(S, (m_g * c + r * (m_g + w)) * poly_bytes) == S
    mids_np = [rand(p, S * r, m_g, 231 + j) for j in range(5)] + [rand(p, S * r, w, 236)]
    luts_np, xs_np = rand(p, S * w, c, 237), rand(p, S, 1, 238)
    mids = [M.from_rns(p, a, True) for a in mids_np]
    luts_all, xs_all = M.from_rns(p, luts_np, True), M.from_rns(p, xs_np, True)
    luts = [luts_all.row_view(s * w, (s + 1) * w) for s in range(S)]
    xs = [xs_all.row_view(s, s + 1) for s in range(S)]
    Q = 1
    for q in moduli:
        Q *= int(q)
    ys = [(s * 0x9E3779B97F4A7C15 + 11) % (Q + 7) for s in range(S)]
    tags = IndexedTags(b"fold_ggh15_", 5, S)
    kernel = "ggh15_lookup_kernel<W, VN, 2, 4>"
    u64p = C.POINTER(C.c_uint64)

    def run(parent, s0, s1):
        outs = [parent.row_view(s * r, (s + 1) * r) for s in range(s0, s1)]
        part = [m.row_view(s0 * r, s1 * r) for m in mids]
        arg, keep, count = hash_tags_arg(KEY, tags[s0:s1])
        y_arr, wpy = M._int_rows(ys[s0:s1])
        with ran.launches() as seen:
            rc = lib().gpupoly_matrix_ggh15_lookup(M._raw_array(outs), count, *[m.raw for m in part], M._raw_array(luts[s0:s1]),
                                                   M._raw_array(xs[s0:s1]), chunk[0], base, y_arr.ctypes.data_as(u64p), wpy, C.byref(arg))
        _ffi.check_status(rc, "gpupoly_matrix_ggh15_lookup")
        del keep
        return seen

    whole, halves = M(p, S * r, c, level, True), M(p, S * r, c, level, True)
    combine_blocks(run(whole, 0, S), kernel, entries)
    for s0, s1 in ((0, S // 2), (S // 2, S)):
        assert run(halves, s0, s1).blocks_of(kernel) == [(s1 - s0) * per_slot]
    assert whole == halves
    got = whole.to_rns()
    slots = list(range(n))
    pairs = sorted({tile_of(e, per_slot, -(-c // 4)) for e in edge_entries(entries)})
    assert pairs == [(0, 0), (S - 1, 3), (S - 1, 9)]
    digits_of = {}
    for s, rt in pairs:
        if s not in digits_of:
            digits_of[s] = digit_rows(gpu, oracle, p, tags[s], d, m_g, chunk, slots)
        v, r0 = digits_of[s], 2 * rt
        rows = slice(s * r + r0, s * r + r0 + 2)
        want = combine_want([m[rows] for m in mids_np], [luts_np[s * w:(s + 1) * w]], [xs_np[s, 0]], v, moduli, n, base, dpt, d, chunk, [ys[s]], 2, slots)[0]
        assert np.array_equal(got[rows], want), (s, r0)


@pytest.mark.parametrize("name", ["u32x2", "u64"])
def test_slot_transfer_eval_folds_both_kernels(gpu, oracle, name):
    """S = 656 outputs of r x c = 20 x 40 at column 3 of m_g = 44, w0 = w1 = 2, two terms each (a plain one and a shifted, scaled
    one whose operands are the next output's): the main kernel has 100 tiles per output, 65600, and the pre-pass one entry
    per four left-factor polynomials, ceil(20 * 44 / 4) + ceil(20 * 2 / 4) = 230 per output, 150880 - three layers, on a grid
    whose x extent is the limbs.  One group.  The plain reference (test_gpu_slot_transfer_eval.plain_eval on the oracle's
    digits) is taken for every pair of output rows that an edge entry of either kernel writes or feeds, by the kernels'
    decodes: the main kernel's tiles 0, 65534 .. 65536 and the last (rows 0..1 of output 0, rows 6..7 and 18..19 of output
    655), and the pre-pass's entries 0, 65534 .. 65536, 131069 .. 131071 and the last (output = entry / 230; tile < 220: four
    polynomials of the r x m_g left factor from 4 * tile, else of the r x w1 one; the polynomial's row is the output row it
    feeds: rows 0..1 of output 0, 18..19 of outputs 284, 569 and 655)."""
    import os

    from mxx_amd.matrix import IndexedTags
    from test_gpu_slot_transfer_eval import plain_eval

    p = target_ring(gpu, oracle, name)
    M, moduli, n, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), PR.digits_per_tower(moduli, base)
    k = L * dpt
    S, r, chunk, w0, w1 = 656, 20, (3, 40), 2, 2
    d = 44 // k
    m_g, c, level = d * k, chunk[1], L - 1
    per_slot = -(-r // 2) * -(-c // 4)
    pre_per_slot = -(-r * m_g // 4) + -(-r * w1 // 4)
    assert (per_slot, pre_per_slot) == (100, 230)
    poly_bytes = L * n * p.ctx().word_bytes()
    assert "MXX_HIP_SLOT_EVAL_BUDGET" not in os.environ
    assert rows_per_group(S, (m_g * c + r * m_g + r * w1) * poly_bytes) == S
    b0_np, pg_np, p1_np = rand(p, r, w0, 241), rand(p, S * w0, c, 242), rand(p, S * w1, c, 243)
    cin_np, mid_np = rand(p, S * r, m_g, 244), rand(p, S * r, w1, 245)
    c_b0, pg_all, p1_all = M.from_rns(p, b0_np, True), M.from_rns(p, pg_np, True), M.from_rns(p, p1_np, True)
    cin_all, mid_all = M.from_rns(p, cin_np, True), M.from_rns(p, mid_np, True)
    pgs = [pg_all.row_view(s * w0, (s + 1) * w0) for s in range(S)]
    p1s = [p1_all.row_view(s * w1, (s + 1) * w1) for s in range(S)]
    cins = [cin_all.row_view(s * r, (s + 1) * r) for s in range(S)]
    mids = [mid_all.row_view(s * r, (s + 1) * r) for s in range(S)]
    kappas = [3, 1, (1 << 32) - 1]

    def spec(s):
        """(source output, shift, kappa, mu) of output s's two terms"""
        nxt = (s + 1) % S
        return [(s, 0, 1, (s * 0x9E3779B97F4A7C15 + 1) % (1 << 70)), (nxt, 1 + s % (2 * n - 1), kappas[s % 3], (s * 0xD1B54A32D192ED03 + 2) % (1 << 40))]

    terms = [[(cins[src], mids[src], shift, kappa, mu) for src, shift, kappa, mu in spec(s)] for s in range(S)]
    tags = IndexedTags(b"fold_transfer_", 0, S, decimal=True)
    kernel = "slot_eval_kernel<W, VN, 2, 4>"
    pre_kernel = "slot_eval_lhs_kernel<uint64_t, 2, kLhsTile>" if name == "u64" else "slot_eval_lhs_kernel<uint32_t, 4, kLhsTile>"

    def run(parent, s0, s1):
        outs = [parent.row_view(s * r, (s + 1) * r) for s in range(s0, s1)]
        with ran.launches() as seen:
            M.slot_transfer_eval(outs, c_b0, pgs[s0:s1], p1s[s0:s1], terms[s0:s1], chunk[0], KEY, tags[s0:s1])
        return seen

    whole, halves = M(p, S * r, c, level, True), M(p, S * r, c, level, True)
    seen = run(whole, 0, S)
    combine_blocks(seen, kernel, S * per_slot)
    assert seen.blocks_of(pre_kernel) == [folded_blocks(S * pre_per_slot, gx=L)] and fold(S * pre_per_slot)[1] == 3, seen.records
    for s0, s1 in ((0, 250), (250, 500), (500, S)):  # the pre-pass stays under the fold below 284 outputs
        seen = run(halves, s0, s1)
        assert seen.blocks_of(kernel) == [(s1 - s0) * per_slot] and seen.blocks_of(pre_kernel) == [L * (s1 - s0) * pre_per_slot], seen.records
    assert whole == halves
    got = whole.to_rns()
    slots = list(range(n))
    pairs = {tile_of(e, per_slot, -(-c // 4)) for e in edge_entries(S * per_slot)}
    assert pairs == {(0, 0), (S - 1, 3), (S - 1, 9)}
    tiles_a = -(-r * m_g // 4)
    pre = set()
    for e in edge_entries(S * pre_per_slot):
        s, tile = divmod(e, pre_per_slot)
        polys, cols = (r * m_g, m_g) if tile < tiles_a else (r * w1, w1)
        p0 = 4 * (tile if tile < tiles_a else tile - tiles_a)
        pre |= {(s, min(q_, polys - 1) // cols // 2) for q_ in range(p0, p0 + 4)}  # (output, the row tile its row lies in)
    assert pre == {(0, 0), (284, 9), (569, 9), (S - 1, 9)} and fold(S * pre_per_slot) == (Y_MAX, 3)
    digits_of = {}
    for s, rt in sorted(pairs | pre):
        if s not in digits_of:
            digits_of[s] = digit_rows(gpu, oracle, p, tags[s], d, m_g, chunk, slots)
        v, r0 = digits_of[s], 2 * rt
        plain_terms = [(cin_np[src * r + r0:src * r + r0 + 2], mid_np[src * r + r0:src * r + r0 + 2], shift, kappa, mu) for src, shift, kappa, mu in spec(s)]
        want = plain_eval(b0_np[r0:r0 + 2], pg_np[s * w0:(s + 1) * w0], p1_np[s * w1:(s + 1) * w1], v, plain_terms, moduli, n)
        assert np.array_equal(got[s * r + r0:s * r + r0 + 2], want), (s, r0)


# ---------------------------------------------------------------------------------------------------
# 8. the batched preimage's gather and scatter: one polynomial of a group's columns per (y, z)
# ---------------------------------------------------------------------------------------------------
# name -> (limb bits, base bits, columns per request, requests per piece)
PREIMAGE_CASES = {"u32": (24, 6, 1025, 10), "u64": (51, 13, 171, 32)}


@pytest.mark.parametrize("name", list(PREIMAGE_CASES))
def test_preimage_gather_and_scatter_fold(gpu, oracle, name):
    """gpupoly_trapdoor_preimage_many at the smallest ring the segmented samplers take, n = 128, with one limb, four digits
    per tower (the most the G-sampler's lane kernel takes) and d = 1; a group is at most 64 requests.
    32-bit words: 64 requests of 1025 columns make the gather's d * 65600 entries fold (two layers) and the scatter's
    (2 + 4) * 65600 (seven); the pieces are the same requests ten at a time under their own seeds (6 * 10250 entries, one
    layer).  64-bit words: the gather folds only above 65535 target columns, where the call's temporaries, counted from
    preimage_group's allocations at 1 KB per polynomial, come to (6 + 4 + 2 + 1 + 1) * 65600 KB = 0.9 GB beside 0.5 GB of
    outputs and targets - computed, not measured, and past what a test may hold; so 64 requests of 171 columns fold the
    scatter alone (6 * 10944 entries, two layers, 150 MB of temporaries), in pieces of 32 requests.
    The plain reference is the CPU restatement of the whole preimage for the requests that hold, by the kernels' decode
    (row = entry / columns, column = entry % columns), entry 0, the three entries around every fold and the last one of
    either kernel: the first and the last request."""
    from mxx_amd.sampler import seed_source
    from test_gpu_preimage_abi import SIGMA, seed_bytes, trapdoor_and_oracle

    bits, base, width, piece_len = PREIMAGE_CASES[name]
    n, depth, d = 128, 1, 1
    p = make_params(gpu, oracle, n, depth, bits, base)
    assert p.ctx().word_bytes() == (8 if name == "u64" else 4)
    moduli = p.moduli()
    M = gpu.GpuDCRTPolyMatrix
    sampler, td, A, (r, e, a) = trapdoor_and_oracle(gpu, oracle, p, n, base, d, seed_bytes(3))
    R, rows = 64, (p.modulus_digits() + 2) * d
    at = R * width
    assert rows == 6 and rows * at > Y_MAX
    targets_np = [rand(p, d, width, 300 + j) for j in range(R)]
    targets = [M.from_rns(p, t, True) for t in targets_np]
    masters = [seed_bytes(80 + j) for j in range(R)]
    draws = [oracle._seed_from(m, i).tobytes() for m in masters for i in (3, 4, 5)]  # request by request: p2, p1, z
    gather, scatter = "preimage_gather_sub_kernel<W, 16 / sizeof(W)>", "preimage_scatter_kernel<W, 16 / sizeof(W)>"
    with seed_source(draws), ran.launches() as seen:
        got = sampler.preimage_many_abi(p, td, A, targets)
    assert seen.blocks_of(scatter) == [folded_blocks(rows * at)], seen.records
    assert seen.blocks_of(gather) == [folded_blocks(d * at) if name == "u32" else d * at], seen.records
    assert fold(rows * at)[1] == (7 if name == "u32" else 2)
    for j0 in range(0, R, piece_len):
        j1 = min(R, j0 + piece_len)
        assert rows * (j1 - j0) * width <= Y_MAX
        with seed_source(draws[3 * j0:3 * j1]), ran.launches() as seen:
            piece = sampler.preimage_many_abi(p, td, A, targets[j0:j1])
        assert seen.blocks_of(gather) == [d * (j1 - j0) * width] and seen.blocks_of(scatter) == [rows * (j1 - j0) * width], seen.records
        for j, x in zip(range(j0, j1), piece):
            assert x == got[j], j
    edges = set(edge_entries(rows * at)) | (set(edge_entries(d * at)) if d * at > Y_MAX + 1 else {0, d * at - 1})
    held = sorted({e % at // width for e in edges})
    assert held == [0, R - 1]
    for j in held:
        assert got[j].size() == (rows, width) and got[j].is_ntt
        want = oracle.preimage(moduli, n, base, SIGMA, r, e, a, targets_np[j], masters[j])
        assert np.array_equal(got[j].to_rns(), want), j
    assert A * got[R // 2] == targets[R // 2]
