"""gpupoly_matrix_decompose_rows / gpupoly_matrix_sample_decomposed_window: a row window of a decomposition.

    out = D[row_start : row_start + R, :],  D = G^-1(S),  row j*k + t*dpt + e of D = digit e of tower t of S[j, .]

Every case is held, bit for bit, to (1) the existing device sequence - an uploaded source or gpu_matrix_sample_distribution_columns,
then gpu_matrix_decompose_base(_small), then gpu_matrix_copy_block of the window's rows - through gpu_matrix_equal (every
residue and the format tag); (2) for decompose_rows, tests/plainref.py alone: `digits` of the uploaded residues and, for an
EVAL result, `ntt_slots` of them (every slot at n = 16, 8 slots otherwise; every coefficient of a COEFF result).  The source is
compared with a copy made before the call."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params

pytestmark = pytest.mark.gpu

DR, SW = "gpupoly_matrix_decompose_rows", "gpupoly_matrix_sample_decomposed_window"
# name -> (n, limbs, limb bits, base bits) through make_params, or (n, explicit moduli spec, base bits).  n16: dpt 3 and 5;
# n256: the double-precision transforms (51 bits), the 64-bit integer path (61), 32-bit words (31); n = 2^14: the grouped
# 32-bit kernel with 28-bit limbs, a context whose moduli fit 3 bytes (PACKED24 sources), one 51-bit limb; 51 + 12 bits: a
# digit of the wide tower exceeds the narrow modulus (the transforms' REDUCE variants)
RINGS = {"n16_dpt3": (16, 3, 18, 6), "n16_dpt5": (16, 3, 18, 4), "n256_51bit": (256, 3, 51, 17), "n256_61bit": (256, 2, 61, 20),
         "n256_31bit": (256, 2, 31, 8), "n16384_28bit": (16384, 2, 28, 14), "n16384_24bit": (16384, 2, 24, 12),
         "n16384_51bit": (16384, 1, 51, 17), "n64_51_12bit": (64, ((51, False), (12, True)), 17)}
SEED = 20261018
_rings = {}


def ring(gpu, oracle, name):
    if name not in _rings:
        spec = RINGS[name]
        if len(spec) == 4:
            n, depth, bits, base = spec
            p = make_params(gpu, oracle, n, depth, bits, base)
        else:
            n, widths, base = spec
            p = gpu.GpuDCRTPolyParams(n, [P.primes(n, bits, 1, low=low)[0] for bits, low in widths], base)
        moduli = [int(q) for q in p.moduli()]
        if n <= 16:
            slots = list(range(n))
        else:
            rng = np.random.default_rng(SEED + n)
            slots = sorted({0, 1, n - 1} | set(rng.choice(np.arange(2, n - 1), 5, replace=False).tolist()))
        _rings[name] = dict(p=p, n=n, moduli=moduli, base=base, dpt=P.digits_per_tower(moduli, base), slots=slots,
                            roots=[P.min_root(q, n) for q in moduli])
        assert _rings[name]["dpt"] == -(-p.crt_bits() // base)
    return _rings[name]


def lib():
    from mxx_amd import _ffi

    return _ffi.lib()


def ok(st, what):
    from mxx_amd import _ffi

    _ffi.check_status(st, what)


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: shape, residues AND format tag (empty matrices included)"""
    eq = C.c_int(0)
    ok(lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value)


def launches():
    return lib().gpupoly_launch_count()


def last_error():
    from mxx_amd import _ffi

    return _ffi.last_error_string()


def seed_of(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(bytes([(tag * 31 + i * 17 + 5) & 0xFF for i in range(32)]))


def digit_count(R, L, small):
    return R["dpt"] if small else R["dpt"] * L


def full_decomposition(gpu, R, src, small, eval_out):
    """the existing entry: every digit row"""
    k = digit_count(R, src.level + 1, small)
    out = gpu.GpuDCRTPolyMatrix(R["p"], src.nrow * k, src.ncol, src.level, eval_out)
    fn = lib().gpu_matrix_decompose_base_small if small else lib().gpu_matrix_decompose_base
    ok(fn(src.raw, R["base"], out.raw), "gpu_matrix_decompose_base")
    return out


def windows(r, k, dpt, towers):
    """(start, end) by name; rows of D are (source row, tower, digit) = (w // k, (w % k) // dpt, w % dpt)"""
    total = r * k
    w = {"whole": (0, total), "empty": (min(3, total), min(3, total)),
         "one_row": (k + 1, k + 2) if r > 1 else (k - 1, k),
         "one_tower": ((r - 1) * k + (towers - 1) * dpt, (r - 1) * k + towers * dpt)}
    if r > 1:
        w["mid_tower_into_next_source_row"] = (1 if dpt > 1 else 0, k + 2)
        assert w["mid_tower_into_next_source_row"][1] <= total
    else:
        w["mid_tower_to_mid_tower"] = (1, k - 1) if k > 2 else (0, 1)
    if r > 2:
        w["partial_whole_partial"] = (k - 1, 2 * k + 1)
    return w


def host_coeff(R, L, rows, cols, seed, top_rows=0):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, q, (rows, cols, R["n"]), dtype=np.uint64) for q in R["moduli"][:L]], axis=2)
    for j in range(min(top_rows, rows)):  # the largest residues: every digit at its maximum
        x[j, 0] = np.asarray(R["moduli"][:L], dtype=np.uint64).reshape(L, 1) - np.uint64(1)
    return x


def plain_rows(R, x, small):
    """G^-1(x) from plainref.digits: (rows * k, cols, L, n) coefficients"""
    rows, cols, L, n = x.shape
    moduli, dpt = R["moduli"][:L], R["dpt"]
    k = digit_count(R, L, small)
    out = np.zeros((rows * k, cols, L, n), dtype=np.uint64)
    for j in range(rows):
        for c in range(cols):
            out[j * k : (j + 1) * k, c] = P.digits(x[j, c], moduli, R["base"], dpt)[:k]  # small: the rows of tower 0
    return out


def plain_slots(R, d):
    rows, cols, L, n = d.shape
    ms = R["moduli"][:L] * (rows * cols)
    roots = R["roots"][:L] * (rows * cols)
    return P.ntt_slots(d.reshape(-1, n), ms, R["slots"], roots).reshape(rows, cols, L, len(R["slots"]))


# (ring, source rows, columns, limbs or None for all): c of 1, 7 and 9 (the 2^14 kernel's grid pads columns to 8), source
# rows 1 and 3, a level below the top
DECOMPOSE_CASES = [("n16_dpt3", 3, 9, None), ("n16_dpt3", 1, 7, None), ("n16_dpt3", 3, 1, 2), ("n16_dpt5", 3, 9, None),
                   ("n16_dpt5", 1, 1, None), ("n256_51bit", 3, 9, None), ("n256_51bit", 1, 7, 2), ("n256_61bit", 3, 9, None),
                   ("n256_31bit", 3, 9, None), ("n256_31bit", 1, 7, None), ("n16384_28bit", 3, 9, None),
                   ("n16384_28bit", 1, 7, None), ("n16384_28bit", 1, 1, 1), ("n16384_24bit", 3, 9, None),
                   ("n16384_51bit", 3, 1, None), ("n64_51_12bit", 3, 9, None), ("n64_51_12bit", 1, 7, None)]


@pytest.mark.parametrize("case", DECOMPOSE_CASES, ids=lambda c: f"{c[0]}-r{c[1]}-c{c[2]}" + (f"-L{c[3]}" if c[3] else ""))
def test_decompose_rows(gpu, oracle, case):
    name, rows, cols, limbs = case
    R = ring(gpu, oracle, name)
    M = gpu.GpuDCRTPolyMatrix
    L = limbs or len(R["moduli"])
    x = host_coeff(R, L, rows, cols, SEED + rows * 16 + cols, top_rows=1)
    src_coeff = M.from_rns(R["p"], x, False)
    src_eval = M.from_rns(R["p"], x, False)
    src_eval.ntt_all_in_place()
    assert src_coeff.level == L - 1 and src_eval.is_ntt and not src_coeff.is_ntt
    keep = {True: src_eval.clone(), False: src_coeff.clone()}
    for small in (False, True):
        k = digit_count(R, L, small)
        want_coeff = plain_rows(R, x, small)
        want_slots = plain_slots(R, want_coeff)
        for src_eval_fmt in (True, False):
            src = src_eval if src_eval_fmt else src_coeff
            for eval_out in (True, False):
                full = full_decomposition(gpu, R, src, small, eval_out)
                for wname, (rs, re) in windows(rows, k, R["dpt"], 1 if small else L).items():
                    what = (wname, rs, re, "small" if small else "full", "src eval" if src_eval_fmt else "src coeff", "out eval" if eval_out else "out coeff")
                    got = src.decompose_rows(rs, re, small, eval_out)
                    assert (got.nrow, got.ncol, got.level) == (re - rs, cols, L - 1), what
                    if re == rs:  # tagged EVAL whatever `out` was created as, like an empty gpu_matrix_decompose_base result
                        assert got.is_ntt and raw_same(got, M(R["p"], 0, cols, L - 1, True)), what
                        continue
                    assert raw_same(got, full.slice(rs, re, 0, cols)), what
                    assert got.is_ntt == eval_out, what
                    res = got.to_rns()
                    if eval_out:
                        assert np.array_equal(res[..., R["slots"]], want_slots[rs:re]), what
                    else:
                        assert np.array_equal(res, want_coeff[rs:re]), what
            assert raw_same(src, keep[src_eval_fmt]), "the source changed"


def test_decompose_rows_packed24_source(gpu, oracle):
    """an EVAL source stored in 3 bytes per residue is unpacked first; its residues do not change"""
    R = ring(gpu, oracle, "n16384_24bit")
    M = gpu.GpuDCRTPolyMatrix
    uni = gpu.DistType.FinRingDist().as_ffi()
    src = M.sample_distribution(R["p"], 3, 9, uni, 0.0, seed_of(gpu, 1))
    twin = M.sample_distribution(R["p"], 3, 9, uni, 0.0, seed_of(gpu, 1))
    x = twin.to_coeff_rns()
    twin_words = M.from_rns(R["p"], x, False)
    twin_words.ntt_all_in_place()
    assert src.layout == "packed24" and src.is_ntt
    k = digit_count(R, 2, False)
    got = src.decompose_rows(1, k + 2)
    want = plain_slots(R, plain_rows(R, x, False)[1 : k + 2])
    assert np.array_equal(got.to_rns()[..., R["slots"]], want)
    assert raw_same(got, full_decomposition(gpu, R, twin_words, False, True).slice(1, k + 2, 0, 9))
    assert raw_same(src, twin_words), "the source changed"


def sampled_columns(gpu, R, level, rows, full_ncol, col0, cols, dist, sigma, seed):
    out = gpu.GpuDCRTPolyMatrix(R["p"], rows, cols, level, True)
    ok(lib().gpu_matrix_sample_distribution_columns(out.raw, dist, sigma, seed, full_ncol, col0), "gpu_matrix_sample_distribution_columns")
    out.is_ntt = True
    return out


def dists(gpu):
    D = gpu.DistType
    return {"uniform": (D.FinRingDist().as_ffi(), 0.0), "gauss": (D.GaussDist(4.578).as_ffi(), 4.578), "bit": (D.BitDist().as_ffi(), 0.0),
            "ternary": (D.TernaryDist().as_ffi(), 0.0)}


def check_sample_windows(gpu, R, rows, cols, full_ncol, col0, L, tag):
    M = gpu.GpuDCRTPolyMatrix
    for dname, (dist, sigma) in dists(gpu).items():
        seed = seed_of(gpu, tag)
        src = sampled_columns(gpu, R, L - 1, rows, full_ncol, col0, cols, dist, sigma, seed)
        for small in (False, True):
            k = digit_count(R, L, small)
            for eval_out in (True, False):
                full = full_decomposition(gpu, R, src, small, eval_out)
                for wname, (rs, re) in windows(rows, k, R["dpt"], 1 if small else L).items():
                    what = (dname, wname, rs, re, "small" if small else "full", "out eval" if eval_out else "out coeff")
                    got = M.sample_distribution_decomposed_window(R["p"], rows, full_ncol, col0, cols, dist, sigma, seed, small, rs, re,
                                                                  eval_out, level=L - 1)
                    assert (got.nrow, got.ncol, got.level) == (re - rs, cols, L - 1), what
                    assert got.is_ntt == (eval_out or re == rs), what
                    want = M(R["p"], 0, cols, L - 1, True) if re == rs else full.slice(rs, re, 0, cols)  # empty: tagged EVAL
                    assert raw_same(got, want), what


# (ring, source rows, columns, full_ncol, col_offset, limbs)
SAMPLE_CASES = [("n16_dpt3", 3, 7, 12, 3, None), ("n16_dpt3", 1, 9, 9, 0, 2), ("n16_dpt5", 3, 1, 4, 3, None),
                ("n256_51bit", 3, 7, 12, 3, None), ("n256_61bit", 1, 9, 11, 1, None), ("n256_31bit", 3, 9, 12, 2, None),
                ("n16384_28bit", 3, 9, 12, 3, None), ("n16384_28bit", 1, 7, 7, 0, 1), ("n16384_24bit", 3, 1, 5, 2, None),
                ("n16384_51bit", 3, 7, 9, 2, None), ("n64_51_12bit", 3, 7, 12, 3, None)]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: f"{c[0]}-r{c[1]}-c{c[2]}of{c[3]}at{c[4]}" + (f"-L{c[5]}" if c[5] else ""))
def test_sample_decomposed_window(gpu, oracle, case):
    name, rows, cols, full_ncol, col0, limbs = case
    R = ring(gpu, oracle, name)
    check_sample_windows(gpu, R, rows, cols, full_ncol, col0, limbs or len(R["moduli"]), 7 + rows + cols)


@pytest.mark.parametrize("name", ["n16_dpt3", "n256_51bit"])
def test_sample_decomposed_window_reference_keying(gpu, oracle, hip_env, name):
    """MXX_HIP_RNG_COMPAT=reference: the window commutes under the reference's keying as well"""
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    R = ring(gpu, oracle, name)
    check_sample_windows(gpu, R, 3, 7, 12, 3, len(R["moduli"]), 40)


def traced(gpu, fn):
    from mxx_amd import _ffi

    gpu.gpu_device_sync()
    _ffi.trace_begin()
    out = fn()
    gpu.gpu_device_sync()
    return out, _ffi.trace_end()


def test_work_follows_the_window(gpu, oracle):
    """n = 2^14, 2 limbs, dpt 2 (k = 4), 3 x 9 source: workgroups of the digit transforms and sampled words of a window are
    those of its rows - counts computed from the shapes (8 * L * ceil(c / 8) workgroups per digit row; a uniform sampling
    thread draws 8 residues of one limb, 256 threads per workgroup)"""
    R = ring(gpu, oracle, "n16384_28bit")
    M = gpu.GpuDCRTPolyMatrix
    n, L, rows, cols, k = R["n"], 2, 3, 9, 4
    assert digit_count(R, L, False) == k
    per_row = 8 * L * ((cols + 7) // 8)
    uni = gpu.DistType.FinRingDist().as_ffi()
    seed = seed_of(gpu, 3)

    def digit_blocks(recs):
        return sum(r["blocks"] for r in recs if "fwd_digits_kernel" in r["kernel"])

    def sample_recs(recs):
        return [r for r in recs if "sample_uniform_kernel" in r["kernel"]]

    def run(rs, re):
        return traced(gpu, lambda: M.sample_distribution_decomposed_window(R["p"], rows, cols, 0, cols, uni, 0.0, seed, False, rs, re))[1]

    whole = run(0, rows * k)
    assert digit_blocks(whole) == per_row * rows * k
    assert [r["blocks"] for r in sample_recs(whole)] == [rows * cols * L * (n // 8) // 256]
    # rows [3, 6): 1 / k of the decomposition (a decompose_chunk window); source rows 0 and 1, every tower
    chunk = run(rows, 2 * rows)
    assert digit_blocks(chunk) == per_row * rows == digit_blocks(whole) // k
    assert [r["blocks"] for r in sample_recs(chunk)] == [2 * cols * L * (n // 8) // 256]
    assert sample_recs(chunk)[0]["bytes"] == 2 * cols * L * n * 4
    # one row, (source row 1, tower 0, digit 1): one source row, one tower
    one = run(k + 1, k + 2)
    assert digit_blocks(one) == per_row
    assert [r["blocks"] for r in sample_recs(one)] == [cols * (n // 8) // 256]
    assert sample_recs(one)[0]["bytes"] == cols * n * 4
    # an EVAL source: the inverse transform runs over the touched source rows only (1 of 3), the digit transforms over the window
    src = M.sample_distribution(R["p"], rows, cols, gpu.DistType.BitDist().as_ffi(), 0.0, seed)
    recs = traced(gpu, lambda: src.decompose_rows(k + 1, k + 3))[1]
    assert digit_blocks(recs) == 2 * per_row
    inv = [r for r in recs if "inv_kernel" in r["kernel"]]
    assert len(inv) == 1 and inv[0]["blocks"] == cols * L, recs
    assert not [r for r in recs if "sample" in r["kernel"]]


def test_refusals_leave_everything(gpu, oracle):
    R = ring(gpu, oracle, "n16_dpt3")
    R2 = ring(gpu, oracle, "n16_dpt5")
    M = gpu.GpuDCRTPolyMatrix
    L, k = 3, 9
    x = host_coeff(R, L, 2, 3, SEED)
    src = M.from_rns(R["p"], x, True)
    sentinel = host_coeff(R, L, 4, 3, SEED + 1)
    out = M.from_rns(R["p"], sentinel, False)  # tagged COEFF: a refused call must not retag it
    uni = gpu.DistType.FinRingDist().as_ffi()
    gauss = gpu.DistType.GaussDist(3.0).as_ffi()
    seed = seed_of(gpu, 5)
    other_ctx = M.from_rns(R2["p"], host_coeff(R2, L, 4, 3, SEED + 2), False)
    low_level = M.from_rns(R["p"], host_coeff(R, 2, 4, 3, SEED + 3), False)
    wide = M.from_rns(R["p"], host_coeff(R, L, 4, 4, SEED + 4), False)
    big = M.from_rns(R["p"], host_coeff(R, L, 2 * k, 3, SEED + 5), True)
    view, view2 = big.row_view(3, 7), big.row_view(5, 9)

    def refused(entry, fn, *needles):
        before = launches()
        assert fn() != 0, (entry, needles)
        msg = last_error()
        assert entry in msg and all(s in msg for s in needles), msg
        assert launches() == before, msg

    dr, sw = lib().gpupoly_matrix_decompose_rows, lib().gpupoly_matrix_sample_decomposed_window
    gpu.gpu_device_sync()
    refused(DR, lambda: dr(None, 6, 0, 0, out.raw))
    refused(DR, lambda: dr(src.raw, 6, 0, 0, None))
    refused(DR, lambda: dr(src.raw, 0, 0, 0, out.raw))
    refused(DR, lambda: dr(src.raw, 63, 0, 0, out.raw))
    refused(DR, lambda: dr(src.raw, 6, 0, 0, other_ctx.raw))
    refused(DR, lambda: dr(src.raw, 6, 0, 0, low_level.raw))
    refused(DR, lambda: dr(src.raw, 6, 0, 0, wide.raw))
    refused(DR, lambda: dr(src.raw, 6, 0, 2 * k - 3, out.raw))  # 4 rows from row 15 of 18
    refused(DR, lambda: dr(src.raw, 6, 1, 2 * 3 - 3, out.raw))  # small: 6 digit rows
    refused(DR, lambda: dr(src.raw, 6, 0, 2 * k + 1, out.raw))
    refused(DR, lambda: dr(big.raw, 6, 0, 0, view.raw), "overlap")  # a row view of the source as the output
    refused(DR, lambda: dr(view.raw, 6, 0, 0, view2.raw), "overlap")  # two views of one parent
    refused(SW, lambda: sw(None, uni, 0.0, seed, 6, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 0, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 63, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, 4, 0.0, seed, 6, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, -1, 0.0, seed, 6, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, gauss, 0.0, seed, 6, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, gauss, -1.0, seed, 6, 0, 2, 3, 0, 0))
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 6, 0, 2, 5, 3, 0))  # columns [3, 6) of 5
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 6, 0, 2, 3, 0, 2 * k - 3))
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 6, 1, 1, 3, 0, 0))  # small: 3 digit rows, 4 asked for
    refused(SW, lambda: sw(out.raw, uni, 0.0, seed, 6, 0, 1 << 40, 1 << 10, 0, 0))  # 2^50 polynomials: the 48-bit stream ids
    gpu.gpu_device_sync()
    assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel)
    # the tag as the library holds it: equal (residues AND tag) to a fresh COEFF upload of the sentinel
    assert raw_same(out, M.from_rns(R["p"], sentinel, False))
    assert np.array_equal(big.to_rns()[3:7], view.to_rns())
    # R = 0 and c = 0 succeed with nothing launched and tag the result EVAL
    for shape in ((0, 3), (4, 0)):
        empty = M(R["p"], shape[0], shape[1], L - 1, False)
        esrc = M(R["p"], 2, shape[1], L - 1, True)
        before = launches()
        assert dr(esrc.raw, 6, 0, 1, empty.raw) == 0, last_error()
        assert sw(empty.raw, uni, 0.0, seed, 6, 0, 2, max(shape[1], 1), 0, 1) == 0, last_error()
        assert launches() == before
        assert raw_same(empty, M(R["p"], shape[0], shape[1], L - 1, True))


def test_mirror_methods_equal_their_old_definitions(gpu, oracle):
    """decompose_chunk, small_decompose_chunk, sample_hash_decomposed_columns and sample_hash_small_decomposed_columns give what
    they gave when they built every digit row: sample_hash_columns(...).decompose() and its row slices"""
    for name in ("n16_dpt3", "n256_51bit", "n16384_28bit"):
        R = ring(gpu, oracle, name)
        p, L, dpt = R["p"], len(R["moduli"]), R["dpt"]
        k = dpt * L
        hs = gpu.GpuDCRTPolyHashSampler()
        key, tag = bytes(range(32)), b"decompose-window"
        for dist in (gpu.DistType.FinRingDist(), gpu.DistType.GaussDist(4.578), gpu.DistType.BitDist(), gpu.DistType.TernaryDist()):
            base = hs.sample_hash_columns(p, key, tag, 3, 12, 3, 7, dist)
            full, small = base.decompose(), base.small_decompose()
            assert (full.nrow, small.nrow) == (3 * k, 3 * dpt)
            assert hs.sample_hash_decomposed_columns(p, key, tag, 3, 12, 3, 7, dist) == full
            assert hs.sample_hash_small_decomposed_columns(p, key, tag, 3, 12, 3, 7, dist) == small
            assert hs.sample_hash_decomposed_columns(p, key, tag, 3, 12, 3, 7, dist, row_start=2, row_end=k + 1) == full.slice_rows(2, k + 1)
            assert hs.sample_hash_small_decomposed_columns(p, key, tag, 3, 12, 3, 7, dist, row_start=1, row_end=dpt + 2) == small.slice_rows(1, dpt + 2)
        for idx in (0, 1, k - 1):
            assert base.decompose_chunk(idx, k) == full.slice_rows(idx * 3, (idx + 1) * 3)
        for idx in (0, dpt - 1):
            assert base.small_decompose_chunk(idx, dpt) == small.slice_rows(idx * 3, (idx + 1) * 3)
        with pytest.raises(AssertionError):
            base.decompose_chunk(k, k)
        with pytest.raises(AssertionError):
            base.decompose_chunk(0, k + 1)
