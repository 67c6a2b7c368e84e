"""GPU against the plain big-integer reference (tests/plainref.py), one cell per modulus width class.

The library picks its kernels by the width of the widest modulus: 32-bit words below 2^31 (signed lazy inverse
butterflies to 24 bits, lazy forms to 25, tight forms at 26..28, the generic fully reduced path at 29..31), 64-bit
words above (double-precision transforms to 51 bits with fold schedules switching at 40 / 49 / 51, lazy integer
forms to 57, non-lazy ones to 61; a `%` reduction for limbs below 33 bits).  Every cell runs both edge primes of its
class - the largest below 2^bits and the smallest above 2^(bits-1) - at a small ring and at a ring that reaches the
LDS / split kernels, plus the parameter sets of the reference's GPU callers at full depth.

Nothing here uses the CPU oracle as the expected value except for the seeded samplers, whose streams only the
oracle restates (tests/test_plainref.py pins the oracle to plainref on the same grid).
"""
import math
import random

import numpy as np
import pytest

import plainref as P
import ran
from conftest import is_prime
from mxx_amd.matrix import _bincode_read_varint

pytestmark = pytest.mark.gpu

SEED = 20261015


def _moduli(n, bits, count=2):
    """`count` largest and `count` smallest primes of the class (fewer where the progression runs out)."""
    hi, lo = [], []
    for low, out in ((False, hi), (True, lo)):
        for c in range(count, 0, -1):
            try:
                out.extend(P.primes(n, bits, c, low=low))
                break
            except ValueError:
                continue
    ms = list(dict.fromkeys(hi + lo))
    assert ms and all(is_prime(q) for q in ms)
    return ms


_PARAMS = {}


def _params(gpu, n, moduli, base):
    key = (n, tuple(moduli), base)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, list(moduli), base)
    return _PARAMS[key]


def _patterns(moduli, n, seed, full=True):
    """(1, P, L, n) inputs: random, all q - 1, alternating 0 / q - 1 at periods 2, 64 and n, a spike at n - 1."""
    rng = np.random.default_rng(seed)
    L = len(moduli)
    top = np.asarray(moduli, dtype=np.uint64).reshape(L, 1) - np.uint64(1)
    pats = [np.stack([rng.integers(0, int(q), n, dtype=np.uint64) for q in moduli])]
    pats.append(np.broadcast_to(top, (L, n)).copy())
    if full:
        for period in sorted({2, min(64, n), n}):
            m = np.broadcast_to(top, (L, n)).copy()
            m[:, (np.arange(n) // max(period // 2, 1)) % 2 == 1] = 0
            pats.append(m)
    spike = np.zeros((L, n), dtype=np.uint64)
    spike[:, n - 1] = top[:, 0]
    pats.append(spike)
    return np.stack(pats)[None]


def _slots(n, count=8):
    if n <= 1024:
        return list(range(n))
    rng = np.random.default_rng(SEED + n)
    return sorted({0, 1, n - 1} | set(rng.integers(0, n, count - 3).tolist()))


_ROOTS = {}


def _root(q, n):
    if (q, n) not in _ROOTS:
        _ROOTS[(q, n)] = P.min_root(q, n)
    return _ROOTS[(q, n)]


def _forward_ref(x, moduli, slots, limbs):
    """plainref slots of every (pattern, limb in `limbs`) vector of x (1, P, L, n): (P, len(limbs), len(slots))."""
    Pn = x.shape[1]
    stacked = x[0][:, limbs].reshape(Pn * len(limbs), -1)
    ms = [moduli[l] for l in limbs] * Pn
    roots = [_root(q, x.shape[-1]) for q in ms]
    return P.ntt_slots(stacked, ms, slots, roots).reshape(Pn, len(limbs), len(slots))


# (bits, n): every class at both its small-ring kernel and its LDS / split kernel
TRANSFORM_CELLS = [
    (10, 4), (10, 64), (12, 4), (12, 64), (15, 4), (15, 512),
    (24, 256), (24, 1 << 14), (25, 256), (25, 1 << 14), (26, 256), (26, 1 << 14), (28, 256), (28, 1 << 16),
    (29, 1024), (29, 1 << 16), (31, 256), (31, 1 << 14), (31, 1 << 16),
    (32, 256), (32, 1 << 14), (33, 256), (33, 1 << 14), (40, 256), (40, 1 << 14), (41, 256), (41, 1 << 14),
    (49, 1 << 14), (50, 1 << 14), (51, 256), (51, 1 << 16), (52, 256), (52, 1 << 14), (57, 256), (57, 1 << 14), (58, 256), (58, 1 << 16),
    (61, 256), (61, 1 << 14), (62, 256), (62, 1 << 14),  # the ABI takes q < 2^62: 62-bit limbs are accepted too
]


def _check_transform(gpu, hip_env, n, moduli, x, paths, u64_limbs=4):
    """Forward against plainref on the chosen slots (every slot up to n = 1024) for the default dispatch; every forced
    path bit-equal to it in full; the inverse of the same patterns as evaluation-domain inputs checked by the forward
    definition; round trips."""
    p = _params(gpu, n, moduli, 1)
    wide = max(moduli) >> 31 != 0
    limbs = list(range(len(moduli))) if not wide else list(range(min(u64_limbs, len(moduli))))
    slots = _slots(n)
    m = gpu.GpuDCRTPolyMatrix.from_rns(p, x, False)
    with ran.launches() as k_default:
        m.ntt_all_in_place()
    fwd = m.to_rns()
    want = _forward_ref(x, moduli, slots, limbs)
    got = fwd[0][:, limbs][:, :, slots]
    assert np.array_equal(got, want), "forward transform differs from plainref"
    m.intt_all_in_place()
    assert np.array_equal(m.to_rns(), x), "round trip"
    e = gpu.GpuDCRTPolyMatrix.from_rns(p, x, True)
    with ran.launches() as k_default_inv:
        e.intt_all_in_place()
    if _path_runs(("MXX_HIP_NTT64", None), n, moduli):  # the default of this class is the double-precision family
        k_default.assert_ran("MXX_HIP_NTT64", None, moduli)
        k_default_inv.assert_ran("MXX_HIP_NTT64", None, moduli)
    inv = e.to_rns()
    back = _forward_ref(inv, moduli, slots, limbs)
    assert np.array_equal(back, x[0][:, limbs][:, :, slots]), "inverse transform: forward definition of its output"
    for name, value in paths:
        hip_env.set(name, value)
        f = gpu.GpuDCRTPolyMatrix.from_rns(p, x, False)
        g = gpu.GpuDCRTPolyMatrix.from_rns(p, x, True)
        with ran.launches() as k:
            f.ntt_all_in_place()
            g.intt_all_in_place()
        # the equal values below cannot tell a forced kernel from the default one it may have fallen back to
        if _path_runs((name, value), n, moduli):
            k.assert_ran(name, value, moduli, forward=True, inverse=True)
        assert np.array_equal(f.to_rns(), fwd), (name, value, "forward")
        assert np.array_equal(g.to_rns(), inv), (name, value, "inverse")
        hip_env.unset(name)


def _forced_paths(moduli):
    paths = [("MXX_HIP_NTT_PATH", "generic"), ("MXX_HIP_NTT_PATH", "global")]
    if max(moduli) >> 31 and max(moduli).bit_length() <= 51:
        paths.append(("MXX_HIP_NTT64", "int"))
    return paths


def _path_runs(pair, n, moduli):
    """Does the kernel family that `pair` forces accept this ring?  None: the pair does not apply to these moduli.
    generic: launch_ntt_typed (ntt.hip) sends a vector beyond 160 KB of LDS to the per-stage kernels instead; global:
    always; the double-precision transforms and their integer counterpart: 64-bit words with every modulus at most 51
    bits (f64_transforms, ntt_lds_u64.hip)."""
    wide = max(moduli) >> 31 != 0
    if pair == ("MXX_HIP_NTT_PATH", "generic"):
        return n * (8 if wide else 4) <= 160 * 1024
    if pair == ("MXX_HIP_NTT_PATH", "global"):
        return True
    if pair[0] == "MXX_HIP_NTT64":
        return True if wide and max(moduli).bit_length() <= 51 else None
    raise KeyError(pair)


def _fused_digits_accept(n, moduli):
    """launch_ntt_digits_u32 / _u64: lazy or tight moduli in 32-bit words (ntt14_switches), lazy ones in 64-bit words, and
    a ring of the table in ntt_rings.h (2^10 .. 2^17 points)"""
    bits = max(moduli).bit_length()
    ok = bits + 7 <= 64 if max(moduli) >> 31 else bits + 4 <= 32
    return ok and 1 << 10 <= n <= 1 << 17


@pytest.mark.parametrize("bits,n", TRANSFORM_CELLS)
def test_transform_edge_primes(gpu, hip_env, bits, n):
    moduli = _moduli(n, bits)
    x = _patterns(moduli, n, SEED + bits * 131 + n, full=n <= (1 << 14) or max(moduli) < 1 << 32)
    _check_transform(gpu, hip_env, n, moduli, x, _forced_paths(moduli))


# the reference callers' parameter sets at full depth: (n, limbs, bits)
REFERENCE_SETS = [(1 << 16, 64, 32), (1 << 14, 32, 24), (1 << 16, 64, 28)]


@pytest.mark.parametrize("n,depth,bits", REFERENCE_SETS)
def test_transform_reference_sets(gpu, hip_env, n, depth, bits):
    moduli = P.primes(n, bits, depth)
    x = _patterns(moduli, n, SEED + depth, full=False)
    _check_transform(gpu, hip_env, n, moduli, x, [("MXX_HIP_NTT_PATH", "global")], u64_limbs=depth)


MIXED_WIDTHS = [(64, (24, 12)), (1 << 14, (51, 33))]  # (n, (bits of the widest limb, bits of a narrow one))


def _mixed_moduli(n, widths):
    return [P.primes(n, widths[0], 1)[0], P.primes(n, widths[1], 1, low=True)[0]]


def test_transform_mixed_widths(gpu, hip_env):
    """The ABI accepts mixed widths; the kernels then pick their forms by the widest limb."""
    for n, widths in MIXED_WIDTHS:
        moduli = _mixed_moduli(n, widths)
        x = _patterns(moduli, n, SEED + n)
        _check_transform(gpu, hip_env, n, moduli, x, _forced_paths(moduli))


# ---------------------------------------------------------------------------------------------- pointwise
POINTWISE_BITS = [10, 12, 15, 24, 25, 26, 28, 29, 31, 32, 33, 40, 41, 51, 52, 57, 58, 61, 62]


@pytest.mark.parametrize("bits", POINTWISE_BITS)
def test_pointwise_ops(gpu, bits):
    n = 64 if bits <= 12 else 256
    moduli = _moduli(n, bits)
    p = _params(gpu, n, moduli, 1)
    L = len(moduli)
    qv = np.asarray(moduli, dtype=object).reshape(1, 1, L, 1)
    rng = np.random.default_rng(SEED + bits)
    top = np.broadcast_to(np.asarray(moduli, dtype=np.uint64).reshape(1, 1, L, 1) - np.uint64(1), (1, 2, L, n))
    rand = np.stack([rng.integers(0, int(q), (2, n), dtype=np.uint64) for q in moduli], axis=1)[None]
    for a, b in ((top.copy(), top.copy()), (rand, top.copy()), (top.copy(), rand[:, ::-1].copy())):
        ga = gpu.GpuDCRTPolyMatrix.from_rns(p, a, True)
        gb = gpu.GpuDCRTPolyMatrix.from_rns(p, b, True)
        ao, bo = a.astype(object), b.astype(object)
        for name, got, want in (
            ("add", ga + gb, (ao + bo) % qv),
            ("sub", ga - gb, (ao - bo) % qv),
            ("neg", -ga, (-ao) % qv),
        ):
            assert np.array_equal(got.to_rns().astype(object), want), name
        prod = (ao * bo) % qv
        got = gpu.GpuDCRTPolyMatrix.from_rns(p, a, True).mul_scalar(gpu.GpuDCRTPolyMatrix.from_rns(p, b[:, :1], True))
        assert np.array_equal(got.to_rns().astype(object), (ao * bo[:, :1]) % qv), "mul_scalar"
        # the entry-wise product of two 1 x 1 matrices is the ring product; in the evaluation domain: slot by slot
        one = gpu.GpuDCRTPolyMatrix.from_rns(p, a[:, :1], True) * gpu.GpuDCRTPolyMatrix.from_rns(p, b[:, :1], True)
        assert np.array_equal(one.to_rns().astype(object), prod[:, :1]), "mul"
        # INTT(a o s): the product's coefficients, checked by the forward definition on all slots
        mi = gpu.GpuDCRTPolyMatrix.from_rns(p, a, True).mul_scalar_intt(gpu.GpuDCRTPolyMatrix.from_rns(p, b[:, :1], True))
        coeff = mi.to_rns()
        want_slots = ((ao * bo[:, :1]) % qv).astype(np.uint64)
        for c in range(2):
            assert np.array_equal(P.ntt_slots(coeff[0, c], moduli, range(n)), want_slots[0, c]), "mul_scalar_intt"


# ---------------------------------------------------------------------------------------------- ring-matrix product
def _lazy_terms(q, wide):
    """How many (q-1)^2 products the accumulator holds on top of a residue: 64-bit for 32-bit words, 128-bit for 64-bit
    words (a context has 64-bit words when any of its moduli reaches 2^31)."""
    acc = 128 if wide else 64
    return ((1 << acc) - q) // ((q - 1) ** 2)


MATMUL_CELLS = [10, 12, 15, 24, 26, 28, 29, 31, 32, 33, 41, 52, 58, 61, 62]
# forced family -> the kernel the dispatcher must then report (gpupoly_context_last_kernel)
U32_MATMUL_PATHS = {None: None, "reg": "matmul_kernel<u32", "lds": "matmul_lds_kernel_u32", "dma": "mmdma::kernel_u32",
                    "wide": "mmdma32::kernel_u32", "mfma": "mmfma::kernel_u32"}
# past this many terms the q - 1 operands of one product would pass 1 GB (24 bits: 2^16 terms; 10..15 bits: the
# bound is capped at 2^20): those cells run a short inner dimension and rely on the wider cells for the bound
MAX_INNER = 4100
KC = 4  # the streamed (dma / wide) kernels take the inner dimension in chunks of 4 and decline any other shape


@pytest.mark.parametrize("bits", MATMUL_CELLS)
def test_ring_matmul(gpu, hip_env, bits):
    n = 64 if bits <= 12 else 256
    _check_matmul(gpu, hip_env, n, _moduli(n, bits))


def test_ring_matmul_mixed_widths(gpu, hip_env):
    """Narrow limbs in a wide context: the 128-bit accumulator's reduction takes its `%` branch below 33 bits."""
    for n, spec in ((64, ((51, False), (12, True))), (256, ((41, False), (31, True))), (256, ((51, False), (33, True))),
                    (64, ((24, False), (12, True)))):
        _check_matmul(gpu, hip_env, n, [P.primes(n, bits, 1, low=low)[0] for bits, low in spec])


def _check_matmul(gpu, hip_env, n, moduli):
    """q - 1 operands in both factors with an inner dimension past the accumulator's lazy bound (a multiple of 4, so
    that the streamed kernels accept it), every forced kernel family for 32-bit words with the kernel that ran checked
    by name; sampled coefficients of a random product against the defining negacyclic sums."""
    p = _params(gpu, n, moduli, 1)
    bits = max(moduli).bit_length()
    L = len(moduli)
    lt = min(_lazy_terms(q, max(moduli) >> 31 != 0) for q in moduli)
    past = -(-(lt + 1) // KC) * KC
    inner = past if past <= MAX_INNER else 8
    paths = U32_MATMUL_PATHS if max(moduli) < 1 << 31 else {None: None}
    qm1 = np.asarray(moduli, dtype=np.uint64).reshape(1, 1, L, 1) - np.uint64(1)
    ga = gpu.GpuDCRTPolyMatrix.from_rns(p, np.broadcast_to(qm1, (2, inner, L, n)).copy(), True)
    gb = gpu.GpuDCRTPolyMatrix.from_rns(p, np.broadcast_to(qm1, (inner, 3, L, n)).copy(), True)
    want_top = np.broadcast_to(np.asarray([inner % q for q in moduli], dtype=np.uint64).reshape(1, 1, L, 1), (2, 3, L, n))
    rng = np.random.default_rng(SEED + bits)
    A = np.stack([rng.integers(0, int(q), (2, 8, n), dtype=np.uint64) for q in moduli], axis=2)
    B = np.stack([rng.integers(0, int(q), (8, 3, n), dtype=np.uint64) for q in moduli], axis=2)
    A[0, 1] = qm1[0, 0]  # an all-(q-1) coefficient entry
    B[1, 2] = qm1[0, 0]
    idx = [0, 1, n // 2, n - 1]
    entries = [(0, 2), (1, 0)]
    want = P.ring_matmul_coeffs(A, B, moduli, entries, idx)
    ca = gpu.GpuDCRTPolyMatrix.from_rns(p, A, False).ensure_eval()
    cb = gpu.GpuDCRTPolyMatrix.from_rns(p, B, False).ensure_eval()
    # the matrix-core kernel takes inner <= 128 and moduli of 9..23 bits whose products fit its epilogue bound; below
    # 2^16 that bound always holds, so there it must run, and above it may decline (the dispatcher then falls back)
    mfma_ok = max(moduli) < 1 << 16 and min(moduli) >= 256
    for path, kernel in paths.items():
        if path is None:
            hip_env.unset("MXX_HIP_MATMUL_PATH")
        else:
            hip_env.set("MXX_HIP_MATMUL_PATH", path)
        for what, lhs, rhs, k in (("q - 1 operands", ga, gb, inner), ("random operands", ca, cb, 8)):
            prod = lhs * rhs
            ran = p.ctx().last_kernel()
            if kernel and (path != "mfma" or (mfma_ok and k <= 128)):
                assert ran.startswith(kernel), (path, what, ran)
            if what == "q - 1 operands":
                assert np.array_equal(prod.to_rns(), want_top), (path, what, ran)
            else:
                c = prod.to_coeff_rns()
                for (r, col, l), vals in want.items():
                    assert [int(c[r, col, l, i]) for i in idx] == vals, (path, ran, r, col, l)


def test_ring_matmul_reference_set(gpu):
    """32 limbs of 24 bits at n = 2^14 (the nested-RNS callers' set): one sampled product."""
    n, depth, bits = 1 << 14, 32, 24
    moduli = P.primes(n, bits, depth)
    p = _params(gpu, n, moduli, 12)
    rng = np.random.default_rng(SEED)
    A = np.stack([rng.integers(0, q, (1, 2, n), dtype=np.uint64) for q in moduli], axis=2)
    B = np.stack([rng.integers(0, q, (2, 1, n), dtype=np.uint64) for q in moduli], axis=2)
    c = (gpu.GpuDCRTPolyMatrix.from_rns(p, A, False).ensure_eval() * gpu.GpuDCRTPolyMatrix.from_rns(p, B, False).ensure_eval())
    c = c.to_coeff_rns()
    idx = [0, 1, n - 1]
    for (r, col, l), vals in P.ring_matmul_coeffs(A, B, moduli, [(0, 0)], idx).items():
        assert [int(c[r, col, l, k]) for k in idx] == vals, l


# ---------------------------------------------------------------------------------------------- decomposition
# (n, moduli spec, base): short last digits, one digit per tower, the reference callers' (bits, base), mixed widths
DECOMPOSE_CELLS = [
    (256, ("edge", 17), 15), (256, ("edge", 15), 13), (64, ("edge", 12), 12), (64, ("edge", 10), 5),
    (64, ("edge", 12), 6), (256, ("edge", 24), 12), (256, ("edge", 28), 14), (256, ("edge", 31), 16),
    (256, ("edge", 32), 16), (256, ("edge", 33), 11), (256, ("edge", 41), 20), (256, ("edge", 61), 20),
    (256, ("edge", 18), 6), (1 << 14, ("edge", 24), 12), (1 << 14, ("edge", 52), 26),
    # the fused double-precision digit kernels (n >= 2^10) at each fold schedule: <4095> to 40 bits, <63> to 49, <15>
    (1 << 14, ("edge", 40), 20), (1 << 14, ("edge", 41), 21), (1 << 14, ("edge", 49), 25), (1 << 14, ("edge", 50), 25),
    (64, ("mixed", (24, 12)), 12), (256, ("mixed", (51, 33)), 17),
]


def _cell_moduli(n, spec):
    if spec[0] == "edge":
        return _moduli(n, spec[1])
    return [P.primes(n, spec[1][0], 1)[0], P.primes(n, spec[1][1], 1, low=True)[0]]


@pytest.mark.parametrize("n,spec,base", DECOMPOSE_CELLS)
def test_decompose(gpu, hip_env, n, spec, base):
    moduli = _cell_moduli(n, spec)
    p = _params(gpu, n, moduli, base)
    L = len(moduli)
    dpt = P.digits_per_tower(moduli, base)
    k = L * dpt
    assert p.modulus_digits() == k
    rows = _patterns(moduli, n, SEED + base)[0]  # (P, L, n)
    M = rows[:, None]  # P x 1 matrix
    want = np.concatenate([P.digits(rows[r], moduli, base, dpt)[:, None] for r in range(rows.shape[0])])
    G = gpu.GpuDCRTPolyMatrix.gadget_matrix(p, rows.shape[0])
    assert np.array_equal(gpu.GpuDCRTPolyMatrix.gadget_matrix(p, 2).to_coeff_rns(), P.gadget(2, moduli, base, n))
    for fused in (None, "1", "0"):  # unset: the fused form is the default
        if fused is None:
            hip_env.unset("MXX_HIP_DECOMPOSE_FUSED")
        else:
            hip_env.set("MXX_HIP_DECOMPOSE_FUSED", fused)
        for eval_in in (False, True):
            src = gpu.GpuDCRTPolyMatrix.from_rns(p, M, False)
            if eval_in:
                src = src.ensure_eval()
            with ran.launches() as launched:
                dec = src.decompose()
            if fused == "0" or _fused_digits_accept(n, moduli):
                launched.assert_ran("MXX_HIP_DECOMPOSE_FUSED", fused, moduli)
            assert dec.size() == (rows.shape[0] * k, 1)
            assert np.array_equal(dec.to_coeff_rns(), want), (fused, eval_in)
            assert G * dec == gpu.GpuDCRTPolyMatrix.from_rns(p, M, False).ensure_eval(), "G G^-1(M) != M"
    hip_env.unset("MXX_HIP_DECOMPOSE_FUSED")
    # S G^-1(B) against S times the plain digits
    rng = np.random.default_rng(SEED + 7)
    S = np.stack([rng.integers(0, q, (1, rows.shape[0] * k, n), dtype=np.uint64) for q in moduli], axis=2)
    gs = gpu.GpuDCRTPolyMatrix.from_rns(p, S, False).ensure_eval()
    got = gs.mul_decompose(gpu.GpuDCRTPolyMatrix.from_rns(p, M, False)).to_coeff_rns()
    idx = [0, 1, n - 1]
    for (r, col, l), vals in P.ring_matmul_coeffs(S, want, moduli, [(0, 0)], idx).items():
        assert [int(got[r, col, l, i]) for i in idx] == vals, ("mul_decompose", l)


# ---------------------------------------------------------------------------------------------- compact wire format
SERDE_CELLS = [(16, 10, 2), (16, 12, 3), (256, 24, 3), (256, 31, 3), (256, 32, 3), (256, 33, 2), (256, 41, 3),
               (256, 61, 3), (256, 62, 3), (1 << 14, 32, 4)]


def _serde_values(moduli, count, limit, seed):
    """`count` integers in [-limit, limit]: the fast-path boundaries of the device store that lie inside, then random
    ones (the compact width is the largest over the matrix, so the limit sets it)."""
    h0 = moduli[0] // 2
    h01 = moduli[0] * moduli[1] // 2
    Q = math.prod(moduli)
    edges = [0, 1, -1, h0, -h0, h0 + 1, -(h0 + 1), h01, -h01, h01 + 1, -(h01 + 1), Q // 2, -(Q // 2)]
    edges = [v for v in edges if abs(v) <= limit]
    rnd = random.Random(seed)
    return edges + [rnd.randint(-limit, limit) for _ in range(count - len(edges))]


@pytest.mark.parametrize("mode", [None, "general"])
@pytest.mark.parametrize("n,bits,depth", SERDE_CELLS)
def test_compact_bytes_coeffs_and_modulus_switch(gpu, hip_env, mode, n, bits, depth):
    moduli = _moduli(n, bits, depth)[:depth]
    assert len(moduli) == depth
    p = _params(gpu, n, moduli, 1)
    Q = math.prod(moduli)
    if mode:
        hip_env.set("MXX_HIP_SERDE", mode)
    for limit in (moduli[0] // 2 + 1, moduli[0] * moduli[1] // 2 + 1, Q // 2):
        limit = min(limit, Q // 2)
        vals = _serde_values(moduli, 2 * n, limit, SEED + bits + limit % 997)
        res = np.asarray([[[[v % q for v in vals[c * n:(c + 1) * n]] for q in moduli] for c in range(2)]], dtype=np.uint64)
        centred = [P.centred_crt(res[0, c, :, i], moduli) for c in range(2) for i in range(n)]
        assert centred == vals
        m = gpu.GpuDCRTPolyMatrix.from_rns(p, res, False)
        with ran.launches() as launched:
            data = m.to_compact_bytes()
        if depth <= 16:  # the store tries its fast kernels up to 16 limbs (serde.hip), unless the switch says general
            launched.assert_ran("MXX_HIP_SERDE", mode, moduli)
        pos = 2
        for _ in range(3):  # level, nrow, ncol
            _, pos = _bincode_read_varint(data, pos)
        width, pos = _bincode_read_varint(data, pos)
        bpc, pos = _bincode_read_varint(data, pos)
        plen, pos = _bincode_read_varint(data, pos)
        assert width == P.compact_width(centred) and bpc == (width + 7) // 8, limit
        assert data[pos:] == P.compact_pack(centred, width), limit
        back = gpu.GpuDCRTPolyMatrix.from_compact_bytes(p, data)
        assert np.array_equal(back.to_rns(), res)
        # a matrix in the evaluation domain goes through the inverse transform first
        e = gpu.GpuDCRTPolyMatrix.from_rns(p, res, False).ensure_eval().to_compact_bytes()
        assert e[1] == 1 and e[2:] == data[2:]  # only the format tag differs
    flat = [c for row in m.coeffs() for poly in row for c in poly]
    assert flat == [v % Q for v in vals]
    for new_mod in (1 << 20, moduli[0]):
        sw = m.modulus_switch(new_mod).coeffs()
        # the params are unchanged: a switched value is stored mod Q (it wraps when new_mod > Q, as at 2 x 10 bits)
        want = [P.modulus_switch(v % Q, Q, new_mod) % Q for v in vals]
        assert [c for row in sw for poly in row for c in poly] == want


# ---------------------------------------------------------------------------------------------- samplers
SAMPLER_SEED = bytes((11 * i + 5) & 0xFF for i in range(32))

# (n, bits, base): limb widths the samplers had not run at; dpt = 2, 2, 1, 2, 2 (short last digit), ...
SAMPLER_CELLS = [(64, 10, 5), (64, 12, 6), (64, 12, 12), (256, 15, 13), (256, 17, 15), (256, 29, 15), (256, 31, 16),
                 (256, 32, 16), (256, 41, 20), (256, 58, 20)]


@pytest.mark.parametrize("n,bits,base", SAMPLER_CELLS)
def test_samplers_new_widths(gpu, oracle, hip_env, n, bits, base):
    moduli = _moduli(n, bits)
    p = _params(gpu, n, moduli, base)
    s = gpu.GpuRngSeed.from_bytes(SAMPLER_SEED)
    for dist, sigma in (("uniform", 0.0), ("gauss", 4.578), ("ternary", 0.0)):
        m = gpu.GpuDCRTPolyMatrix.sample_distribution(p, 2, 3, oracle.DIST[dist], sigma, s)
        assert np.array_equal(m.to_coeff_rns(), oracle.sample_distribution(2, 3, moduli, n, dist, sigma, s)), dist
    M = _patterns(moduli, n, SEED + base)[0][:4].reshape(2, 2, len(moduli), n)
    c = ((1 << base) + 1) * 4.578
    want = oracle.gauss_samp_gq(M, moduli, base, c, s)
    hip_env.unset("MXX_HIP_GSAMP")
    lanes = gpu.GpuDCRTPolyMatrix.from_rns(p, M, False).gauss_samp_gq_arb_base(c, 4.578, s)
    hip_env.set("MXX_HIP_GSAMP", "simple")
    simple = gpu.GpuDCRTPolyMatrix.from_rns(p, M, False).gauss_samp_gq_arb_base(c, 4.578, s)
    assert lanes == simple
    assert np.array_equal(lanes.to_coeff_rns(), want)
    if P.digits_per_tower(moduli, base) >= 2:
        G = gpu.GpuDCRTPolyMatrix.gadget_matrix(p, 2)
        assert G * lanes == gpu.GpuDCRTPolyMatrix.from_rns(p, M, False).ensure_eval()
    # dpt = 1: the sampler reproduces the reference's last-digit formula, which adds base * z
    # (trapdoor.hip:138; reference MatrixTrapdoor.cu:811-814), so G z = M does not hold there by design; oracle parity
    # and the agreement of the two kernel forms above are what is asserted.


def _descending_basis(n, bits, count):
    """The reference's basis rule: the largest primes = 1 (mod 2n) below 2^bits, descending (it does not stop at
    2^(bits-1): 32 limbs of 24 bits at n = 2^14 end at 9011201, just above it)."""
    out, q = [], (1 << bits) + 1
    while len(out) < count:
        q -= 2 * n
        if is_prime(q):
            out.append(q)
    return out


# one trapdoor per reference caller's (bits, base), at a reduced ring and depth: (n, depth, bits, base, d)
TRAPDOOR_CELLS = [(256, 3, 32, 16, 1), (256, 3, 28, 14, 1), (256, 4, 24, 12, 2), (4, 4, 12, 12, 1), (2, 2, 10, 5, 1),
                  (2, 1, 12, 6, 1), (4, 6, 18, 6, 1)]


@pytest.mark.parametrize("n,depth,bits,base,d", TRAPDOOR_CELLS)
def test_trapdoor_reference_parameter_sets(gpu, n, depth, bits, base, d):
    from mxx_amd.trapdoor import compute_preimage_norm

    moduli = _descending_basis(n, bits, depth)
    p = _params(gpu, n, moduli, base)
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, A = sampler.trapdoor(p, d)
    k = p.modulus_digits()
    rei = td.r.concat_rows([td.e, gpu.GpuDCRTPolyMatrix.identity(p, d * k)])
    assert A * rei == gpu.GpuDCRTPolyMatrix.gadget_matrix(p, d)
    if P.digits_per_tower(moduli, base) < 2:
        return  # dpt = 1: the G-sampler's base * z term (see test_samplers_new_widths) breaks A x = target by design
    target = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, d, 2, gpu.DistType.FinRingDist())
    x = sampler.preimage(p, td, A, target)
    assert A * x == target
    Q = p.modulus()
    worst = max(min(v, Q - v) for row in x.coeffs() for poly in row for v in poly)
    # where the bound exceeds Q / 2 (the 2 x 1 x 12-bit set: about 1.4e5 against 2046) it holds for any residue, so
    # that cell checks A x = target only
    assert 0 < worst < compute_preimage_norm(math.sqrt(n), d * k, float(1 << base))


def test_modulus_of_63_bits_is_refused_through_the_abi(gpu):
    """The widest class ends below 2^62: a 63-bit prime fails at context creation with the library's own message, not
    with wrong residues later."""
    from mxx_amd._ffi import GpuPolyError

    q = P.primes(4, 63, 1)[0]
    with pytest.raises(GpuPolyError, match=r"modulus must be < 2\^62"):
        gpu.GpuDCRTPolyParams(4, [q], 1)
    with pytest.raises(GpuPolyError, match=r"modulus must be < 2\^62"):
        gpu.GpuDCRTPolyParams(4, [P.primes(4, 61, 1)[0], q], 1)  # one such limb in an otherwise valid basis


# ---------------------------------------------------------------------------------------------- forced kernel paths
def _transform_pairs(moduli_of):
    """the pairs _check_transform asserts for a case, by the same predicate (_path_runs)"""
    def pair_fn(pair):
        def f(c):
            moduli = moduli_of(c)
            if pair[1] is not None and pair not in c.get("paths", _forced_paths(moduli)):
                return None
            return _path_runs(pair, c["n"], moduli)
        return f
    return {pair: pair_fn(pair) for pair in (("MXX_HIP_NTT_PATH", "generic"), ("MXX_HIP_NTT_PATH", "global"),
                                             ("MXX_HIP_NTT64", "int"), ("MXX_HIP_NTT64", None))}


def _class_of(moduli_of):
    return lambda c: ran.Launched.word_class(moduli_of(c))


_EDGE = lambda c: _moduli(c["n"], c["bits"])  # noqa: E731
_REFSET = lambda c: P.primes(c["n"], c["bits"], 2)  # noqa: E731 - the class of the set; its depth does not matter here
_MIXED = lambda c: _mixed_moduli(c["n"], c["widths"])  # noqa: E731
_CELL = lambda c: _cell_moduli(c["n"], c["spec"])  # noqa: E731

# test -> pairs -> case -> True (asserts that the forced kernel ran) / False (the kernel declines the case) / None (the
# case does not use the pair); evaluated over the parameter lists by tests/test_ran_table_host.py
FORCED = {
    "test_transform_edge_primes": {"cls": _class_of(_EDGE), "pairs": _transform_pairs(_EDGE)},
    "test_transform_reference_sets": {"cls": _class_of(_REFSET), "fixed": {"paths": [("MXX_HIP_NTT_PATH", "global")]},
                                      "pairs": _transform_pairs(_REFSET)},
    "test_transform_mixed_widths": {"cls": _class_of(_MIXED), "cases": [dict(n=n, widths=w) for n, w in MIXED_WIDTHS],
                                    "pairs": _transform_pairs(_MIXED)},
    "test_decompose": {"cls": _class_of(_CELL), "pairs": {
        ("MXX_HIP_DECOMPOSE_FUSED", None): lambda c: _fused_digits_accept(c["n"], _CELL(c)),
        ("MXX_HIP_DECOMPOSE_FUSED", "1"): lambda c: _fused_digits_accept(c["n"], _CELL(c)),
        ("MXX_HIP_DECOMPOSE_FUSED", "0"): lambda c: True}},
    "test_compact_bytes_coeffs_and_modulus_switch": {"pairs": {
        ("MXX_HIP_SERDE", None): lambda c: c["depth"] <= 16 if c["mode"] is None else None,
        ("MXX_HIP_SERDE", "general"): lambda c: c["depth"] <= 16 if c["mode"] == "general" else None}},
}
