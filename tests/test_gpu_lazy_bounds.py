"""GPU: every transform kernel shape with its own lazy-reduction schedule, driven by the worst-case inputs of
tests/lazymodel.py and held to plainref (tests/plainref.py) only.

Each case runs forward and inverse at a class edge - the largest prime below 2^bits and the smallest above
2^(bits-1) - on all q - 1, the forward path constructions (integer and double products), the inverse group search
and a uniform vector, and checks by name (the library's launch trace) that the family the case is about ran.  The
widths include both sides of every threshold the kernels are selected by (24 / 25 / 26, 28 / 29, 40 / 41, 49 / 50 / 51,
57 / 58): run against a library whose threshold is shifted by one bit, the cells beside it take the shifted path, and
tests/test_lazymodel.py states for each shift whether these vectors then fail (TIGHT forms at 29 bits) or the
shift is proven slack.
"""
import numpy as np
import pytest

import lazymodel as LM
import plainref as P

pytestmark = pytest.mark.gpu

SEED = 20261017
_PARAMS = {}
_ROOTS = {}


def _params(gpu, n, moduli):
    key = (n, tuple(moduli))
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, list(moduli), 1)
    return _PARAMS[key]


def _root(q, n):
    if (q, n) not in _ROOTS:
        _ROOTS[(q, n)] = P.min_root(q, n)
    return _ROOTS[(q, n)]


def _slots(n, q):
    """Every slot up to 1024 points for 32-bit moduli; plainref's big-integer path (64-bit moduli) costs n operations
    per slot and row, so those check 64 slots at small rings and 6 beyond 1024 points - the four ends of the
    bit-reversed order and two seeded ones."""
    wide = q >> 32 != 0
    if n <= 1024 and not wide:
        return list(range(n))
    rng = np.random.default_rng(SEED + n)
    count = 64 if n <= 1024 else (2 if wide else 12)
    return sorted({0, 1, n // 2, n - 1} | set(rng.integers(0, n, count).tolist()))


def _inputs(moduli, n, randoms=1, search=True):
    """(1, k, L, n): the candidate vectors of every limb (lazymodel.candidates)."""
    logn = n.bit_length() - 1
    rows = []
    for q in moduli:
        bits = q.bit_length()
        W = LM.word_size(bits)
        ip, cap = None, 31
        if search and 10 <= logn <= 17 and not (W == 64 and bits <= 51):
            ip = LM.int_schedule(W, logn)[2]
            cap = LM.TIGHT_CAP if W == 32 and 26 <= bits <= 28 else 31
        rows.append(LM.candidates(q, n, W, ip, cap, seed=SEED + bits, randoms=randoms, tries=12 if W == 32 else 4))
    k = min(len(r) for r in rows)
    return np.stack([r[:k] for r in rows], axis=1)[None]


def _ref(x2d, q, slots):
    return P.ntt_slots(x2d, [q] * x2d.shape[0], slots, [_root(q, x2d.shape[-1])] * x2d.shape[0])


def _traced(gpu, fn):
    from mxx_amd import _ffi

    gpu.gpu_device_sync()
    _ffi.trace_begin()
    out = fn()
    gpu.gpu_device_sync()
    return out, [t["kernel"] for t in _ffi.trace_end()]


def _check(gpu, moduli, n, x, fam, limbs=None):
    """Forward on the sampled slots equals plainref; the inverse of the same vectors as evaluation-domain inputs
    transforms back to them under plainref; the traced kernels carry the family's names."""
    p = _params(gpu, n, moduli)
    limbs = range(len(moduli)) if limbs is None else limbs
    slots = _slots(n, max(moduli))

    def fwd():
        m = gpu.GpuDCRTPolyMatrix.from_rns(p, x, False)
        m.ntt_all_in_place()
        return m.to_rns()

    def inv():
        m = gpu.GpuDCRTPolyMatrix.from_rns(p, x, True)
        m.intt_all_in_place()
        return m.to_rns()

    y, fnames = _traced(gpu, fwd)
    z, inames = _traced(gpu, inv)
    if fam is not None:
        assert any(fam[0] in k for k in fnames), (fam, fnames)
        assert any(fam[1] in k for k in inames), (fam, inames)
    k = x.shape[1]
    for l in limbs:
        q = moduli[l]
        # one plainref pass for both checks: the forward inputs and the inverse outputs stacked
        ref = _ref(np.concatenate([x[0, :, l], z[0, :, l]]), q, slots)
        assert np.array_equal(y[0, :, l][:, slots], ref[:k]), ("forward", q, n)
        assert np.array_equal(ref[k:], x[0, :, l][:, slots]), ("inverse", q, n)


def _edges(n, bits):
    return list(dict.fromkeys([P.primes(n, bits, 1)[0], P.primes(n, bits, 1, low=True)[0]]))


F64_SMALL = ("nttf::small_kernel", "nttf::small_kernel")
F64_LDS = ("nttf::fwd_kernel", "nttf::inv_kernel")
F64_SPLIT = ("nttf::head_kernel", "nttf::tail_kernel")
LDS = ("ntt_fwd_lazy_kernel", "ntt_inv_lazy_kernel")
NTT14 = ("ntt14::fwd_kernel", "ntt14::inv_kernel")
SPLIT = ("ntt_fwd_head_kernel", "ntt_inv_tail_kernel")

# (bits, logn, env, family): env = (name, value) or None; family None where the class has no lazy form
CELLS = [
    # double precision: small_kernel, whole vector, head / tail, at every ELIM edge
    (51, 8, None, F64_SMALL), (50, 9, None, F64_SMALL),
    (51, 10, None, F64_LDS), (51, 13, None, F64_LDS), (51, 14, None, F64_LDS),
    (50, 12, None, F64_LDS), (49, 12, None, F64_LDS), (41, 13, None, F64_LDS), (40, 13, None, F64_LDS),
    (51, 15, None, F64_SPLIT), (51, 16, None, F64_SPLIT), (51, 17, None, F64_SPLIT), (50, 16, None, F64_SPLIT),
    # 32-bit lazy and TIGHT forms, whole vector in LDS (2^10..2^13, 2^15)
    (25, 10, None, LDS), (25, 13, None, LDS), (25, 15, None, LDS), (26, 12, None, LDS), (26, 15, None, LDS),
    (28, 10, None, LDS), (28, 13, None, LDS), (28, 15, None, LDS), (29, 13, None, None), (29, 15, None, None),
    # 2^14: grouped signed / unsigned, whole
    (24, 14, None, NTT14), (25, 14, None, NTT14), (24, 14, ("MXX_HIP_NTT14", "unsigned"), NTT14),
    (24, 14, ("MXX_HIP_NTT14", "whole"), LDS), (26, 14, None, NTT14), (28, 14, None, NTT14),
    (28, 14, ("MXX_HIP_NTT14", "whole"), LDS), (29, 14, None, None),
    # split head / tail, 32-bit words
    (25, 16, None, SPLIT), (25, 17, None, SPLIT), (26, 16, None, SPLIT), (28, 16, None, SPLIT), (28, 17, None, SPLIT),
    (29, 16, None, None),
    # 64-bit integer lazy forms: whole vector, split from 2^15, and MXX_HIP_NTT64=int below 2^51
    (57, 10, None, LDS), (57, 14, None, LDS), (57, 15, None, SPLIT), (57, 16, None, SPLIT), (57, 17, None, SPLIT),
    (58, 13, None, None), (58, 16, None, None),
    (51, 12, ("MXX_HIP_NTT64", "int"), LDS), (51, 16, ("MXX_HIP_NTT64", "int"), SPLIT),
]


@pytest.mark.parametrize("bits,logn,env,fam", CELLS)
def test_transform_worst_case(gpu, hip_env, bits, logn, env, fam):
    n = 1 << logn
    if env:
        hip_env.set(*env)
    for q in _edges(n, bits):
        _check(gpu, [q], n, _inputs([q], n), fam)


# the fused product + inverse (gpupoly_matrix_mul_scalar_intt).  Its load is a Montgomery product, a w 2^-32, so the
# operand is a = c 2^32 w^-1 (lazymodel.mulw_operand): the butterflies then start from the constructed vector c itself,
# and the last stage's constants restore the 2^32 - the output is INTT(a o w) = INTT(c 2^32).
MULW_CELLS = [(25, 13), (24, 14), (25, 14), (28, 14), (26, 15), (28, 16), (25, 17), (28, 17)]


def _mulw_kernels(bits, logn):
    """The launches of the fused path (ntt_lds_u32.hip launch_mul_intt_u32); the fallback (ntt.hip: point-wise product
    then the plain inverse) adds an elementwise_kernel launch in front."""
    if logn >= 16:
        return ["ntt_inv_lazy_kernel", "ntt_inv_tail_kernel"]  # launch_split_mulw
    if logn == 14 and bits <= 25:
        return ["ntt14::inv_kernel"]  # grouped MULW kernel
    return ["ntt_inv_lazy_kernel"]  # launch_lazy_mulw


@pytest.mark.parametrize("bits,logn", MULW_CELLS)
def test_mul_scalar_intt_worst_case(gpu, bits, logn):
    n = 1 << logn
    for q in _edges(n, bits):
        p = _params(gpu, n, [q])
        c = _inputs([q], n)
        rng = np.random.default_rng(SEED + logn)
        w = rng.integers(1, q, n, dtype=np.uint64)
        a = LM.mulw_operand(c, w.reshape(1, 1, 1, n), q)
        assert np.array_equal(LM.mont_load(a, w.reshape(1, 1, 1, n), q), c)  # the kernel's load hands over c
        A = gpu.GpuDCRTPolyMatrix.from_rns(p, a, True)
        B = gpu.GpuDCRTPolyMatrix.from_rns(p, w.reshape(1, 1, 1, n), True)
        res, names = _traced(gpu, lambda: A.mul_scalar_intt(B))
        want = _mulw_kernels(bits, logn)
        assert len(names) == len(want) and all(k in name for k, name in zip(want, names)), (want, names)
        # the result is INTT(a o w) by definition; a o w = c 2^32 (mod q), the factor the last stage puts back
        out = res.to_rns()
        slots = _slots(n, q)
        prod = ((a[0, :, 0].astype(object) * w.astype(object)) % q).astype(np.uint64)
        assert np.array_equal(prod, ((c[0, :, 0].astype(object) * ((1 << 32) % q)) % q).astype(np.uint64))
        assert np.array_equal(_ref(out[0, :, 0], q, slots), prod[:, slots]), ("mul_scalar_intt", q, n)


# the reference callers' sets (n, limbs, bits) and M4's GGH15 chain ring (n = 256, 12 x 51-bit limbs)
REFERENCE_SETS = [(1 << 16, 64, 32, None), (1 << 14, 32, 24, NTT14), (1 << 16, 64, 28, SPLIT), (256, 12, 51, F64_SMALL)]


@pytest.mark.parametrize("n,depth,bits,fam", REFERENCE_SETS)
def test_reference_sets_worst_case(gpu, n, depth, bits, fam):
    moduli = P.primes(n, bits, depth)
    x = _inputs(moduli, n, randoms=0, search=False)
    _check(gpu, moduli, n, x, fam, limbs=[0, depth // 2, depth - 1])
