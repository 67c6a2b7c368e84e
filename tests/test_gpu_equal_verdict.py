"""gpu_matrix_equal against host ground truth.

About fifteen test files rest on "the fused entry equals the literal sequence, bit for bit" through this one function
(their `_equal` helpers and GpuDCRTPolyMatrix.__eq__).  Here its verdict is held to numpy's on operands that reach the
device through from_rns alone, so a planted difference depends on no other device operation: every word position of a
small matrix, every bit range of a word, the wave / block / grid-stride edges of equal_kernel (arith.hip: 8192 blocks of
256 threads, an early exit per wave, one atomicOr per wave into a 4-byte flag from the context's block cache), the
extent of views and of matrices below the top level, PACKED24 operands, and the tag checks that return before a launch.

A "difference" is one word replaced by another canonical residue of the same limb.  Every case runs in a 32-bit context
(24-bit moduli) and a 64-bit context (51-bit moduli), calls the C entry and the mirror's `==`, and the two must agree.
"""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from mxx_amd import _ffi

pytestmark = pytest.mark.gpu

SEED = 20261020
CLASSES = [pytest.param(24, id="u32"), pytest.param(51, id="u64")]
GRID_WORDS = 8192 * 256  # one full sweep of equal_kernel's capped grid

_PARAMS = {}


def _params(gpu, n, bits, depth, base=4):
    key = (n, bits, depth, base)
    if key not in _PARAMS:
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, P.primes(n, bits, depth), base)
    return _PARAMS[key]


def _random(rng, rows, cols, moduli, n):
    """(rows, cols, L, n) canonical residues: word w of the flat array is word w of the device matrix"""
    return np.stack([rng.integers(0, int(q), (rows, cols, n), dtype=np.uint64) for q in moduli], axis=2)


def _limb_of(host, w):
    return (w // host.shape[3]) % host.shape[2]


def _perturbed(host, moduli, words, delta=None):
    """a copy of `host` whose flat words `words` are other canonical residues of their limbs (old + delta mod q)"""
    out = host.copy()
    flat = out.reshape(-1)
    for w in words:
        q = int(moduli[_limb_of(host, w)])
        d = 1 + (w * 2654435761 + 12345) % (q - 1) if delta is None else delta
        assert 0 < d < q
        flat[w] = (int(flat[w]) + d) % q
    assert all(out.reshape(-1)[w] != host.reshape(-1)[w] for w in words)
    return out


def _verdict(a, b):
    """the C entry's out_equal; the mirror's == must say the same"""
    eq = C.c_int(7)
    assert _ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)) == 0, _ffi.last_error_string()
    assert eq.value in (0, 1)
    assert (a == b) is bool(eq.value), "GpuDCRTPolyMatrix.__eq__ disagrees with gpu_matrix_equal"
    return bool(eq.value)


def _both_orders(a, b):
    v = _verdict(a, b)
    assert _verdict(b, a) is v, "the verdict depends on the argument order"
    return v


def _up(gpu, p, host, ev=True):
    return gpu.GpuDCRTPolyMatrix.from_rns(p, host, ev)


# ------------------------------------------------------------------------------------------------ 1. every position
@pytest.mark.parametrize("bits", CLASSES)
def test_every_word_position_of_a_small_matrix(gpu, bits):
    """3 x 5 at n = 16, L = 3: 720 words, each perturbed in turn; both argument orders; a second allocation with the same
    content compares equal."""
    n, L = 16, 3
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    host = _random(np.random.default_rng(SEED + bits), 3, 5, moduli, n)
    assert host.size == 720
    a = _up(gpu, p, host)
    twin = _up(gpu, p, host.copy())
    assert twin.raw.value != a.raw.value
    assert _both_orders(a, twin) is True
    missed = [w for w in range(host.size) if _both_orders(a, _up(gpu, p, _perturbed(host, moduli, [w])))]
    assert not missed, f"equal although word(s) {missed} differ"
    assert _both_orders(a, twin) is True


# ------------------------------------------------------------------------------------------------ 2. which bits
@pytest.mark.parametrize("bits,delta", [(24, 1), (24, 1 << 23), (51, 1), (51, 1 << 31), (51, 1 << 32), (51, 1 << 50)])
def test_a_difference_in_any_bit_range_of_a_word(gpu, bits, delta):
    """one word 0 against exactly `delta` (a single bit, below q): the low bit, the top bit of the low half, the low bit of
    the upper half and the top bit of a 51-bit residue; at the first, a middle and the last word"""
    n, L = 16, 3
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    assert all(delta < q for q in moduli) and all(q.bit_length() == bits for q in moduli)
    host = _random(np.random.default_rng(SEED + 1), 2, 3, moduli, n)
    for w in (0, host.size // 2 + 5, host.size - 1):
        base = host.copy()
        base.reshape(-1)[w] = 0
        other = _perturbed(base, moduli, [w], delta)
        assert int(other.reshape(-1)[w]) == delta
        assert _both_orders(_up(gpu, p, base), _up(gpu, p, other)) is False, (w, delta)
        assert _both_orders(_up(gpu, p, base), _up(gpu, p, base.copy())) is True


# ------------------------------------------------------------------------------------------------ 3. wave, block, grid edges
@pytest.mark.parametrize("bits", CLASSES)
@pytest.mark.parametrize("total", [2, 62, 64, 66, 254, 256, 258, 510, 512, 514])
def test_wave_and_block_edges(gpu, bits, total):
    """1 x k at n = 2, L = 1: word counts around one wave, one block and two blocks; the difference at word 0, at the last
    word, and in every word"""
    n = 2
    p = _params(gpu, n, bits, 1)
    moduli = p.moduli()
    host = _random(np.random.default_rng(SEED + total), 1, total // n, moduli, n)
    assert host.size == total
    a = _up(gpu, p, host)
    assert _both_orders(a, _up(gpu, p, host.copy())) is True
    for words in ([0], [total - 1], list(range(total))):
        assert _both_orders(a, _up(gpu, p, _perturbed(host, moduli, words))) is False, (total, words[:2])


@pytest.mark.parametrize("bits", CLASSES)
def test_just_over_one_grid_sweep(gpu, bits):
    """1 x 1025 at n = 1024, L = 2: 2 099 200 words, 2 048 past the 8192 x 256 threads of the capped grid, so the first
    2 048 threads take a second trip.  The difference at word 0, at the last word of the first sweep, at the first word
    of the second, in the middle, at the last word, and in every word."""
    n, L, cols = 1024, 2, 1025
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    host = _random(np.random.default_rng(SEED + 3), 1, cols, moduli, n)
    total = host.size
    assert GRID_WORDS < total == 2_099_200
    a = _up(gpu, p, host)
    assert _both_orders(a, _up(gpu, p, host.copy())) is True
    for w in (0, GRID_WORDS - 1, GRID_WORDS, total // 2 + 77, total - 1):
        assert _both_orders(a, _up(gpu, p, _perturbed(host, moduli, [w]))) is False, w
    qv = np.asarray(moduli, dtype=np.uint64).reshape(1, 1, L, 1)
    every = (host + np.uint64(1)) % qv
    assert not (every == host).any()
    assert _both_orders(a, _up(gpu, p, every)) is False
    assert _both_orders(a, _up(gpu, p, host.copy())) is True


# ------------------------------------------------------------------------------------------------ 4. the flag
@pytest.mark.parametrize("bits", CLASSES)
def test_the_flag_is_fresh_on_every_call(gpu, bits):
    """unequal, equal, unequal x 3, equal, equal on one context: the 4-byte flag block goes back to the context's cache
    holding 1 after every "not equal" and must be cleared before the next kernel reads it"""
    n, L = 16, 3
    p = _params(gpu, n, bits, L)
    moduli = p.moduli()
    host = _random(np.random.default_rng(SEED + 4), 2, 2, moduli, n)
    a, same = _up(gpu, p, host), _up(gpu, p, host.copy())
    others = [_up(gpu, p, _perturbed(host, moduli, [w])) for w in (0, 100, host.size - 1)]
    sequence = [others[0], same, others[0], others[1], others[2], same, same]
    want = [np.array_equal(host, m.to_rns()) for m in sequence]
    assert want == [False, True, False, False, False, True, True]
    assert [_verdict(a, m) for m in sequence] == want


# ------------------------------------------------------------------------------------------------ 5. views and levels
def _view_cases(host, first_row, last_row):
    """(flat word of the 4 x 3 parent, whether it lies in rows [first_row, last_row))"""
    row_words = host[0].size
    return [(first_row * row_words - 1, False), (last_row * row_words, False), (first_row * row_words, True),
            (last_row * row_words - 1, True)]


@pytest.mark.parametrize("bits", CLASSES)
@pytest.mark.parametrize("kind", ["row_view", "reshape_view", "row_view_level_0", "reshape_view_level_0"])
def test_extent_of_views_and_levels(gpu, bits, kind):
    """Rows [1, 3) of a 4 x 3 parent, as a row view and as a 3 x 2 reshape view of that row view, at the top level and
    at level 0 of a depth-3 context (words = polys x n there): equal to from_rns of those rows; a difference in the
    parent one word before or after the view changes nothing, one at the view's first or last word does."""
    n, depth = 16, 3
    p = _params(gpu, n, bits, depth)
    L = 1 if kind.endswith("level_0") else depth
    moduli = p.moduli()[:L]
    host = _random(np.random.default_rng(SEED + 5), 4, 3, moduli, n)

    def view_of(parent_host):
        parent = _up(gpu, p, parent_host)
        assert parent.level == L - 1
        v = parent.row_view(1, 3)
        return v.reshape_view(3, 2) if kind.startswith("reshape") else v

    want_host = host[1:3].reshape(3, 2, L, n) if kind.startswith("reshape") else host[1:3]
    want = _up(gpu, p, np.ascontiguousarray(want_host))
    assert _both_orders(view_of(host), want) is True
    for w, inside in _view_cases(host, 1, 3):
        assert _both_orders(view_of(_perturbed(host, moduli, [w])), want) is (not inside), (kind, w, inside)
    # the whole parent under another shape: its extent is the parent's
    whole = _up(gpu, p, host)
    flat = _up(gpu, p, host.reshape(2, 6, L, n))
    assert _both_orders(whole.reshape_view(2, 6), flat) is True
    for w in (0, host.size - 1):
        assert _both_orders(_up(gpu, p, _perturbed(host, moduli, [w])).reshape_view(2, 6), flat) is False, w


# ------------------------------------------------------------------------------------------------ 6. layouts
def _uniform(gpu, p, hip_env, packed):
    seed = gpu.GpuRngSeed.from_bytes(bytes((37 * i + 11) & 0xFF for i in range(32)))
    if not packed:
        hip_env.set("MXX_HIP_PACK24", "0")
    m = gpu.GpuDCRTPolyMatrix.sample_distribution(p, 2, 3, gpu.DistType.FinRingDist().as_ffi(), 0.0, seed)
    if not packed:
        hip_env.unset("MXX_HIP_PACK24")
    assert m.layout == ("packed24" if packed else "words")
    return m


def test_packed24_operands(gpu, hip_env):
    """a PACKED24 uniform sample against its words twin, in both orders, and against a second packed sample of the same
    seed: equal, and the packed operand ends as words; a from_rns copy with its last word perturbed: not equal.  Every
    case samples afresh - a compared matrix is unpacked."""
    n, L = 1024, 3
    p = _params(gpu, n, 24, L)
    moduli = p.moduli()
    for lhs_packed, rhs_packed in ((True, False), (False, True), (True, True)):
        a, b = _uniform(gpu, p, hip_env, lhs_packed), _uniform(gpu, p, hip_env, rhs_packed)
        assert _verdict(a, b) is True, (lhs_packed, rhs_packed)
        assert a.layout == "words" and b.layout == "words"
    host = _uniform(gpu, p, hip_env, False).to_rns()
    other = _up(gpu, p, _perturbed(host, moduli, [host.size - 1]))
    assert _verdict(_uniform(gpu, p, hip_env, True), other) is False
    assert _verdict(other, _uniform(gpu, p, hip_env, True)) is False
    same = _up(gpu, p, host)
    packed = _uniform(gpu, p, hip_env, True)
    assert _verdict(packed, same) is True and packed.layout == "words"


# ------------------------------------------------------------------------------------------------ 7. tags and shapes
@pytest.mark.parametrize("bits", CLASSES)
def test_tag_and_shape_mismatches_return_before_any_launch(gpu, bits):
    n, depth = 16, 3
    p = _params(gpu, n, bits, depth)
    other_ctx = _params(gpu, n, bits, depth, base=5)  # the same moduli in a context of its own
    assert other_ctx.ctx_raw().value != p.ctx_raw().value
    moduli = p.moduli()
    # words below every modulus, so that the same flat words are canonical under any shape and level
    words = np.random.default_rng(SEED + 7).integers(0, min(moduli), 6 * depth * n, dtype=np.uint64)
    a = _up(gpu, p, words.reshape(2, 3, depth, n))
    lib = _ffi.lib()

    def refused(x, y):
        eq = C.c_int(7)
        c0 = lib.gpupoly_launch_count()
        st = lib.gpu_matrix_equal(x.raw, y.raw, C.byref(eq))
        assert lib.gpupoly_launch_count() == c0, "a mismatch of tags or shapes must not launch"
        assert st == 0 and eq.value == 0
        assert (x == y) is False

    for x, y in ((a, _up(gpu, p, words.reshape(3, 2, depth, n))),                       # shape
                 (a, _up(gpu, p, words.reshape(2, 3, depth, n)[:, :, :2].copy())),      # level, the same shape
                 (_up(gpu, p, words[:6 * n].reshape(1, 2, 3, n)), _up(gpu, p, words[:6 * n].reshape(1, 3, 2, n))),  # level, the same words
                 (a, _up(gpu, p, words.reshape(2, 3, depth, n), ev=False)),             # format tag
                 (a, _up(gpu, other_ctx, words.reshape(2, 3, depth, n)))):              # context
        refused(x, y)
        refused(y, x)
    same = _up(gpu, p, words.reshape(2, 3, depth, n))
    c0 = lib.gpupoly_launch_count()
    assert _verdict(a, same) is True
    assert lib.gpupoly_launch_count() > c0  # the counter does move when the kernel runs
    # null arguments: an error, and "not equal" where the verdict could be written
    assert lib.gpu_matrix_equal(a.raw, same.raw, None) != 0
    for x, y in ((None, same.raw), (a.raw, None), (None, None)):
        eq = C.c_int(7)
        assert lib.gpu_matrix_equal(x, y, C.byref(eq)) != 0 and eq.value == 0


# ------------------------------------------------------------------------------------------------ 8. property check
@pytest.mark.parametrize("bits", CLASSES)
def test_random_pairs_agree_with_numpy(gpu, bits):
    """200 seeded pairs of random small shapes (at most 1 000 words, any level of a depth-3 context): half identical, half
    with 1 to 3 planted differences; verdict == array_equal of what the device holds == the host arrays' comparison"""
    rng = np.random.default_rng(SEED + bits)
    seen = {True: 0, False: 0}
    for i in range(200):
        n = int(rng.choice([2, 4, 8, 16]))
        L = int(rng.integers(1, 4))
        while True:
            rows, cols = int(rng.integers(1, 9)), int(rng.integers(1, 9))
            if rows * cols * L * n <= 1000:
                break
        p = _params(gpu, n, bits, 3)
        moduli = p.moduli()[:L]
        host = _random(rng, rows, cols, moduli, n)
        other = host.copy()
        if i % 2:
            planted = sorted(set(rng.integers(0, host.size, int(rng.integers(1, 4))).tolist()))
            other = _perturbed(host, moduli, planted)
        ev = bool(rng.integers(0, 2))
        a, b = _up(gpu, p, host, ev), _up(gpu, p, other, ev)
        want = np.array_equal(host, other)
        assert want is (i % 2 == 0)
        assert np.array_equal(a.to_rns(), b.to_rns()) is want
        assert _both_orders(a, b) is want, (i, host.shape, np.flatnonzero(host.reshape(-1) != other.reshape(-1)).tolist())
        seen[want] += 1
    assert seen == {True: 100, False: 100}
