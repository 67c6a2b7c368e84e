"""GPU: the preimage targets of many LUT rows of one column chunk of the LWE public lookup in one call
(`gpupoly_matrix_lwe_targets`, mxx_amd/lwe_lookup.py).

Everything in the target formula is exact arithmetic on canonical residues, so the bar is equality, bit for bit
(gpu_matrix_equal), with `build_adjusted_target_chunk` - the reference's function (src/lookup/lwe/pubkey_gpu.rs:193-222)
restated with the mirror's older operations, one row at a time.  That literal target is computed once per (context, d, chunk,
entry, x, y) and shared by the row counts.  Independently of the engine the same targets are computed with tests/plainref.py
fed with the CPU restatement's samples from the ORIGINAL formula (A_z - G o x) D, which the entry never evaluates: it reads
x U off the digits, so the comparison also proves G G^-1(U) = U.  The combine kernel alone
(`gpupoly_matrix_lwe_targets_combine`, which takes the digits and the product as given) is held to plainref in every modulus
width class with operands no sampler produces: every residue of A_lt and of the digits q - 1, a product of zeros (entering as
q), y = 2^(bits - 1) - 1 and, for every limb and digit, a row whose weight there is q - 1 - dpt products of (q - 1)^2 and
two addends of q on top of q - 1, the lazy accumulator's bound (the largest 31-bit limbs hold 4 terms: exactly dpt = 2 and
the two addends, and the second base there, dpt = 6, folds inside the sum; the any-dpt form also runs at 62 bits, dpt = 11).
End to end, K_high chunks sampled for the targets satisfy the lookup relation exactly."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import BASES, CLASSES, _cell, _eval_slots, _params, _rand, _top
from test_gpu_lut_targets import CONTEXTS, full_modulus, y_values

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_lwe_targets"
COMBINE = "gpupoly_matrix_lwe_targets_combine"
KEY = bytes((11 * i + 6) & 0xFF for i in range(32))
GATE_ID, LUT_ID, SLOT = 17, 3, 2
XS = (0, 1, (1 << 32) + 5, (1 << 64) - 1)  # the last one exceeds every q
ENTRIES = (7, 3, 7, 100, 12)  # they repeat and are not consecutive
_SHARED, _LITERAL = {}, {}


def shared_of(gpu, oracle, ctx, d):
    from mxx_amd import lwe_lookup

    if (ctx, d) not in _SHARED:
        p = make_params(gpu, oracle, *CONTEXTS[ctx])
        moduli, n, m = p.moduli(), p.ring_dimension(), d * p.modulus_digits()
        a_z = gpu.GpuDCRTPolyMatrix.from_rns(p, oracle.random_matrix(500 + 10 * d, d, m, moduli, n), True)
        a_lt = lwe_lookup.derive_a_lt_matrix(p, d, KEY, GATE_ID, SLOT)
        _SHARED[(ctx, d)] = lwe_lookup.LweShared(p, KEY, GATE_ID, LUT_ID, SLOT, a_z, a_lt)
    return _SHARED[(ctx, d)]


def literal(gpu, oracle, ctx, d, chunk, row):
    from mxx_amd import lwe_lookup

    key = (ctx, d, chunk, row)
    if key not in _LITERAL:
        _LITERAL[key] = lwe_lookup.build_adjusted_target_chunk(shared_of(gpu, oracle, ctx, d), *row, *chunk)
    return _LITERAL[key]


def chunks_of(p, d):
    dpt = -(-p.crt_bits() // p.base_bits())
    k = p.modulus_digits()
    m = d * k
    out = {"first": (0, min(4, m)), "across a tower": (dpt - 1, 2), "ragged last": (m - 1, 1)}
    if d > 1:
        out["across a source row"] = (k - 1, 2)
    return out


def rows_of(moduli, T):
    """(entry, x, y): every (x, y) pair within 20 rows; tags repeat with the entries"""
    ys = y_values(moduli)
    return [(ENTRIES[t % 5], XS[t % 4], ys[t % 5]) for t in range(T)]


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal function; 2. a group boundary
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_one_call_equals_the_literal_function_row_by_row(gpu, oracle, ctx, d):
    from mxx_amd import lwe_lookup

    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    assert sh.a_lt == gpu.GpuDCRTPolyHashSampler().sample_hash(p, KEY, f"A_LT_{GATE_ID}_slot{SLOT}".encode(), d, sh.m_g, gpu.DistType.FinRingDist())
    for name, chunk in chunks_of(p, d).items():
        for T in (1, 3, 65):
            rows = rows_of(p.moduli(), T)
            got = lwe_lookup.lwe_target_chunks(sh, rows, chunk)
            assert len(got) == T
            for t, row in enumerate(rows):
                assert got[t].size() == (d, chunk[1]) and got[t].is_ntt
                assert got[t] == literal(gpu, oracle, ctx, d, chunk, row), f"{name} chunk {chunk}, row {t} of {T}: (entry, x, y) = {row}"
        # the same rows in another order: every row's target is its own
        rows = rows_of(p.moduli(), 7)[::-1]
        for row, target in zip(rows, lwe_lookup.lwe_target_chunks(sh, rows, chunk)):
            assert target == literal(gpu, oracle, ctx, d, chunk, row), (name, row)
    assert lwe_lookup.lwe_target_chunks(sh, [], chunks_of(p, d)["first"]) == []


def test_a_row_group_boundary_inside_the_call(gpu, oracle):
    """More rows than one group's digit scratch holds cannot be reached with test-sized operands (the cap is 1 GiB); the rows
    of a second call continue the first one's, which is what a group boundary does inside the entry: tags, constants and
    outputs start at the group's first row."""
    from mxx_amd import lwe_lookup

    sh = shared_of(gpu, oracle, "n16_51", 2)
    chunk = (5, 3)
    rows = rows_of(sh.params.moduli(), 9)
    whole = lwe_lookup.lwe_target_chunks(sh, rows, chunk)
    parts = lwe_lookup.lwe_target_chunks(sh, rows[:4], chunk) + lwe_lookup.lwe_target_chunks(sh, rows[4:], chunk)
    assert len(whole) == len(parts) == 9
    for a, b in zip(whole, parts):
        assert a == b


# ---------------------------------------------------------------------------------------------------
# 3. independence from the engine: plainref fed with the CPU restatement's samples, the ORIGINAL formula
# ---------------------------------------------------------------------------------------------------
def gadget_slots(moduli, base, n, d):
    """G_d in the evaluation domain, (d, d k, L, n): its entries are constants, their own transform"""
    G = P.gadget(d, moduli, base, n)
    assert not G[..., 1:].any()
    return np.broadcast_to(G[..., :1], G.shape).copy()


def times_constant(a, value, moduli):
    """a o value for an integer constant, limb by limb"""
    L = len(moduli)
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    v_col = np.asarray([int(value) % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    return ((a.astype(object) * v_col) % q_col).astype(np.uint64)


def minus(a, b, moduli):
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, len(moduli), 1)
    return ((a.astype(object) - b.astype(object)) % q_col).astype(np.uint64)


@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_targets_equal_the_plain_reference(gpu, oracle, ctx):
    from mxx_amd import lwe_lookup

    d, T = 2, 3
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k = L * dpt
    m = d * k
    slots = list(range(n))
    a_z, a_lt = sh.a_z.to_rns(), sh.a_lt.to_rns()
    G = gadget_slots(moduli, base, n, d)
    for chunk in ((0, 4), (k - 1, 2)):
        cols = slice(chunk[0], chunk[0] + chunk[1])
        rows = rows_of(moduli, 20)[7:7 + T]  # x 2^64 - 1 with Q - 1, x 0 with Q + 5, x 1 with the three-word y
        got = lwe_lookup.lwe_target_chunks(sh, rows, chunk)
        for (entry, x, y), target in zip(rows, got):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, sh.tag(entry)),
                                           full_ncol=m, col_offset=chunk[0])
            v = np.zeros((m, chunk[1], L, n), dtype=np.uint64)
            for r in range(d):
                for cc in range(chunk[1]):
                    v[r * k:(r + 1) * k, cc] = _eval_slots(P.digits(u[r, cc], moduli, base, dpt), moduli, slots)
            ext = minus(a_z, times_constant(G, x, moduli), moduli)  # A_z - G o x
            addend = minus(a_lt[:, cols], times_constant(G[:, cols], y, moduli), moduli)  # A_lt[:, chunk] - G[:, chunk] o y
            want = P.slot_mul_sum(addend, [ext], [v], moduli, True)
            assert np.array_equal(target.to_rns(), want), (ctx, chunk, entry, x, y)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """Both operands and the outputs at level 0 / 1 of a three-limb context: m = d * dpt * (level + 1) with dpt from the
    CONTEXT's crt_bits (one width per basis here, so plainref derives the same dpt from the truncated basis), the hashed
    samples of limbs 0..level only, and the plain reference above handed moduli[: level + 1]; then the combine alone."""
    n, d, T = 16, 2, 3
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    m = d * k
    slots = list(range(n))
    a_z, a_lt = oracle.random_matrix(540 + level, d, m, moduli, n), oracle.random_matrix(545 + level, d, m, moduli, n)
    g_az, g_alt = M.from_rns(p, a_z, True), M.from_rns(p, a_lt, True)
    G = gadget_slots(moduli, base, n, d)
    tag = lambda entry: f"lwe_low_level_{entry}".encode("ascii")  # noqa: E731
    for chunk in ((0, min(4, m)), (k - 1, 2)):
        cols = slice(chunk[0], chunk[0] + chunk[1])
        rows = rows_of(moduli, 20)[7:7 + T]
        got = M.lwe_targets(g_az, g_alt, chunk[0], chunk[1], [y for _, _, y in rows], [x for _, x, _ in rows], KEY, [tag(e) for e, _, _ in rows])
        for (entry, x, y), target in zip(rows, got):
            assert target.level == level and target.is_ntt and target.size() == (d, chunk[1])
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tag(entry)),
                                           full_ncol=m, col_offset=chunk[0])
            v = np.zeros((m, chunk[1], L, n), dtype=np.uint64)
            for r in range(d):
                for cc in range(chunk[1]):
                    v[r * k:(r + 1) * k, cc] = _eval_slots(P.digits(u[r, cc], moduli, base, dpt), moduli, slots)
            ext = minus(a_z, times_constant(G, x, moduli), moduli)
            addend = minus(a_lt[:, cols], times_constant(G[:, cols], y, moduli), moduli)
            want = P.slot_mul_sum(addend, [ext], [v], moduli, True)
            assert np.array_equal(target.to_rns(), want), (bits, level, chunk, entry, x, y)
    rng = np.random.default_rng(2100 + bits + level)
    digits, prod = _rand(rng, m, T * m, moduli, n), _rand(rng, d, T * m, moduli, n)
    ys = [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(T)]
    xs = [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(T)]
    got = combine(gpu, p, a_lt, digits, prod, T, 0, m, ys, xs)
    for t in range(T):
        block = slice(t * m, (t + 1) * m)
        addend = minus(minus(a_lt, times_constant(G, ys[t], moduli), moduli), prod[:, block], moduli)
        want = P.slot_mul_sum(addend, [times_constant(G, xs[t], moduli)], [digits[:, block]], moduli, False)
        assert np.array_equal(got[t], want), (bits, level, t)


# ---------------------------------------------------------------------------------------------------
# 4. the combine alone at the accumulator's bound, in every width class
# ---------------------------------------------------------------------------------------------------
def combine(gpu, p, a_lt, digits, prod, T, col_start, c, ys, xs):
    """gpupoly_matrix_lwe_targets_combine over uploaded residues -> the T outputs' residues"""
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    ops = [M.from_rns(p, np.ascontiguousarray(a), True) for a in (a_lt, digits, prod)]
    outs = [M(p, a_lt.shape[0], c, a_lt.shape[2] - 1, False) for _ in range(T)]
    words = [M._int_words(y) for y in ys]
    wpy = max(len(w) for w in words)
    y_arr = np.zeros((T, wpy), dtype=np.uint64)
    for t, w in enumerate(words):
        y_arr[t, :len(w)] = w
    x_arr = np.array(xs, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    st = _ffi.lib().gpupoly_matrix_lwe_targets_combine(M._raw_array(outs), T, ops[0].raw, ops[1].raw, ops[2].raw, col_start, p.base_bits(),
                                                       y_arr.ctypes.data_as(u64p), wpy, x_arr.ctypes.data_as(u64p))
    _ffi.check_status(st, COMBINE)
    for o in outs:
        o.is_ntt = True  # the entry tags its outputs EVAL
    return [o.to_rns() for o in outs]


@pytest.mark.parametrize("bits", CLASSES)
def test_combine_kernel_alone_in_every_width_class(gpu, bits):
    n, moduli, bases, slots = _cell(("class", bits))
    L = len(moduli)
    for base in BASES[bits]:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        d, k = 1, L * dpt
        m = d * k  # the chunk is every (tower, digit) column
        G = gadget_slots(moduli, base, n, d)
        # worst case: row (l, e) has x = (q_l - 1) B^(-e) mod q_l, whose weight for digit e is q_l - 1 in limb l; y = 2^(bits - 1) - 1
        # is below every modulus of the class
        xs = [(int(q) - 1) * pow(pow(2, base * e, int(q)), -1, int(q)) % int(q) for q in moduli for e in range(dpt)]
        for l, q in enumerate(moduli):
            for e in range(dpt):
                assert xs[l * dpt + e] * pow(2, base * e, int(q)) % int(q) == int(q) - 1
        T = len(xs)
        ys = [(1 << (bits - 1)) - 1] * T
        rng = np.random.default_rng(2000 + bits)
        for kind in ("top", "random"):
            if kind == "top":
                a_lt, digits, prod = _top(d, m, moduli, n), _top(m, T * m, moduli, n), np.zeros((d, T * m, L, n), dtype=np.uint64)
            else:
                a_lt, digits, prod = _rand(rng, d, m, moduli, n), _rand(rng, m, T * m, moduli, n), _rand(rng, d, T * m, moduli, n)
                ys = [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(T)]
                xs = [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(T)]
            got = combine(gpu, p, a_lt, digits, prod, T, 0, m, ys, xs)
            for t in range(T):
                block = slice(t * m, (t + 1) * m)
                addend = minus(minus(a_lt, times_constant(G, ys[t], moduli), moduli), prod[:, block], moduli)
                want = P.slot_mul_sum(addend, [times_constant(G, xs[t], moduli)], [digits[:, block]], moduli, False, slots)  # + (G o x) digits
                assert np.array_equal(got[t][..., slots], want), (bits, base, kind, t)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(got[t], np.broadcast_to(want[..., :1], got[t].shape)), (bits, base, t)


# ---------------------------------------------------------------------------------------------------
# 5. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi, lwe_lookup
    from mxx_amd.matrix import hash_tags_arg

    ctx, d = "n16_24", 2
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m, c, T = sh.m_g, 2, 3
    top = len(moduli) - 1
    sentinel = oracle.random_matrix(93, d, c, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    u64p = C.POINTER(C.c_uint64)
    y_arr = np.arange(1, 2 * T + 1, dtype=np.uint64)
    x_arr = np.arange(T, dtype=np.uint64)
    arg, keep, _ = hash_tags_arg(KEY, sh.tags([4, 9, 4]))
    bad_form, keep2, _ = hash_tags_arg(KEY, sh.tags([4, 9, 4]))
    bad_form.form = 9
    ws = dict(a_z=sh.a_z, a_lt=sh.a_lt)
    coeff_w = sh.a_z.clone()
    coeff_w.intt_all_in_place()
    low = M(p, d, m, 0, True)
    narrow = M(p, d, m - 1, top, True)
    foreign = M(other, d, d * other.modulus_digits(), top, True)
    digits = M.from_rns(p, oracle.random_matrix(95, m, T * c, moduli, n), True)
    product = M.from_rns(p, oracle.random_matrix(96, d, T * c, moduli, n), True)

    def raw_outs(outs, arr=True):
        return None if not arr else (C.c_void_p * max(len(outs), 1))(*[None if o is None else o.raw.value for o in outs])

    def call(outs, T_=T, col_start=1, base_bits=base, y=y_arr, wpy=2, x=x_arr, tags=arg, arr=True, **over):
        w = dict(ws, **over)
        return lib.gpupoly_matrix_lwe_targets(raw_outs(outs, arr), T_, *[None if w[name] is None else w[name].raw for name in ("a_z", "a_lt")],
                                              col_start, base_bits, None if y is None else y.ctypes.data_as(u64p), wpy,
                                              None if x is None else x.ctypes.data_as(u64p), None if tags is None else C.byref(tags))

    def call_combine(outs, T_=T, col_start=1, base_bits=base, y=y_arr, wpy=2, x=x_arr, arr=True, **over):
        w = dict(a_lt=sh.a_lt, digits=digits, product=product)
        w.update(over)
        return lib.gpupoly_matrix_lwe_targets_combine(raw_outs(outs, arr), T_, *[None if w[name] is None else w[name].raw for name in ("a_lt", "digits", "product")],
                                                      col_start, base_bits, None if y is None else y.ctypes.data_as(u64p), wpy,
                                                      None if x is None else x.ctypes.data_as(u64p))

    def view_of(w):
        return w.reshape_view(d * m // c, c)

    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null y_words": (lambda o: call(o, y=None), "null"),
        "null x": (lambda o: call(o, x=None), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "null a_z": (lambda o: call(o, a_z=None), "null"),
        "null a_lt": (lambda o: call(o, a_lt=None), "null"),
        "context mismatch": (lambda o: call(o, a_z=foreign), "mismatch"),
        "output of another context": (lambda o: call([o[0], M(other, d, c, top, True), o[2]]), "mismatch"),
        "level mismatch": (lambda o: call(o, a_z=low), "mismatch"),
        "output level": (lambda o: call([o[0], o[1], M(p, d, c, 0, True)]), "mismatch"),
        "operand shape": (lambda o: call(o, a_z=narrow), "shape"),
        "a_lt shape": (lambda o: call(o, a_lt=narrow), "shape"),
        "output rows": (lambda o: call([o[0], o[1], M(p, d + 1, c, top, True)]), "shape"),
        "operand not EVAL": (lambda o: call(o, a_z=coeff_w), "Eval"),
        "a_lt not EVAL": (lambda o: call(o, a_lt=coeff_w), "Eval"),
        "chunk past m": (lambda o: call(o, col_start=m - 1), "past"),
        "col_start past m": (lambda o: call(o, col_start=m + 1), "past"),
        "outputs of different widths": (lambda o: call([o[0], o[1], M(p, d, c + 1, top, True)]), "width"),
        "words_per_y 0": (lambda o: call(o, wpy=0), "words_per_y"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "output overlaps a_z": (lambda o: call([o[0], view_of(sh.a_z).row_view(0, d), o[2]]), "overlap"),
        "output overlaps a_lt": (lambda o: call([view_of(sh.a_lt).row_view(d, 2 * d), o[1], o[2]]), "overlap"),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
    }
    combine_cases = {
        "null outs": (lambda o: call_combine(o, arr=False), "null"),
        "null output": (lambda o: call_combine([None, o[1], o[2]]), "null"),
        "null x": (lambda o: call_combine(o, x=None), "null"),
        "null digits": (lambda o: call_combine(o, digits=None), "null"),
        "null product": (lambda o: call_combine(o, product=None), "null"),
        "null a_lt": (lambda o: call_combine(o, a_lt=None), "null"),
        "digits shape": (lambda o: call_combine(o, digits=product), "shape"),
        "product shape": (lambda o: call_combine(o, product=digits), "shape"),
        "product of another context": (lambda o: call_combine(o, product=M(other, d, T * c, top, True)), "mismatch"),
        "digits not EVAL": (lambda o: call_combine(o, digits=M(p, m, T * c, top, False)), "Eval"),
        "chunk past m": (lambda o: call_combine(o, col_start=m - 1), "past"),
        "words_per_y 0": (lambda o: call_combine(o, wpy=0), "words_per_y"),
        "base_bits 63": (lambda o: call_combine(o, base_bits=63), "base_bits"),
        "output overlaps the product": (lambda o: call_combine([o[0], o[1], product.reshape_view(d * T, c).row_view(0, d)]), "overlap"),
        "output overlaps the digits": (lambda o: call_combine([digits.reshape_view(m * T, c).row_view(d, 2 * d), o[1], o[2]]), "overlap"),
    }
    kept = {name: w.to_rns() for name, w in dict(ws, digits=digits, product=product).items()}

    def check(entry, name, fn, word):
        outs = [M.from_rns(p, sentinel, False) for _ in range(T)]  # COEFF-tagged: a tag flipped to EVAL would change the read-out
        gpu.gpu_device_sync()
        c0 = lib.gpupoly_launch_count()
        _ffi.trace_begin()
        rc = fn(outs)
        msg = _ffi.last_error_string()
        trace = _ffi.trace_end()
        assert rc != 0, name
        assert entry + ":" in msg and word in msg, (name, msg)
        assert trace == [] and lib.gpupoly_launch_count() == c0, (name, trace)
        for o in outs:
            assert not o.is_ntt and np.array_equal(o.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(ENTRY, name, fn, word)
    for name, (fn, word) in combine_cases.items():
        check(COMBINE, name, fn, word)
    # an output that overlaps another output through a row view of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, 3 * d, c, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, d), parent.row_view(d - 1, 2 * d - 1), parent.row_view(2 * d, 3 * d)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY + ":" in _ffi.last_error_string()
    assert call_combine(views) != 0 and "overlap" in _ffi.last_error_string() and COMBINE + ":" in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for name, w in dict(ws, digits=digits, product=product).items():
        assert np.array_equal(w.to_rns(), kept[name]), name
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and T = 0 launches nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(T)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * d, (t + 1) * d) for t in range(3)]
    assert call(disjoint) == 0
    for o, v in zip(outs, disjoint):
        o.is_ntt = v.is_ntt = True
        assert o == v
    assert call_combine([M.from_rns(p, sentinel, False) for _ in range(T)]) == 0
    gpu.gpu_device_sync()
    c0 = lib.gpupoly_launch_count()
    _ffi.trace_begin()
    assert call([], T_=0) == 0 and call([], T_=0, arr=False, y=None, x=None, tags=None, a_z=None, a_lt=None) == 0
    assert call_combine([], T_=0, arr=False, y=None, x=None, a_lt=None, digits=None, product=None) == 0
    assert _ffi.trace_end() == [] and lib.gpupoly_launch_count() == c0
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the literal loop
    rows, chunk = rows_of(moduli, 3), (1, 2)
    default = lwe_lookup.lwe_target_chunks(sh, rows, chunk)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check(ENTRY, "reference keying", lambda o: call(o), "unsupported")
    assert call_combine([M.from_rns(p, sentinel, False) for _ in range(T)]) == 0  # no sampling: any keying
    fallen = lwe_lookup.lwe_target_chunks(sh, rows, chunk)
    for t, row in enumerate(rows):
        assert fallen[t] == lwe_lookup.build_adjusted_target_chunk(sh, *row, *chunk)
        assert not (fallen[t] == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert lwe_lookup.lwe_target_chunks(sh, rows, chunk)[2] == default[2]
    del keep, keep2


# ---------------------------------------------------------------------------------------------------
# 6. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_row_count(gpu, oracle):
    from mxx_amd import _ffi, lwe_lookup

    sh = shared_of(gpu, oracle, "n256_51", 2)
    chunk = (0, 4)
    rows = [(3 * t + 1, t, 5 * t + 2) for t in range(64)]

    def kernels(fn):
        _ffi.trace_begin()
        fn()
        return [e["kernel"] for e in _ffi.trace_end() if e["threads"]]  # copies are traced with no threads

    many = kernels(lambda: lwe_lookup.lwe_target_chunks(sh, rows, chunk))
    two = kernels(lambda: lwe_lookup.lwe_target_chunks(sh, rows[:2], chunk))
    loop = kernels(lambda: [lwe_lookup.build_adjusted_target_chunk(sh, *row, *chunk) for row in rows[:2]])
    print(f"launches: 64 rows {len(many)} {many}, 2 rows {len(two)}, the literal loop for 2 rows {len(loop)}")
    assert many == two and 0 < len(many) < len(loop)
    assert sum("lwe_combine_kernel" in name for name in many) == 1


# ---------------------------------------------------------------------------------------------------
# 7. end to end: K_high chunks of the targets satisfy the lookup relation exactly
# ---------------------------------------------------------------------------------------------------
def test_public_lookup_end_to_end(gpu, oracle):
    from mxx_amd import lwe_lookup
    from test_gpu_preimage_abi import explicit_seeds, seed_bytes, trapdoor_and_oracle

    ctx, d = "n256_51", 2
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, n, p.base_bits(), d, seed_bytes(9))
    m = sh.m_g
    rows = [(5, 12345, full_modulus(moduli) - 1), (41, (1 << 32) + 5, 3)]
    chunks = [(c0, min(4, m - c0)) for c0 in range(0, m, 4)]
    assert chunks[-1][1] < 4  # a ragged last chunk
    k_high = [[] for _ in rows]
    for j, chunk in enumerate(chunks):
        pairs = lwe_lookup.sample_lwe_preimages(sh, sampler, td, A, rows, chunk, _seeds=explicit_seeds(gpu, len(rows), 700 + 10 * j))
        assert len(pairs) == len(rows)
        for r, (target, x_high) in enumerate(pairs):
            assert x_high.size() == ((p.modulus_digits() + 2) * d, chunk[1]) and A * x_high == target
            k_high[r].append(x_high)
    s = M.from_rns(p, oracle.random_matrix(77, 1, d, moduli, n), True)
    G = M.gadget_matrix(p, d)
    c_b = s * A  # noise-free encodings
    for r, (entry, x, y) in enumerate(rows):
        c_z = s * (sh.a_z - G * gpu.GpuDCRTPoly.from_usize_to_constant(p, x))
        got = lwe_lookup.public_lookup(sh, c_b, c_z, k_high[r], entry)
        assert got.size() == (1, m) and got.is_ntt
        assert got == s * (sh.a_lt - G * gpu.GpuDCRTPoly.from_elem_to_constant(p, y)), (entry, x, y)
        parts = [c_b * kh + c_z * lwe_lookup.derive_k_low_chunk(sh, entry, *chunk) for kh, chunk in zip(k_high[r], chunks)]
        assert got == parts[0].concat_columns(parts[1:]), (entry, x, y)
