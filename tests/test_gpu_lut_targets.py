"""GPU: the preimage targets of many LUT rows of one column chunk in one call (`gpupoly_matrix_lut_targets`, mxx_amd/lookup.py;
DESIGN.md section 5r).

Everything in the target formula is exact arithmetic on canonical residues, so the bar is equality, bit for bit
(gpu_matrix_equal), with `build_lut_preimage_target_chunk` - the reference's function (src/lookup/ggh15/pubkey_gpu.rs:379-415)
restated with the mirror's older operations, one row at a time.  That literal target is computed once per (context, d, chunk,
idx, y) and shared by the row counts.  Independently of the engine the same targets are computed with tests/plainref.py fed
with the CPU restatement's samples, and the combine kernel alone (`gpupoly_matrix_lut_targets_combine`, which takes the
product [top; bottom] as given) is held to plainref in every modulus width class with operands no sampler produces: every
residue q - 1, idx = q - 1 in a limb, and y = 2^(bits - 1) - 1, whose digits below the last are all ones - dpt + 1 products of
(q - 1)^2-sized terms on top of two addends, the lazy accumulator's bound (past it where the window is shorter: 31 bits)."""
import ctypes as C

import numpy as np
import pytest

import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import BASES, CLASSES, _cell, _eval_slots, _params, _rand, _top

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_lut_targets"
COMBINE = "gpupoly_matrix_lut_targets_combine"
# (n, depth, bits, base_bits): 32-bit words packed and unpacked, 64-bit words, the GGH15 chain's ring
CONTEXTS = {"n16_24": (16, 2, 24, 12), "n16_28": (16, 2, 28, 14), "n16_51": (16, 2, 51, 17), "n256_51": (256, 3, 51, 17)}
KEY = bytes((9 * i + 4) & 0xFF for i in range(32))
LUT_ID = 3
IDXS = (0, 1, (1 << 32) + 5, (1 << 64) - 1)  # the last one exceeds every 24-bit q (and every other)
_SHARED, _LITERAL = {}, {}


def full_modulus(moduli):
    Q = 1
    for q in moduli:
        Q *= int(q)
    return Q


def y_values(moduli):
    Q = full_modulus(moduli)
    three_words = int.from_bytes(bytes((41 * i + 23) & 0xFF for i in range(24)), "little") | (1 << 191)
    return (0, 1, Q - 1, Q + 5, three_words)


def shared_of(gpu, oracle, ctx, d):
    from mxx_amd import lookup

    if (ctx, d) not in _SHARED:
        p = make_params(gpu, oracle, *CONTEXTS[ctx])
        moduli, n, m = p.moduli(), p.ring_dimension(), d * p.modulus_digits()
        ws = [gpu.GpuDCRTPolyMatrix.from_rns(p, oracle.random_matrix(300 + 10 * d + i, d, m, moduli, n), True) for i in range(4)]
        _SHARED[(ctx, d)] = lookup.LutShared(p, KEY, LUT_ID, *ws)
    return _SHARED[(ctx, d)]


def literal(gpu, oracle, ctx, d, chunk, idx, y):
    from mxx_amd import lookup

    key = (ctx, d, chunk, idx, y)
    if key not in _LITERAL:
        _LITERAL[key] = lookup.build_lut_preimage_target_chunk(shared_of(gpu, oracle, ctx, d), idx, y, *chunk)
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
    """every (idx, y) pair within 20 rows; tags repeat with the indices"""
    ys = y_values(moduli)
    return [(IDXS[t % 4], ys[t % 5]) for t in range(T)]


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal function
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_one_call_equals_the_literal_function_row_by_row(gpu, oracle, ctx, d):
    from mxx_amd import lookup

    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    for name, chunk in chunks_of(p, d).items():
        for T in (1, 3, 65):
            rows = rows_of(p.moduli(), T)
            got = lookup.lut_preimage_target_chunks(sh, rows, chunk)
            assert len(got) == T
            for t, (idx, y) in enumerate(rows):
                assert got[t].size() == (d, chunk[1]) and got[t].is_ntt
                assert got[t] == literal(gpu, oracle, ctx, d, chunk, idx, y), f"{name} chunk {chunk}, row {t} of {T}: idx={idx} y={y}"
        # the same rows in another order: every row's target is its own
        rows = rows_of(p.moduli(), 7)[::-1]
        for (idx, y), target in zip(rows, lookup.lut_preimage_target_chunks(sh, rows, chunk)):
            assert target == literal(gpu, oracle, ctx, d, chunk, idx, y), (name, idx, y)
    # consecutive indices: the tags are generated on the device (the decimal form grows a digit at 100)
    chunk = chunks_of(p, d)["first"]
    rows = [(98 + t, 5 * t + 2) for t in range(4)]
    assert isinstance(sh.tags([i for i, _ in rows]), gpu.IndexedTags)
    for (idx, y), target in zip(rows, lookup.lut_preimage_target_chunks(sh, rows, chunk)):
        assert target == lookup.build_lut_preimage_target_chunk(sh, idx, y, *chunk), idx
    assert lookup.lut_preimage_target_chunks(sh, [], chunk) == []


def test_a_row_group_boundary_inside_the_call(gpu, oracle):
    """More rows than one group's digit scratch holds cannot be reached with test-sized operands (the cap is 1 GiB); the rows
    of a second call continue the first one's, which is what a group boundary does inside the entry: tags, constants and
    outputs start at the group's first row."""
    from mxx_amd import lookup

    sh = shared_of(gpu, oracle, "n16_51", 2)
    chunk = (5, 3)
    rows = rows_of(sh.params.moduli(), 9)
    whole = lookup.lut_preimage_target_chunks(sh, rows, chunk)
    parts = lookup.lut_preimage_target_chunks(sh, rows[:4], chunk) + lookup.lut_preimage_target_chunks(sh, rows[4:], chunk)
    for a, b in zip(whole, parts):
        assert a == b


def test_the_preimage_of_a_target_maps_back_to_it(gpu, oracle):
    from mxx_amd import lookup
    from test_gpu_preimage_abi import explicit_seeds, seed_bytes, trapdoor_and_oracle

    ctx, d = "n256_51", 2
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    sampler, td, A, _ = trapdoor_and_oracle(gpu, oracle, p, p.ring_dimension(), p.base_bits(), d, seed_bytes(7))
    rows, chunk = [(5, 12345), ((1 << 32) + 5, full_modulus(p.moduli()) - 1)], (p.modulus_digits() - 1, 4)
    pairs = lookup.sample_lut_preimages(sh, sampler, td, A, rows, chunk, _seeds=explicit_seeds(gpu, 2, 900))
    assert len(pairs) == 2
    for (idx, y), (target, x) in zip(rows, pairs):
        assert target == literal(gpu, oracle, ctx, d, chunk, idx, y)
        assert x.size() == ((p.modulus_digits() + 2) * d, 4) and A * x == target


# ---------------------------------------------------------------------------------------------------
# 2. independence from the engine: plainref fed with the CPU restatement's samples
# ---------------------------------------------------------------------------------------------------
def gy_block(moduli, n, base, dpt, y, d, chunk):
    """G^-1(G_d[:, chunk] o y) as (m, c, L, n) evaluation-domain residues: constants, their own transform"""
    L = len(moduli)
    k = L * dpt
    const = np.asarray([[y % int(q)] for q in moduli], dtype=np.uint64)  # coefficient 0 of the constant polynomial y
    block = P.gadget_scalar_digits(const, moduli, base, dpt)  # (k, k, L, 1): the digits are constants too
    out = np.zeros((d * k, chunk[1], L, n), dtype=np.uint64)
    for cc in range(chunk[1]):
        j, rem = divmod(chunk[0] + cc, k)
        out[j * k:(j + 1) * k, cc] = block[:, rem]  # broadcast over the slots
    return out


@pytest.mark.parametrize("ctx", ["n16_24", "n16_51"])
def test_targets_equal_the_plain_reference(gpu, oracle, ctx):
    from mxx_amd import lookup

    d, T = 2, 3
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    moduli, n, base = p.moduli(), p.ring_dimension(), p.base_bits()
    L, dpt = len(moduli), P.digits_per_tower(moduli, base)
    k = L * dpt
    m = d * k
    slots = list(range(n))
    w_id, w_gy, w_v, w_vx = (w.to_rns() for w in (sh.w_identity, sh.w_gy, sh.w_v, sh.w_vx))
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    for chunk in ((0, 4), (k - 1, 2)):
        rows = rows_of(moduli, 20)[7:7 + T]  # idx 2^64 - 1 with Q - 1, idx 0 with Q + 5, idx 1 with the three-word y
        got = lookup.lut_preimage_target_chunks(sh, rows, chunk)
        for (idx, y), target in zip(rows, got):
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, sh.tag(idx)),
                                           full_ncol=m, col_offset=chunk[0])
            v = np.zeros((m, chunk[1], L, n), dtype=np.uint64)
            for r in range(d):
                for cc in range(chunk[1]):
                    v[r * k:(r + 1) * k, cc] = _eval_slots(P.digits(u[r, cc], moduli, base, dpt), moduli, slots)
            v_idx = ((v.astype(object) * (np.asarray([idx % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1))) % q_col).astype(np.uint64)
            want = P.slot_mul_sum(w_id[:, chunk[0]:chunk[0] + chunk[1]], [w_gy, w_v, w_vx],
                                  [gy_block(moduli, n, base, dpt, y, d, chunk), v, v_idx], moduli, False)
            assert np.array_equal(target.to_rns(), want), (ctx, chunk, idx, y)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("bits,base", [(24, 12), (51, 17)])
def test_operands_below_the_top_level_equal_the_plain_reference(gpu, oracle, bits, base, level):
    """The four operands and the outputs at level 0 / 1 of a three-limb context: m = d * dpt * (level + 1) with dpt from the
    CONTEXT's crt_bits (these bases have one width, so plainref derives the same dpt from the truncated basis), the hashed
    samples of limbs 0..level only, and the plain reference above handed moduli[: level + 1]; then the combine kernel alone
    with operands at the level."""
    n, d, T = 16, 2, 3
    p = make_params(gpu, oracle, n, 3, bits, base)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()[: level + 1]
    L, dpt = level + 1, -(-p.crt_bits() // base)
    assert P.digits_per_tower(moduli, base) == dpt
    k = L * dpt
    m = d * k
    slots = list(range(n))
    w_id, w_gy, w_v, w_vx = (oracle.random_matrix(340 + level + i, d, m, moduli, n) for i in range(4))
    ws = [M.from_rns(p, w, True) for w in (w_id, w_gy, w_v, w_vx)]
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    tag = lambda idx: f"ggh15_lut_v_idx_{LUT_ID}_{idx}".encode("ascii")  # noqa: E731
    for chunk in ((0, min(4, m)), (k - 1, 2)):
        rows = rows_of(moduli, 20)[7:7 + T]
        got = M.lut_targets(*ws, chunk[0], chunk[1], [y for _, y in rows], [i for i, _ in rows], KEY, [tag(i) for i, _ in rows])
        for (idx, y), target in zip(rows, got):
            assert target.level == level and target.is_ntt and target.size() == (d, chunk[1])
            u = oracle.sample_distribution(d, chunk[1], moduli, n, "uniform", 0.0, gpu.hash_seed_for_matrix(KEY, tag(idx)),
                                           full_ncol=m, col_offset=chunk[0])
            v = np.zeros((m, chunk[1], L, n), dtype=np.uint64)
            for r in range(d):
                for cc in range(chunk[1]):
                    v[r * k:(r + 1) * k, cc] = _eval_slots(P.digits(u[r, cc], moduli, base, dpt), moduli, slots)
            v_idx = ((v.astype(object) * (np.asarray([idx % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1))) % q_col).astype(np.uint64)
            want = P.slot_mul_sum(w_id[:, chunk[0]:chunk[0] + chunk[1]], [w_gy, w_v, w_vx],
                                  [gy_block(moduli, n, base, dpt, y, d, chunk), v, v_idx], moduli, False)
            assert np.array_equal(target.to_rns(), want), (bits, level, chunk, idx, y)
    # the combine kernel alone: the product [top; bottom] as given, every (tower, digit) column of the level
    rng = np.random.default_rng(2000 + bits + level)
    prod = _rand(rng, 2 * d, T * m, moduli, n)
    ys = [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(T)]
    idxs = [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(T)]
    got = combine(gpu, p, w_id, w_gy, prod, T, 0, m, ys, idxs)
    for t in range(T):
        idx_l = np.asarray([idxs[t] % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
        top, bot = prod[:d, t * m:(t + 1) * m].astype(object), prod[d:, t * m:(t + 1) * m].astype(object)
        addend = ((w_id.astype(object) + top + idx_l * bot) % q_col).astype(np.uint64)
        want = P.slot_mul_sum(addend, [w_gy], [gy_block(moduli, n, base, dpt, ys[t], d, (0, m))], moduli, False)
        assert np.array_equal(got[t], want), (bits, level, t)


def combine(gpu, p, w_id, w_gy, prod, T, col_start, c, ys, idxs):
    """gpupoly_matrix_lut_targets_combine over uploaded residues -> the T outputs' residues"""
    from mxx_amd import _ffi

    M = gpu.GpuDCRTPolyMatrix
    ops = [M.from_rns(p, x, True) for x in (w_id, w_gy, prod)]
    outs = [M(p, w_id.shape[0], c, w_id.shape[2] - 1, False) for _ in range(T)]
    words = [M._int_words(y) for y in ys]
    wpy = max(len(w) for w in words)
    y_arr = np.zeros((T, wpy), dtype=np.uint64)
    for t, w in enumerate(words):
        y_arr[t, :len(w)] = w
    i_arr = np.array(idxs, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    st = _ffi.lib().gpupoly_matrix_lut_targets_combine(M._raw_array(outs), T, ops[0].raw, ops[1].raw, ops[2].raw, col_start, p.base_bits(),
                                                       y_arr.ctypes.data_as(u64p), wpy, i_arr.ctypes.data_as(u64p))
    _ffi.check_status(st, COMBINE)
    for o in outs:
        o.is_ntt = True  # the entry tags its outputs EVAL
    return [o.to_rns() for o in outs]


@pytest.mark.parametrize("bits", CLASSES)
def test_combine_kernel_alone_in_every_width_class(gpu, bits):
    n, moduli, bases, slots = _cell(("class", bits))
    L = len(moduli)
    q_col = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
    Q = full_modulus(moduli)
    for base in BASES[bits]:
        p = _params(gpu, n, moduli, base)
        dpt = P.digits_per_tower(moduli, base)
        d, k = 1, L * dpt
        m, chunk = d * k, (0, d * k)  # every (tower, digit) column
        # worst case: every residue q - 1; row t < L has idx = q_t - 1 (limb t multiplies (q - 1)(q - 1)), the last row 2^64 - 1;
        # y = 2^(bits - 1) - 1 is below every modulus of the class, so its digits below the last are 2^base - 1 in every tower
        ys = [(1 << (bits - 1)) - 1] * L + [Q - 1]
        idxs = [int(q) - 1 for q in moduli] + [(1 << 64) - 1]
        T = L + 1
        rng = np.random.default_rng(1000 + bits)
        for kind in ("top", "random"):
            if kind == "top":
                w_id, w_gy, prod = _top(d, m, moduli, n), _top(d, m, moduli, n), _top(2 * d, T * m, moduli, n)
            else:
                w_id, w_gy, prod = _rand(rng, d, m, moduli, n), _rand(rng, d, m, moduli, n), _rand(rng, 2 * d, T * m, moduli, n)
                ys = [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(T)]
                idxs = [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(T)]
            got = combine(gpu, p, w_id, w_gy, prod, T, 0, m, ys, idxs)
            for t in range(T):
                idx_l = np.asarray([idxs[t] % int(q) for q in moduli], dtype=object).reshape(1, 1, L, 1)
                top, bot = prod[:d, t * m:(t + 1) * m].astype(object), prod[d:, t * m:(t + 1) * m].astype(object)
                addend = ((w_id.astype(object) + top + idx_l * bot) % q_col).astype(np.uint64)
                want = P.slot_mul_sum(addend, [w_gy], [gy_block(moduli, n, base, dpt, ys[t], d, chunk)], moduli, False, slots)
                assert np.array_equal(got[t][..., slots], want), (bits, base, kind, t)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(got[t], np.broadcast_to(want[..., :1], got[t].shape)), (bits, base, t)


# ---------------------------------------------------------------------------------------------------
# 3. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi, lookup
    from mxx_amd.matrix import hash_tags_arg

    ctx, d = "n16_24", 2
    sh = shared_of(gpu, oracle, ctx, d)
    p = sh.params
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    m, c, T = d * p.modulus_digits(), 2, 3
    sentinel = oracle.random_matrix(93, d, c, moduli, n)
    other = make_params(gpu, oracle, *CONTEXTS["n16_28"])
    u64p = C.POINTER(C.c_uint64)
    y_arr = np.arange(1, 2 * T + 1, dtype=np.uint64)
    i_arr = np.arange(T, dtype=np.uint64)
    arg, keep, _ = hash_tags_arg(KEY, [b"a", b"bb", b"ccc"])
    bad_form, keep2, _ = hash_tags_arg(KEY, [b"a", b"bb", b"ccc"])
    bad_form.form = 9
    ws = dict(w_identity=sh.w_identity, w_gy=sh.w_gy, w_v=sh.w_v, w_vx=sh.w_vx)
    coeff_w = sh.w_v.clone()
    coeff_w.intt_all_in_place()
    low = M(p, d, m, 0, True)
    narrow = M(p, d, m - 1, len(moduli) - 1, True)
    foreign = M(other, d, d * other.modulus_digits(), len(moduli) - 1, True)

    def call(outs, T_=T, col_start=1, base_bits=base, y=y_arr, wpy=2, idx=i_arr, tags=arg, arr=True, **over):
        w = dict(ws, **over)
        raw = None if not arr else (C.c_void_p * max(len(outs), 1))(*[None if o is None else o.raw.value for o in outs])
        return lib.gpupoly_matrix_lut_targets(raw, T_, *[None if w[name] is None else w[name].raw for name in ("w_identity", "w_gy", "w_v", "w_vx")],
                                              col_start, base_bits, None if y is None else y.ctypes.data_as(u64p), wpy,
                                              None if idx is None else idx.ctypes.data_as(u64p), None if tags is None else C.byref(tags))

    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null y_words": (lambda o: call(o, y=None), "null"),
        "null idx": (lambda o: call(o, idx=None), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "null operand": (lambda o: call(o, w_gy=None), "null"),
        "context mismatch": (lambda o: call(o, w_vx=foreign), "mismatch"),
        "output of another context": (lambda o: call([o[0], M(other, d, c, len(moduli) - 1, True), o[2]]), "mismatch"),
        "level mismatch": (lambda o: call(o, w_v=low), "mismatch"),
        "operand shape": (lambda o: call(o, w_gy=narrow), "shape"),
        "output rows": (lambda o: call([o[0], o[1], M(p, d + 1, c, len(moduli) - 1, True)]), "shape"),
        "operand not EVAL": (lambda o: call(o, w_v=coeff_w), "Eval"),
        "chunk past m": (lambda o: call(o, col_start=m - 1), "past"),
        "col_start past m": (lambda o: call(o, col_start=m + 1), "past"),
        "outputs of different widths": (lambda o: call([o[0], o[1], M(p, d, c + 1, len(moduli) - 1, True)]), "width"),
        "words_per_y 0": (lambda o: call(o, wpy=0), "words_per_y"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "output overlaps w_identity": (lambda o: call([o[0], sh.w_identity.reshape_view(d * m // c, c).row_view(0, d), o[2]]), "overlap"),
        "output overlaps w_gy": (lambda o: call([sh.w_gy.reshape_view(d * m // c, c).row_view(d, 2 * d), o[1], o[2]]), "overlap"),
        "output overlaps w_v": (lambda o: call([o[0], o[1], sh.w_v.reshape_view(d * m // c, c).row_view(0, d)]), "overlap"),
        "output overlaps w_vx": (lambda o: call([o[0], sh.w_vx.reshape_view(d * m // c, c).row_view(2, 2 + d), o[2]]), "overlap"),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
    }
    operands = {name: w.to_rns() for name, w in ws.items()}

    def check(name, fn, word):
        outs = [M.from_rns(p, sentinel, False) for _ in range(T)]  # COEFF-tagged: a tag flipped to EVAL would change the read-out
        c0 = lib.gpupoly_launch_count()
        assert fn(outs) != 0, name
        msg = _ffi.last_error_string()
        assert ENTRY in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        for o in outs:
            assert not o.is_ntt and np.array_equal(o.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # an output that overlaps another output through a row view of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, 3 * d, c, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, d), parent.row_view(d - 1, 2 * d - 1), parent.row_view(2 * d, 3 * d)]
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for name, w in ws.items():
        assert np.array_equal(w.to_rns(), operands[name]), name
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and T = 0 launches nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(T)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * d, (t + 1) * d) for t in range(3)]
    assert call(disjoint) == 0
    for o, v in zip(outs, disjoint):
        o.is_ntt = v.is_ntt = True
        assert o == v
    c0 = lib.gpupoly_launch_count()
    assert call([], T_=0) == 0 and call([], T_=0, arr=False, y=None, idx=None, tags=None) == 0 and lib.gpupoly_launch_count() == c0
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the literal loop
    rows, chunk = rows_of(moduli, 3), (1, 2)
    default = lookup.lut_preimage_target_chunks(sh, rows, chunk)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    fallen = lookup.lut_preimage_target_chunks(sh, rows, chunk)
    for t, (idx, y) in enumerate(rows):
        assert fallen[t] == lookup.build_lut_preimage_target_chunk(sh, idx, y, *chunk)
        assert not (fallen[t] == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert lookup.lut_preimage_target_chunks(sh, rows, chunk)[2] == default[2]
    del keep, keep2


# ---------------------------------------------------------------------------------------------------
# 4. launches
# ---------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_row_count(gpu, oracle):
    from mxx_amd import _ffi, lookup

    sh = shared_of(gpu, oracle, "n256_51", 2)
    chunk = (0, 4)
    rows = [(t, 3 * t + 1) for t in range(64)]

    def kernels(fn):
        _ffi.trace_begin()
        fn()
        return [e["kernel"] for e in _ffi.trace_end() if e["threads"]]  # copies are traced with no threads

    many = kernels(lambda: lookup.lut_preimage_target_chunks(sh, rows, chunk))
    two = kernels(lambda: lookup.lut_preimage_target_chunks(sh, rows[:2], chunk))
    loop = kernels(lambda: [lookup.build_lut_preimage_target_chunk(sh, i, y, *chunk) for i, y in rows[:2]])
    print(f"launches: 64 rows {len(many)} {many}, 2 rows {len(two)}, the literal loop for 2 rows {len(loop)}")
    assert many == two and 0 < len(many) < len(loop)
