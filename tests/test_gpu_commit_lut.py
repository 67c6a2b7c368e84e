"""GPU: the message blocks of the commitment-based public lookup for many LUT rows in one call
(`gpupoly_matrix_commit_lut_messages`, mxx_amd/commit_lookup.py).

msg_t = [A_out_g - G_d o y_t | 0] + R_t - P_g G^-1((B_1 V_t + R_t) o (idx_t + 1)^-1) is exact arithmetic on canonical residues, so
the bar is equality, bit for bit, with the reference's sequence through the mirror's older operations
(`message_block_literal`, one row at a time).  The formula needs no public parameters: the verifier is a uniform random EVAL
matrix.  A literal stream is computed once per case and shared.  The combine entry alone
(`gpupoly_matrix_commit_lut_messages_combine`, R and the digits given) is held to tests/plainref.py in every modulus width
class with operands no sampler produces; and with the shared Wee25 parameters, a real trapdoor and noise-free encodings the
two evaluators return exactly s (A_out - G o y), the reference's own acceptance test (src/lookup/commit_eval.rs:680-825)."""
import ctypes as C

import numpy as np
import pytest

import commit_lut_levels  # noqa: F401  (the entries' rows of the lower-level coverage table)
import plainref as P
from conftest import make_params
from test_gpu_fused_width_classes import BASES, CLASSES, MIXED, MIXED_BASES, _rand, _top, _windows
from test_gpu_lut_targets import full_modulus
from test_gpu_modulus_classes import _moduli, _params

pytestmark = pytest.mark.gpu

ENTRY = "gpupoly_matrix_commit_lut_messages"
COMBINE = "gpupoly_matrix_commit_lut_messages_combine"
KERNEL = "commit_lut_combine_kernel"
KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
SIGMA, TREE_BASE = 4.578, 2
# name -> (n, depth, bits, base, d)
CASES = {"n128_24_d1": (128, 2, 24, 12, 1), "n256_51_d2": (256, 3, 51, 17, 2)}
GATE_A, GATE_B = 9, 4  # given in this order; the layout sorts them: gate 4 owns [0, 3), gate 9 owns [3, 7)
_WORLD = {}


def luts_of(moduli):
    """LUT 0 (gate 9), four rows: get(x) = ((x + 1) mod 4, y) - the row index is neither the position nor consecutive from it;
    LUT 1 (gate 4), three rows in place.  y up to the full modulus - 1: more than 64 bits where the basis has them"""
    Q = full_modulus(moduli)
    ys = [Q - 1, 0, (Q >> 1) + 12345, 7]
    return {0: {x: ((x + 1) % 4, ys[x]) for x in range(4)}, 1: {x: (x, (Q // 3 + 17 * x) % Q) for x in range(3)}}


class World:
    """what the tests of one case share, computed once and left unchanged"""

    def __init__(self, gpu, oracle, case):
        from mxx_amd import commit_lookup as cl
        from mxx_amd.bgg import BggPublicKey
        from mxx_amd.commit import Wee25Commit

        n, depth, bits, base, d = CASES[case]
        self.gpu, self.case, self.d = gpu, case, d
        p = self.p = make_params(gpu, oracle, n, depth, bits, base)
        M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
        self.commit = Wee25Commit(p, d, TREE_BASE, SIGMA)
        self.m_g, self.m_b = self.commit.m_g, self.commit.m_b
        rand = lambda seed, rows, cols: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, n), True)  # noqa: E731
        key = lambda seed: BggPublicKey(rand(seed, d, self.m_g), True)  # noqa: E731
        self.luts = luts_of(moduli)
        self.gate_states = [(GATE_A, 0, key(700), key(701)), (GATE_B, 1, key(702), key(703))]
        self.b_1 = cl.derive_b_1_matrix(p, d, self.m_b, KEY)
        self.padded_len = 8
        self.verifier_all = rand(710, self.m_b, self.padded_len * self.m_b)
        self._slices = {}
        self.stream = cl.CommitMsgStream(p, self.commit, None, self.b_1, KEY, self.luts, self.gate_states, verifier_of=self.verifier_of)
        assert (self.stream.padded_len, self.stream.lut_vector_len) == (8, 7)
        assert self.stream.layout.lut_gate_start_ids == {GATE_B: 0, GATE_A: 3}
        self.literal = self.stream.message_blocks_literal(range(8))

    def verifier_slice(self, pos):
        if pos not in self._slices:
            self._slices[pos] = self.verifier_all.slice_columns(pos * self.m_b, (pos + 1) * self.m_b)
        return self._slices[pos]

    def verifier_of(self, positions):
        parts = [self.verifier_slice(pos) for pos in positions]
        return parts[0] if len(parts) == 1 else parts[0].concat_columns(parts[1:])

    def operands(self):
        return [self.b_1, self.verifier_all] + [pk.matrix for st in self.gate_states for pk in st[2:]]

    def call_args(self, positions):
        """the arguments of GpuDCRTPolyMatrix.commit_lut_messages for the stream positions (all below lut_vector_len) against
        the WHOLE random verifier: vslot is the verifier position itself"""
        rows = [self.stream.row(i) for i in positions]
        gates = sorted({r[0] for r in rows})
        ops = [self.stream.gate_operands(g) for g in gates]
        from mxx_amd import commit_lookup as cl

        return dict(b_1=self.b_1, verifier=self.verifier_all, vslots=[r[4] for r in rows], pubkey_sums=[o[0] for o in ops], a_outs=[o[1] for o in ops],
                    gate_of_row=[gates.index(r[0]) for r in rows], ys=[r[3] for r in rows], idxs=[r[2] for r in rows], key=KEY,
                    tags=[cl.r_g_i_tag(r[1], r[2]) for r in rows])

    def messages(self, positions, **over):
        args = self.call_args(positions)
        args.update(over)
        return self.gpu.GpuDCRTPolyMatrix.commit_lut_messages(**args)


def world_of(gpu, oracle, case):
    if case not in _WORLD:
        _WORLD[case] = World(gpu, oracle, case)
    return _WORLD[case]


# ---------------------------------------------------------------------------------------------------
# 1. one call against the literal per-row sequence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_batched_equals_literal_row_by_row(gpu, oracle, case):
    wd = world_of(gpu, oracle, case)
    M = gpu.GpuDCRTPolyMatrix
    before = [(m.is_ntt, m.to_rns()) for m in wd.operands()]
    # the LUT of gate 9 names rows 1, 2, 3, 0: vslot is neither consecutive nor the row's place; y passes 64 bits at 51-bit limbs
    assert [wd.stream.row(i)[2] for i in range(3, 7)] == [1, 2, 3, 0] and [wd.stream.row(i)[4] for i in range(3, 7)] == [4, 5, 6, 3]
    if case == "n256_51_d2":
        assert max(y for lut in wd.luts.values() for _, y in lut.values()) >> 64
    got = wd.stream.message_blocks(range(8))  # two gates share the call; position 7 is padding
    assert len(got) == 8
    for i, (a, b) in enumerate(zip(got, wd.literal)):
        assert a.size() == (wd.d, wd.m_b) and a.is_ntt and a.level == b.level
        assert a == b, (case, i)
    assert got[7] == M.zero(wd.p, wd.d, wd.m_b)
    # one gate with consecutive indices (the indexed decimal tags), one gate with a rotated LUT (a table), a lone row, another order
    for positions in (range(0, 3), range(3, 7), [5], [6, 0, 3, 2], [7, 1]):
        for i, a in zip(positions, wd.stream.message_blocks(positions)):
            assert a == wd.literal[i], (case, list(positions), i)
    assert wd.stream.message_blocks([]) == [] and wd.stream.message_blocks([7])[0] == wd.literal[7]
    # the indexed form gives the table's matrices
    from mxx_amd import IndexedTags, commit_lookup as cl

    indexed = wd.messages(range(0, 3), tags=IndexedTags(cl.r_g_i_prefix(GATE_B), 0, 3, decimal=True))
    for i, a in enumerate(indexed):
        assert a == wd.literal[i], (case, i)
    # the gadget term hits only the block row that matches: with d = 2 rows 0 and 1 differ in where G o y lands
    if wd.d == 2:
        k = wd.m_g // 2
        a_out = wd.stream.gate_operands(1)[1]
        r = cl.derive_r_g_i_matrix(wd.p, 2, wd.m_b, KEY, GATE_A, 1)
        canc = cl.derive_canceler_matrix(wd.p, wd.b_1, wd.verifier_slice(4), r, 1)
        rest = (a_out.concat_columns([M.zero(wd.p, 2, wd.m_b - wd.m_g)]) + r - wd.stream.gate_operands(1)[0] * canc.decompose()) - got[3]
        res = rest.to_rns()  # = [G_d o y | 0]
        assert res[0, :k].any() and not res[0, k:].any() and res[1, k:2 * k].any() and not res[1, :k].any() and not res[1, 2 * k:].any()
    # every input, residues and tag, as it was
    for m, (tag, res) in zip(wd.operands(), before):
        assert m.is_ntt == tag and np.array_equal(m.to_rns(), res)


def test_operands_below_the_top_level_equal_the_literal(gpu, oracle):
    """Every matrix of the call at level 1 of a three-limb 24-bit context: k = dpt * 2 with dpt from the CONTEXT's crt_bits (one
    width per basis, so the two-limb context over the same first two primes has the same dpt), R_t sampled in limbs 0 and 1
    only.  The literal leg runs at the top level of that two-limb context over the same residues; then the combine entry with
    R and the digits of the literal leg given."""
    from mxx_amd import commit_lookup as cl

    n, base, d, level = 128, 12, 1, 1
    p3 = make_params(gpu, oracle, n, 3, 24, base)
    moduli = p3.moduli()[: level + 1]
    p2 = _params(gpu, n, moduli, base)
    M = gpu.GpuDCRTPolyMatrix
    k = (level + 1) * (-(-p3.crt_bits() // base))
    assert p2.modulus_digits() == k and -(-p2.crt_bits() // base) == -(-p3.crt_bits() // base)
    m_g, m_b = d * k, d * (k + 2)
    rnd = lambda seed, rows, cols: oracle.random_matrix(seed, rows, cols, moduli, n)  # noqa: E731
    low = lambda a: M.from_rns(p3, a, True)  # noqa: E731  (two limbs: level 1 of the three-limb context)
    top = lambda a: M.from_rns(p2, a, True)  # noqa: E731
    one, inp, ver = rnd(720, d, m_g), rnd(721, d, m_g), rnd(722, m_b, 3 * m_b)
    Q = full_modulus(moduli)
    rows = [(0, 2, Q - 1, 2), (1, 0, 12345, 0), (2, 1, Q // 2, 1)]  # (position, idx, y, verifier slot)
    gate = 6
    b_1, a_out = cl.derive_b_1_matrix(p2, d, m_b, KEY), cl.derive_a_out_matrix(p2, d, KEY, gate)
    literal, rs, digits = [], [], []
    for _, idx, y, slot in rows:
        v = top(ver[:, slot * m_b:(slot + 1) * m_b])
        literal.append(cl.message_block_literal(p2, b_1, v, KEY, gate, idx, y, top(one), top(inp), m_g, m_b))
        r = cl.derive_r_g_i_matrix(p2, d, m_b, KEY, gate, idx)
        rs.append(r.to_rns())
        digits.append(cl.derive_canceler_matrix(p2, b_1, v, r, idx).decompose().ensure_eval().to_rns())
    sums, g_aout = low((one + inp) % np.asarray(moduli, dtype=np.uint64).reshape(1, 1, -1, 1)), low(a_out.to_rns())
    assert sums.level == level and g_aout.level == level
    got = M.commit_lut_messages(low(b_1.to_rns()), low(ver), [r[3] for r in rows], [sums], [g_aout], [0] * 3, [r[2] for r in rows],
                                [r[1] for r in rows], KEY, [cl.r_g_i_tag(gate, r[1]) for r in rows])
    given = M.commit_lut_messages_combine(low(np.concatenate(rs, axis=1)), low(np.concatenate(digits, axis=1)), [sums], [g_aout], [0] * 3,
                                          [r[2] for r in rows])
    for t in range(3):
        assert got[t].level == level and got[t].is_ntt and got[t].size() == (d, m_b)
        assert np.array_equal(got[t].to_rns(), literal[t].to_rns()), t
        assert given[t] == got[t], t


# ---------------------------------------------------------------------------------------------------
# 2. the combine entry alone against plainref in every width class
# ---------------------------------------------------------------------------------------------------
N_CLASS, D_CLASS, T_CLASS = 64, 2, 3
CELLS = [("class", b) for b in CLASSES] + [("mixed", i) for i in range(len(MIXED))]


def _cell_id(cell):
    return f"{cell[1]}bit" if cell[0] == "class" else "mixed_" + "_".join(str(b) for b, _ in MIXED[cell[1]][1])


def gadget_slots(d, moduli, base, n):
    """G_d in the evaluation domain: constants, the same word in every slot"""
    g = P.gadget(d, moduli, base, n)
    return np.broadcast_to(g[..., :1], g.shape).copy()


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_combine_entry_alone_in_every_width_class(gpu, cell):
    """out_t = [A_out - G o y_t | 0] + R_t - P_g digits_t with plainref's integers alone.  "top": every residue q - 1 in P_g and
    the digits, so each of the m_g = d k terms is (q - 1)^2 and a lazy window no longer than m_g is filled to its bound (the 31- and 62-bit
    classes; passed, with a fold inside the sum, wherever it is shorter); R, A_out and y o G at q - 1 as well."""
    n, d, T = N_CLASS, D_CLASS, T_CLASS
    if cell[0] == "class":
        moduli, bases = _moduli(n, cell[1]), BASES[cell[1]]
    else:
        moduli, bases = [P.primes(n, bits, 1, low=low)[0] for bits, low in MIXED[cell[1]][1]], MIXED_BASES[cell[1]]
    M, L = gpu.GpuDCRTPolyMatrix, len(moduli)
    windows = _windows(moduli)
    qcol = np.asarray([int(q) for q in moduli], dtype=object).reshape(1, 1, -1, 1)
    Q = full_modulus(moduli)
    for base in bases:
        p = _params(gpu, n, moduli, base)
        k = L * P.digits_per_tower(moduli, base)
        m_g, m_b = d * k, d * (k + 2)
        if cell in (("class", 31), ("class", 62)):
            # the shortest window filled to its bound (62 bits at base 31: 16 terms in a window of 16) or passed, a fold inside
            # the sum; the second base of either class passes the longest window as well
            assert min(windows) <= m_g and (base != 6 or max(windows) < m_g), (cell, base, windows, m_g)
        slots = list(range(n)) if k <= 16 else [0, 1, 17, 31, 32, 46, 62, 63]
        G = gadget_slots(d, moduli, base, n)
        rng = np.random.default_rng(4100 + 7 * base + sum(int(q) % 1000 for q in moduli))
        up = lambda a: M.from_rns(p, np.ascontiguousarray(a), True)  # noqa: E731
        for kind in ("top", "random"):
            make = (lambda rows, cols: _top(rows, cols, moduli, n)) if kind == "top" else (lambda rows, cols: _rand(rng, rows, cols, moduli, n))
            sums, a_outs = [make(d, m_g) for _ in range(2)], [make(d, m_g) for _ in range(2)]
            r, digits = make(d, T * m_b), make(m_g, T * m_b)
            gate_of_row = [1, 0, 1]
            ys = [Q - 1, 0, Q // 3] if kind == "top" else [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % Q for _ in range(T)]
            got = M.commit_lut_messages_combine(up(r), up(digits), [up(a) for a in sums], [up(a) for a in a_outs], gate_of_row, ys)
            for t in range(T):
                g = gate_of_row[t]
                block = slice(t * m_b, (t + 1) * m_b)
                gy = (G.astype(object) * [[[[ys[t] % int(q)] for q in moduli]]]) % qcol
                head = (a_outs[g].astype(object) - gy) % qcol
                addend = r[:, block].astype(object)
                addend[:, :m_g] += head
                addend = (addend % qcol).astype(np.uint64)
                want = P.slot_mul_sum(addend, [sums[g]], [digits[:, block]], moduli, True, slots)
                assert got[t].size() == (d, m_b) and got[t].is_ntt
                res = got[t].to_rns()
                assert np.array_equal(res[..., slots], want), (cell, base, kind, t)
                if kind == "top":  # constant operands: every slot holds the same word
                    assert np.array_equal(res, np.broadcast_to(res[..., :1], res.shape)), (cell, base, t)


# ---------------------------------------------------------------------------------------------------
# 3. launches and groups
# ---------------------------------------------------------------------------------------------------
def test_the_launches_depend_on_neither_the_row_count_nor_the_gate_count(gpu, oracle):
    from mxx_amd import _ffi

    wd = world_of(gpu, oracle, "n128_24_d1")
    lib = _ffi.lib()

    def launches(positions, **over):
        c0 = lib.gpupoly_launch_count()
        wd.messages(positions, **over)
        return lib.gpupoly_launch_count() - c0

    def trace(positions):
        _ffi.trace_begin()
        wd.messages(positions)
        return [e["kernel"] for e in _ffi.trace_end() if e["threads"]]

    wd.messages(range(7))  # operands stored packed are unpacked by the first call that reads them
    two, seven = launches([3, 4]), launches(range(7))
    assert two == seven and two > 0, (two, seven)
    kernels = trace(range(7))
    assert kernels == trace([3, 4]) and sum(KERNEL in name for name in kernels) == 1 and sum("commit_canceler_kernel" in name for name in kernels) == 1
    # one gate against three: the same rows' operands under three gate numbers
    args = wd.call_args(range(3))
    one_gate = launches(range(3))
    three = launches(range(3), pubkey_sums=args["pubkey_sums"] * 3, a_outs=args["a_outs"] * 3, gate_of_row=[0, 1, 2])
    assert one_gate == three == seven
    for a, i in zip(wd.messages(range(3), pubkey_sums=args["pubkey_sums"] * 3, a_outs=args["a_outs"] * 3, gate_of_row=[2, 0, 1]), range(3)):
        assert a == wd.literal[i], i


@pytest.mark.parametrize("case", list(CASES))
def test_three_groups_equal_the_one_group_call(gpu, oracle, hip_env, case):
    """a fresh context created under a budget of three rows' digit scratch: seven rows go as 3 + 3 + 1"""
    wd = world_of(gpu, oracle, case)
    p = wd.p
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    word = 8 if max(moduli) >> 31 else 4
    row_bytes = wd.m_g * wd.m_b * len(moduli) * n * word
    whole = wd.messages(range(7))
    hip_env.set("MXX_HIP_COMMIT_LUT_BUDGET", str(3 * row_bytes))
    fresh = gpu.GpuDCRTPolyParams(n, list(moduli), p.base_bits())
    there = lambda m: M.from_rns(fresh, m.to_rns(), True)  # noqa: E731
    args = wd.call_args(range(7))
    for name in ("b_1", "verifier"):
        args[name] = there(args[name])
    for name in ("pubkey_sums", "a_outs"):
        args[name] = [there(m) for m in args[name]]
    from mxx_amd import _ffi

    _ffi.trace_begin()
    grouped = M.commit_lut_messages(**args)
    kernels = [e["kernel"] for e in _ffi.trace_end() if e["threads"]]
    assert sum(KERNEL in name for name in kernels) == 3
    for i, (a, b) in enumerate(zip(grouped, whole)):
        assert np.array_equal(a.to_rns(), b.to_rns()) and b == wd.literal[i], (case, i)
    # one row per group, the indexed tags cut per group
    hip_env.set("MXX_HIP_COMMIT_LUT_BUDGET", "1")
    from mxx_amd import IndexedTags, commit_lookup as cl

    args = wd.call_args(range(3))
    got = M.commit_lut_messages(**dict(args, tags=IndexedTags(cl.r_g_i_prefix(GATE_B), 0, 3, decimal=True)))
    hip_env.unset("MXX_HIP_COMMIT_LUT_BUDGET")
    for i, a in enumerate(got):
        assert a == wd.literal[i], (case, i)


# ---------------------------------------------------------------------------------------------------
# 4. refusals: nothing launched, every output (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi, commit_lookup as cl
    from mxx_amd.matrix import hash_tags_arg

    wd = world_of(gpu, oracle, "n128_24_d1")
    p = wd.p
    M, moduli, n, lib, base = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib(), p.base_bits()
    d, m_g, m_b, T, top = wd.d, wd.m_g, wd.m_b, 3, len(p.moduli()) - 1
    a = wd.call_args([3, 0, 5])  # two gates: gate_of_row = [1, 0, 1]
    assert a["gate_of_row"] == [1, 0, 1]
    sums, a_outs, b_1, ver = a["pubkey_sums"], a["a_outs"], a["b_1"], a["verifier"]
    sentinel = oracle.random_matrix(96, d, m_b, moduli, n)
    other = make_params(gpu, oracle, 128, 2, 28, 14)
    arg, keep, _ = hash_tags_arg(KEY, a["tags"])
    bad_form, keep2, _ = hash_tags_arg(KEY, a["tags"])
    bad_form.form = 9
    coeff = {name: m.clone() for name, m in (("b_1", b_1), ("verifier", ver), ("sum", sums[1]), ("a_out", a_outs[0]))}
    for m in coeff.values():
        m.intt_all_in_place()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    y_arr, wpy = M._int_rows(a["ys"])

    def array(ms):
        return None if ms is None else (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.raw.value for m in ms])

    def u64(values):
        return None if values is None else np.array(values, dtype=np.uint64).ctypes.data_as(u64p)

    def call(outs, T_=T, b=b_1, v=ver, vslot=a["vslots"], s=sums, ao=a_outs, ngates=2, gate=a["gate_of_row"], base_bits=base, y=y_arr, words=wpy,
             idx=a["idxs"], tags=arg, arr=True):
        g = None if gate is None else np.array(gate, dtype=np.uint32)
        return lib.gpupoly_matrix_commit_lut_messages(array(outs) if arr else None, T_, None if b is None else b.raw, None if v is None else v.raw,
                                                      u64(vslot), array(s), array(ao), ngates, None if g is None else g.ctypes.data_as(u32p), base_bits,
                                                      None if y is None else y.ctypes.data_as(u64p), words, u64(idx), None if tags is None else C.byref(tags))

    def swap(ms, at, m):
        return [m if j == at else x for j, x in enumerate(ms)]

    def rows_of(m, lo, hi):  # d x m_b views into an operand's storage
        return m.reshape_view(m.nrow * m.ncol // m_b, m_b).row_view(lo, hi)

    new = lambda rows, cols, params=p, level=top: M(params, rows, cols, level, True)  # noqa: E731
    wide_op = M.from_rns(p, oracle.random_matrix(97, d, m_g * m_b, moduli, n), True)  # a d x m_g operand cut out of it, an output out of the same words
    cases = {
        "null outs": (lambda o: call(o, arr=False), "null"),
        "null output": (lambda o: call([o[0], None, o[2]]), "null"),
        "null b_1": (lambda o: call(o, b=None), "null"),
        "null verifier": (lambda o: call(o, v=None), "null"),
        "null vslot": (lambda o: call(o, vslot=None), "null"),
        "null pubkey_sums": (lambda o: call(o, s=None), "null"),
        "null pubkey_sums entry": (lambda o: call(o, s=[sums[0], None]), "null"),
        "null a_outs": (lambda o: call(o, ao=None), "null"),
        "null a_outs entry": (lambda o: call(o, ao=[None, a_outs[1]]), "null"),
        "null gate_of_row": (lambda o: call(o, gate=None), "null"),
        "null y_words": (lambda o: call(o, y=None), "null"),
        "null idx": (lambda o: call(o, idx=None), "null"),
        "null tags": (lambda o: call(o, tags=None), "null"),
        "no gates": (lambda o: call(o, ngates=0), "gates"),
        "gate_of_row past the gates": (lambda o: call(o, gate=[1, 0, 2]), "(row 2)"),
        "vslot past the verifier": (lambda o: call(o, vslot=[4, 8, 6]), "(row 1)"),
        "verifier columns no multiple of its rows": (lambda o: call(o, v=new(m_b, 8 * m_b + 1)), "shape mismatch"),
        "verifier rows": (lambda o: call(o, v=new(m_b + 1, 8 * (m_b + 1))), "shape mismatch"),
        "verifier of no blocks": (lambda o: call(o, v=new(m_b, 0)), "shape mismatch"),
        "b_1 columns": (lambda o: call(o, b=new(d, m_b + 1)), "shape mismatch"),
        "pubkey sum columns": (lambda o: call(o, s=swap(sums, 1, new(d, m_g + 1))), "(gate 1)"),
        "a_out rows": (lambda o: call(o, ao=swap(a_outs, 1, new(d + 1, m_g))), "shape mismatch"),
        "output columns": (lambda o: call(swap(o, 2, new(d, m_g))), "(row 2)"),
        "output rows": (lambda o: call(swap(o, 1, new(d + 1, m_b))), "shape mismatch"),
        "b_1 of another context": (lambda o: call(o, b=new(d, m_b, other)), "context mismatch"),
        "verifier of another context": (lambda o: call(o, v=new(m_b, 8 * m_b, other)), "context mismatch"),
        "pubkey sum of another context": (lambda o: call(o, s=swap(sums, 1, new(d, m_g, other))), "context mismatch (gate 1)"),
        "output of another context": (lambda o: call(swap(o, 1, new(d, m_b, other))), "context mismatch (row 1)"),
        "b_1 of another level": (lambda o: call(o, b=new(d, m_b, level=0)), "level mismatch"),
        "verifier of another level": (lambda o: call(o, v=new(m_b, 8 * m_b, level=0)), "level mismatch"),
        "a_out of another level": (lambda o: call(o, ao=swap(a_outs, 1, new(d, m_g, level=0))), "level mismatch (gate 1)"),
        "output of another level": (lambda o: call(swap(o, 2, new(d, m_b, level=0))), "level mismatch (row 2)"),
        "b_1 not EVAL": (lambda o: call(o, b=coeff["b_1"]), "Eval"),
        "verifier not EVAL": (lambda o: call(o, v=coeff["verifier"]), "Eval"),
        "pubkey sum not EVAL": (lambda o: call(o, s=swap(sums, 1, coeff["sum"])), "Eval"),
        "a_out not EVAL": (lambda o: call(o, ao=swap(a_outs, 0, coeff["a_out"])), "Eval"),
        "words_per_y 0": (lambda o: call(o, words=0), "words_per_y"),
        "base_bits 0": (lambda o: call(o, base_bits=0), "base_bits"),
        "base_bits 63": (lambda o: call(o, base_bits=63), "base_bits"),
        "idx + 1 a multiple of q_0": (lambda o: call(o, idx=[1, int(moduli[0]) - 1, 3]), "(row 1)"),
        "idx + 1 a multiple of q_1": (lambda o: call(o, idx=[1, 2, 5 * int(moduli[1]) - 1]), "(row 2)"),
        "unknown tag form": (lambda o: call(o, tags=bad_form), ""),
        "the same output twice": (lambda o: call([o[0], o[1], o[0]]), "overlap"),
        "output overlaps b_1": (lambda o: call(swap(o, 1, rows_of(b_1, 0, d))), "overlap"),
        "output overlaps the verifier": (lambda o: call(swap(o, 2, rows_of(ver, 3, 3 + d))), "overlap"),
        "output overlaps a gate's operand": (lambda o: call(swap(o, 0, rows_of(wide_op, 0, d)), s=swap(sums, 0, wide_op.reshape_view(d * m_b, m_g).row_view(0, d))),
                                             "overlap"),
    }
    held_mats = [b_1, ver, wide_op] + sums + a_outs
    held = [m.to_rns() for m in held_mats]

    def check(name, fn, word, entry=ENTRY):
        # COEFF-tagged: a tag flipped to EVAL would change the read-out
        outs = [M.from_rns(p, sentinel, False) for _ in range(T)]
        before = [(o.is_ntt, o.to_rns()) for o in outs]
        _ffi.trace_begin()
        c0 = lib.gpupoly_launch_count()
        rc = fn(outs)
        msg = _ffi.last_error_string()
        assert _ffi.trace_end() == [] and lib.gpupoly_launch_count() == c0, name
        assert rc != 0, name
        assert entry + ":" in msg and word in msg, (name, msg)
        for o, (tag, res) in zip(outs, before):
            assert o.is_ntt == tag and np.array_equal(o.to_rns(), res), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # two outputs overlapping through views of one parent
    parent = M.from_rns(p, oracle.random_matrix(94, 3 * d + 1, m_b, moduli, n), False)
    before = parent.to_rns()
    views = [parent.row_view(0, d), parent.row_view(0, d), parent.row_view(2 * d, 3 * d)]  # two objects over the same rows
    c0 = lib.gpupoly_launch_count()
    assert call(views) != 0 and "overlap" in _ffi.last_error_string() and ENTRY in _ffi.last_error_string()
    assert lib.gpupoly_launch_count() == c0 and np.array_equal(parent.to_rns(), before)
    for m, res in zip(held_mats, held):
        assert np.array_equal(m.to_rns(), res)
    # the same call succeeds once the fault is gone - disjoint row views as outputs included - and T = 0 launches nothing
    outs = [M.from_rns(p, sentinel, False) for _ in range(T)]
    assert call(outs) == 0
    disjoint = [parent.row_view(t * d, (t + 1) * d) for t in range(3)]
    assert call(disjoint) == 0
    for i, o, v in zip([3, 0, 5], outs, disjoint):
        o.is_ntt = v.is_ntt = True
        assert o == v and o == wd.literal[i]
    c0 = lib.gpupoly_launch_count()
    assert call([], T_=0) == 0
    assert call([], T_=0, arr=False, b=None, v=None, vslot=None, s=None, ao=None, ngates=0, gate=None, y=None, idx=None, tags=None) == 0
    assert lib.gpupoly_launch_count() == c0
    # the combine entry names itself, counts R and the digits as operands and takes any keying
    r_st, digits = new(d, T * m_b), new(m_g, T * m_b)
    g_arr = np.array(a["gate_of_row"], dtype=np.uint32)

    def combine(outs, r=r_st, dg=digits, ngates=2):
        return lib.gpupoly_matrix_commit_lut_messages_combine(array(outs), T, None if r is None else r.raw, None if dg is None else dg.raw, array(sums),
                                                              array(a_outs), ngates, g_arr.ctypes.data_as(u32p), base, y_arr.ctypes.data_as(u64p), wpy)

    check("combine: digits shape", lambda o: combine(o, dg=new(m_g, T * m_b + 1)), "shape", COMBINE)
    check("combine: r_stacked shape", lambda o: combine(o, r=new(d + 1, T * m_b)), "shape", COMBINE)
    check("combine: null digits", lambda o: combine(o, dg=None), "null", COMBINE)
    check("combine: no gates", lambda o: combine(o, ngates=0), "gates", COMBINE)
    check("combine: output overlaps the digits", lambda o: combine(swap(o, 1, rows_of(digits, 0, d))), "overlap", COMBINE)
    check("combine: output overlaps r_stacked", lambda o: combine(swap(o, 1, rows_of(r_st, 1, 1 + d))), "overlap", COMBINE)
    # the reference's own keying has no block form: "unsupported", and the mirror falls back to the per-row loop
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda o: call(o), "unsupported")
    assert combine([M.from_rns(p, sentinel, False) for _ in range(T)]) == 0  # no sampling: any keying
    fallen = wd.stream.message_blocks([3, 0])
    want = wd.stream.message_blocks_literal([3, 0])
    for t in range(2):
        assert fallen[t] == want[t] and not (fallen[t] == wd.literal[[3, 0][t]])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert wd.stream.message_blocks([3])[0] == wd.literal[3]
    del keep, keep2


def test_an_index_without_an_inverse_in_a_12_bit_class_is_refused(gpu):
    """idx = q_0 - 1 fits every word there is: idx + 1 = 0 mod q_0 has no inverse"""
    from mxx_amd import _ffi

    n, d = 64, 1
    moduli = _moduli(n, 12)
    p = _params(gpu, n, moduli, 6)
    M, lib = gpu.GpuDCRTPolyMatrix, _ffi.lib()
    k = len(moduli) * P.digits_per_tower(moduli, 6)
    m_g, m_b = d * k, d * (k + 2)
    rng = np.random.default_rng(77)
    up = lambda rows, cols: M.from_rns(p, _rand(rng, rows, cols, moduli, n), True)  # noqa: E731
    b_1, ver, sums, a_out = up(d, m_b), up(m_b, 2 * m_b), up(d, m_g), up(d, m_g)
    sentinel = _rand(rng, d, m_b, moduli, n)
    outs = [M.from_rns(p, sentinel, False) for _ in range(2)]
    c0 = lib.gpupoly_launch_count()
    with pytest.raises(_ffi.GpuPolyError) as err:
        M.commit_lut_messages(b_1, ver, [0, 1], [sums], [a_out], [0, 0], [5, 6], [3, int(moduli[0]) - 1], KEY, [b"R_1_3", b"R_1_x"], outs=outs)
    assert ENTRY + ":" in str(err.value) and "inverse" in str(err.value) and "(row 1)" in str(err.value)
    assert lib.gpupoly_launch_count() == c0
    for o in outs:
        o.is_ntt = False  # the mirror's tag follows the library's, which the refusal left alone
        assert np.array_equal(o.to_rns(), sentinel)
    # the neighbouring index is served, and equals the formula through the older operations
    from mxx_amd import commit_lookup as cl

    idx = int(moduli[0]) - 2
    got = M.commit_lut_messages(b_1, ver, [1], [sums], [a_out], [0], [6], [idx], KEY, [b"R_1_y"])[0]
    r = gpu.GpuDCRTPolyHashSampler().sample_hash(p, KEY, b"R_1_y", d, m_b, gpu.DistType.FinRingDist())
    canc = cl.derive_canceler_matrix(p, b_1, ver.slice_columns(m_b, 2 * m_b), r, idx)
    head = a_out - M.gadget_matrix(p, d) * gpu.GpuDCRTPoly.from_elem_to_constant(p, 6)
    assert got == head.concat_columns([M.zero(p, d, m_b - m_g)]) + r - sums * canc.decompose()


# ---------------------------------------------------------------------------------------------------
# 5. end to end, noise-free: the reference's test_commit_plt_eval_single_input on the shared Wee25 parameters
# ---------------------------------------------------------------------------------------------------
def test_noise_free_lookup_returns_the_encoding_of_the_lut_value(gpu, oracle):
    from mxx_amd import bgg, commit_lookup as cl
    from test_gpu_wee25_commit import KEY as WKEY, SECRET, SIGMA as WSIGMA, TREE_BASE as WBASE, concat, state

    w, _, _, pp = state(gpu, oracle)
    p, d = w.params, SECRET
    M, Poly = gpu.GpuDCRTPolyMatrix, gpu.GpuDCRTPoly
    plt = {k: (k, k % 2) for k in range(4)}  # setup_lsb_bit_lut (:658-674) with four rows
    gate_id, lut_id, x = 5, 0, 3
    pubkeys = bgg.BGGPublicKeySampler(WKEY, d).sample(p, b"commit_plt_eval", [True])
    s_mat = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, 1, d, gpu.DistType.TernaryDist())
    secrets = [s_mat.entry(0, j) for j in range(d)]
    plaintexts = [Poly.from_usize_to_constant(p, x)]
    enc_one, enc1 = bgg.BGGEncodingSampler(p, secrets, None).sample(p, pubkeys, plaintexts)
    trap = gpu.GpuDCRTPolyTrapdoorSampler(p, WSIGMA)
    b0_trapdoor, b0 = trap.trapdoor(p, d)
    s_vec = M.from_poly_vec(p, [secrets])
    c_b0 = s_vec * b0
    # the public-key evaluator, then the commitment of every LUT matrix
    key_eval = cl.CommitBGGPubKeyPltEvaluator.setup(p, d, WSIGMA, WBASE, WKEY, pp)
    result_pubkey = key_eval.public_lookup(p, plt, enc_one.pubkey, enc1.pubkey, gate_id, lut_id)
    gate_states, luts = list(key_eval.gate_states.values()), dict(key_eval.luts)
    preimage = key_eval.commit_all_lut_matrices(p, b0, b0_trapdoor)
    stream, cache = key_eval.stream, key_eval.commit_cache
    assert (stream.padded_len, stream.lut_vector_len) == (4, 4) and set(cache) == {(0, 2), (2, 2), (0, 4)}
    assert b0 * preimage == cache[(0, 4)] + key_eval.b_1
    # the encoding evaluator
    c_b = s_vec * pp.b
    enc_eval = cl.CommitBGGEncodingPltEvaluator.setup(p, WSIGMA, WBASE, WKEY, luts, gate_states, c_b0, c_b, preimage, cache, pp)
    result = enc_eval.public_lookup(p, plt, enc_one, enc1, gate_id, lut_id)
    assert result.pubkey.matrix == result_pubkey.matrix and result.pubkey.reveal_plaintext
    expected_plaintext = Poly.from_elem_to_constant(p, plt[x][1])
    assert plt[x][1] == 1 and result.plaintext == expected_plaintext
    expected_vector = s_vec * (result.pubkey.matrix - M.gadget_matrix(p, d) * expected_plaintext)
    assert result.vector.size() == (1, w.m_g) and result.vector == expected_vector
    # the stream the evaluators built is the literal one, and the commitment opens to it
    blocks = enc_eval.msg_blocks
    for a, b in zip(blocks, stream.message_blocks_literal(range(4))):
        assert a == b
    col_range = range(2, 3)
    opening = w.open(blocks, col_range, pp, cache)
    assert w.verify(concat(blocks), cache[(0, 4)], opening, col_range, pp)
