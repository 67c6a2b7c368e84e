"""The commitment-based public lookup (src/lookup/commit_eval.rs): the third lookup back end of the reference, over the Wee25
commitment (mxx_amd/commit.py).  Every lookup gate g with LUT rows (idx, y) contributes one d x m_b message block per row to a
stream that is committed once; the block of row t is (build_msg_stream_for_lut_eval, :417-522)

    R_t        = sample_hash(key, "R_<g>_<idx_t>", d, m_b, FinRingDist)
    canceler_t = (B_1 V_t + R_t) * (idx_t + 1)^-1,                 V_t the verifier slice of stream position start_g + idx_t
    msg_t      = [ A_out_g - G_d * y_t | 0 ] + R_t - (A_in,g + A_one,g) G^-1(canceler_t),

so that the opening of position start_g + idx cancels everything but s (A_out - G y).  `lut_layout`, `compute_padded_len` and
`lut_gate_index` restate :524-585, the `derive_*` functions :587-637 with the reference's tag strings,
`message_block_literal` the per-row sequence of :461-517 statement by statement - the comparison leg - and
`CommitMsgStream.message_blocks` builds the blocks of a range in ONE library call (gpupoly_matrix_commit_lut_messages;
DESIGN.md section 5zb).  `CommitBGGPubKeyPltEvaluator` and `CommitBGGEncodingPltEvaluator` are the two evaluators with the
preimage of the commitment and the commit cache handed over in memory; the stream is built once and kept.  A LUT is a
mapping from the input x to its row (idx, y) - what `plt.get` gives - whose length is its row count.  Lookup buffers,
storage files and the circuit walk that collects the gate states are not mirrored: the gate states are passed in."""
from __future__ import annotations

from dataclasses import dataclass

from . import _ffi
from .bgg import BggEncoding, BggPublicKey
from .commit import Wee25Commit
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler
from .trapdoor import GpuDCRTPolyTrapdoorSampler

B1_TAG = b"COMMIT_LUT_B1"


# ---------------------------------------------------------------------- layout (:524-585)
@dataclass
class LutLayout:
    """LutLayout (:548-554); a gate range is (start, end, gate_id, lut_id, one_pubkey, input_pubkey)"""

    lut_gate_start_ids: dict
    lut_vector_len: int
    padded_len: int
    gate_ranges: list


def compute_padded_len(tree_base: int, lut_vector_len: int) -> int:
    """:568-574"""
    padded_len = tree_base
    while padded_len < lut_vector_len:
        padded_len *= tree_base
    return padded_len


def lut_gate_index(start_ids: dict, gate_id: int, lut_input_index: int) -> int:
    """:576-585"""
    if gate_id not in start_ids:
        raise KeyError(f"missing LUT gate start id for gate {gate_id}")
    return start_ids[gate_id] + lut_input_index


def lut_layout(luts: dict, gate_states, tree_base: int) -> LutLayout:
    """build_lut_gate_layout and build_lut_layout_for_eval (:524-566): the gates sorted by id, each with the consecutive
    stream positions of its LUT's rows.  `gate_states` lists (gate_id, lut_id, one_pubkey, input_pubkey)."""
    ordered = sorted(gate_states, key=lambda state: state[0])
    start_ids, gate_ranges, cursor = {}, [], 0
    for gate_id, lut_id, one_pubkey, input_pubkey in ordered:
        if lut_id not in luts:
            raise KeyError(f"missing LUT for lut_id={lut_id}")
        start_idx = cursor
        end_idx = start_idx + len(luts[lut_id])
        start_ids[gate_id] = start_idx
        gate_ranges.append((start_idx, end_idx, gate_id, lut_id, one_pubkey, input_pubkey))
        cursor = end_idx
    gate_ranges.sort(key=lambda r: r[0])
    return LutLayout(start_ids, cursor, compute_padded_len(tree_base, cursor), gate_ranges)


# ---------------------------------------------------------------------- the derived matrices (:587-637)
def a_out_tag(gate_id: int) -> bytes:
    return f"A_OUT_{gate_id}".encode("ascii")


def r_g_i_tag(gate_id: int, index: int) -> bytes:
    return f"R_{gate_id}_{index}".encode("ascii")


def r_g_i_prefix(gate_id: int) -> bytes:
    return f"R_{gate_id}_".encode("ascii")


def derive_a_out_matrix(params, row_size: int, hash_key: bytes, gate_id: int, hash_name: str = "keccak256") -> GpuDCRTPolyMatrix:
    """:587-601"""
    m = row_size * params.modulus_digits()
    return GpuDCRTPolyHashSampler(hash_name).sample_hash(params, hash_key, a_out_tag(gate_id), row_size, m, DistType.FinRingDist())


def derive_r_g_i_matrix(params, row_size: int, m_b: int, hash_key: bytes, gate_id: int, index: int,
                        hash_name: str = "keccak256") -> GpuDCRTPolyMatrix:
    """:603-625"""
    return GpuDCRTPolyHashSampler(hash_name).sample_hash(params, hash_key, r_g_i_tag(gate_id, index), row_size, m_b, DistType.FinRingDist())


def derive_b_1_matrix(params, secret_size: int, m_b: int, hash_key: bytes, hash_name: str = "keccak256") -> GpuDCRTPolyMatrix:
    """:113-121, :254-262"""
    return GpuDCRTPolyHashSampler(hash_name).sample_hash(params, hash_key, B1_TAG, secret_size, m_b, DistType.FinRingDist())


def derive_canceler_matrix(params, b_1, verifier_slice, r_g_i, idx: int) -> GpuDCRTPolyMatrix:
    """:627-637; mod_inverse_mod_q is the inverse modulo the full modulus"""
    idx_inverse = pow(int(idx) + 1, -1, params.modulus())
    return (b_1 * verifier_slice + r_g_i) * GpuDCRTPoly.from_biguint_to_constant(params, idx_inverse)


def message_block_literal(params, b_1, verifier_slice, hash_key: bytes, gate_id: int, idx: int, y: int, one_pubkey_matrix,
                          input_pubkey_matrix, m_g: int, m_b: int, hash_name: str = "keccak256") -> GpuDCRTPolyMatrix:
    """The message block of one LUT row as the reference builds it (:480-516), statement by statement: the comparison leg."""
    secret_size = one_pubkey_matrix.nrow
    gadget = GpuDCRTPolyMatrix.gadget_matrix(params, secret_size)
    y_poly = GpuDCRTPoly.from_elem_to_constant(params, int(y))
    a_out = derive_a_out_matrix(params, secret_size, hash_key, gate_id, hash_name)
    r_g_i = derive_r_g_i_matrix(params, secret_size, m_b, hash_key, gate_id, idx, hash_name)
    canceler = derive_canceler_matrix(params, b_1, verifier_slice, r_g_i, idx)
    padded = (a_out - gadget * y_poly).concat_columns([GpuDCRTPolyMatrix.zero(params, secret_size, m_b - m_g)])
    pubkey_sum = input_pubkey_matrix + one_pubkey_matrix
    return padded + r_g_i - pubkey_sum * canceler.decompose()


# ---------------------------------------------------------------------- the stream
class CommitMsgStream:
    """The message stream of build_msg_stream_for_lut_eval (:417-522) over `gate_states` and `luts`: `padded_len` blocks of
    d x m_b, the rows of the gates in the layout's order and zero blocks behind them.  `verifier_of(positions)` gives
    [V_p for p in positions] side by side, m_b x (len * m_b); by default the commitment's verifier over the public
    parameters."""

    def __init__(self, params, wee25_commit: Wee25Commit, wee25_public_params, b_1, hash_key: bytes, luts: dict, gate_states,
                 hash_name: str = "keccak256", verifier_of=None):
        gate_states = list(gate_states)
        if not gate_states:
            raise ValueError("no LUT gates found for commit evaluator")
        self.params, self.commit, self.public_params, self.b_1 = params, wee25_commit, wee25_public_params, b_1
        self.hash_key, self.hash_name, self.luts = bytes(hash_key), hash_name, luts
        self.secret_size = gate_states[0][2].matrix.nrow
        self.m_g, self.m_b = wee25_commit.m_g, wee25_commit.m_b
        self.layout = lut_layout(luts, gate_states, wee25_commit.tree_base)
        self.padded_len, self.lut_vector_len = self.layout.padded_len, self.layout.lut_vector_len
        self._verifier_of = verifier_of
        self._gate = {}  # position in gate_ranges -> (pubkey sum, A_out)

    def __len__(self) -> int:
        return self.padded_len

    def verifier(self, positions) -> GpuDCRTPolyMatrix:
        positions = list(positions)
        if self._verifier_of is not None:
            return self._verifier_of(positions)
        return self.commit.verifier(self.padded_len, positions, self.public_params)

    def row(self, global_idx: int):
        """(position of the gate in the layout, gate_id, idx, y, verifier position) of stream position global_idx (:465-481)"""
        for g, (start, end, gate_id, lut_id, _, _) in enumerate(self.layout.gate_ranges):
            if start <= global_idx < end:
                lut_input_index = global_idx - start
                lut = self.luts[lut_id]
                if lut_input_index not in lut:
                    raise KeyError(f"LUT entry {lut_input_index} missing")
                idx, y = lut[lut_input_index]
                return g, gate_id, int(idx), int(y), start + int(idx)
        raise KeyError(f"missing LUT range for index {global_idx}")

    def gate_operands(self, g: int):
        """(A_in,g + A_one,g, A_out_g) of the gate at position g of the layout, made once"""
        if g not in self._gate:
            _, _, gate_id, _, one_pubkey, input_pubkey = self.layout.gate_ranges[g]
            a_out = derive_a_out_matrix(self.params, self.secret_size, self.hash_key, gate_id, self.hash_name).ensure_eval()
            self._gate[g] = ((input_pubkey.matrix + one_pubkey.matrix).ensure_eval(), a_out)
        return self._gate[g]

    def zero_block(self) -> GpuDCRTPolyMatrix:
        return GpuDCRTPolyMatrix.zero(self.params, self.secret_size, self.m_b)

    def message_blocks_literal(self, index_range) -> list:
        """The closure of :450-519 over `index_range`, one row at a time: the comparison leg."""
        index_range = list(index_range)
        if not index_range:
            return []
        verifier_range = self.verifier(index_range)
        place = {pos: j for j, pos in enumerate(index_range)}
        out = []
        for global_idx in index_range:
            if global_idx >= self.lut_vector_len:
                out.append(self.zero_block())
                continue
            g, gate_id, idx, y, verifier_idx = self.row(global_idx)
            if verifier_idx in place:
                local_idx = place[verifier_idx]
                verifier_slice = verifier_range.slice_columns(self.m_b * local_idx, self.m_b * (local_idx + 1))
            else:
                verifier_slice = self.verifier([verifier_idx])
            _, _, _, _, one_pubkey, input_pubkey = self.layout.gate_ranges[g]
            out.append(message_block_literal(self.params, self.b_1, verifier_slice, self.hash_key, gate_id, idx, y, one_pubkey.matrix,
                                             input_pubkey.matrix, self.m_g, self.m_b, self.hash_name))
        return out

    def message_blocks(self, index_range) -> list:
        """The blocks of the stream positions `index_range`: ONE library call for the rows below lut_vector_len and zero
        matrices for the padding.  The verifier slices come from one verifier call over the positions the rows name; the tags
        go in the indexed decimal form where the rows are one gate's with consecutive indices, and as a table otherwise.
        Where the library answers "unsupported" (MXX_HIP_RNG_COMPAT=reference) and for hashes without a device form the
        literal loop runs: the same matrices either way."""
        index_range = list(index_range)
        live = [i for i in index_range if i < self.lut_vector_len]
        if not live or not GpuDCRTPolyHashSampler(self.hash_name)._on_device():
            return self.message_blocks_literal(index_range)
        rows = [self.row(i) for i in live]
        positions = sorted({r[4] for r in rows})
        slot = {pos: j for j, pos in enumerate(positions)}
        gates = sorted({r[0] for r in rows})
        gate_at = {g: j for j, g in enumerate(gates)}
        operands = [self.gate_operands(g) for g in gates]
        idxs = [r[2] for r in rows]
        if len(gates) == 1 and all(b == a + 1 for a, b in zip(idxs, idxs[1:])):
            tags = IndexedTags(r_g_i_prefix(rows[0][1]), idxs[0], len(idxs), decimal=True)
        else:
            tags = [r_g_i_tag(r[1], r[2]) for r in rows]
        try:
            made = GpuDCRTPolyMatrix.commit_lut_messages(self.b_1.ensure_eval(), self.verifier(positions).ensure_eval(), [slot[r[4]] for r in rows],
                                                         [sums for sums, _ in operands], [a_out for _, a_out in operands],
                                                         [gate_at[r[0]] for r in rows], [r[3] for r in rows], idxs, self.hash_key, tags,
                                                         self.hash_name)
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
            return self.message_blocks_literal(index_range)
        made = dict(zip(live, made))
        return [made[i] if i in made else self.zero_block() for i in index_range]


# ---------------------------------------------------------------------- the evaluators
class CommitBGGPubKeyPltEvaluator:
    """CommitBGGPubKeyPltEvaluator (:76-208)"""

    def __init__(self, params, hash_key: bytes, trapdoor_sigma: float, wee25_commit: Wee25Commit, wee25_public_params, b_1,
                 hash_name: str = "keccak256"):
        self.params, self.hash_key, self.trapdoor_sigma, self.hash_name = params, bytes(hash_key), float(trapdoor_sigma), hash_name
        self.wee25_commit, self.wee25_public_params, self.b_1 = wee25_commit, wee25_public_params, b_1
        self.gate_states, self.luts = {}, {}
        self.commit_cache, self.stream = None, None

    @classmethod
    def setup(cls, params, secret_size: int, trapdoor_sigma: float, tree_base: int, hash_key: bytes, wee25_public_params,
              hash_name: str = "keccak256") -> "CommitBGGPubKeyPltEvaluator":
        """:97-134"""
        wee25_commit = Wee25Commit(params, secret_size, tree_base, trapdoor_sigma, hash_name)
        assert wee25_public_params.b.ncol == wee25_commit.m_b, "wee25 public params column size mismatch"
        b_1 = derive_b_1_matrix(params, secret_size, wee25_commit.m_b, hash_key, hash_name)
        return cls(params, hash_key, trapdoor_sigma, wee25_commit, wee25_public_params, b_1, hash_name)

    def public_lookup(self, params, plt, one: BggPublicKey, input: BggPublicKey, gate_id: int, lut_id: int) -> BggPublicKey:
        """:187-207"""
        self.luts.setdefault(lut_id, plt)
        row_size = input.matrix.nrow
        self.gate_states[gate_id] = (gate_id, lut_id, one, input)
        return BggPublicKey(derive_a_out_matrix(params, row_size, self.hash_key, gate_id, self.hash_name), True)

    def commit_all_lut_matrices(self, params, b0_matrix, b0_trapdoor, _seeds=None) -> GpuDCRTPolyMatrix:
        """:136-179: the stream over the collected gates, its commitment, and the preimage of commit + B_1 under the
        trapdoor of b0 - returned, where the reference puts it into a lookup buffer.  The commitment's nodes stay in
        `self.commit_cache`, the stream in `self.stream`."""
        luts, self.luts = self.luts, {}
        gate_states, self.gate_states = list(self.gate_states.values()), {}
        self.stream = CommitMsgStream(params, self.wee25_commit, self.wee25_public_params, self.b_1, self.hash_key, luts, gate_states,
                                      self.hash_name)
        blocks = self.stream.message_blocks(range(self.stream.padded_len))
        self.commit_cache = {}
        commit = self.wee25_commit.commit(blocks, self.wee25_public_params, self.commit_cache)
        target = commit + self.b_1
        trapdoor_sampler = GpuDCRTPolyTrapdoorSampler(params, self.trapdoor_sigma)
        return trapdoor_sampler.preimage(params, b0_trapdoor, b0_matrix, target, _seeds=_seeds)


class CommitBGGEncodingPltEvaluator:
    """CommitBGGEncodingPltEvaluator (:210-408).  `setup` takes the gate states and LUTs that the reference's collector pass
    over the circuit gathers, and the preimage of the commitment and the commit cache in memory."""

    def __init__(self, params, wee25_commit, wee25_public_params, hash_key, b_1, c_b, c_commit, commit_cache, luts, gate_states, stream,
                 hash_name: str = "keccak256"):
        self.params, self.wee25_commit, self.wee25_public_params = params, wee25_commit, wee25_public_params
        self.hash_key, self.hash_name, self.b_1, self.c_b, self.c_commit = bytes(hash_key), hash_name, b_1, c_b, c_commit
        self.commit_cache, self.luts, self.gate_states, self.stream = commit_cache, luts, gate_states, stream
        self.lut_gate_start_ids = stream.layout.lut_gate_start_ids
        self.msg_blocks = stream.message_blocks(range(stream.padded_len))  # built once and kept

    @classmethod
    def setup(cls, params, trapdoor_sigma: float, tree_base: int, hash_key: bytes, luts: dict, gate_states, c_b0, c_b, preimage,
              commit_cache: dict, wee25_public_params, hash_name: str = "keccak256") -> "CommitBGGEncodingPltEvaluator":
        """:236-328"""
        gate_states = list(gate_states)
        secret_size = gate_states[0][2].matrix.nrow
        wee25_commit = Wee25Commit(params, secret_size, tree_base, trapdoor_sigma, hash_name)
        b_1 = derive_b_1_matrix(params, secret_size, wee25_commit.m_b, hash_key, hash_name)
        stream = CommitMsgStream(params, wee25_commit, wee25_public_params, b_1, hash_key, luts, gate_states, hash_name)
        assert (0, stream.padded_len) in commit_cache, "commit cache not found for this stream length"
        c_commit = c_b0 * preimage
        return cls(params, wee25_commit, wee25_public_params, hash_key, b_1, c_b, c_commit, commit_cache, luts, gate_states, stream, hash_name)

    def public_lookup(self, params, plt, one: BggEncoding, input: BggEncoding, gate_id: int, lut_id: int) -> BggEncoding:
        """:336-407"""
        x = input.plaintext
        assert x is not None, "the BGG encoding should reveal plaintext for public lookup"
        x_u64 = x.const_coeff_u64()
        if x_u64 not in plt:
            raise KeyError(f"{x_u64} not found in LUT for gate {gate_id}")
        k, y = plt[x_u64]
        k, y = int(k), int(y)
        y_poly = GpuDCRTPoly.from_elem_to_constant(params, y)
        lut_vector_idx = lut_gate_index(self.lut_gate_start_ids, gate_id, k)
        col_range = range(lut_vector_idx, lut_vector_idx + 1)
        opening = self.wee25_commit.open(self.msg_blocks, col_range, self.wee25_public_params, self.commit_cache)
        verifier = self.wee25_commit.verifier(self.stream.padded_len, col_range, self.wee25_public_params)
        secret_size = input.pubkey.matrix.nrow
        m_b = self.wee25_commit.m_b
        r_g_i = derive_r_g_i_matrix(params, secret_size, m_b, self.hash_key, gate_id, k, self.hash_name)
        canceler = derive_canceler_matrix(params, self.b_1, verifier, r_g_i, k)
        c_lut = self.c_commit * verifier + self.c_b * opening
        c_x = (input.vector + one.vector) * canceler.decompose()
        c_out = (c_lut + c_x).slice_columns(0, self.wee25_commit.m_g)
        a_out = derive_a_out_matrix(params, secret_size, self.hash_key, gate_id, self.hash_name)
        return BggEncoding(c_out, BggPublicKey(a_out, True), y_poly)
