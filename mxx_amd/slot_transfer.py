"""The slot-transfer public key's gate preimage targets (src/slot_transfer/bgg_pubkey_gpu.rs:371-407,409-471): one target
per destination slot and column chunk of the wave that sample_gate_batch_gpu builds (:820-950),

    target_t = s_t A_out[:, chunk]  -  (lhs_t G^-1(a_t[:, chunk])) o scalar_t  +  E_t,

A_out the gate's d x m_g hash sample ("slot_transfer_gate_a_out_<gate>"), d = secret_size, m_g = d * modulus_digits, and for
the slot-reduce gates ("slot_reduce_gate_a_out_<gate>") with sum_src (s_src a_in_t) G^-1(a_t[:, chunk]) x^src in the middle.
`build_gate_target_chunk` and `build_slot_reduce_gate_target_chunk` are the reference's functions restated with the mirror's
operations, one request at a time; `gate_target_chunks` and `slot_reduce_gate_target_chunks` build the targets of a wave of
requests with a number of launches that does not depend on the wave (gpupoly_matrix_mul_decompose_pairs; DESIGN.md section
5t); `sample_gate_preimages` feeds them into the batched preimage.  The second half of the file is the online side, what an
evaluator runs once per gate, slot and evaluation (src/slot_transfer/bgg_poly_encoding.rs:119-386): see the comment there."""
from __future__ import annotations

from dataclasses import dataclass, field

from . import _ffi
from .lookup import sample_error_matrix
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler, sample_gpu_stack_with_seeds


@dataclass
class SlotGateShared:
    """What every request of a wave shares (GpuSlotGateDeviceShared of the reference plus the key and the secret size)."""

    params: object
    hash_key: bytes
    secret_size: int
    hash_name: str = "keccak256"

    @property
    def m_g(self) -> int:
        return self.secret_size * self.params.modulus_digits()

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    def a_out_tag(self, gate_id: int) -> bytes:
        return f"slot_transfer_gate_a_out_{gate_id}".encode("ascii")

    def reduce_a_out_tag(self, gate_id: int) -> bytes:
        return f"slot_reduce_gate_a_out_{gate_id}".encode("ascii")

    def a_out_columns(self, tag: bytes, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
        return self.sampler().sample_hash_columns(self.params, self.hash_key, tag, self.secret_size, self.m_g, col_start, col_len,
                                                  DistType.FinRingDist())


def build_gate_target_chunk(shared: SlotGateShared, gate_id, lhs_input, s_j, a_j, scalar_poly, error_seed, error_sigma, col_start,
                            col_len) -> GpuDCRTPolyMatrix:
    """build_gate_target_chunk_gpu (bgg_pubkey_gpu.rs:371-407), statement by statement: the comparison leg."""
    p, d = shared.params, shared.secret_size
    lhs_chunk = s_j * shared.a_out_columns(shared.a_out_tag(gate_id), col_start, col_len)
    a_j_chunk = a_j.slice_columns(col_start, col_start + col_len).decompose()
    rhs_chunk = lhs_input * a_j_chunk
    if scalar_poly is not None:
        rhs_chunk = rhs_chunk.mul_scalar(scalar_poly)
    target_chunk = lhs_chunk - rhs_chunk
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def build_slot_reduce_gate_target_chunk(shared: SlotGateShared, gate_id, a_in, dst_slot, slot_secrets, slot_as, error_seed, error_sigma,
                                        col_start, col_len) -> GpuDCRTPolyMatrix:
    """build_slot_reduce_gate_target_chunk_gpu (bgg_pubkey_gpu.rs:409-471): `slot_secrets[s]` (d x d) and `slot_as[s]` (d x m_g)
    by slot, num_slots = len(slot_secrets); one product against the digit matrix per source slot."""
    p, d = shared.params, shared.secret_size
    s_dst = slot_secrets[dst_slot]
    lhs_chunk = s_dst * shared.a_out_columns(shared.reduce_a_out_tag(gate_id), col_start, col_len)
    a_dst_chunk = slot_as[dst_slot].slice_columns(col_start, col_start + col_len).decompose()
    rhs_acc = GpuDCRTPolyMatrix.zero(p, d, col_len)
    for src_slot in range(len(slot_secrets)):
        lhs_input = slot_secrets[src_slot] * a_in
        scalar_poly = GpuDCRTPolyMatrix.monomial(p, 1, 1, src_slot)
        rhs_chunk = (lhs_input * a_dst_chunk).mul_scalar(scalar_poly)
        rhs_acc.add_in_place(rhs_chunk)
    target_chunk = lhs_chunk - rhs_acc
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def _stack_rows(mats) -> GpuDCRTPolyMatrix:
    """[mats[0]; mats[1]; ..] of matrices of one shape in one launch per 64 of them: row-major storage makes the stack the
    concatenation of the blocks' polynomials, so each goes in as one 1 x (rows cols) row"""
    nrow, ncol = mats[0].nrow, mats[0].ncol
    for m in mats:
        assert (m.nrow, m.ncol) == (nrow, ncol), "stacked matrices share one shape"
    flat = GpuDCRTPolyMatrix.concat_columns_of([m.ensure_eval().reshape_view(1, nrow * ncol) for m in mats])
    return flat.reshape_view(len(mats) * nrow, ncol)


def _target_stack(shared: SlotGateShared, tag: bytes, s_list, error_seeds, error_sigma, chunk) -> GpuDCRTPolyMatrix:
    """[s_0; s_1; ..] A_out[:, chunk] + [E_0; E_1; ..]: one stacked product, one Gaussian block sample (none when error_sigma
    == 0, as in the reference) and their sum in place"""
    col_start, col_len = chunk
    p, d = shared.params, shared.secret_size
    assert error_sigma >= 0.0, f"error_sigma {error_sigma} must be nonnegative"
    count = len(s_list)
    stack = _stack_rows(s_list) * shared.a_out_columns(tag, col_start, col_len)
    if error_sigma != 0.0:
        prod = stack
        stack = sample_gpu_stack_with_seeds(p, d, col_len, DistType.GaussDist(error_sigma), error_seeds).reshape_view(count * d, col_len)
        stack.add_in_place(prod)
    return stack


def gate_target_chunks(shared: SlotGateShared, gate_id, lhs_inputs, s_js, a_js, scalars, error_seeds, error_sigma, chunk) -> list:
    """[build_gate_target_chunk(shared, gate_id, lhs_inputs[t], s_js[t], a_js[t], scalars[t], error_seeds[t], error_sigma,
    *chunk) for t] with launches that do not depend on the request count: the stack [s_t A_out[:, chunk] + E_t], then ONE
    mul_decompose_pairs that subtracts (lhs_t G^-1(a_t[:, chunk])) o scalar_t from its rows in place.  `scalars` may be None
    or hold None entries.  The targets are row views of the one stack (no copies; the batched preimage takes them as they
    are); modular sums are exact, so every target equals the per-request leg bit for bit."""
    lhs_inputs, s_js, a_js, error_seeds = list(lhs_inputs), list(s_js), list(a_js), list(error_seeds)
    count, d = len(s_js), shared.secret_size
    scalars = [None] * count if scalars is None else list(scalars)
    assert len(lhs_inputs) == len(a_js) == len(scalars) == len(error_seeds) == count, "gate_target_chunks: one entry per request"
    if count == 0:
        return []
    col_start, col_len = chunk
    stack = _target_stack(shared, shared.a_out_tag(gate_id), s_js, error_seeds, error_sigma, chunk)
    rows = [stack.row_view(t * d, (t + 1) * d) for t in range(count)]
    GpuDCRTPolyMatrix.mul_decompose_pairs(lhs_inputs, a_js, col_start, col_len, scalars=scalars, addends=rows, negate=True, outs=rows)
    return rows


def slot_reduce_gate_target_chunks(shared: SlotGateShared, gate_id, a_ins, dst_slots, slot_secrets, slot_as, error_seeds, error_sigma,
                                   chunk) -> list:
    """[build_slot_reduce_gate_target_chunk(shared, gate_id, a_ins[t], dst_slots[t], slot_secrets, slot_as, error_seeds[t],
    error_sigma, *chunk) for t].  sum_src ((s_src a_in) D) x^src = (sum_src (s_src a_in) x^src) D holds exactly in R_q and
    every residue is canonical, so the num_slots products per request against the digit matrix D are never run: the left
    operands are ONE product of the stacked secrets by [a_in | a_in' | ..] (each distinct input once) and ONE monomial_sum
    over its row views, cut into the requests' operands by one split, and one mul_decompose_pairs covers all requests."""
    a_ins, dst_slots, error_seeds = list(a_ins), [int(s) for s in dst_slots], list(error_seeds)
    count, d, m_g = len(dst_slots), shared.secret_size, shared.m_g
    num_slots = len(slot_secrets)
    assert len(a_ins) == len(error_seeds) == count, "slot_reduce_gate_target_chunks: one entry per request"
    if count == 0:
        return []
    col_start, col_len = chunk
    secrets = [slot_secrets[s] for s in range(num_slots)]
    # the distinct inputs (the requests of one gate usually share theirs), each multiplied once
    distinct, where = [], {}
    for a in a_ins:
        if id(a) not in where:
            where[id(a)] = len(distinct)
            distinct.append(a.ensure_eval())
    wide = distinct[0] if len(distinct) == 1 else GpuDCRTPolyMatrix.concat_columns_of(distinct)
    prod = _stack_rows(secrets) * wide  # (num_slots d) x (inputs m_g)
    summed = GpuDCRTPolyMatrix.monomial_sum([prod.row_view(s * d, (s + 1) * d) for s in range(num_slots)], range(num_slots))
    lefts = [summed] if len(distinct) == 1 else summed.split_columns([m_g] * len(distinct))
    stack = _target_stack(shared, shared.reduce_a_out_tag(gate_id), [slot_secrets[s] for s in dst_slots], error_seeds, error_sigma, chunk)
    rows = [stack.row_view(t * d, (t + 1) * d) for t in range(count)]
    GpuDCRTPolyMatrix.mul_decompose_pairs([lefts[where[id(a)]] for a in a_ins], [slot_as[s] for s in dst_slots], col_start, col_len,
                                          addends=rows, negate=True, outs=rows)
    return rows


def sample_gate_preimages(shared: SlotGateShared, trap_sampler, trapdoor, public_matrix, targets, _seeds=None) -> list:
    """The preimages of a wave's targets for one column chunk - what sample_gate_batch_gpu hands to preimage_batched_sharded
    (bgg_pubkey_gpu.rs:842) for one device: `targets` from `gate_target_chunks` or `slot_reduce_gate_target_chunks`, then
    `preimage_many_abi` (one gpupoly_trapdoor_preimage_many call).  Returns [(target, preimage)] per request."""
    preimages = trap_sampler.preimage_many_abi(shared.params, trapdoor, public_matrix, targets, _seeds=_seeds)
    return list(zip(targets, preimages))


# ---------------------------------------------------------------------------------------------------------------------------
# The online side: what an evaluator runs once per gate, slot and evaluation (src/slot_transfer/bgg_poly_encoding.rs:119-386,
# on the device src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786).  With c_b0 the encoding under B0 (r x w0), Pg_s the stored
# gate preimage (w0 x m_g), P0_src (w0 x w1) and P1_s (w1 x m_g) the stored slot preimages and A_s the hash sample under
# "slot_transfer_slot_a_<s>", a destination slot s with terms t has
#
#     out_s = c_b0 Pg_s + sum_t x^shift_t o kappa_t o ( c_in_t G^-1(A_s) + mu_t o ((c_b0 P0_src_t) P1_s) ).
#
# `output_slot` and `slot_reduce_output_slot` are the reference's functions restated with the mirror's older operations, one
# destination at a time; `slot_transfer_slots` and `slot_reduce_slots` make the outputs of all destinations with stage 1 once
# per distinct source and ONE library call per output chunk (gpupoly_matrix_slot_transfer_eval);
# `slot_transfer` and `slot_reduce` are the whole gates with their output plaintexts.
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class SlotEvalShared:
    """What every destination slot of an evaluation shares: the key, the encoding c_b0 (r x w0, NTT domain) and the stored
    preimages, given as matrices through three accessors (reading them from storage is storage.py's): `p0_chunks(slot)` the
    column chunks of P0_slot in order, `p1_chunk(slot, col_start, col_len)` and `gate_chunk(gate_id, slot, col_start, col_len)`
    the chunk [col_start, col_start + col_len) of P1_slot and of Pg_(gate, slot)."""

    params: object
    hash_key: bytes
    secret_size: int
    c_b0: GpuDCRTPolyMatrix
    p0_chunks: object
    p1_chunk: object
    gate_chunk: object
    hash_name: str = "keccak256"
    _cache: dict = field(default_factory=dict, repr=False)

    @classmethod
    def from_matrices(cls, params, hash_key: bytes, secret_size: int, c_b0, p0_by_slot, p1_by_slot, gate_by_gate_slot,
                      hash_name: str = "keccak256") -> "SlotEvalShared":
        """the accessors over whole matrices: p0_by_slot[slot] (w0 x w1), p1_by_slot[slot] (w1 x m_g) and
        gate_by_gate_slot[(gate_id, slot)] (w0 x m_g); a chunk is sliced once and kept"""
        shared = cls(params, hash_key, secret_size, c_b0, None, None, None, hash_name)
        cache = shared._cache

        def cut(kind, key, full, col_start, col_len):
            at = (kind, key, col_start, col_len)
            if at not in cache:
                cache[at] = full if (col_start, col_len) == (0, full.ncol) else full.slice_columns(col_start, col_start + col_len)
            return cache[at]

        shared.p0_chunks = lambda slot: [p0_by_slot[slot]]
        shared.p1_chunk = lambda slot, col_start, col_len: cut("p1", slot, p1_by_slot[slot], col_start, col_len)
        shared.gate_chunk = lambda gate_id, slot, col_start, col_len: cut("pg", (gate_id, slot), gate_by_gate_slot[(gate_id, slot)], col_start, col_len)
        return shared

    @property
    def m_g(self) -> int:
        return self.secret_size * self.params.modulus_digits()

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    def slot_a_tag(self, dst_slot: int) -> bytes:
        return f"slot_transfer_slot_a_{dst_slot}".encode("ascii")

    def slot_a_tags(self, dst_slots):
        """the destinations' tags: generated on the device from the first index where they are consecutive, a table otherwise"""
        dst_slots = [int(s) for s in dst_slots]
        if dst_slots and dst_slots == list(range(dst_slots[0], dst_slots[0] + len(dst_slots))):
            return IndexedTags(b"slot_transfer_slot_a_", dst_slots[0], len(dst_slots), decimal=True)
        return [self.slot_a_tag(s) for s in dst_slots]

    def slot_a(self, dst_slot: int) -> GpuDCRTPolyMatrix:
        """slot_a_for_params (bgg_poly_encoding.rs:64-78)"""
        return self.sampler().sample_hash(self.params, self.hash_key, self.slot_a_tag(dst_slot), self.secret_size, self.m_g, DistType.FinRingDist())

    def column_chunks(self, chunk: int) -> list:
        """[(col_start, col_len)] of the m_g output columns in chunks of `chunk` (the last one may be shorter)"""
        chunk = int(chunk)
        assert chunk >= 1, "the column chunk has one column at least"
        return [(c0, min(chunk, self.m_g - c0)) for c0 in range(0, self.m_g, chunk)]


def _concat(parts) -> GpuDCRTPolyMatrix:
    """the reference's `if chunks.len() == 1 { the chunk } else { first.concat_columns_owned(rest) }`"""
    parts = list(parts)
    return parts[0] if len(parts) == 1 else parts[0].concat_columns(parts[1:])


def _constant_term(plaintext) -> int:
    """`src_plaintext.coeffs_biguints().into_iter().next()`: the constant coefficient, an integer below Q"""
    return int(plaintext.coeffs()[0])


def _literal_parts(shared: SlotEvalShared, gate_id, src_slot: int, dst_slot: int, chunk: int):
    """(c_transfer, c_gate) of one (source, destination): c_b0 against the P0 chunks, that against the P1 chunks, c_b0 against
    the gate chunks - one product per chunk and a concatenation, as the reference's left_mul_chunked_checkpoint_column loops"""
    c_b0 = shared.c_b0
    c_b0_slot_preimage_b0 = _concat([c_b0 * p0 for p0 in shared.p0_chunks(src_slot)])
    cols = shared.column_chunks(chunk)
    c_transfer = _concat([c_b0_slot_preimage_b0 * shared.p1_chunk(dst_slot, c0, cl) for c0, cl in cols])
    c_gate = _concat([c_b0 * shared.gate_chunk(gate_id, dst_slot, c0, cl) for c0, cl in cols])
    return c_transfer, c_gate


def output_slot(shared: SlotEvalShared, gate_id, input_vectors, plaintexts, src_slots, dst_slot: int, chunk: int):
    """output_slot_for_params (bgg_poly_encoding.rs:119-248), statement by statement: the comparison leg.  input_vectors[s]
    (r x m_g) and plaintexts[s] (a GpuDCRTPoly) by source slot, src_slots[dst] = (source slot, None or the u32 scalar).
    Returns (out_vector, output_plaintext)."""
    p = shared.params
    src_slot, scalar = src_slots[dst_slot]
    src_slot = int(src_slot)
    assert src_slot < len(input_vectors), f"source slot index {src_slot} out of range for input slot count {len(input_vectors)}"
    input_vector = input_vectors[src_slot]
    output_plaintext = GpuDCRTPoly.from_biguint_to_constant(p, _constant_term(plaintexts[src_slot]))
    c_transfer, c_gate = _literal_parts(shared, gate_id, src_slot, dst_slot, chunk)
    slot_a_decomposed = shared.slot_a(dst_slot).decompose()
    transfer_plaintext_term = c_transfer.mul_scalar(output_plaintext)
    pre_out = (input_vector * slot_a_decomposed) + transfer_plaintext_term
    if scalar is not None:
        scalar_poly = GpuDCRTPoly.from_usize_to_constant(p, int(scalar))
        pre_out = pre_out.mul_scalar(scalar_poly)
        output_plaintext = output_plaintext * scalar_poly
    return c_gate + pre_out, output_plaintext


def slot_reduce_output_slot(shared: SlotEvalShared, gate_id, inputs, plaintexts_by_input, dst_slot: int, num_slots: int, chunk: int):
    """slot_reduce_output_slot_for_params (bgg_poly_encoding.rs:250-386), statement by statement: inputs[dst][src] the input
    vectors of encoding `dst` by slot, plaintexts_by_input[dst][src] its plaintexts.  Returns (out_vector, output_plaintext)."""
    p = shared.params
    vectors = inputs[dst_slot]
    assert len(vectors) >= num_slots, f"slot_reduce input {dst_slot} has {len(vectors)} slots, expected at least {num_slots}"
    assert num_slots >= 1, "slot_reduce output slot requires at least one source slot"
    slot_a_decomposed = shared.slot_a(dst_slot).decompose()
    output_plaintext = GpuDCRTPoly.const_zero(p)
    pre_out_terms = []
    c_gate = None
    for src_slot in range(num_slots):
        input_vector = vectors[src_slot]
        plaintext_term = GpuDCRTPoly.from_biguint_to_constant(p, _constant_term(plaintexts_by_input[dst_slot][src_slot]))
        c_transfer, gate = _literal_parts(shared, gate_id, src_slot, dst_slot, chunk)
        c_gate = gate if c_gate is None else c_gate
        monomial = [0] * p.ring_dimension()
        monomial[src_slot] = 1
        scalar_poly = GpuDCRTPoly.from_u32s(p, monomial)
        output_plaintext = output_plaintext + plaintext_term * scalar_poly
        transfer_plaintext_term = c_transfer.mul_scalar(plaintext_term)
        pre_out_terms.append(((input_vector * slot_a_decomposed) + transfer_plaintext_term).mul_scalar(scalar_poly))
    pre_out = pre_out_terms[0]
    for term in pre_out_terms[1:]:
        pre_out = pre_out + term
    return c_gate + pre_out, output_plaintext


def transfer_mids(shared: SlotEvalShared, sources) -> dict:
    """STAGE 1: {src: c_b0 P0_src} for the distinct sources, one product per stored chunk of P0_src in ONE mul_batch call, the
    chunks of a source concatenated"""
    distinct = sorted({int(s) for s in sources})
    chunks = [shared.p0_chunks(s) for s in distinct]
    flat = [c for cs in chunks for c in cs]
    prods = GpuDCRTPolyMatrix.mul_batch([shared.c_b0] * len(flat), flat) if flat else []
    mids, at = {}, 0
    for s, cs in zip(distinct, chunks):
        mids[s] = _concat(prods[at:at + len(cs)])
        at += len(cs)
    return mids


def _eval_slots(shared: SlotEvalShared, gate_id, dst_slots, terms_by_out, chunk: int, literal) -> list:
    """the r x m_g outputs of the destinations `dst_slots` from their terms, one library call per output chunk writing in
    place; `literal(dst)` is the per-slot leg where the library answers "unsupported" or the hash has no device form"""
    dst_slots = list(dst_slots)
    if not dst_slots:
        return []
    if shared.sampler()._on_device():
        c_b0 = shared.c_b0
        outs = [GpuDCRTPolyMatrix(shared.params, c_b0.nrow, shared.m_g, c_b0.level, True) for _ in dst_slots]
        tags = shared.slot_a_tags(dst_slots)
        try:
            for c0, cl in shared.column_chunks(chunk):
                GpuDCRTPolyMatrix.slot_transfer_eval(outs, c_b0, [shared.gate_chunk(gate_id, s, c0, cl) for s in dst_slots],
                                                     [shared.p1_chunk(s, c0, cl) for s in dst_slots], terms_by_out, c0, shared.hash_key, tags,
                                                     shared.hash_name, dst_col=c0)
            return outs
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
    return [literal(s) for s in dst_slots]


def slot_transfer_slots(shared: SlotEvalShared, gate_id, input_vectors, mus, src_slots, chunk: int) -> list:
    """[output_slot(..., dst, chunk)[0] for every destination dst] - the loop of evaluate_slot_transfer_slots_gpu
    (bgg_poly_encoding_gpu.rs:748-786) - with c_b0 P0_src once per distinct source and ONE library call per output chunk.
    mus[s] is the constant coefficient of source slot s's plaintext, src_slots[dst] = (source, None or scalar)."""
    src_slots = [(int(s), None if k is None else int(k)) for s, k in src_slots]
    mids = transfer_mids(shared, [s for s, _ in src_slots])
    terms = [[(input_vectors[s], mids[s], 0, 1 if k is None else k, int(mus[s]))] for s, k in src_slots]

    def literal(dst):
        plaintexts = {s: GpuDCRTPoly.from_biguint_to_constant(shared.params, int(mus[s])) for s in {src_slots[dst][0]}}
        return output_slot(shared, gate_id, input_vectors, plaintexts, src_slots, dst, chunk)[0]

    return _eval_slots(shared, gate_id, range(len(src_slots)), terms, chunk, literal)


def slot_reduce_slots(shared: SlotEvalShared, gate_id, inputs, mus, num_slots: int, chunk: int) -> list:
    """[slot_reduce_output_slot(..., dst, num_slots, chunk)[0] for dst < len(inputs)]: inputs[dst][src] the input vectors,
    mus[dst][src] the constant coefficients of their plaintexts.  The num_slots products per destination against P1_dst and
    G^-1(A_dst) become one: the terms' left factors are summed first."""
    num_slots = int(num_slots)
    assert num_slots >= 1, "slot_reduce output slot requires at least one source slot"
    mids = transfer_mids(shared, range(num_slots)) if len(inputs) else {}
    terms = [[(inputs[dst][src], mids[src], src, 1, int(mus[dst][src])) for src in range(num_slots)] for dst in range(len(inputs))]

    def literal(dst):
        plaintexts = {dst: [GpuDCRTPoly.from_biguint_to_constant(shared.params, int(mu)) for mu in mus[dst][:num_slots]]}
        return slot_reduce_output_slot(shared, gate_id, inputs, plaintexts, dst, num_slots, chunk)[0]

    return _eval_slots(shared, gate_id, range(len(inputs)), terms, chunk, literal)


def slot_transfer(shared: SlotEvalShared, gate_id, input_vectors, plaintexts, src_slots, chunk: int):
    """The whole slot_transfer gate: (output vectors, output plaintexts) per destination, the plaintexts const(mu_src) * kappa"""
    p = shared.params
    mus = {s: _constant_term(plaintexts[s]) for s in {int(s) for s, _ in src_slots}}
    vectors = slot_transfer_slots(shared, gate_id, input_vectors, mus, src_slots, chunk)
    outs = []
    for s, k in src_slots:
        pt = GpuDCRTPoly.from_biguint_to_constant(p, mus[int(s)])
        outs.append(pt if k is None else pt * GpuDCRTPoly.from_usize_to_constant(p, int(k)))
    return vectors, outs


def slot_reduce(shared: SlotEvalShared, gate_id, inputs, plaintexts_by_input, num_slots: int, chunk: int):
    """The whole slot_reduce gate: (output vectors, output plaintexts) per destination, the plaintexts
    sum_src const(mu_src) * x^src"""
    p = shared.params
    mus = [[_constant_term(pt) for pt in pts[:num_slots]] for pts in plaintexts_by_input]
    vectors = slot_reduce_slots(shared, gate_id, inputs, mus, num_slots, chunk)
    outs = []
    for row in mus:
        pt = GpuDCRTPoly.const_zero(p)
        for src, mu in enumerate(row):
            pt = pt + GpuDCRTPoly.from_biguint_to_constant(p, mu) * GpuDCRTPoly.const_rotate_poly(p, src)
        outs.append(pt)
    return vectors, outs
