"""The slot-transfer public key's gate preimage targets (src/slot_transfer/bgg_pubkey_gpu.rs:371-407,409-471): one target
per destination slot and column chunk of the wave that sample_gate_batch_gpu builds (:820-950),

    target_t = s_t A_out[:, chunk]  -  (lhs_t G^-1(a_t[:, chunk])) o scalar_t  +  E_t,

A_out the gate's d x m_g hash sample ("slot_transfer_gate_a_out_<gate>"), d = secret_size, m_g = d * modulus_digits, and for
the slot-reduce gates ("slot_reduce_gate_a_out_<gate>") with sum_src (s_src a_in_t) G^-1(a_t[:, chunk]) x^src in the middle.
`build_gate_target_chunk` and `build_slot_reduce_gate_target_chunk` are the reference's functions restated with the mirror's
operations, one request at a time; `gate_target_chunks` and `slot_reduce_gate_target_chunks` build the targets of a wave of
requests with a number of launches that does not depend on the wave (gpupoly_matrix_mul_decompose_pairs; DESIGN.md section
5t); `sample_gate_preimages` feeds them into the batched preimage."""
from __future__ import annotations

from dataclasses import dataclass

from .lookup import sample_error_matrix
from .matrix import GpuDCRTPolyMatrix
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
