"""The online side of the GGH15 lookup: the public lookup an evaluator runs for every lookup gate, slot and evaluation
(src/lookup/ggh15/encoding.rs:172-300, build_public_lookup_output_chunk; device path
src/lookup/ggh15/poly_encoding_gpu.rs:338-567,686-1420).  With d the secret size, k = modulus_digits, m_g = d k,
w = d (k + 2), c_b0 r x w, c_in (`input_vector`) r x m_g, x the slot's plaintext, (k_s, y_s) = plt.get(x):

    out[:, chunk] = c_b0 P_id[:, chunk] + c_b0 (P_gy G^-1(G_d[:, chunk] o y)) + c_b0 (P_v V) + c_b0 (P_vx (V o x))
                    - c_b0 (P_g1 K[:, chunk]) + (c_in G^-1(U_g)) V,
    V = G^-1 of columns `chunk` of the d x m_g matrix hash-sampled under "ggh15_lut_v_idx_<lut>_<k_s>",
    U_g the d x m_g matrix under "ggh15_lut_u_g_matrix_<gate>", K the LUT-row preimage lut_aux_<lut>_idx<k_s>.

`build_public_lookup_output_chunk` is the reference's function restated with the mirror's older operations, one slot and
one chunk at a time, in the reference's own association order: the comparison leg.  `public_lookup_slots` evaluates many
slots of one gate: stage 1 - everything that depends on neither the LUT row nor the chunk - as six products of the stacked
c_b0 / c_in with the existing entries, then one library call per column chunk (gpupoly_matrix_ggh15_lookup; DESIGN.md
section 5w).  Exact ring arithmetic on canonical residues: the same matrices either way, bit for bit."""
from __future__ import annotations

from dataclasses import dataclass, field

from . import _ffi
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler


@dataclass
class PublicLookupShared:
    """What every slot of one lookup gate shares (GGH15PublicLookupSharedState of the reference plus the key, the ids, the
    LUT and its row preimages, which the reference reads from its checkpoint directory): the five gate preimages in the
    NTT domain - preimage_gate1 w x w, the four preimage_gate2_* w x m_g - the LUT as x -> (k, y) and the LUT-row
    preimages (w x m_g) by k."""

    params: object
    hash_key: bytes
    gate_id: int
    lut_id: int
    d: int
    preimage_gate1: GpuDCRTPolyMatrix
    preimage_gate2_identity: GpuDCRTPolyMatrix
    preimage_gate2_gy: GpuDCRTPolyMatrix
    preimage_gate2_v: GpuDCRTPolyMatrix
    preimage_gate2_vx: GpuDCRTPolyMatrix
    lut: dict
    lut_preimages: dict
    hash_name: str = "keccak256"
    chunk_width: int = 0  # the reference's column chunk width (column_chunk_bounds); 0: one chunk of m_g columns
    _chunks: dict = field(default_factory=dict, repr=False)

    @property
    def m_g(self) -> int:
        return self.d * self.params.modulus_digits()

    @property
    def w(self) -> int:
        """trapdoor_public_column_count: d (modulus_digits + 2)"""
        return self.d * (self.params.modulus_digits() + 2)

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    def get(self, x_u64: int):
        """plt.get: (k, y) of the LUT row of x"""
        if x_u64 not in self.lut:
            raise KeyError(f"{x_u64} not found in LUT for gate {self.gate_id}")
        k, y = self.lut[x_u64]
        return int(k), int(y)

    def v_tag(self, k: int) -> bytes:
        return f"ggh15_lut_v_idx_{self.lut_id}_{k}".encode("ascii")

    def v_tags(self, ks):
        """the slots' tags: generated on the device where the row indices are consecutive, a table of literal tags otherwise"""
        ks = list(ks)
        if ks and all(b == a + 1 for a, b in zip(ks, ks[1:])):
            return IndexedTags(f"ggh15_lut_v_idx_{self.lut_id}_".encode("ascii"), ks[0], len(ks), decimal=True)
        return [self.v_tag(k) for k in ks]

    def u_g_tag(self) -> bytes:
        return f"ggh15_lut_u_g_matrix_{self.gate_id}".encode("ascii")

    def column_chunks(self, chunk_width=None) -> list:
        """[(col_start, col_len)] over the m_g output columns (column_chunk_bounds for every chunk index)"""
        width = int(chunk_width or self.chunk_width or self.m_g)
        return [(c0, min(width, self.m_g - c0)) for c0 in range(0, self.m_g, width)]

    def lut_preimage_chunk(self, k: int, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
        """read_matrix_column_chunk of lut_aux_<lut>_idx<k>: one matrix per (row, chunk), shared by the slots that hit the row"""
        key = (k, col_start, col_len)
        if key not in self._chunks:
            self._chunks[key] = self.lut_preimages[k].slice_columns(col_start, col_start + col_len)
        return self._chunks[key]


def build_public_lookup_output_chunk(shared: PublicLookupShared, c_b0, input_vector, x: GpuDCRTPoly, col_start: int,
                                     col_len: int) -> GpuDCRTPolyMatrix:
    """build_public_lookup_output_chunk (encoding.rs:172-300), statement by statement, for the chunk
    [col_start, col_start + col_len): the comparison leg.  The checkpointed operands are the matrices of `shared`;
    mul_chunked_checkpoint_with_rhs - a product summed over waves of the inner dimension - is the product itself."""
    p, d, m_g = shared.params, shared.d, shared.m_g
    x_u64 = x.const_coeff_u64()
    k, y = shared.get(x_u64)
    y_poly = GpuDCRTPoly.from_elem_to_constant(p, y)
    gy = GpuDCRTPolyMatrix.gadget_matrix(p, d) * y_poly
    col_end = col_start + col_len
    assert col_end <= m_g

    c_const_chunk = c_b0 * shared.preimage_gate2_identity.slice_columns(col_start, col_end)  # left_mul_chunked_checkpoint_column

    gy_decomposed_chunk = gy.slice_columns(col_start, col_end).decompose()
    gy_mid = shared.preimage_gate2_gy * gy_decomposed_chunk
    c_const_chunk.add_in_place(c_b0 * gy_mid)

    v_idx_chunk = shared.sampler().sample_hash_decomposed_columns(p, shared.hash_key, shared.v_tag(k), d, m_g, col_start, col_len,
                                                                  DistType.FinRingDist())
    v_mid = shared.preimage_gate2_v * v_idx_chunk
    c_const_chunk.add_in_place(c_b0 * v_mid)

    vx_rhs_chunk = v_idx_chunk * x
    vx_mid = shared.preimage_gate2_vx * vx_rhs_chunk
    c_const_chunk.add_in_place(c_b0 * vx_mid)

    preimage_lut_chunk = shared.lut_preimage_chunk(k, col_start, col_len)
    preimage_lut_in_b0_basis = shared.preimage_gate1 * preimage_lut_chunk
    c_const_chunk = c_const_chunk - (c_b0 * preimage_lut_in_b0_basis)
    c_x_chunk_acc = None
    for inner_start, inner_len in shared.column_chunks():
        u_g_decomposed_chunk = shared.sampler().sample_hash_decomposed_columns(p, shared.hash_key, shared.u_g_tag(), d, m_g, inner_start,
                                                                               inner_len, DistType.FinRingDist())
        lhs_mid = input_vector * u_g_decomposed_chunk
        v_rhs = v_idx_chunk.slice(inner_start, inner_start + inner_len, 0, col_len)
        randomized_mid = lhs_mid * v_rhs
        if c_x_chunk_acc is not None:
            c_x_chunk_acc.add_in_place(randomized_mid)
        else:
            c_x_chunk_acc = randomized_mid
    assert c_x_chunk_acc is not None, "public lookup randomized chunk accumulation must be non-empty"
    c_const_chunk.add_in_place(c_x_chunk_acc)
    return c_const_chunk


def _literal_slot(shared, c_b0, input_vector, x, chunks) -> GpuDCRTPolyMatrix:
    parts = [build_public_lookup_output_chunk(shared, c_b0, input_vector, x, c0, cl) for c0, cl in chunks]
    return parts[0].concat_columns(parts[1:])


def public_lookup_stage1(shared: PublicLookupShared, c_b0s, input_vectors) -> list:
    """(mid_identity, mid_gy, mid_v, mid_vx, mid_rand, mid_gate1) for the slots' c_b0 / c_in stacked by rows: six products
    with a shared right operand, each of the five preimages and G^-1(U_g) read once for all slots and chunks."""
    c_b0s, input_vectors = list(c_b0s), list(input_vectors)
    p = shared.params
    b0 = c_b0s[0].concat_rows(c_b0s[1:])
    c_in = input_vectors[0].concat_rows(input_vectors[1:])
    u_g_decomposed = shared.sampler().sample_hash_decomposed(p, shared.hash_key, shared.u_g_tag(), shared.d, shared.m_g, DistType.FinRingDist())
    return [b0 * shared.preimage_gate2_identity, b0 * shared.preimage_gate2_gy, b0 * shared.preimage_gate2_v, b0 * shared.preimage_gate2_vx,
            c_in * u_g_decomposed, b0 * shared.preimage_gate1]


def public_lookup_stage2(shared: PublicLookupShared, mids, rows, xs, chunk) -> list:
    """one gpupoly_matrix_ggh15_lookup call: the slots' r x col_len outputs for `chunk` = (col_start, col_len); `rows` the
    slots' (k, y), `xs` their plaintexts"""
    col_start, col_len = chunk
    ks = [k for k, _ in rows]
    return GpuDCRTPolyMatrix.ggh15_lookup(mids, [shared.lut_preimage_chunk(k, col_start, col_len) for k in ks],
                                          [x.ensure_eval_domain().inner for x in xs], col_start, col_len, [y for _, y in rows],
                                          shared.hash_key, shared.v_tags(ks), shared.hash_name)


def public_lookup_slots(shared: PublicLookupShared, c_b0s, input_vectors, xs, chunk_width=None) -> list:
    """[(the slot's r x m_g output vector, y_s)] for the slots of one gate: what the reference's per-slot loop over
    build_public_lookup_output_chunk and its column concatenation give.  Stage 1 once for all slots, then one library call
    per column chunk.  Where the library answers "unsupported" (MXX_HIP_RNG_COMPAT=reference) and for hashes without a
    device form the literal per-slot loop runs: the same matrices either way."""
    c_b0s, input_vectors, xs = list(c_b0s), list(input_vectors), list(xs)
    assert len(c_b0s) == len(input_vectors) == len(xs), "public_lookup_slots: one c_b0, input vector and plaintext per slot"
    if not xs:
        return []
    rows = [shared.get(x.const_coeff_u64()) for x in xs]
    chunks = shared.column_chunks(chunk_width)
    if shared.sampler()._on_device():
        try:
            mids = public_lookup_stage1(shared, c_b0s, input_vectors)
            per_chunk = [public_lookup_stage2(shared, mids, rows, xs, chunk) for chunk in chunks]
            return [(per_chunk[0][s].concat_columns([part[s] for part in per_chunk[1:]]), rows[s][1]) for s in range(len(xs))]
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
    return [(_literal_slot(shared, c_b0s[s], input_vectors[s], xs[s], chunks), rows[s][1]) for s in range(len(xs))]
