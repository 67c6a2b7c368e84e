"""The LWE public lookup (src/lookup/lwe/pubkey_gpu.rs:193-222,397-520, src/lookup/lwe/utils.rs:23-45,152-178,
src/lookup/lwe/encoding_gpu.rs:142-223): per (gate, slot), LUT row (entry, x, y) and column chunk the preprocessing samples a
preimage K_high of

    target = A_lt[:, chunk] - G_d[:, chunk] o y - (A_z - G_d o x) K_low,
    K_low = G^-1 of columns `chunk` of the d x m matrix hash-sampled under "LWE_R_G_<gate>_<lut>_<entry>_slot<slot>",

x the row's LUT input and y its value, both constant polynomials, and the online side evaluates
c_b K_high + c_z K_low chunk by chunk.  `build_adjusted_target_chunk` is the reference's function restated with the
mirror's operations, one row at a time; `lwe_target_chunks` builds the targets of many rows in one library call
(gpupoly_matrix_lwe_targets); `sample_lwe_preimages` feeds them into the batched preimage, the body
of the reference's `wave` loop; `public_lookup` is the online side for one LUT row of one slot, `public_lookup_slots` for
many slots of one gate with one library call per output chunk (gpupoly_matrix_lwe_lookup), and
`public_lookup_poly` the body of the evaluator's public_lookup_poly_gpu (src/lookup/lwe/poly_encoding_gpu.rs:389-463) on top."""
from __future__ import annotations

from dataclasses import dataclass

from . import _ffi
from .matrix import GpuDCRTPolyMatrix
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler


@dataclass
class LweShared:
    """What every LUT row of one (gate, slot) shares: the key, the ids the tags are made of and the gate's input and output
    public-key matrices A_z and A_lt (d x m_g, NTT domain; LoadedLweChunkTask of the reference holds them per task)."""

    params: object
    hash_key: bytes
    gate_id: int
    lut_id: int
    slot_idx: object  # None or the slot's index: the tags say "slot0" for None
    a_z: GpuDCRTPolyMatrix
    a_lt: GpuDCRTPolyMatrix
    hash_name: str = "keccak256"

    @property
    def d(self) -> int:
        return self.a_lt.nrow

    @property
    def m_g(self) -> int:
        return self.d * self.params.modulus_digits()

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    def tag(self, entry_idx: int) -> bytes:
        """k_low_tag_for_slot (utils.rs:118-125)"""
        return f"LWE_R_G_{self.gate_id}_{self.lut_id}_{entry_idx}_slot{self.slot_idx or 0}".encode("ascii")

    def tags(self, entry_idxs) -> list:
        """the rows' tags as a table: the entry index stands in the middle of the tag, so no indexed form generates them"""
        return [self.tag(i) for i in entry_idxs]


def derive_a_lt_matrix(params, d: int, hash_key: bytes, gate_id: int, slot_idx=None, hash_name: str = "keccak256") -> GpuDCRTPolyMatrix:
    """derive_a_lt_matrix_for_slot (utils.rs:23-45)"""
    tag = f"A_LT_{gate_id}_slot{slot_idx or 0}".encode("ascii")
    return GpuDCRTPolyHashSampler(hash_name).sample_hash(params, hash_key, tag, d, d * params.modulus_digits(), DistType.FinRingDist())


def derive_k_low_chunk(shared: LweShared, entry_idx: int, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
    """derive_k_low_chunk_for_slot (utils.rs:152-178) for the chunk [col_start, col_start + col_len)"""
    return shared.sampler().sample_hash_decomposed_columns(shared.params, shared.hash_key, shared.tag(entry_idx), shared.d, shared.m_g,
                                                           col_start, col_len, DistType.FinRingDist())


def build_adjusted_target_chunk(shared: LweShared, entry_idx: int, x: int, y: int, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
    """build_adjusted_target_chunk (pubkey_gpu.rs:193-222), statement by statement: the comparison leg."""
    p, d = shared.params, shared.d
    col_end = col_start + col_len
    assert 0 <= col_start <= col_end <= shared.m_g and shared.a_lt.ncol == shared.m_g
    gadget = GpuDCRTPolyMatrix.gadget_matrix(p, d)  # GpuLweDeviceShared::gadget
    x_poly = GpuDCRTPoly.from_usize_to_constant(p, int(x))
    y_poly = GpuDCRTPoly.from_elem_to_constant(p, int(y))
    ext_matrix = shared.a_z - (gadget * x_poly)
    gadget_chunk = gadget.slice_columns(col_start, col_end)
    target_chunk = shared.a_lt.slice_columns(col_start, col_end) - (gadget_chunk * y_poly)
    k_low_chunk = derive_k_low_chunk(shared, entry_idx, col_start, col_len)
    return target_chunk - (ext_matrix * k_low_chunk)


def lwe_target_chunks(shared: LweShared, rows, chunk) -> list:
    """[build_adjusted_target_chunk(shared, entry, x, y, *chunk) for entry, x, y in rows] in ONE library call: `rows` is a
    sequence of (entry_idx, x, y) triples, `chunk` = (col_start, col_len).  Where the library answers "unsupported"
    (MXX_HIP_RNG_COMPAT=reference) and for hashes without a device form the literal loop runs: the same matrices either way."""
    rows = [(int(i), int(x), int(y)) for i, x, y in rows]
    col_start, col_len = chunk
    if rows and shared.sampler()._on_device():
        try:
            return GpuDCRTPolyMatrix.lwe_targets(shared.a_z, shared.a_lt, col_start, col_len, [y for _, _, y in rows], [x for _, x, _ in rows],
                                                 shared.hash_key, shared.tags([i for i, _, _ in rows]), shared.hash_name)
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
    return [build_adjusted_target_chunk(shared, i, x, y, col_start, col_len) for i, x, y in rows]


def sample_lwe_preimages(shared: LweShared, trap_sampler, trapdoor, public_matrix, rows, chunk, _seeds=None) -> list:
    """The K_high chunks of the rows for one column chunk - the body of the wave loop of store_chunk_tasks_gpu
    (pubkey_gpu.rs:224-263,288-395) for the pending rows of one (gate, slot, chunk) on one device: the targets in one call,
    then `preimage_many_abi` (one gpupoly_trapdoor_preimage_many call).  Returns [(target, K_high chunk)] per row."""
    targets = lwe_target_chunks(shared, rows, chunk)
    preimages = trap_sampler.preimage_many_abi(shared.params, trapdoor, public_matrix, targets, _seeds=_seeds)
    return list(zip(targets, preimages))


def public_lookup(shared: LweShared, c_b: GpuDCRTPolyMatrix, c_z: GpuDCRTPolyMatrix, k_high_chunks, entry_idx: int) -> GpuDCRTPolyMatrix:
    """The online side (compute_wave and reduce_contribution_bytes_by_chunk, encoding_gpu.rs:142-223) for the LUT row
    `entry_idx`: out[:, chunk] = c_b K_high_chunk + c_z K_low_chunk for the consecutive column chunks whose K_high parts
    `k_high_chunks` lists in order (their widths are the chunks').  c_b is the encoding under the trapdoor's public matrix,
    c_z the input encoding (r x m_g).  Each chunk is one fused product sum written in place (mul_sum with dst_col): no
    per-family temporaries, no compact-bytes round trip, no concatenation."""
    k_high_chunks = list(k_high_chunks)
    assert sum(kh.ncol for kh in k_high_chunks) == shared.m_g, "public_lookup: the K_high chunks cover the m_g columns"
    out = GpuDCRTPolyMatrix(shared.params, c_b.nrow, shared.m_g, c_b.level, True)
    col_start = 0
    for k_high in k_high_chunks:
        k_low = derive_k_low_chunk(shared, entry_idx, col_start, k_high.ncol)
        GpuDCRTPolyMatrix.mul_sum([c_b, c_z], [k_high, k_low], out=out, dst_col=col_start)
        col_start += k_high.ncol
    return out


def public_lookup_slots(shareds, c_bs, c_zs, k_high_chunks_by_slot, entry_idxs) -> list:
    """[public_lookup(shareds[s], c_bs[s], c_zs[s], k_high_chunks_by_slot[s], entry_idxs[s]) for every slot s] - the slot loop
    of public_lookup_poly_gpu (poly_encoding_gpu.rs:419-453) around public_lookup_slot_gpu (encoding_gpu.rs:225-370) - for
    the slots of ONE gate: the S full-width r x m_g outputs are allocated once and every output chunk of all slots is ONE
    library call that writes in place (gpupoly_matrix_lwe_lookup with dst_col).  The slots share the key, the gate and
    LUT ids and the chunk widths; a K_high chunk, c_b or c_z may serve several slots.  Where the library answers
    "unsupported" (MXX_HIP_RNG_COMPAT=reference) and for hashes without a device form the per-slot `public_lookup` runs: the
    same matrices either way."""
    shareds, c_bs, c_zs, entry_idxs = list(shareds), list(c_bs), list(c_zs), [int(i) for i in entry_idxs]
    by_slot = [list(chunks) for chunks in k_high_chunks_by_slot]
    count = len(shareds)
    assert len(c_bs) == len(c_zs) == len(by_slot) == len(entry_idxs) == count, "public_lookup_slots: one c_b, c_z, chunk list and LUT row per slot"
    if count == 0:
        return []
    first = shareds[0]
    for sh in shareds:
        assert (sh.params, sh.hash_key, sh.gate_id, sh.lut_id, sh.hash_name, sh.m_g) == \
            (first.params, first.hash_key, first.gate_id, first.lut_id, first.hash_name, first.m_g), "public_lookup_slots: the slots of one gate"
    widths = [kh.ncol for kh in by_slot[0]]
    assert sum(widths) == first.m_g, "public_lookup_slots: the K_high chunks cover the m_g columns"
    for chunks in by_slot:
        assert [kh.ncol for kh in chunks] == widths, "public_lookup_slots: the slots' chunks have the same widths"
    if first.sampler()._on_device():
        tags = [sh.tag(i) for sh, i in zip(shareds, entry_idxs)]
        outs = [GpuDCRTPolyMatrix(first.params, c_b.nrow, first.m_g, c_b.level, True) for c_b in c_bs]
        try:
            col_start = 0
            for j, width in enumerate(widths):
                GpuDCRTPolyMatrix.lwe_lookup(outs, c_bs, [chunks[j] for chunks in by_slot], c_zs, col_start, first.hash_key, tags,
                                             first.hash_name, dst_col=col_start)
                col_start += width
            return outs
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
    return [public_lookup(shareds[s], c_bs[s], c_zs[s], by_slot[s], entry_idxs[s]) for s in range(count)]


def public_lookup_poly(params, hash_key: bytes, gate_id: int, lut_id: int, plt, d: int, c_bs, input_vectors, plaintexts, k_high_blobs,
                       slot_idxs=None, hash_name: str = "keccak256", wave_slots=None):
    """The body of public_lookup_poly_gpu (poly_encoding_gpu.rs:389-463) for the slots of one BggPolyEncoding: `plt` maps a
    slot's plaintext constant x to its LUT row (k, y) (plt.get, encoding_gpu.rs:245-249); c_bs[s] is the slot's encoding under
    the trapdoor's public matrix, input_vectors[s] its input encoding, plaintexts[s] its plaintext polynomial.
    `k_high_blobs(k, slot_idx)` gives the compact bytes of the stored K_high chunks of LUT row k in column order (the
    reference reads them from its checkpoint directory, load_wave).  slot_idxs: what the tags and A_lt are derived with per
    slot - None for every slot, as the reference passes (poly_encoding_gpu.rs:436).  The S A_lt matrices are ONE
    `sample_hash_many` call; the slots go in waves of `wave_slots` (default: all), a wave's K_high chunks - one per distinct
    (row, slot index, chunk) - are loaded by ONE `from_compact_bytes_many` call and its output vectors made by
    `public_lookup_slots`.  Returns (the slots' r x m_g vectors, A_lt per slot, y per slot)."""
    c_bs, input_vectors, plaintexts = list(c_bs), list(input_vectors), list(plaintexts)
    count = len(plaintexts)
    assert len(c_bs) == len(input_vectors) == count, "public_lookup_poly: one c_b, input vector and plaintext per slot"
    slot_idxs = [None] * count if slot_idxs is None else list(slot_idxs)
    assert len(slot_idxs) == count
    rows = []
    for x in plaintexts:
        x_u64 = x.const_coeff_u64()
        if x_u64 not in plt:
            raise KeyError(f"{x_u64} not found in the LUT of gate {gate_id}")
        k, y = plt[x_u64]
        rows.append((int(k), int(y)))
    sampler = GpuDCRTPolyHashSampler(hash_name)
    a_lts = sampler.sample_hash_many(params, hash_key, [f"A_LT_{gate_id}_slot{i or 0}".encode("ascii") for i in slot_idxs], d,
                                     d * params.modulus_digits(), DistType.FinRingDist())
    shareds = [LweShared(params, hash_key, gate_id, lut_id, i, None, a_lt, hash_name) for i, a_lt in zip(slot_idxs, a_lts)]
    vectors = []
    step = count if not wave_slots else int(wave_slots)
    for lo in range(0, count, max(step, 1)):
        wave = range(lo, min(lo + step, count))
        keys = {}
        blobs = []
        for s in wave:
            key = (rows[s][0], slot_idxs[s] or 0)
            if key not in keys:
                mine = list(k_high_blobs(rows[s][0], slot_idxs[s]))
                keys[key] = (len(blobs), len(mine))
                blobs += mine
        loaded = GpuDCRTPolyMatrix.from_compact_bytes_many(params, blobs)
        for m in loaded:
            m.ntt_all_in_place()
        by_slot = []
        for s in wave:
            at, n = keys[(rows[s][0], slot_idxs[s] or 0)]
            by_slot.append(loaded[at:at + n])
        vectors += public_lookup_slots([shareds[s] for s in wave], [c_bs[s] for s in wave], [input_vectors[s] for s in wave], by_slot,
                                       [rows[s][0] for s in wave])
    return vectors, a_lts, [y for _, y in rows]
