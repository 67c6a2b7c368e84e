"""The GGH15 LUT preprocessing's preimage targets (src/lookup/ggh15/pubkey_gpu.rs:379-415,540-640; CPU twin
src/lookup/ggh15/pubkey.rs:241-275,441-460): one target per LUT row and column chunk,

    target = W_id[:, chunk] + W_gy G^-1(G_d[:, chunk] o y) + W_v V + W_vx (V o idx),
    V = G^-1 of columns `chunk` of the d x m matrix hash-sampled under "ggh15_lut_v_idx_<lut>_<idx>",

y the row's LUT value and idx its index, both constant polynomials.  `build_lut_preimage_target_chunk` is the reference's
function restated with the mirror's operations, one row at a time; `lut_preimage_target_chunks` builds the targets of
many rows in one library call (gpupoly_matrix_lut_targets); `sample_lut_preimages` feeds them into
the batched preimage, the body of the reference's `wave` loop."""
from __future__ import annotations

from dataclasses import dataclass

from . import _ffi
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler


@dataclass
class LutShared:
    """What every row of one LUT shares (GpuLutDeviceShared of the reference plus the key and the LUT's id): the four
    d x m blocks in the NTT domain, m = d * modulus_digits."""

    params: object
    hash_key: bytes
    lut_id: int
    w_identity: GpuDCRTPolyMatrix
    w_gy: GpuDCRTPolyMatrix
    w_v: GpuDCRTPolyMatrix
    w_vx: GpuDCRTPolyMatrix
    hash_name: str = "keccak256"

    @property
    def d(self) -> int:
        return self.w_identity.nrow

    def tag(self, idx: int) -> bytes:
        return f"ggh15_lut_v_idx_{self.lut_id}_{idx}".encode("ascii")

    def tags(self, idxs):
        """the rows' tags: generated on the device where the indices are consecutive, a table of literal tags otherwise"""
        idxs = list(idxs)
        if idxs and all(b == a + 1 for a, b in zip(idxs, idxs[1:])):
            return IndexedTags(f"ggh15_lut_v_idx_{self.lut_id}_".encode("ascii"), idxs[0], len(idxs), decimal=True)
        return [self.tag(i) for i in idxs]


def build_lut_preimage_target_chunk(shared: LutShared, idx: int, y: int, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
    """build_lut_preimage_target_chunk_gpu (pubkey_gpu.rs:379-415), statement by statement: the comparison leg."""
    p, d = shared.params, shared.d
    m = d * p.modulus_digits()
    col_end = col_start + col_len
    assert col_end <= m and shared.w_identity.ncol == m
    local_y_poly = GpuDCRTPoly.from_elem_to_constant(p, int(y))
    idx_poly = GpuDCRTPoly.from_usize_to_constant(p, int(idx))
    target_chunk = shared.w_identity.slice(0, d, col_start, col_end)
    gy_chunk = (GpuDCRTPolyMatrix.gadget_matrix(p, d).slice(0, d, col_start, col_end) * local_y_poly).decompose()
    target_chunk.add_in_place(shared.w_gy * gy_chunk)
    v_idx_chunk = GpuDCRTPolyHashSampler(shared.hash_name).sample_hash_decomposed_columns(
        p, shared.hash_key, shared.tag(idx), d, m, col_start, col_len, DistType.FinRingDist())
    target_chunk.add_in_place(shared.w_v * v_idx_chunk)
    vx_rhs_chunk = v_idx_chunk * idx_poly
    target_chunk.add_in_place(shared.w_vx * vx_rhs_chunk)
    return target_chunk


def lut_preimage_target_chunks(shared: LutShared, rows, chunk) -> list:
    """[build_lut_preimage_target_chunk(shared, idx, y, *chunk) for idx, y in rows] in ONE library call: `rows` is a sequence
    of (idx, y) pairs, `chunk` = (col_start, col_len).  Where the library answers "unsupported" (MXX_HIP_RNG_COMPAT=reference)
    and for hashes without a device form the literal loop runs: the same matrices either way."""
    rows = [(int(i), int(y)) for i, y in rows]
    col_start, col_len = chunk
    if rows and GpuDCRTPolyHashSampler(shared.hash_name)._on_device():
        idxs = [i for i, _ in rows]
        try:
            return GpuDCRTPolyMatrix.lut_targets(shared.w_identity, shared.w_gy, shared.w_v, shared.w_vx, col_start, col_len,
                                                 [y for _, y in rows], idxs, shared.hash_key, shared.tags(idxs), shared.hash_name)
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
    return [build_lut_preimage_target_chunk(shared, i, y, col_start, col_len) for i, y in rows]


def sample_lut_preimages(shared: LutShared, trap_sampler, trapdoor, public_matrix, rows, chunk, _seeds=None) -> list:
    """The preimages of the rows' targets for one column chunk - the body of the `wave` loop of sample_lut_preimages_gpu
    (pubkey_gpu.rs:590-613) for one device: the targets in one call, then `preimage_many_abi` (one
    gpupoly_trapdoor_preimage_many call).  Returns [(target, preimage)] per row."""
    targets = lut_preimage_target_chunks(shared, rows, chunk)
    preimages = trap_sampler.preimage_many_abi(shared.params, trapdoor, public_matrix, targets, _seeds=_seeds)
    return list(zip(targets, preimages))
