"""The GGH15 LUT preprocessing's preimage targets (src/lookup/ggh15/pubkey_gpu.rs:379-415,540-640; CPU twin
src/lookup/ggh15/pubkey.rs:241-275,441-460): one target per LUT row and column chunk,

    target = W_id[:, chunk] + W_gy G^-1(G_d[:, chunk] o y) + W_v V + W_vx (V o idx),
    V = G^-1 of columns `chunk` of the d x m matrix hash-sampled under "ggh15_lut_v_idx_<lut>_<idx>",

y the row's LUT value and idx its index, both constant polynomials.  `build_lut_preimage_target_chunk` is the reference's
function restated with the mirror's operations, one row at a time; `lut_preimage_target_chunks` builds the targets of
many rows in one library call (gpupoly_matrix_lut_targets); `sample_lut_preimages` feeds them into
the batched preimage, the body of the reference's `wave` loop.

The other half of the preprocessing, the five gate stages of `sample_gate_preimages_batch_gpu` (pubkey_gpu.rs:649-1000),
has one target per gate, stage and column chunk (pubkey_gpu.rs:418-537),

    target = S_g W[:, chunk] + high + E,    S_g the gate's ternary d x d secret, E = sample_error_matrix(d, chunk width),

restated one gate at a time by `build_gate_stage1_target_chunk` .. `build_gate_stage5_target_chunk` and built for all gates
of a wave at once by `gate_stage_targets` and the `gate_stageN_targets` wrappers;
`sample_gate_preimages` feeds a stage's targets into the batched preimage."""
from __future__ import annotations

from dataclasses import dataclass

from . import _ffi
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .poly import GpuDCRTPoly
from .sampler import DistType, GpuDCRTPolyHashSampler, sample_gpu_matrix_with_seed, sample_gpu_stack_with_seeds


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


# ---- the gate stages (pubkey_gpu.rs:418-537,649-1000) ---------------------------------------------------------------------
@dataclass
class GateShared:
    """What every gate of one LUT shares in the gate stages (GpuGateDeviceShared of the reference plus the key and the
    LUT's id): b1 (d rows) and the three d x m_g blocks in the NTT domain, m_g = d * modulus_digits."""

    params: object
    hash_key: bytes
    lut_id: int
    b1_matrix: GpuDCRTPolyMatrix
    w_identity: GpuDCRTPolyMatrix
    w_gy: GpuDCRTPolyMatrix
    w_v: GpuDCRTPolyMatrix
    hash_name: str = "keccak256"

    @property
    def d(self) -> int:
        return self.w_identity.nrow

    @property
    def m_g(self) -> int:
        return self.d * self.params.modulus_digits()

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    def a_out_tag(self, gate_id: int) -> bytes:
        return f"ggh15_gate_a_out_{gate_id}".encode("ascii")

    def u_g_tag(self, gate_id: int) -> bytes:
        return f"ggh15_lut_u_g_matrix_{gate_id}".encode("ascii")

    def w_vx_columns(self, col_start: int, col_len: int) -> GpuDCRTPolyMatrix:
        """derive_w_block_with_tag_columns(lut_id, "block_vx", ..) (pubkey.rs:671-691)"""
        return self.sampler().sample_hash_columns(self.params, self.hash_key, f"ggh15_lut_w_block_vx_{self.lut_id}".encode("ascii"),
                                                  self.d, self.m_g, col_start, col_len, DistType.FinRingDist())


def sample_gate_secret(params, d: int, seed) -> GpuDCRTPolyMatrix:
    """s_g = sample_uniform(d, d, TernaryDist) (pubkey_gpu.rs:680) under a given seed"""
    return sample_gpu_matrix_with_seed(params, d, d, DistType.TernaryDist(), seed)


def sample_error_matrix(params, nrow: int, ncol: int, error_sigma: float, seed) -> GpuDCRTPolyMatrix:
    """sample_error_matrix (pubkey.rs:227-239) under a given seed: zero when error_sigma == 0"""
    assert error_sigma >= 0.0, f"error_sigma {error_sigma} must be nonnegative"
    if error_sigma == 0.0:
        return GpuDCRTPolyMatrix.zero(params, nrow, ncol)
    return sample_gpu_matrix_with_seed(params, nrow, ncol, DistType.GaussDist(error_sigma), seed)


def build_gate_stage1_target_chunk(shared: GateShared, s_seed, error_seed, error_sigma, col_start, col_len) -> GpuDCRTPolyMatrix:
    """build_gate_stage1_target_chunk_gpu (pubkey_gpu.rs:418-430), statement by statement: the comparison leg."""
    p, d = shared.params, shared.d
    s_g = sample_gate_secret(p, d, s_seed)
    target_chunk = s_g * shared.b1_matrix.slice(0, d, col_start, col_start + col_len)
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def build_gate_stage2_target_chunk(shared: GateShared, gate_id, s_seed, error_seed, error_sigma, col_start, col_len) -> GpuDCRTPolyMatrix:
    """build_gate_stage2_identity_target_chunk_gpu (pubkey_gpu.rs:432-459)"""
    p, d = shared.params, shared.d
    s_g = sample_gate_secret(p, d, s_seed)
    target_chunk = s_g * shared.w_identity.slice(0, d, col_start, col_start + col_len)
    out_chunk = shared.sampler().sample_hash_columns(p, shared.hash_key, shared.a_out_tag(gate_id), d, shared.m_g, col_start, col_len,
                                                     DistType.FinRingDist())
    target_chunk.add_in_place(out_chunk)
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def build_gate_stage3_target_chunk(shared: GateShared, s_seed, error_seed, error_sigma, col_start, col_len) -> GpuDCRTPolyMatrix:
    """build_gate_stage3_gy_target_chunk_gpu (pubkey_gpu.rs:461-478)"""
    p, d = shared.params, shared.d
    s_g = sample_gate_secret(p, d, s_seed)
    target_chunk = s_g * shared.w_gy.slice(0, d, col_start, col_start + col_len)
    target_high_chunk = -GpuDCRTPolyMatrix.gadget_matrix(p, d).slice(0, d, col_start, col_start + col_len)
    target_chunk.add_in_place(target_high_chunk)
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def build_gate_stage4_target_chunk(shared: GateShared, gate_id, s_seed, input_matrix, error_seed, error_sigma, col_start,
                                   col_len) -> GpuDCRTPolyMatrix:
    """build_gate_stage4_v_target_chunk_gpu (pubkey_gpu.rs:480-509)"""
    p, d = shared.params, shared.d
    s_g = sample_gate_secret(p, d, s_seed)
    target_chunk = s_g * shared.w_v.slice(0, d, col_start, col_start + col_len)
    u_g_decomposed_chunk = shared.sampler().sample_hash_decomposed_columns(p, shared.hash_key, shared.u_g_tag(gate_id), d, shared.m_g,
                                                                           col_start, col_len, DistType.FinRingDist())
    target_high_chunk = -(input_matrix * u_g_decomposed_chunk)
    target_chunk.add_in_place(target_high_chunk)
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def build_gate_stage5_target_chunk(shared: GateShared, s_seed, u_g_matrix, error_seed, error_sigma, col_start, col_len) -> GpuDCRTPolyMatrix:
    """build_gate_stage5_target_chunk_gpu (pubkey_gpu.rs:511-537)"""
    p, d = shared.params, shared.d
    s_g = sample_gate_secret(p, d, s_seed)
    target_high_vx_chunk = u_g_matrix.slice(0, d, col_start, col_start + col_len)  # build_stage5_target_high_vx_chunk
    w_block_vx_chunk = shared.w_vx_columns(col_start, col_len)
    target_chunk = s_g * w_block_vx_chunk
    target_chunk.add_in_place(target_high_vx_chunk)
    target_chunk.add_in_place(sample_error_matrix(p, d, col_len, error_sigma, error_seed))
    return target_chunk


def gate_stage_targets(params, s_seeds, w_chunk, error_seeds, error_sigma, high=None, negate_high: bool = False) -> list:
    """target_t = S_t w_chunk + E_t (+- high_t) for the T gates of one stage and one column chunk, the launches not depending
    on T: S_t = sample_gate_secret(d, s_seeds[t]), E_t = sample_error_matrix(d, c, error_sigma, error_seeds[t]), w_chunk d x c.
    The T secrets are one stacked ternary block sample read as (T d) x d, the T errors one stacked Gaussian block sample read
    as (T d) x c, and because w_chunk is shared, [S_0; ..; S_(T-1)] w_chunk = [S_0 w_chunk; ..] is ONE product, added to the
    error stack in place (no error sample and no addition when error_sigma == 0, as in the reference).  The product and the
    sum are two calls, not one mul_sum: mul_sum chooses between its one-launch kernel and a product plus a combine pass at
    8 rows, so its launches - not its result - would depend on T, and above 8 rows (more than four gates at d = 2) it is
    these two passes anyway.  `high`: a (T d) x c stack of per-gate terms, or one d x c matrix shared by all gates, which
    is stacked T times in one launch (ones(T x 1) (x) high); added (subtracted with negate_high) in one further pass.  The
    targets are row views of the one stack (no copies; the batched preimage takes them as they are); modular sums are
    exact, so every target equals the per-gate leg bit for bit."""
    s_seeds, error_seeds = list(s_seeds), list(error_seeds)
    count, d, c = len(s_seeds), w_chunk.nrow, w_chunk.ncol
    assert len(error_seeds) == count, "gate_stage_targets: one error seed per gate"
    assert error_sigma >= 0.0, f"error_sigma {error_sigma} must be nonnegative"
    if count == 0:
        return []
    s_stack = sample_gpu_stack_with_seeds(params, d, d, DistType.TernaryDist(), s_seeds).reshape_view(count * d, d)
    stack = s_stack * w_chunk
    if error_sigma != 0.0:
        prod = stack
        stack = sample_gpu_stack_with_seeds(params, d, c, DistType.GaussDist(error_sigma), error_seeds).reshape_view(count * d, c)
        stack.add_in_place(prod)
    if high is not None:
        assert high.ncol == c and high.nrow in (d, count * d), "gate_stage_targets: high is d x c (shared) or (T d) x c"
        if high.nrow != count * d:  # (a shared high of a single gate is the stack of its one term)
            high = GpuDCRTPolyMatrix.from_coeffs(params, [[[1]]] * count).tensor(high)
        if negate_high:
            stack.sub_in_place(high)
        else:
            stack.add_in_place(high)
    return [stack.row_view(t * d, (t + 1) * d) for t in range(count)]


def gate_stage1_targets(shared: GateShared, s_seeds, error_seeds, error_sigma, chunk) -> list:
    """[build_gate_stage1_target_chunk(shared, s, e, error_sigma, *chunk) for s, e in zip(s_seeds, error_seeds)]"""
    col_start, col_len = chunk
    w = shared.b1_matrix.slice(0, shared.d, col_start, col_start + col_len)
    return gate_stage_targets(shared.params, s_seeds, w, error_seeds, error_sigma)


def gate_stage2_targets(shared: GateShared, gate_ids, s_seeds, error_seeds, error_sigma, chunk) -> list:
    """stage 2 of the gates `gate_ids`: high_t = the chunk's columns of the gate's "ggh15_gate_a_out_<gate>" sample, gate by gate"""
    col_start, col_len = chunk
    p, d = shared.params, shared.d
    w = shared.w_identity.slice(0, d, col_start, col_start + col_len)
    outs = [shared.sampler().sample_hash_columns(p, shared.hash_key, shared.a_out_tag(g), d, shared.m_g, col_start, col_len,
                                                 DistType.FinRingDist()) for g in gate_ids]
    high = outs[0].concat_rows(outs[1:]) if outs else None
    return gate_stage_targets(p, s_seeds, w, error_seeds, error_sigma, high)


def gate_stage3_targets(shared: GateShared, s_seeds, error_seeds, error_sigma, chunk) -> list:
    """stage 3: high = -G[:, chunk], shared by all gates and never cut out of the full gadget matrix (gadget_block)"""
    col_start, col_len = chunk
    p, d = shared.params, shared.d
    w = shared.w_gy.slice(0, d, col_start, col_start + col_len)
    high = GpuDCRTPolyMatrix.gadget_block(p, d, col_start, col_start + col_len, negate=True)
    return gate_stage_targets(p, s_seeds, w, error_seeds, error_sigma, high)


def gate_stage4_targets(shared: GateShared, gate_ids, s_seeds, input_matrices, error_seeds, error_sigma, chunk) -> list:
    """stage 4: high_t = -input_t G^-1(U_t[:, chunk]), U_t the gate's "ggh15_lut_u_g_matrix_<gate>" sample: the digit chunks
    of all gates in one call (sample_hash_decomposed_columns_many), the T products in one (mul_batch)"""
    col_start, col_len = chunk
    p, d = shared.params, shared.d
    w = shared.w_v.slice(0, d, col_start, col_start + col_len)
    digits = shared.sampler().sample_hash_decomposed_columns_many(p, shared.hash_key, [shared.u_g_tag(g) for g in gate_ids], d, shared.m_g,
                                                                  col_start, col_len, DistType.FinRingDist())
    prods = GpuDCRTPolyMatrix.mul_batch(list(input_matrices), digits)
    high = prods[0].concat_rows(prods[1:]) if prods else None
    return gate_stage_targets(p, s_seeds, w, error_seeds, error_sigma, high, negate_high=True)


def gate_stage5_targets(shared: GateShared, s_seeds, u_g_matrices, error_seeds, error_sigma, chunk) -> list:
    """stage 5: W = the chunk's columns of the LUT's block_vx sample, high_t = U_t[:, chunk]"""
    col_start, col_len = chunk
    p, d = shared.params, shared.d
    w = shared.w_vx_columns(col_start, col_len)
    cuts = [u.slice(0, d, col_start, col_start + col_len) for u in u_g_matrices]
    high = cuts[0].concat_rows(cuts[1:]) if cuts else None
    return gate_stage_targets(p, s_seeds, w, error_seeds, error_sigma, high)


def sample_gate_preimages(shared: GateShared, trap_sampler, trapdoor, public_matrix, targets, _seeds=None) -> list:
    """The preimages of one stage's targets for one column chunk - the body of a stage's `wave` loop in
    sample_gate_preimages_batch_gpu (pubkey_gpu.rs:693-721 and its four siblings) for one device: `targets` from a
    `gate_stageN_targets` call, then `preimage_many_abi` (one gpupoly_trapdoor_preimage_many call).  Returns
    [(target, preimage)] per gate."""
    preimages = trap_sampler.preimage_many_abi(shared.params, trapdoor, public_matrix, targets, _seeds=_seeds)
    return list(zip(targets, preimages))
