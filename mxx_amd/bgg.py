"""The BGG+ samplers (src/bgg/sampler.rs:38-412; on the device src/bgg/sampler_gpu.rs:81-172): public keys A_i, and the
encodings

    vector_i = t A_i - pt_i o (t G) + e_i,        pt_0 = 1,

of P = 1 + #plaintexts inputs under the secret t - `BGGEncodingSampler` with t = s, `BGGPolyEncodingSampler` per slot with
t_slot = s S_slot for a ternary d x d mask S_slot.  The reference's poly-encoding sampler is a loop over the slots of a dozen
matrix operations each (`sample_poly_encoding_vectors_literal` restates it, the comparison leg); here the slots' secrets are
ONE product s [S_0 | S_1 | ...] viewed as the S x d matrix T, and every vector of every slot comes out of ONE library call
(gpupoly_matrix_bgg_encode_slots).  A `BggPolyEncoding` keeps its S x m matrix on the device and
serves a slot's vector as a row view of it."""
from __future__ import annotations

from dataclasses import dataclass

from . import _ffi
from .matrix import GpuDCRTPolyMatrix
from .poly import GpuDCRTPoly
from .sampler import (DistType, GpuDCRTPolyHashSampler, random_gpu_rng_seed, sample_gpu_matrix_with_seed)

RAGGED = "BGGPolyEncodingSampler::sample requires all plaintext rows to have the same num_slots"
KEY_COUNT = "BGGPolyEncodingSampler::sample requires public_keys.len() == plaintexts.len() + 1"
MASK_COUNT = "BGGPolyEncodingSampler::sample requires one secret mask matrix per slot"


@dataclass
class BggPublicKey:
    """src/bgg/public_key.rs: the d x m matrix A and whether the plaintext under it may be revealed"""

    matrix: GpuDCRTPolyMatrix
    reveal_plaintext: bool


@dataclass
class BggEncoding:
    """src/bgg/encoding.rs: the 1 x m vector, its public key and the plaintext where the key reveals it"""

    vector: GpuDCRTPolyMatrix
    pubkey: BggPublicKey
    plaintext: object  # GpuDCRTPoly or None


class BggPolyEncoding:
    """src/bgg/poly_encoding.rs: one input's encoding in every slot.  `matrix` is S x m, row `slot` the slot's vector (the
    reference keeps S compact byte strings); `plaintexts` is the S x (P - 1) matrix of the sampler's call and `index` this
    input's place among the P, or None where the key does not reveal the plaintext."""

    def __init__(self, params, matrix: GpuDCRTPolyMatrix, pubkey: BggPublicKey, plaintexts, index: int):
        self.params, self.matrix, self.pubkey, self.index = params, matrix, pubkey, index
        self._plaintexts = plaintexts if pubkey.reveal_plaintext else None
        self._revealed = bool(pubkey.reveal_plaintext)

    @property
    def num_slots(self) -> int:
        return self.matrix.nrow

    def vector(self, slot: int) -> GpuDCRTPolyMatrix:
        """the slot's 1 x m vector: a row view, no copy"""
        assert 0 <= slot < self.num_slots, "slot out of range"
        return self.matrix.row_view(slot, slot + 1)

    def plaintext(self, slot: int):
        """the slot's plaintext, or None where the public key hides it; input 0's is the constant 1"""
        assert 0 <= slot < self.num_slots, "slot out of range"
        if not self._revealed:
            return None
        if self.index == 0:
            return GpuDCRTPoly.const_one(self.params)
        return self._plaintexts.entry(slot, self.index - 1)


def effective_gauss_sigma(gauss_sigma):
    """src/bgg/sampler_gpu.rs:28-33: a sigma of 0 samples no error, like None"""
    return None if gauss_sigma is None or gauss_sigma == 0.0 else gauss_sigma


class BGGPublicKeySampler:
    """src/bgg/sampler.rs:38-96"""

    def __init__(self, hash_key: bytes, d: int, hash_name: str = "keccak256"):
        self.hash_key, self.d, self.hash_name = bytes(hash_key), d, hash_name

    def sample(self, params, tag: bytes, reveal_plaintexts) -> list:
        """one hash sample d x (m * inputs) and its column slices (:68-95); input 0 is the constant 1 and always revealed"""
        reveal = [True] + [bool(r) for r in reveal_plaintexts]
        columns = self.d * params.modulus_digits()
        all_matrix = GpuDCRTPolyHashSampler(self.hash_name).sample_hash(params, self.hash_key, bytes(tag), self.d, columns * len(reveal),
                                                                        DistType.FinRingDist())
        return [BggPublicKey(all_matrix.slice_columns(columns * i, columns * (i + 1)), r) for i, r in enumerate(reveal)]


def _as_matrix(poly):
    return poly.inner if hasattr(poly, "inner") else poly


def _plaintext_matrix(params, rows, num_slots):
    """the S x (P - 1) matrix whose entry (slot, i) is rows[i][slot] (polynomials, 1 x 1 matrices or compact bytes), or None
    without plaintexts; an S x (P - 1) matrix is taken as it is"""
    if isinstance(rows, GpuDCRTPolyMatrix):
        return rows if rows.ncol else None
    if not rows:
        return None
    flat = [p for row in rows for p in row]
    if flat and isinstance(flat[0], (bytes, bytearray, memoryview)):
        flat = GpuDCRTPolyMatrix.from_compact_bytes_many(params, flat)
        rows = [flat[i * num_slots:(i + 1) * num_slots] for i in range(len(rows))]
    return GpuDCRTPolyMatrix.from_poly_vec(params, [[rows[i][s] for i in range(len(rows))] for s in range(num_slots)])


def encode_slots(params, secrets, matrices, plaintexts, gauss_sigma, seeds) -> list:
    """The library call behind both samplers: the P output matrices S x m for `secrets` S x d.  Where the library answers
    "unsupported" (a ring below n = 128, MXX_HIP_RNG_COMPAT=reference) every slot's error comes from the plain sampler, the
    rows are stacked and the combine entry runs: the same matrices either way."""
    sigma = effective_gauss_sigma(gauss_sigma)
    if sigma is None:
        return GpuDCRTPolyMatrix.bgg_encode_slots(secrets, matrices, plaintexts, 0.0, None)
    try:
        return GpuDCRTPolyMatrix.bgg_encode_slots(secrets, matrices, plaintexts, sigma, seeds)
    except _ffi.GpuPolyError as e:
        if "unsupported" not in str(e):
            raise
    columns = sum(a.ncol for a in matrices)
    rows = [sample_gpu_matrix_with_seed(params, 1, columns, DistType.GaussDist(sigma), seed) for seed in seeds]
    errors = rows[0].concat_rows(rows[1:])
    return GpuDCRTPolyMatrix.bgg_encode_slots_combine(secrets, matrices, plaintexts, errors)


def _draw_seeds(count, given):
    seeds = [random_gpu_rng_seed() for _ in range(count)] if given is None else list(given)
    assert len(seeds) == count, "one seed per slot"
    return seeds


class BGGEncodingSampler:
    """src/bgg/sampler.rs:98-183"""

    def __init__(self, params, secrets, gauss_sigma=None):
        self.secret_vec = GpuDCRTPolyMatrix.from_poly_vec(params, [list(secrets)])
        self.gauss_sigma = gauss_sigma

    def sample(self, params, public_keys, plaintexts, _seeds=None) -> list:
        """:133-182 as one library call with S = 1.  One seed is drawn when there is an error (`_seeds`, tests: [seed])."""
        public_keys, plaintexts = list(public_keys), list(plaintexts)
        assert len(public_keys) == len(plaintexts) + 1, "BGGEncodingSampler::sample requires public_keys.len() == plaintexts.len() + 1"
        sigma = effective_gauss_sigma(self.gauss_sigma)
        seeds = _draw_seeds(1, _seeds) if sigma is not None else None
        pt = GpuDCRTPolyMatrix.from_poly_vec(params, [plaintexts]) if plaintexts else None
        vectors = encode_slots(params, self.secret_vec.ensure_eval(), [pk.matrix for pk in public_keys], pt, sigma, seeds)
        all_pt = [GpuDCRTPoly.const_one(params)] + plaintexts
        return [BggEncoding(v, pk, p if pk.reveal_plaintext else None) for v, pk, p in zip(vectors, public_keys, all_pt)]

    def sample_literal(self, params, public_keys, plaintexts, _seeds=None) -> list:
        """:133-182 statement by statement with the older operations and the same seed: the comparison leg"""
        public_keys = list(public_keys)
        secret_vec = self.secret_vec
        log_base_q = params.modulus_digits()
        packed_input_size = 1 + len(plaintexts)
        plaintexts = [GpuDCRTPoly.const_one(params)] + list(plaintexts)
        secret_vec_size = secret_vec.ncol
        columns = secret_vec_size * log_base_q * packed_input_size
        sigma = effective_gauss_sigma(self.gauss_sigma)
        if sigma is None:
            error = GpuDCRTPolyMatrix.zero(params, 1, columns)
        else:
            error = sample_gpu_matrix_with_seed(params, 1, columns, DistType.GaussDist(sigma), _draw_seeds(1, _seeds)[0])
        all_public_key_matrix = public_keys[0].matrix.concat_columns([pk.matrix for pk in public_keys[1:]])
        first_term = secret_vec * all_public_key_matrix
        gadget = GpuDCRTPolyMatrix.gadget_matrix(params, secret_vec_size)
        encoded_polys_vec = GpuDCRTPolyMatrix.from_poly_vec(params, [plaintexts])
        second_term = encoded_polys_vec.tensor(secret_vec * gadget)
        all_vector = first_term - second_term + error
        m = secret_vec_size * log_base_q
        return [BggEncoding(all_vector.slice_columns(m * i, m * (i + 1)), pk, p if pk.reveal_plaintext else None)
                for i, (pk, p) in enumerate(zip(public_keys, plaintexts))]


def sample_poly_encoding_vectors_literal(params, base_secret_vec, all_public_key_matrix, gadget, plaintexts, slot_secret_mats, num_slots,
                                         packed_input_size, ncol, gauss_sigma, _seeds=None) -> list:
    """sample_poly_encoding_vectors_gpu (src/bgg/sampler_gpu.rs:110-160) statement by statement with the older operations:
    plaintexts[i][slot] and slot_secret_mats[slot] are compact bytes as there (polynomials and matrices are taken as they
    are), one seed per slot in slot order when there is an error.  Returns [input][slot] -> the 1 x ncol vector (the
    reference stores its compact bytes)."""
    gauss_sigma = effective_gauss_sigma(gauss_sigma)
    seeds = _draw_seeds(num_slots, _seeds) if gauss_sigma is not None else None
    encoding_vectors = [[] for _ in range(packed_input_size)]
    load = lambda cls, x: cls.from_compact_bytes(params, x) if isinstance(x, (bytes, bytearray, memoryview)) else x
    for slot in range(num_slots):
        slot_secret_mat = load(GpuDCRTPolyMatrix, slot_secret_mats[slot])
        transformed_secret_vec = base_secret_vec * slot_secret_mat
        if gauss_sigma is None:
            error = GpuDCRTPolyMatrix.zero(params, 1, ncol * packed_input_size)
        else:
            error = sample_gpu_matrix_with_seed(params, 1, ncol * packed_input_size, DistType.GaussDist(gauss_sigma), seeds[slot])
        slot_plaintexts = [GpuDCRTPoly.const_one(params)] + [load(GpuDCRTPoly, row[slot]) for row in plaintexts]
        encoded_polys_vec = GpuDCRTPolyMatrix.from_poly_vec(params, [slot_plaintexts])
        first_term = transformed_secret_vec * all_public_key_matrix
        second_term = encoded_polys_vec.tensor(transformed_secret_vec * gadget)
        all_vector = first_term - second_term + error
        for idx in range(packed_input_size):
            encoding_vectors[idx].append(all_vector.slice_columns(ncol * idx, ncol * (idx + 1)))
    return encoding_vectors


class BGGPolyEncodingSampler:
    """src/bgg/sampler.rs:185-412"""

    def __init__(self, params, secrets, gauss_sigma=None):
        self.secret_vec = GpuDCRTPolyMatrix.from_poly_vec(params, [list(secrets)])
        self.gauss_sigma = gauss_sigma

    @staticmethod
    def assert_uniform_num_slots(plaintexts) -> int:
        if isinstance(plaintexts, GpuDCRTPolyMatrix):
            return plaintexts.nrow
        num_slots = len(plaintexts[0]) if len(plaintexts) else 0
        assert all(len(row) == num_slots for row in plaintexts), RAGGED
        return num_slots

    def sample_slot_secret_mats(self, params, num_slots: int, _seeds=None) -> GpuDCRTPolyMatrix:
        """:382-411 as ONE seeded-blocks call: the d x (S d) matrix [S_0 | S_1 | ...], block `slot` bit for bit the
        sample_uniform(d, d, TernaryDist) under the slot's seed; a fresh seed per slot in slot order (`_seeds`: tests).
        Under MXX_HIP_RNG_COMPAT=reference ("unsupported") the blocks are sampled one by one and concatenated."""
        d = self.secret_vec.ncol
        seeds = _draw_seeds(num_slots, _seeds)
        if num_slots == 0 or d == 0:
            return GpuDCRTPolyMatrix.zero(params, d, d * num_slots)
        try:
            return GpuDCRTPolyMatrix.sample_distribution_blocks(params, seeds, DistType.TernaryDist().as_ffi(), nrow=d, seg_cols=[d] * num_slots)
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
        blocks = [sample_gpu_matrix_with_seed(params, d, d, DistType.TernaryDist(), seed) for seed in seeds]
        return blocks[0].concat_columns(blocks[1:])

    def _stacked_masks(self, params, slot_secret_mats, num_slots) -> GpuDCRTPolyMatrix:
        """[S_0 | S_1 | ...] from what `sample` is given: that matrix itself, or one mask per slot as compact bytes or as a matrix"""
        d = self.secret_vec.ncol
        if isinstance(slot_secret_mats, GpuDCRTPolyMatrix):
            assert slot_secret_mats.ncol == d * num_slots, MASK_COUNT
            return slot_secret_mats
        mats = list(slot_secret_mats)
        assert len(mats) == num_slots, MASK_COUNT
        if mats and isinstance(mats[0], (bytes, bytearray, memoryview)):
            mats = GpuDCRTPolyMatrix.from_compact_bytes_many(params, mats)
        return mats[0].ensure_eval().concat_columns(mats[1:]) if mats else GpuDCRTPolyMatrix.zero(params, d, 0)

    def slot_secrets(self, params, slot_secret_mats, num_slots) -> GpuDCRTPolyMatrix:
        """T, S x d: row `slot` is s S_slot - ONE product s [S_0 | S_1 | ...] viewed slot by slot"""
        d = self.secret_vec.ncol
        stacked = self._stacked_masks(params, slot_secret_mats, num_slots)
        return (self.secret_vec.ensure_eval() * stacked).reshape_view(num_slots, d)

    def sample(self, params, public_keys, plaintexts, slot_secret_mats=None, _seeds=None) -> list:
        """:224-364: plaintexts[i][slot] (polynomials or compact bytes; or the S x (P - 1) matrix itself) -> one
        BggPolyEncoding per input.  One product for the slots' secrets and one library call for every vector of every slot;
        the error seeds are drawn per slot in slot order (`_seeds`: tests)."""
        public_keys = list(public_keys)
        num_slots = self.assert_uniform_num_slots(plaintexts)
        inputs = plaintexts.ncol if isinstance(plaintexts, GpuDCRTPolyMatrix) else len(plaintexts)
        assert len(public_keys) == inputs + 1, KEY_COUNT
        if slot_secret_mats is None:
            slot_secret_mats = self.sample_slot_secret_mats(params, num_slots)
        sigma = effective_gauss_sigma(self.gauss_sigma)
        seeds = _draw_seeds(num_slots, _seeds) if sigma is not None else None
        pt = _plaintext_matrix(params, plaintexts, num_slots)
        m = self.secret_vec.ncol * params.modulus_digits()
        if num_slots == 0:
            vectors = [GpuDCRTPolyMatrix.new_empty(params, 0, m) for _ in public_keys]
        else:
            secrets = self.slot_secrets(params, slot_secret_mats, num_slots)
            vectors = encode_slots(params, secrets, [pk.matrix for pk in public_keys], pt, sigma, seeds)
        return [BggPolyEncoding(params, v, pk, pt, i) for i, (v, pk) in enumerate(zip(vectors, public_keys))]

    def sample_with_fresh_slot_secret_mats(self, params, public_keys, plaintexts, _seeds=None):
        """:366-380: (encodings, [S_0 | S_1 | ...])"""
        num_slots = self.assert_uniform_num_slots(plaintexts)
        slot_secret_mats = self.sample_slot_secret_mats(params, num_slots)
        return self.sample(params, public_keys, plaintexts, slot_secret_mats, _seeds=_seeds), slot_secret_mats
