"""Distribution / hash samplers on the GPU (src/sampler/gpu.rs:16-253, src/sampler/mod.rs:12-120)."""
from __future__ import annotations

import hashlib
import os
from dataclasses import dataclass

from . import _ffi
from ._ffi import GpuRngSeed
from .matrix import DEVICE_HASHES, GpuDCRTPolyMatrix, IndexedTags, device_hash_seeds  # noqa: F401
from .poly import GpuDCRTPoly


@dataclass(frozen=True)
class DistType:
    """`DistType` (src/sampler/mod.rs:12-26)."""

    kind: str
    sigma: float = 0.0

    @staticmethod
    def FinRingDist():
        return DistType("fin_ring")

    @staticmethod
    def GaussDist(sigma: float):
        return DistType("gauss", float(sigma))

    @staticmethod
    def BitDist():
        return DistType("bit")

    @staticmethod
    def TernaryDist():
        return DistType("ternary")

    def as_ffi(self) -> int:
        return {
            "fin_ring": _ffi.GPU_MATRIX_DIST_UNIFORM,
            "gauss": _ffi.GPU_MATRIX_DIST_GAUSS,
            "bit": _ffi.GPU_MATRIX_DIST_BIT,
            "ternary": _ffi.GPU_MATRIX_DIST_TERNARY,
        }[self.kind]


_seed_source = None  # test-only hook: a callable returning 32 bytes per draw (see seed_source)


def random_gpu_rng_seed() -> GpuRngSeed:
    """OS randomness, as the reference (src/sampler/gpu.rs:138-142)."""
    if _seed_source is not None:
        return GpuRngSeed.from_bytes(_seed_source())
    return GpuRngSeed.from_bytes(os.urandom(32))


class seed_source:
    """Test-only: `with seed_source(iterable_of_32_byte_seeds):` makes every seed the samplers would
    draw from the OS come from the iterable instead, in call order, so a whole trapdoor / preimage
    chain can be replayed against the CPU restatement.  Not thread-safe; production code never sets it."""

    def __init__(self, seeds):
        self._it = iter(seeds)

    def __enter__(self):
        global _seed_source
        self._prev = _seed_source
        _seed_source = lambda: next(self._it)
        return self

    def __exit__(self, *exc):
        global _seed_source
        _seed_source = self._prev
        return False


_KECCAK_RC = (
    0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
    0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
    0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
    0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008,
)
_KECCAK_ROT = ((0, 36, 3, 41, 18), (1, 44, 10, 45, 2), (62, 6, 43, 15, 61), (28, 55, 25, 21, 56), (27, 20, 39, 8, 14))
_M64 = (1 << 64) - 1


def keccak256(data: bytes) -> bytes:
    """Keccak-256 with the original 0x01 padding (what `keccak_asm::Keccak256` computes; hashlib's sha3_256 is the NIST
    variant with 0x06 padding).  The reference's tests instantiate the hash sampler with it (src/sampler/gpu.rs:267).
    Pure Python: it only ever hashes a key, a tag and a counter into a 32-byte seed."""
    rate = 136
    msg = bytearray(data)
    msg.append(0x01)
    while len(msg) % rate:
        msg.append(0)
    msg[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]  # a[x][y]
    rol = lambda v, n: ((v << n) | (v >> (64 - n))) & _M64 if n else v
    for off in range(0, len(msg), rate):
        for i in range(rate // 8):
            a[i % 5][i // 5] ^= int.from_bytes(msg[off + 8 * i : off + 8 * i + 8], "little")
        for rc in _KECCAK_RC:
            c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
            d = [c[(x - 1) % 5] ^ rol(c[(x + 1) % 5], 1) for x in range(5)]
            a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
            b = [[0] * 5 for _ in range(5)]
            for x in range(5):
                for y in range(5):
                    b[y][(2 * x + 3 * y) % 5] = rol(a[x][y], _KECCAK_ROT[x][y])
            a = [[b[x][y] ^ ((~b[(x + 1) % 5][y]) & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
            a[0][0] ^= rc
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def _digest(hash_name: str, data: bytes) -> bytes:
    if hash_name in ("keccak256", "keccak_256"):
        return keccak256(data)
    return hashlib.new(hash_name, data).digest()


def hash_seed_for_matrix(key: bytes, tag: bytes, hash_name: str = "keccak256") -> GpuRngSeed:
    """H("GpuDCRTPolyHashSampler/v2" || key || tag || ctr_le32), src/sampler/gpu.rs:118-136; H is generic in the
    reference (its tests and callers use Keccak256), any hashlib name is accepted as well."""
    assert len(key) == 32
    out = b""
    counter = 0
    while len(out) < 32:
        out += _digest(hash_name, b"GpuDCRTPolyHashSampler/v2" + bytes(key) + bytes(tag) + (counter & 0xFFFFFFFF).to_bytes(4, "little"))
        counter += 1
    return GpuRngSeed.from_bytes(out[:32])


def sample_gpu_matrix_with_seed(params, nrow, ncol, dist: DistType, seed: GpuRngSeed) -> GpuDCRTPolyMatrix:
    if nrow == 0 or ncol == 0:
        return GpuDCRTPolyMatrix.zero(params, nrow, ncol)
    return GpuDCRTPolyMatrix.sample_distribution(params, nrow, ncol, dist.as_ffi(), dist.sigma, seed)


def sample_gpu_matrix_native(params, nrow, ncol, dist: DistType) -> GpuDCRTPolyMatrix:
    """a fresh seed per call (sampler/gpu.rs:144-151)"""
    return sample_gpu_matrix_with_seed(params, nrow, ncol, dist, random_gpu_rng_seed())


def sample_gpu_matrix_with_seed_columns(params, nrow, total_ncol, col_start, col_len, dist, seed):
    if nrow == 0 or col_len == 0:
        return GpuDCRTPolyMatrix.zero(params, nrow, col_len)
    return GpuDCRTPolyMatrix.sample_distribution_columns(
        params, nrow, total_ncol, col_start, col_len, dist.as_ffi(), dist.sigma, seed
    )


def sample_gpu_stack_with_seeds(params, nrow, ncol, dist: DistType, seeds) -> GpuDCRTPolyMatrix:
    """The len(seeds) x (nrow * ncol) matrix whose row t is sample_gpu_matrix_with_seed(params, nrow, ncol, dist, seeds[t])
    in row-major order: one stacked-layout call (the Gaussian blocks for GaussDist, the seeded blocks otherwise); where
    the library answers "unsupported" the rows are sampled one by one and copied in - the same matrix either way."""
    seeds = list(seeds)
    polys = nrow * ncol
    if not seeds or polys == 0:
        return GpuDCRTPolyMatrix.zero(params, len(seeds), polys)
    try:
        if dist.kind == "gauss":
            return GpuDCRTPolyMatrix.sample_gauss_blocks(params, seeds, dist.sigma, block_polys=polys)
        return GpuDCRTPolyMatrix.sample_distribution_blocks(params, seeds, dist.as_ffi(), block_polys=polys)
    except _ffi.GpuPolyError as e:
        if "unsupported" not in str(e):
            raise
    out = GpuDCRTPolyMatrix.new_empty(params, len(seeds), polys)
    for t, seed in enumerate(seeds):
        block = sample_gpu_matrix_with_seed(params, nrow, ncol, dist, seed)
        out.copy_block_from(block.reshape_view(1, polys), t, 0, 0, 0, 1, polys)
    return out


class GpuDCRTPolyUniformSampler:
    """`PolyUniformSampler` for the GPU (src/sampler/gpu.rs:16-46)."""

    def sample_uniform(self, params, nrow, ncol, dist: DistType) -> GpuDCRTPolyMatrix:
        return sample_gpu_matrix_with_seed(params, nrow, ncol, dist, random_gpu_rng_seed())

    def sample_uniform_many(self, params, nrow, ncol, dist: DistType, count, _seeds=None) -> GpuDCRTPolyMatrix:
        """`count` independent sample_uniform(params, nrow, ncol, dist) draws as one stack: the count x (nrow * ncol) matrix
        whose row t is draw t in row-major order (reshape_view / row_view give the matrices), sampled in one call - the
        per-gate `US::sample_uniform` calls of the GGH15 gate stages (src/lookup/ggh15/pubkey_gpu.rs:418-537) and of
        src/bgg/sampler_gpu.rs:125-135.  A fresh seed per draw, as the loop takes them; `_seeds` (tests) gives them."""
        seeds = [random_gpu_rng_seed() for _ in range(count)] if _seeds is None else list(_seeds)
        assert len(seeds) == count, "sample_uniform_many: one seed per draw"
        return sample_gpu_stack_with_seeds(params, nrow, ncol, dist, seeds)

    def sample_poly(self, params, dist: DistType) -> GpuDCRTPoly:
        return self.sample_uniform(params, 1, 1, dist).entry(0, 0)


class GpuDCRTPolyHashSampler:
    """`PolyHashSampler<[u8;32]>` for the GPU (src/sampler/gpu.rs:48-116); H defaults to Keccak256, the hash the
    reference instantiates it with."""

    def __init__(self, hash_name: str = "keccak256"):
        self.hash_name = hash_name

    def _on_device(self) -> bool:
        """whether tags are hashed on the device (gpupoly_hash_seeds, gpupoly_matrix_sample_hash_blocks; DESIGN.md section
        5q): the two Keccak paddings.  Any other hashlib name is hashed on the host - the same seeds either way."""
        return self.hash_name in DEVICE_HASHES

    def _seed(self, params, key, tag) -> GpuRngSeed:
        return self._seeds(key, [tag], params)[0]

    def sample_hash(self, params, key: bytes, tag: bytes, nrow, ncol, dist: DistType) -> GpuDCRTPolyMatrix:
        return sample_gpu_matrix_with_seed(params, nrow, ncol, dist, self._seed(params, key, tag))

    def sample_hash_columns(self, params, key, tag, nrow, total_ncol, col_start, col_len, dist):
        seed = self._seed(params, key, tag)
        return sample_gpu_matrix_with_seed_columns(params, nrow, total_ncol, col_start, col_len, dist, seed)

    def sample_hash_decomposed(self, params, key, tag, nrow, ncol, dist):
        """== sample_hash(...).decompose() (src/sampler/gpu.rs:91-103), in one extension call."""
        seed = self._seed(params, key, tag)
        return GpuDCRTPolyMatrix.sample_distribution_decomposed(params, nrow, ncol, dist.as_ffi(), dist.sigma, seed)

    def sample_hash_small_decomposed(self, params, key, tag, nrow, ncol, dist):
        """== sample_hash(...).small_decompose() (src/sampler/gpu.rs:104-115), in one extension call."""
        seed = self._seed(params, key, tag)
        return GpuDCRTPolyMatrix.sample_distribution_decomposed(params, nrow, ncol, dist.as_ffi(), dist.sigma, seed, True)

    def sample_hash_decomposed_columns(self, params, key, tag, nrow, total_ncol, col_start, col_len, dist,
                                       row_start=0, row_end=None):
        """== sample_hash_columns(...).decompose() (the trait default, src/sampler/mod.rs:84-97), in one extension call;
        with row_start / row_end, its rows [row_start, row_end) - the `rhs_full.slice(inner_start, ..)` of
        src/lookup/ggh15/poly_encoding_gpu.rs:515,566 - of which only those are computed."""
        seed = self._seed(params, key, tag)
        return GpuDCRTPolyMatrix.sample_distribution_decomposed_window(
            params, nrow, total_ncol, col_start, col_len, dist.as_ffi(), dist.sigma, seed, False, row_start, row_end)

    def sample_hash_small_decomposed_columns(self, params, key, tag, nrow, total_ncol, col_start, col_len, dist,
                                             row_start=0, row_end=None):
        """== sample_hash_columns(...).small_decompose() (the trait default, src/sampler/mod.rs:111-124), likewise"""
        seed = self._seed(params, key, tag)
        return GpuDCRTPolyMatrix.sample_distribution_decomposed_window(
            params, nrow, total_ncol, col_start, col_len, dist.as_ffi(), dist.sigma, seed, True, row_start, row_end)

    # ---- many tags in one call (gpupoly_matrix_sample_distribution_blocks, gpupoly_matrix_sample_hash_blocks; DESIGN.md
    # sections 5p, 5q) ------------------------------------------------------------------------------------------------
    def _seeds(self, key, tags, params=None):
        """[hash_seed_for_matrix(key, tag) for tag in tags]: one gpupoly_hash_seeds call per 2^20 tags on `params`' context
        where the hash has a device form, the host definition otherwise"""
        if params is not None and self._on_device():
            tags = tags if isinstance(tags, IndexedTags) else list(tags)
            seeds = []
            for lo in range(0, len(tags), 1 << 20):
                seeds += device_hash_seeds(params, key, tags[lo : lo + (1 << 20)], self.hash_name)
            return seeds
        return [hash_seed_for_matrix(key, tag, self.hash_name) for tag in tags]

    def _hash_blocks(self, params, key, tags, dist, **shape):
        """sample_hash_blocks (sample_hash_gauss_blocks for GaussDist) where the hash has a device form and the library does
        not answer "unsupported"; else None"""
        if not self._on_device():
            return None
        try:
            if dist.kind == "gauss":
                return GpuDCRTPolyMatrix.sample_hash_gauss_blocks(params, key, tags, dist.sigma, hash_name=self.hash_name, **shape)
            return GpuDCRTPolyMatrix.sample_hash_blocks(params, key, tags, dist.as_ffi(), hash_name=self.hash_name, **shape)
        except _ffi.GpuPolyError as e:
            if "unsupported" not in str(e):
                raise
        return None

    def sample_hash_many(self, params, key: bytes, tags, nrow, ncol, dist: DistType) -> list:
        """== [sample_hash(params, key, tag, nrow, ncol, dist) for tag in tags] - the tagged loops of
        src/commit/wee25.rs:687-703, src/lookup/ggh15/pubkey_gpu.rs:924,1296 and src/lookup/lwe/pubkey_gpu.rs:559,616.
        Under a Keccak hash: ONE columns-layout sample with the tags hashed on the device (no seeds on the host; an
        `IndexedTags` is not even uploaded) per 2^20 tags - the Gaussian blocks for GaussDist -, and
        one split_columns per 64 of them.  Otherwise one columns-layout sample and one split_columns per 64 tags over host- or
        device-derived seeds (Gaussian requests through the Gaussian segments).  Where the library answers "unsupported"
        (MXX_HIP_RNG_COMPAT=reference, rings the Gaussian entries do not cover) the tags are sampled one by one: the same
        matrices either way."""
        tags = tags if isinstance(tags, IndexedTags) else list(tags)
        if nrow == 0 or ncol == 0:
            return [GpuDCRTPolyMatrix.zero(params, nrow, ncol) for _ in range(len(tags))]
        outs = []
        for lo in range(0, len(tags), 1 << 20):  # the entry's block limit; "unsupported" is the first call's answer or nobody's
            part = tags[lo : lo + (1 << 20)]
            wide = self._hash_blocks(params, key, part, dist, nrow=nrow, seg_cols=[ncol] * len(part))
            if wide is None:
                break
            for at in range(0, len(part), 64):
                width = min(64, len(part) - at)
                piece = wide if width == len(part) else wide.slice_columns(at * ncol, (at + width) * ncol)
                outs.extend(piece.split_columns([ncol] * width))
        if len(outs) == len(tags):
            return outs
        outs = []
        seeds = self._seeds(key, tags, params)
        for lo in range(0, len(tags), 64):
            chunk = seeds[lo : lo + 64]
            widths = [ncol] * len(chunk)
            try:
                if dist.kind == "gauss":
                    wide = GpuDCRTPolyMatrix.sample_distribution_segments(params, nrow, widths, dist.as_ffi(), dist.sigma, chunk)
                else:
                    wide = GpuDCRTPolyMatrix.sample_distribution_blocks(params, chunk, dist.as_ffi(), nrow=nrow, seg_cols=widths)
            except _ffi.GpuPolyError as e:
                if "unsupported" not in str(e):
                    raise
                outs.extend(sample_gpu_matrix_with_seed(params, nrow, ncol, dist, s) for s in chunk)
                continue
            outs.extend(wide.split_columns(widths))
        return outs

    def sample_hash_decomposed_columns_many(self, params, key: bytes, tags, nrow, total_ncol, col_start, col_len, dist: DistType) -> list:
        """== [sample_hash_decomposed_columns(params, key, tag, nrow, total_ncol, col_start, col_len, dist) for tag in tags]:
        the same column chunk of many tags' decomposed matrices - the V of every LUT row of a wave
        (src/lookup/ggh15/pubkey_gpu.rs:398-407).  Uniform / bit / ternary under a Keccak hash: ONE
        gpupoly_matrix_sample_hash_decomposed_blocks call per 2^20 tags and one split_columns per 64
        of them.  The Gaussian distribution, other hashes and the library's "unsupported" answer (MXX_HIP_RNG_COMPAT=reference) go tag by tag:
        the same matrices either way."""
        tags = tags if isinstance(tags, IndexedTags) else list(tags)
        count = len(tags)
        if dist.kind != "gauss" and self._on_device() and 0 < count <= 1 << 20:
            try:
                out = GpuDCRTPolyMatrix.sample_hash_decomposed_blocks(params, key, tags, nrow, total_ncol, col_start, col_len, dist.as_ffi(),
                                                                      hash_name=self.hash_name)
            except _ffi.GpuPolyError as e:
                if "unsupported" not in str(e):
                    raise
                out = None
            if out is not None:
                parts = []
                for at in range(0, count, 64):
                    width = min(64, count - at)
                    piece = out if width == count else out.slice_columns(at * col_len, (at + width) * col_len)
                    parts.extend(piece.split_columns([col_len] * width))
                return parts
        return [self.sample_hash_decomposed_columns(params, key, tag, nrow, total_ncol, col_start, col_len, dist) for tag in tags]

    def sample_hash_stacked(self, params, key: bytes, tags, nrow, ncol, dist: DistType) -> GpuDCRTPolyMatrix:
        """The len(tags) x (nrow * ncol) matrix whose row t is sample_hash(params, key, tags[t], nrow, ncol, dist) in
        row-major order, sampled in one stacked-layout call - under a Keccak hash with the tags hashed on the device, no seeds
        on the host; where the library answers "unsupported" (MXX_HIP_RNG_COMPAT=reference, a Gaussian request on a ring
        below n = 128) the rows are sampled one by one and copied in."""
        tags = tags if isinstance(tags, IndexedTags) else list(tags)
        polys = nrow * ncol
        if not len(tags) or polys == 0:
            return GpuDCRTPolyMatrix.zero(params, len(tags), polys)
        if len(tags) <= 1 << 20:
            out = self._hash_blocks(params, key, tags, dist, block_polys=polys)
            if out is not None:
                return out
        return sample_gpu_stack_with_seeds(params, nrow, ncol, dist, self._seeds(key, tags, params))

    def sample_hash_weighted_sum(self, params, key: bytes, tags, weights, nrow, ncol, addend=None, negate: bool = False,
                                 max_stack_bytes: int = 1 << 30) -> GpuDCRTPolyMatrix:
        """addend +- sum_t sample_hash(params, key, tags[t], nrow, ncol, FinRingDist) o weights[0, t]: every sampled
        nrow x ncol matrix multiplied by one polynomial and summed.  `weights` is a 1 x len(tags) EVAL matrix, `addend`
        None or an nrow x ncol EVAL matrix (left as it is).

        This is `commit_base` of src/commit/wee25.rs:858-883, `acc += sample_hash(tag(j * m_g + r)) * a_{j,r}` over the
        columns j of the message and the digit rows r of G^-1(msg[:, j]), in three calls:
            D = msg.decompose()                                          # m_g x cols
            weights = D.transpose().reshape_view(1, cols * m_g)          # a_{j,r} at column j * m_g + r
            sampler.sample_hash_weighted_sum(params, key, tags, weights, secret_size, m_b)
        The tags' matrices are sampled straight into one stacked T x (nrow * ncol) matrix (sample_hash_stacked), so the
        sum is the one-row product weights * stack - the shape the packed skinny kernel streams at 3 bytes per residue
        where the moduli fit - instead of a sample, a scalar product, an addition and a temporary per term.  The tags go
        in chunks whose stack stays within max_stack_bytes (in 4- or 8-byte words; at least one tag per chunk): per chunk
        one stacked sample, one product, one accumulation into a 1 x (nrow * ncol) row.  The result is that row seen as
        nrow x ncol (reshape_view): no copy."""
        tags = tags if isinstance(tags, IndexedTags) else list(tags)
        polys = nrow * ncol
        assert weights.is_ntt and (weights.nrow, weights.ncol) == (1, len(tags)), "sample_hash_weighted_sum: weights is a 1 x len(tags) EVAL matrix"
        if addend is not None:
            assert addend.is_ntt and (addend.nrow, addend.ncol) == (nrow, ncol) and addend.level == weights.level, \
                "sample_hash_weighted_sum: the addend is an nrow x ncol EVAL matrix at the weights' level"
        assert weights.level == params.crt_depth() - 1, "sample_hash_weighted_sum: full level"
        acc = None if addend is None else addend.reshape_view(1, polys)
        own = False  # acc is still the caller's addend: read only, the first sum goes into a fresh row
        if polys:
            poly_bytes = (weights.level + 1) * params.ring_dimension() * params.ctx().word_bytes()
            step = max(1, int(max_stack_bytes) // (polys * poly_bytes))
            dist = DistType.FinRingDist()
            for lo in range(0, len(tags), step):
                hi = min(lo + step, len(tags))
                stack = self.sample_hash_stacked(params, key, tags[lo:hi], nrow, ncol, dist)
                w = weights if (lo, hi) == (0, len(tags)) else weights.slice_columns(lo, hi)
                term = w * stack  # 1 x polys; a packed stack is read as it lies
                if acc is None:
                    acc = -term if negate else term
                elif not own:
                    acc = acc - term if negate else acc + term
                elif negate:
                    acc.sub_in_place(term)
                else:
                    acc.add_in_place(term)
                own = True
        if acc is None:
            acc = GpuDCRTPolyMatrix.zero(params, 1, polys)
        elif not own:  # no term: the result must not share the addend's storage
            acc = acc.clone()
        return acc.reshape_view(nrow, ncol)
