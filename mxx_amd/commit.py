"""The Wee25 commitment (src/commit/wee25.rs): `Wee25Commit` and `Wee25PublicParams` with the mirror's operations.

The public parameters hold one trapdoor preimage per index idx < pp_size = tree_base * m_b * m_g and column part of the
m_b x (l * k) Gaussian matrix T_bottom (l = tree_base * m_b, k = modulus_digits), of the target (:696-728)

    target(idx, p) = G_s * J(idx, p) - W_idx * T_bottom[:, p * m_b .. (p + 1) * m_b),
    W_idx = sample_hash(key, "wee25_w_block_" || idx as 8 little-endian bytes, s, m_b, FinRingDist),

J(idx, p) the rows G^-1(row_i) of build_j_2m_block (:536-584).  `build_j_2m_block` and `t_top_target_block` are the
reference's statements restated one by one, the comparison leg; `t_top_target_blocks` builds the targets of many indices
and parts in ONE library call (gpupoly_matrix_wee25_targets); `sample_t_top_preimages` feeds them
into the batched preimage, the body of the reference's t_top loop; `sample_public_params` is that loop in waves.  The
commitment, the opening and the verifier (:760-1194) are literal restatements, so the reference's acceptance predicate
runs against the batched parameters; `commit_base` alone is batched (sample_hash_weighted_sum).  Checkpoint files and
resume are not mirrored."""
from __future__ import annotations

from dataclasses import dataclass, field

from . import _ffi
from .matrix import GpuDCRTPolyMatrix, IndexedTags
from .sampler import DistType, GpuDCRTPolyHashSampler, GpuDCRTPolyUniformSampler
from .trapdoor import GpuDCRTPolyTrapdoorSampler

W_BLOCK_PREFIX = b"wee25_w_block_"


@dataclass
class Wee25PublicParams:
    """Wee25PublicParams (:39-45): b, the parts of T_bottom and the t_top blocks keyed (idx, col_start) - matrices, or their
    compact bytes as the reference stores them."""

    b: GpuDCRTPolyMatrix
    hash_key: bytes
    t_bottom_parts: list
    t_top: dict = field(default_factory=dict)


def _matrix(params, block):
    """a stored block as a matrix (M::from_compact_bytes where it is stored as bytes)"""
    return GpuDCRTPolyMatrix.from_compact_bytes(params, block).ensure_eval() if isinstance(block, (bytes, bytearray)) else block


def _concat_columns(mats):
    return mats[0] if len(mats) == 1 else mats[0].concat_columns(mats[1:])


class Wee25Commit:
    """Wee25Commit (:29-37, `new`): m_g = secret_size * modulus_digits, m_b = secret_size * (modulus_digits + 2), the column
    count of the trapdoor's public matrix."""

    def __init__(self, params, secret_size: int, tree_base: int, trapdoor_sigma: float, hash_name: str = "keccak256"):
        assert secret_size >= 1 and tree_base >= 2
        self.params, self.secret_size, self.tree_base = params, int(secret_size), int(tree_base)
        self.trapdoor_sigma, self.hash_name = float(trapdoor_sigma), hash_name
        self.hash_key = None  # the key of the W blocks: sample_public_params sets it, the target builders take it or this
        self.log_base_q = params.modulus_digits()
        self.m_g = self.secret_size * self.log_base_q
        self.m_b = self.secret_size * (self.log_base_q + 2)

    # ------------------------------------------------------------------ sizes, tags, the hit of an index
    @property
    def pp_size(self) -> int:
        return self.tree_base * self.m_b * self.m_g

    @property
    def l(self) -> int:
        return self.tree_base * self.m_b

    @property
    def j_2m_cols(self) -> int:
        return self.l * self.log_base_q

    @property
    def nparts(self) -> int:
        return self.j_2m_cols // self.m_b

    def sampler(self) -> GpuDCRTPolyHashSampler:
        return GpuDCRTPolyHashSampler(self.hash_name)

    @staticmethod
    def tag(idx: int) -> bytes:
        """:693-695"""
        return W_BLOCK_PREFIX + int(idx).to_bytes(8, "little")

    @staticmethod
    def tags(first: int, count: int) -> IndexedTags:
        """the tags of the consecutive indices first .. first + count - 1, generated on the device"""
        return IndexedTags(W_BLOCK_PREFIX, first, count)

    def j_2m_hit(self, idx: int):
        """(i*, kk, first global column): the one non-zero row of build_j_2m_block(idx, .) before decomposition is row i*,
        holding g[kk] * g[s'] at the global columns first + s', s' < modulus_digits - the closed form of the arithmetic
        of :549-575 (tests/test_wee25_structure.py compares them for every index)."""
        k = self.log_base_q
        bg, rho = divmod(int(idx), self.m_g)
        return rho // k, rho % k, bg * k

    def _key(self, hash_key) -> bytes:
        key = self.hash_key if hash_key is None else hash_key
        assert key is not None and len(key) == 32, "Wee25Commit: a 32-byte hash key (argument or self.hash_key)"
        return bytes(key)

    def w_block(self, idx: int, hash_key=None) -> GpuDCRTPolyMatrix:
        """:696-703"""
        return self.sampler().sample_hash(self.params, self._key(hash_key), self.tag(idx), self.secret_size, self.m_b, DistType.FinRingDist())

    # ------------------------------------------------------------------ the literal leg
    def build_j_2m_block(self, idx: int, col_start: int) -> GpuDCRTPolyMatrix:
        """build_j_2m_block (:536-584), statement by statement."""
        p, m_g, m_b, k = self.params, self.m_g, self.m_b, self.log_base_q
        gadget_row = GpuDCRTPolyMatrix.gadget_matrix(p, 1).get_row(0)
        col_end = col_start + m_b
        assert col_end <= self.j_2m_cols
        block_group = idx // m_g
        assert block_group < self.l
        rows = []
        for i in range(self.secret_size):
            r = idx * self.secret_size + i
            r_g_start = r * k
            slice_start = block_group * m_g * m_g
            offset = r_g_start - slice_start
            step = m_g + 1
            row_mat = GpuDCRTPolyMatrix.zero(p, 1, m_b)
            c = (offset + step - 1) // step
            if c < m_g:
                pos = slice_start + c * step
                if pos <= r_g_start + k - 1:
                    coeff = gadget_row[pos - r_g_start]
                    for s in range(k):
                        global_col = block_group * k + s
                        if global_col < col_start or global_col >= col_end:
                            continue
                        row_mat.set_entry(0, global_col - col_start, coeff * gadget_row[s])
            rows.append(row_mat.decompose())
        return rows[0].concat_rows(rows[1:])

    def t_top_target_block(self, idx: int, col_start: int, t_bottom_part, hash_key=None) -> GpuDCRTPolyMatrix:
        """The target of (idx, col_start) as the reference builds it (:696-719): the comparison leg."""
        p = self.params
        w_block = self.w_block(idx, hash_key)
        gadget = GpuDCRTPolyMatrix.gadget_matrix(p, self.secret_size)
        wt_bottom = w_block * _matrix(p, t_bottom_part)
        j_2m_block = self.build_j_2m_block(idx, col_start)
        gadget_j_2m_block = gadget * j_2m_block
        return gadget_j_2m_block - wt_bottom

    # ------------------------------------------------------------------ the batched leg
    def t_top_target_blocks(self, t_bottom, idxs, part_start: int = 0, nparts=None, hash_key=None) -> list:
        """[[t_top_target_block(idx, (part_start + p) * m_b, part part_start + p of t_bottom) for p < nparts] for idx in idxs] in
        ONE library call.  `t_bottom` is the whole m_b x j_2m_cols matrix.  A consecutive run of indices sends its tags in
        the indexed form, anything else as a table.  Where the library answers "unsupported"
        (MXX_HIP_RNG_COMPAT=reference) and for hashes without a device form the literal loop runs: the same matrices
        either way."""
        idxs, hash_key = [int(i) for i in idxs], self._key(hash_key)
        m_b = self.m_b
        assert t_bottom.nrow == m_b and t_bottom.ncol % m_b == 0
        nparts = t_bottom.ncol // m_b - part_start if nparts is None else int(nparts)
        if idxs and nparts and self.sampler()._on_device():
            run = all(b == a + 1 for a, b in zip(idxs, idxs[1:]))
            tags = self.tags(idxs[0], len(idxs)) if run else [self.tag(i) for i in idxs]
            try:
                return GpuDCRTPolyMatrix.wee25_targets(t_bottom, part_start, nparts, self.secret_size, idxs, hash_key, tags, self.hash_name)
            except _ffi.GpuPolyError as e:
                if "unsupported" not in str(e):
                    raise
        parts = [t_bottom.slice_columns((part_start + q) * m_b, (part_start + q + 1) * m_b) for q in range(nparts)]
        return [[self.t_top_target_block(i, (part_start + q) * m_b, parts[q], hash_key) for q in range(nparts)] for i in idxs]

    def sample_t_top_preimages(self, trap_sampler, trapdoor, b, t_bottom, idxs, part_start: int = 0, nparts=None, _seeds=None,
                               hash_key=None) -> dict:
        """The t_top blocks of `idxs` x the parts - the body of the loop of :679-753 for one wave: the targets in one call,
        then `preimage_many_abi` (one gpupoly_trapdoor_preimage_many call) over all of them, index by index and part by
        part.  `_seeds`: one (p2, p1, z) seed triple per target in that order.  Returns {(idx, col_start): (target, preimage)}."""
        idxs = [int(i) for i in idxs]
        nparts = t_bottom.ncol // self.m_b - part_start if nparts is None else int(nparts)
        targets = self.t_top_target_blocks(t_bottom, idxs, part_start, nparts, hash_key)
        flat = [t for row in targets for t in row]
        preimages = trap_sampler.preimage_many_abi(self.params, trapdoor, b, flat, _seeds=_seeds)
        out, at = {}, 0
        for idx, row in zip(idxs, targets):
            for q, target in enumerate(row):
                out[(idx, (part_start + q) * self.m_b)] = (target, preimages[at])
                at += 1
        return out

    def sample_public_params(self, hash_key: bytes, batch: int = 8, as_bytes: bool = False, _setup=None, _seeds=None) -> Wee25PublicParams:
        """sample_public_params (:494-758) in memory: the trapdoor, T_bottom in one Gaussian call, t_top in waves of `batch`
        indices (wee25_topj_parallel_batch), each wave one target call and one preimage call.  `as_bytes`: the blocks
        stored as compact bytes (into_compact_bytes_many), as the reference stores them.  `_setup` = (trapdoor, b,
        t_bottom) already sampled and `_seeds` = {(idx, col_start): seed triple} make two runs comparable."""
        p, m_b = self.params, self.m_b
        self.hash_key = bytes(hash_key)
        trap_sampler = GpuDCRTPolyTrapdoorSampler(p, self.trapdoor_sigma)
        if _setup is None:
            trapdoor, b = trap_sampler.trapdoor(p, self.secret_size)
            t_bottom = GpuDCRTPolyUniformSampler().sample_uniform(p, m_b, self.j_2m_cols, DistType.GaussDist(self.trapdoor_sigma))
        else:
            trapdoor, b, t_bottom = _setup
        assert b.ncol == m_b, "Wee25PublicParams m_b mismatch"
        col_starts = list(range(0, self.j_2m_cols, m_b))
        t_bottom_parts = [t_bottom.slice_columns(c, c + m_b) for c in col_starts]
        t_top = {}
        for chunk_start in range(0, self.pp_size, max(1, int(batch))):
            idxs = list(range(chunk_start, min(chunk_start + max(1, int(batch)), self.pp_size)))
            seeds = None if _seeds is None else [_seeds[(i, c)] for i in idxs for c in col_starts]
            wave = self.sample_t_top_preimages(trap_sampler, trapdoor, b, t_bottom, idxs, _seeds=seeds)
            keys = list(wave)
            blocks = [wave[key][1] for key in keys]
            if as_bytes:
                blocks = GpuDCRTPolyMatrix.into_compact_bytes_many(blocks)
            t_top.update(zip(keys, blocks))
        if as_bytes:
            t_bottom_parts = GpuDCRTPolyMatrix.into_compact_bytes_many(t_bottom_parts)
        return Wee25PublicParams(b, bytes(hash_key), t_bottom_parts, t_top)

    # ------------------------------------------------------------------ commit
    def assert_stream_len(self, cols: int) -> None:
        """:1196-1215"""
        assert cols >= self.tree_base
        while cols > self.tree_base:
            assert cols % self.tree_base == 0, "message block count must be a power of tree_base"
            cols //= self.tree_base
        assert cols == self.tree_base

    def commit_base_literal(self, msg, public_params) -> GpuDCRTPolyMatrix:
        """commit_base (:842-884) term by term: the comparison leg."""
        p = self.params
        acc = GpuDCRTPolyMatrix.zero(p, self.secret_size, self.m_b)
        for j in range(msg.ncol):
            decomposed_col = msg.get_column_matrix_decompose(j)
            for r in range(self.m_g):
                acc = acc + self.w_block(j * self.m_g + r, public_params.hash_key) * decomposed_col.entry(r, 0)
        return acc

    def commit_base(self, msg, public_params) -> GpuDCRTPolyMatrix:
        """commit_base (:842-884) in the three calls of `sample_hash_weighted_sum`'s docstring."""
        assert (msg.nrow, msg.ncol) == (self.secret_size, self.tree_base * self.m_b)
        d = msg.ensure_eval().decompose().ensure_eval()  # m_g x cols
        weights = d.transpose().reshape_view(1, msg.ncol * self.m_g)  # a_{j,r} at column j * m_g + r
        return self.sampler().sample_hash_weighted_sum(self.params, public_params.hash_key, self.tags(0, msg.ncol * self.m_g), weights,
                                                       self.secret_size, self.m_b)

    def commit(self, msg_blocks, public_params, cache=None) -> GpuDCRTPolyMatrix:
        """commit (:760-773): `msg_blocks` is the list of s x m_b message blocks; `cache` (a dict) receives the nodes keyed
        (offset, len), as CommitCache holds them."""
        self.assert_stream_len(len(msg_blocks))
        return self.commit_recursive(list(msg_blocks), 0, public_params, {} if cache is None else cache)

    def commit_recursive(self, blocks, offset, public_params, cache) -> GpuDCRTPolyMatrix:
        """commit_recursive (:798-840)"""
        cols = len(blocks)
        if cols == self.tree_base:
            commit = self.commit_base(_concat_columns(blocks), public_params)
            cache[(offset, cols)] = commit
            return commit
        child_cols = cols // self.tree_base
        commits = [self.commit_recursive(blocks[i * child_cols:(i + 1) * child_cols], offset + i * child_cols, public_params, cache)
                   for i in range(self.tree_base)]
        commit = self.commit_base(_concat_columns(commits), public_params)
        cache[(offset, cols)] = commit
        return commit

    # ------------------------------------------------------------------ verifier
    def verifier_base(self, public_params, is_leaf: bool) -> GpuDCRTPolyMatrix:
        """verifier_base (:1170-1194)"""
        p = self.params
        t_bottom = _concat_columns([_matrix(p, part) for part in public_params.t_bottom_parts])
        if is_leaf:
            return t_bottom * GpuDCRTPolyMatrix.identity(p, self.l).decompose()
        return t_bottom

    def verifier_recursive(self, base, base_last, cols, col_idx, cache) -> GpuDCRTPolyMatrix:
        """verifier_recursive (:1120-1168)"""
        if (cols, col_idx) in cache:
            return cache[(cols, col_idx)]
        if cols == self.tree_base:
            result = base_last.slice_columns(self.m_b * col_idx, self.m_b * (col_idx + 1))
        else:
            child_cols = cols // self.tree_base
            child_col = self.verifier_recursive(base, base_last, child_cols, col_idx % child_cols, cache)
            slice_width = base.ncol // self.tree_base
            sibling_idx = col_idx // child_cols
            result = base.slice_columns(slice_width * sibling_idx, slice_width * (sibling_idx + 1)) * child_col.decompose()
        cache[(cols, col_idx)] = result
        return result

    def verifier(self, cols: int, col_range, public_params) -> GpuDCRTPolyMatrix:
        """verifier (:1079-1118); `col_range` None or a range of message blocks"""
        col_range = range(cols) if col_range is None else col_range
        assert len(col_range) > 0
        self.assert_stream_len(cols)
        base, base_last, cache = self.verifier_base(public_params, False), self.verifier_base(public_params, True), {}
        return _concat_columns([self.verifier_recursive(base, base_last, cols, c, cache) for c in col_range])

    # ------------------------------------------------------------------ open
    def open_base(self, msg, col_idx: int, public_params, is_leaf: bool) -> GpuDCRTPolyMatrix:
        """open_base (:993-1077)"""
        p, m_b, k = self.params, self.m_b, self.log_base_q
        assert (msg.nrow, msg.ncol) == (self.secret_size, self.tree_base * m_b) and col_idx < self.tree_base
        slice_width = m_b * k
        col_start = slice_width * col_idx
        part_col_starts = [col_start + m_b * digit_idx for digit_idx in range(k)]
        acc = GpuDCRTPolyMatrix.zero(p, m_b, slice_width)
        for j in range(msg.ncol):
            decomposed_col = msg.get_column_matrix_decompose(j)
            for r in range(self.m_g):
                part_idx = j * self.m_g + r
                t_part = _concat_columns([_matrix(p, public_params.t_top[(part_idx, c)]) for c in part_col_starts])
                acc = acc + t_part * decomposed_col.entry(r, 0)
        if is_leaf:
            return acc * GpuDCRTPolyMatrix.identity(p, m_b).decompose()
        return acc

    def open_recursive(self, blocks, offset, col_idx, v_base, v_base_last, public_params, commit_cache, z_prime_cache, verifier_cache):
        """open_recursive (:933-991)"""
        cols = len(blocks)
        if cols == self.tree_base:
            return self.open_base(_concat_columns(blocks), col_idx, public_params, True)
        child_cols = cols // self.tree_base
        child_col_idx, sibling_idx = col_idx % child_cols, col_idx // child_cols
        commits_msg = _concat_columns([commit_cache[(offset + j * child_cols, child_cols)] for j in range(self.tree_base)])
        z_prime_key = (offset, cols, sibling_idx)
        if z_prime_key not in z_prime_cache:
            z_prime_cache[z_prime_key] = self.open_base(commits_msg, sibling_idx, public_params, False)
        z_prime = z_prime_cache[z_prime_key]
        z_child = self.open_recursive(blocks[child_cols * sibling_idx:child_cols * (sibling_idx + 1)], offset + child_cols * sibling_idx,
                                      child_col_idx, v_base, v_base_last, public_params, commit_cache, z_prime_cache, verifier_cache)
        verifier = self.verifier_recursive(v_base, v_base_last, child_cols, child_col_idx, verifier_cache)
        return z_prime * verifier.decompose() + z_child

    def open(self, msg_blocks, col_range, public_params, commit_cache) -> GpuDCRTPolyMatrix:
        """open (:886-931): `commit_cache` is the dict `commit` filled for these blocks"""
        blocks = list(msg_blocks)
        self.assert_stream_len(len(blocks))
        v_base, v_base_last = self.verifier_base(public_params, False), self.verifier_base(public_params, True)
        z_prime_cache, verifier_cache = {}, {}
        col_range = range(len(blocks)) if col_range is None else col_range
        assert len(col_range) > 0 and col_range[-1] < len(blocks)
        return _concat_columns([self.open_recursive(blocks, 0, c, v_base, v_base_last, public_params, commit_cache, z_prime_cache,
                                                    verifier_cache) for c in col_range])

    def verify(self, msg, commit, opening, col_range, public_params) -> bool:
        """verify (:775-796): commit * verifier == msg[:, range] - b * opening"""
        assert msg.nrow == self.secret_size and msg.ncol % self.m_b == 0
        verifier = self.verifier(msg.ncol // self.m_b, col_range, public_params)
        target_msg = msg if col_range is None else msg.slice_columns(self.m_b * col_range[0], self.m_b * (col_range[-1] + 1))
        return commit * verifier == target_msg - public_params.b * opening
