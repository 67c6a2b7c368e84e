"""`GpuDCRTPolyMatrix` — host-side mirror of the reference's GPU matrix wrapper.

Same names, argument meaning and error behaviour as
`src/matrix/gpu_dcrt_poly.rs:221-1678,1716-1895` (the `PolyMatrix` trait is
`src/matrix/mod.rs:45-379`); every method is a thin sequence of C-ABI calls into
libgpupoly (include/gpupoly.h).  Host data crosses the boundary as numpy uint64
arrays in the wire layout (rows, cols, level+1, n) — the `[poly][limb][n]` u64
layout of `load/store_rns_bytes` (gpu_dcrt_poly.rs:576-663).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref

import numpy as np

from . import _ffi
from ._ffi import GPU_POLY_FORMAT_COEFF, GPU_POLY_FORMAT_EVAL, GpuRngSeed, check_status
from .params import GpuDCRTPolyParams


def mul_decompose_column_chunk_width_is_set() -> bool:
    return bool(os.environ.get("MXX_MUL_DECOMPOSE_COLUMN_CHUNK_WIDTH"))


def mul_decompose_column_chunk_width() -> int:
    """`MXX_MUL_DECOMPOSE_COLUMN_CHUNK_WIDTH`, default 1 (src/env.rs of the reference)."""
    try:
        return max(1, int(os.environ.get("MXX_MUL_DECOMPOSE_COLUMN_CHUNK_WIDTH", "1")))
    except ValueError:
        return 1


def _bincode_varint(v: int) -> bytes:
    """bincode 2 `config::standard()` unsigned varint (u16/u32/u64/usize)."""
    if v < 251:
        return bytes([v])
    if v < 1 << 16:
        return bytes([251]) + v.to_bytes(2, "little")
    if v < 1 << 32:
        return bytes([252]) + v.to_bytes(4, "little")
    return bytes([253]) + v.to_bytes(8, "little")


def _bincode_read_varint(data: bytes, pos: int):
    tag = data[pos]
    if tag < 251:
        return tag, pos + 1
    width = {251: 2, 252: 4, 253: 8}[tag]
    return int.from_bytes(data[pos + 1 : pos + 1 + width], "little"), pos + 1 + width


def block_size() -> int:
    """`BLOCK_SIZE`, default 100 (src/env.rs:175-178): entries per side of a stored matrix block."""
    try:
        value = int(os.environ.get("BLOCK_SIZE", "100"))
    except ValueError:
        return 100
    return value if value >= 1 else 100  # the reference parses a usize: "0" would never advance, a negative value does not parse


def block_offsets(rng: range, block: int) -> list:
    """[start, start + block, ..., stop] (gpu_dcrt_poly.rs:1899-1909)."""
    assert block > 0, "block_offsets: block must be positive"
    offsets, cur = [rng.start], rng.start
    while cur < rng.stop:
        cur = min(cur + block, rng.stop)
        offsets.append(cur)
    return offsets


def rns_bytes_len_for_level(params, level: int) -> int:
    """(level + 1) * n * 8: one polynomial in the `[limb][n]` u64 wire layout (gpu_dcrt_poly.rs:1916-1920)."""
    assert level < params.crt_depth(), "invalid RNS byte length level"
    return (level + 1) * params.ring_dimension() * 8


def rns_bytes_len(params) -> int:
    """gpu_dcrt_poly.rs:1911-1914."""
    return rns_bytes_len_for_level(params, max(params.crt_depth() - 1, 0))


def one_rns_bytes(params) -> bytes:
    """EVAL wire bytes of the constant polynomial 1 (gpu_dcrt_poly.rs:1922-1932)."""
    if rns_bytes_len(params) == 0:
        return b""
    one = GpuDCRTPolyMatrix.identity(params, 1)
    return one.to_rns().tobytes()


class GpuDCRTMatrixRnsSnapshot:
    """Host copy of a matrix in the u64 wire layout with its shape, level and format tag
    (gpu_dcrt_poly.rs:72-120): what callers keep between devices / across a device reset."""

    __slots__ = ("_nrow", "_ncol", "_level", "_is_ntt", "_bytes_per_poly", "_bytes")

    def __init__(self, nrow, ncol, level, is_ntt, bytes_per_poly, data):
        self._nrow, self._ncol, self._level, self._is_ntt = int(nrow), int(ncol), int(level), bool(is_ntt)
        self._bytes_per_poly = int(bytes_per_poly)
        self._bytes = bytes(data)

    def nrow(self) -> int:
        return self._nrow

    def ncol(self) -> int:
        return self._ncol

    def level(self) -> int:
        return self._level

    def is_ntt(self) -> bool:
        return self._is_ntt

    def bytes_per_poly(self) -> int:
        return self._bytes_per_poly

    def bytes(self) -> bytes:
        return self._bytes

    def validate_for_params(self, params) -> None:
        assert self._level < params.crt_depth(), "invalid RNS snapshot level"
        assert self._bytes_per_poly == rns_bytes_len_for_level(params, self._level), "RNS snapshot bytes_per_poly mismatch"
        assert len(self._bytes) == self._nrow * self._ncol * self._bytes_per_poly, "RNS snapshot byte length mismatch"

    def __eq__(self, other) -> bool:
        if not isinstance(other, GpuDCRTMatrixRnsSnapshot):
            return NotImplemented
        return all(getattr(self, f) == getattr(other, f) for f in self.__slots__)

    def __repr__(self) -> str:
        return (f"GpuDCRTMatrixRnsSnapshot(nrow={self._nrow}, ncol={self._ncol}, level={self._level}, "
                f"is_ntt={self._is_ntt}, bytes_per_poly={self._bytes_per_poly}, bytes={len(self._bytes)})")


def _bincode_read_nested_bytes(data: bytes) -> list:
    """bincode 2 `config::standard()` Vec<Vec<Vec<u8>>>: varint lengths, raw bytes innermost."""
    pos = 0
    nrows, pos = _bincode_read_varint(data, pos)
    out = []
    for _ in range(nrows):
        ncols, pos = _bincode_read_varint(data, pos)
        row = []
        for _ in range(ncols):
            blen, pos = _bincode_read_varint(data, pos)
            assert pos + blen <= len(data), "truncated matrix block file"
            row.append(data[pos : pos + blen])
            pos += blen
        out.append(row)
    return out


def _bincode_nested_bytes(entries) -> bytes:
    """inverse of `_bincode_read_nested_bytes` (what the reference's `write_to_files` side produces)."""
    parts = [_bincode_varint(len(entries))]
    for row in entries:
        parts.append(_bincode_varint(len(row)))
        for e in row:
            parts.append(_bincode_varint(len(e)))
            parts.append(bytes(e))
    return b"".join(parts)


# ---- pinned host staging, one grow-only buffer per thread (compact wire format: device -> host at PCIe rate) ----------
_pinned_tls = threading.local()


def _pinned_capacity() -> int:
    return getattr(_pinned_tls, "size", 0)


def _pinned_buffer(nbytes: int) -> int:
    """address of this thread's pinned buffer, at least `nbytes` long (gpu_pinned_alloc; released when the thread ends)"""
    if _pinned_capacity() < nbytes:
        old = getattr(_pinned_tls, "holder", None)
        if old is not None:
            old.release()
        size = max(nbytes, 1 << 20)
        ptr = _ffi.lib().gpu_pinned_alloc(size)
        if not ptr:
            _pinned_tls.holder, _pinned_tls.size = None, 0
            raise _ffi.GpuPolyError(f"gpu_pinned_alloc({size}) failed: {_ffi.last_error_string()}")
        _pinned_tls.holder, _pinned_tls.size = _PinnedBlock(ptr), size
    return _pinned_tls.holder.ptr


class _PinnedBlock:
    def __init__(self, ptr):
        self.ptr = ptr
        self._fin = weakref.finalize(self, _ffi.lib().gpu_pinned_free, C.c_void_p(ptr))

    def release(self):
        self._fin()


class GpuP1CovarianceCache:
    def __init__(self, raw, params=None):
        self.raw = raw
        self.params = params  # the C object frees into its context's allocator: the context must outlive it (the Rust side holds an Arc)
        self._finalizer = weakref.finalize(self, _ffi.lib().gpu_matrix_destroy_p1_covariance_cache, raw)


def _max_along(entries, axis, nrow, ncol):
    """[row][col] values -> the whole-matrix max (axis=None), per row (1), per column (0) or as they are ("entries")"""
    if isinstance(axis, str):
        if axis != "entries":
            raise ValueError(f"axis must be None, 0, 1 or 'entries' (got {axis!r})")
        return entries
    if axis is None:
        return max((v for row in entries for v in row), default=0)
    if axis == 1:
        return [max(row, default=0) for row in entries]
    if axis == 0:
        return [max((entries[r][c] for r in range(nrow)), default=0) for c in range(ncol)]
    raise ValueError(f"axis must be None, 0, 1 or 'entries' (got {axis!r})")


DEVICE_HASHES = {"keccak256": _ffi.GPUPOLY_HASH_KECCAK256, "keccak_256": _ffi.GPUPOLY_HASH_KECCAK256, "sha3_256": _ffi.GPUPOLY_HASH_SHA3_256}


class IndexedTags:
    """The tags prefix || encoding(first + t), t < count, of the reference's indexed loops: the index as 8 little-endian
    bytes (`b"wee25_w_block_" || idx.to_le_bytes()`, src/commit/wee25.rs:687-703) or, with `decimal`, in ASCII decimal
    (`format!("ggh15_lut_v_idx_{}_{}", lut_id, idx)`, src/lookup/ggh15/pubkey_gpu.rs:398-401).  A sequence of the literal
    tags - len, iteration, indexing, slicing (a slice of step 1 is an IndexedTags again) - which the device-side hash
    entries take as it is: the tags are then generated on the device (GPUPOLY_TAGS_INDEXED_*), prefix at most 64 bytes."""

    __slots__ = ("prefix", "first", "count", "decimal")

    def __init__(self, prefix: bytes, first: int, count: int, decimal: bool = False):
        prefix, first, count = bytes(prefix), int(first), int(count)
        if first < 0 or count < 0 or (count and first + count - 1 >= 1 << 64):
            raise ValueError("IndexedTags: the indices must stay within 64 bits")
        self.prefix, self.first, self.count, self.decimal = prefix, first, count, bool(decimal)

    def __len__(self) -> int:
        return self.count

    def tag(self, t: int) -> bytes:
        idx = self.first + t
        return self.prefix + (str(idx).encode("ascii") if self.decimal else idx.to_bytes(8, "little"))

    def __iter__(self):
        return (self.tag(t) for t in range(self.count))

    def __getitem__(self, item):
        if isinstance(item, slice):
            lo, hi, step = item.indices(self.count)
            if step == 1:
                return IndexedTags(self.prefix, self.first + lo, max(hi - lo, 0), self.decimal)
            return [self.tag(t) for t in range(lo, hi, step)]
        t = item + self.count if item < 0 else item
        if not 0 <= t < self.count:
            raise IndexError("IndexedTags index out of range")
        return self.tag(t)

    def __repr__(self):
        return f"IndexedTags({self.prefix!r}, {self.first}, {self.count}, decimal={self.decimal})"


def hash_tags_arg(key: bytes, tags, hash_name: str = "keccak256"):
    """(GpuHashTags, the buffers it points into, number of tags) for `tags`: an IndexedTags whose prefix fits goes in an
    indexed form, anything else as a table of its literal tags."""
    if hash_name not in DEVICE_HASHES:
        raise ValueError(f"no device-side hash {hash_name!r}")
    key = bytes(key)
    assert len(key) == 32
    arg = _ffi.GpuHashTags()
    arg.hash = DEVICE_HASHES[hash_name]
    arg.key[:] = key
    if isinstance(tags, IndexedTags) and len(tags.prefix) <= 64:
        buf = C.create_string_buffer(tags.prefix, max(len(tags.prefix), 1))
        arg.form = _ffi.GPUPOLY_TAGS_INDEXED_DECIMAL if tags.decimal else _ffi.GPUPOLY_TAGS_INDEXED_LE64
        arg.tags = C.cast(buf, C.c_void_p)
        arg.tag_offsets = None
        arg.prefix_len, arg.first_index = len(tags.prefix), tags.first
        return arg, (buf,), len(tags)
    literal = [bytes(t) for t in tags]
    offsets = (C.c_size_t * (len(literal) + 1))()
    at = 0
    for t, tag in enumerate(literal):
        at += len(tag)
        offsets[t + 1] = at
    packed = b"".join(literal)
    buf = C.create_string_buffer(packed, max(len(packed), 1))
    arg.form = _ffi.GPUPOLY_TAGS_TABLE
    arg.tags = C.cast(buf, C.c_void_p)
    arg.tag_offsets = offsets
    return arg, (buf, offsets), len(literal)


def device_hash_seeds(params, key: bytes, tags, hash_name: str = "keccak256") -> list:
    """[hash_seed_for_matrix(key, tag, hash_name) for tag in tags], hashed on the device (gpupoly_hash_seeds)."""
    arg, keep, count = hash_tags_arg(key, tags, hash_name)
    if count == 0:
        return []
    seeds = (GpuRngSeed * count)()
    check_status(_ffi.lib().gpupoly_hash_seeds(params.ctx().raw, C.byref(arg), count, seeds), "gpupoly_hash_seeds")
    del keep
    out = []
    for s in seeds:  # copies: the array's elements are views of its memory
        c = GpuRngSeed()
        c.words[:] = s.words[:]
        out.append(c)
    return out


class GpuDCRTPolyMatrix:
    __slots__ = ("params", "nrow", "ncol", "level", "is_ntt", "raw", "_finalizer", "_parent", "_version", "__weakref__")

    # ------------------------------------------------------------------ construction
    def __init__(self, params: GpuDCRTPolyParams, nrow: int, ncol: int, level: int, is_ntt: bool):
        """`new_empty_with_state` (gpu_dcrt_poly.rs:222-256): contents undefined."""
        if not (0 <= level < params.crt_depth()):
            raise AssertionError("invalid level for matrix create")
        raw = C.c_void_p()
        fmt = GPU_POLY_FORMAT_EVAL if is_ntt else GPU_POLY_FORMAT_COEFF
        st = _ffi.lib().gpu_matrix_create(params.ctx_raw(), level, nrow, ncol, fmt, C.byref(raw))
        check_status(st, f"gpu_matrix_create(nrow={nrow}, ncol={ncol}, level={level}, format={fmt})")
        self.params = params
        self.nrow = nrow
        self.ncol = ncol
        self.level = level
        self.is_ntt = is_ntt
        self.raw = raw
        self._parent = None  # set on row views: the matrix whose storage this one shares
        self._version = 0  # bumped by every in-place write (and on the parent of a view): keys caches derived from the contents
        self._finalizer = weakref.finalize(self, _ffi.lib().gpu_matrix_destroy, raw)

    @property
    def layout(self) -> str:
        """How the device stores the residues now (gpupoly_matrix_layout): "words", or "packed24" - 3 bytes per residue,
        what a uniform sample of a context whose moduli are all below 2^24 starts as until an operation without a
        packed path unpacks it (once).  Results never depend on it."""
        out = C.c_int(-1)
        check_status(_ffi.lib().gpupoly_matrix_layout(self.raw, C.byref(out)), "gpupoly_matrix_layout")
        return "packed24" if out.value == 1 else "words"

    @classmethod
    def new_empty(cls, params, nrow, ncol) -> "GpuDCRTPolyMatrix":
        return cls(params, nrow, ncol, params.crt_depth() - 1, True)

    @classmethod
    def zero(cls, params, nrow, ncol) -> "GpuDCRTPolyMatrix":
        return cls._new_zero_with_state(params, nrow, ncol, params.crt_depth() - 1, True)

    new_zero = zero  # gpu_dcrt_poly.rs:367-370

    @classmethod
    def _new_zero_with_state(cls, params, nrow, ncol, level, is_ntt) -> "GpuDCRTPolyMatrix":
        out = cls(params, nrow, ncol, level, is_ntt)
        if nrow == 0 or ncol == 0:
            return out
        # the reference uploads a host vector of zeros (gpu_dcrt_poly.rs:343-365); one device memset here
        check_status(_ffi.lib().gpupoly_matrix_fill_zero(out.raw), "gpupoly_matrix_fill_zero")
        return out

    @classmethod
    def from_rns(cls, params, data: np.ndarray, eval_format: bool) -> "GpuDCRTPolyMatrix":
        """Upload wire-layout residues (rows, cols, L, n)."""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        rows, cols, L, n = data.shape
        if n != params.ring_dimension():
            raise ValueError("ring dimension mismatch")
        out = cls(params, rows, cols, L - 1, eval_format)
        out.load_rns(data, eval_format)
        return out

    @classmethod
    def from_coeff_words(cls, params, words: np.ndarray, eval_format: bool = True, level=None) -> "GpuDCRTPolyMatrix":
        """Extension: big-integer coefficients as little-endian 64-bit words, shape (nrow, ncol, k, wpc) with
        k <= ring dimension (missing coefficients are 0), reduced mod every limb on the device
        (gpupoly_matrix_load_coeff_words; any value of wpc words, not only those below Q).  EVAL unless eval_format is
        false; at `level` (full level by default)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim != 4:
            raise ValueError("from_coeff_words: words must have shape (nrow, ncol, k, words_per_coeff)")
        nrow, ncol = words.shape[:2]
        out = cls(params, nrow, ncol, params.crt_depth() - 1 if level is None else level, eval_format)
        out.load_coeff_words(words, eval_format)
        return out

    @classmethod
    def from_coeffs(cls, params, rows, eval_format: bool = True) -> "GpuDCRTPolyMatrix":
        """The inverse of coeffs(): rows[r][c] is a sequence of at most ring-dimension non-negative python ints (shorter
        ones are padded with zeros; values at or above Q are reduced), the result is at full level, EVAL unless
        eval_format is false.  The ints become 64-bit words in one pass over a bytes buffer and the device reduces them
        mod every limb (from_coeff_words): no big-integer arithmetic on the host."""
        nrow = len(rows)
        ncol = len(rows[0]) if nrow else 0
        if nrow == 0 or ncol == 0:
            return cls.new_empty(params, nrow, ncol)
        polys = []
        for row in rows:
            assert len(row) == ncol, "row length mismatch in from_coeffs"
            polys.extend(row)
        k = max(len(poly) for poly in polys)
        assert k <= params.ring_dimension(), "more coefficients than the ring dimension"
        flat = []
        for poly in polys:
            flat.extend(map(int, poly))
            flat.extend([0] * (k - len(poly)))
        if flat and min(flat) < 0:
            raise ValueError("from_coeffs: negative coefficient (coefficients are unsigned)")
        wpc = max(1, -(-max(flat, default=0).bit_length() // 64))
        if wpc == 1:
            words = np.array(flat, dtype=np.uint64)
        else:
            step = 8 * wpc
            words = np.frombuffer(b"".join([c.to_bytes(step, "little") for c in flat]), dtype=np.uint64)
        return cls.from_coeff_words(params, words.reshape(nrow, ncol, k, wpc), eval_format)

    @classmethod
    def from_cpu_matrix(cls, params, coeff_residues: np.ndarray) -> "GpuDCRTPolyMatrix":
        """`from_cpu_matrix` (gpu_dcrt_poly.rs:769-817): CPU matrices travel as EVAL residues."""
        return cls.from_rns(params, coeff_residues, True)

    @classmethod
    def identity(cls, params, size, scalar=None) -> "GpuDCRTPolyMatrix":
        """`identity` (gpu_dcrt_poly.rs:1158-1188); built on the device (gpupoly_matrix_fill_identity)."""
        out = cls.new_empty(params, size, size)
        if size == 0:
            return out
        s_raw = None
        if scalar is not None:
            sm = scalar.inner if hasattr(scalar, "inner") else scalar
            sm = sm.ensure_eval()
            s_raw = sm.raw
        check_status(_ffi.lib().gpupoly_matrix_fill_identity(out.raw, s_raw), "gpupoly_matrix_fill_identity")
        return out

    @classmethod
    def gadget_matrix(cls, params, size) -> "GpuDCRTPolyMatrix":
        if size == 0:
            return cls.zero(params, 0, 0)
        out = cls.new_empty(params, size, size * params.modulus_digits())
        check_status(_ffi.lib().gpu_matrix_fill_gadget(out.raw, params.base_bits()), "gpu_matrix_fill_gadget")
        out.is_ntt = True
        return out

    @classmethod
    def small_gadget_matrix(cls, params, size) -> "GpuDCRTPolyMatrix":
        if size == 0:
            return cls.zero(params, 0, 0)
        k = -(-params.crt_bits() // params.base_bits())
        out = cls.new_empty(params, size, size * k)
        check_status(_ffi.lib().gpu_matrix_fill_small_gadget(out.raw, params.base_bits()), "gpu_matrix_fill_small_gadget")
        out.is_ntt = True
        return out

    # ------------------------------------------------------------------ host transfer
    def _bytes_per_poly(self) -> int:
        return (self.level + 1) * self.params.ring_dimension() * 8

    def _touch(self) -> None:
        """contents (or the format tag) are about to change in place: anything cached from them is stale"""
        m = self
        while m is not None:
            m._version += 1
            m = m._parent

    def content_version(self) -> int:
        """changes whenever this object's storage was rewritten in place through the host mirror (own writes and writes
        through row views); caches derived from the contents key on (object, content_version())"""
        return self._version

    def load_rns(self, data: np.ndarray, eval_format: bool) -> None:
        """`load_rns_bytes` (gpu_dcrt_poly.rs:629-663)."""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        if data.size == 0:
            self.is_ntt = eval_format
            return
        if data.size != self.nrow * self.ncol * (self.level + 1) * self.params.ring_dimension():
            raise ValueError("load_rns: size mismatch")
        events = C.c_void_p()
        fmt = GPU_POLY_FORMAT_EVAL if eval_format else GPU_POLY_FORMAT_COEFF
        self._touch()
        st = _ffi.lib().gpu_matrix_load_rns_batch(self.raw, data.ctypes.data, self._bytes_per_poly(), fmt, C.byref(events))
        check_status(st, "gpu_matrix_load_rns_batch")
        _ffi.wait_and_destroy_events(events)
        self.is_ntt = eval_format

    def load_coeff_words(self, words: np.ndarray, eval_format: bool = True) -> None:
        """Overwrite this matrix with the coefficients `words` spells, shape (nrow, ncol, k, wpc) (from_coeff_words):
        one call of gpupoly_matrix_load_coeff_words at this matrix's level."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim != 4 or words.shape[:2] != (self.nrow, self.ncol):
            raise ValueError("load_coeff_words: words must have shape (nrow, ncol, k, words_per_coeff)")
        k, wpc = words.shape[2:]
        fmt = GPU_POLY_FORMAT_EVAL if eval_format else GPU_POLY_FORMAT_COEFF
        self._touch()
        ptr = words.ctypes.data_as(C.POINTER(C.c_uint64)) if words.size else None
        st = _ffi.lib().gpupoly_matrix_load_coeff_words(self.raw, ptr, wpc, k, fmt)
        check_status(st, "gpupoly_matrix_load_coeff_words")
        self.is_ntt = eval_format

    def to_rns(self) -> np.ndarray:
        """`store_rns_bytes` in the current format (gpu_dcrt_poly.rs:576-596)."""
        n = self.params.ring_dimension()
        out = np.empty((self.nrow, self.ncol, self.level + 1, n), dtype=np.uint64)  # every word is written below
        if out.size == 0:
            return out
        events = C.c_void_p()
        fmt = GPU_POLY_FORMAT_EVAL if self.is_ntt else GPU_POLY_FORMAT_COEFF
        st = _ffi.lib().gpu_matrix_store_rns_batch(self.raw, out.ctypes.data, self._bytes_per_poly(), fmt, C.byref(events))
        check_status(st, "gpu_matrix_store_rns_batch")
        _ffi.wait_and_destroy_events(events)
        return out

    # ---- the reference's byte-slice forms of the same transfers (gpu_dcrt_poly.rs:576-596,629-711) ----------------
    def bytes_per_poly(self) -> int:
        return self._bytes_per_poly()

    def load_rns_bytes(self, data, bytes_per_poly: int, fmt: int) -> None:
        """`load_rns_bytes(bytes, bytes_per_poly, format)`: polynomials `bytes_per_poly` apart, retagged to `fmt`."""
        if len(data) == 0 or bytes_per_poly == 0:
            return
        buf = np.frombuffer(data, dtype=np.uint8)
        assert len(buf) >= self.nrow * self.ncol * bytes_per_poly, "load_rns_bytes: buffer too small"
        events = C.c_void_p()
        self._touch()
        st = _ffi.lib().gpu_matrix_load_rns_batch(self.raw, buf.ctypes.data, bytes_per_poly, fmt, C.byref(events))
        check_status(
            st,
            f"gpu_matrix_load_rns_batch(nrow={self.nrow}, ncol={self.ncol}, level={self.level}, current_ntt={self.is_ntt}, "
            f"format={fmt}, bytes={len(buf)}, bytes_per_poly={bytes_per_poly}, ring_dim={self.params.ring_dimension()}, "
            f"crt_depth={self.params.crt_depth()})",
        )
        _ffi.wait_and_destroy_events(events)
        self.is_ntt = fmt == GPU_POLY_FORMAT_EVAL

    def store_rns_bytes(self, bytes_out, bytes_per_poly: int, fmt: int) -> None:
        """`store_rns_bytes(bytes_out, bytes_per_poly, format)` into a writable buffer (bytearray / numpy uint8);
        `fmt` must be the matrix's current format (the library refuses a conversion, MatrixSerde.cu:765-768)."""
        if len(bytes_out) == 0 or bytes_per_poly == 0:
            return
        buf = np.frombuffer(bytes_out, dtype=np.uint8)
        assert buf.flags.writeable, "store_rns_bytes needs a writable buffer"
        assert len(buf) >= self.nrow * self.ncol * bytes_per_poly, "store_rns_bytes: buffer too small"
        events = C.c_void_p()
        st = _ffi.lib().gpu_matrix_store_rns_batch(self.raw, buf.ctypes.data, bytes_per_poly, fmt, C.byref(events))
        check_status(st, "gpu_matrix_store_rns_batch")
        _ffi.wait_and_destroy_events(events)

    def to_rns_snapshot(self) -> "GpuDCRTMatrixRnsSnapshot":
        bpp = rns_bytes_len_for_level(self.params, self.level)
        data = bytearray(self.nrow * self.ncol * bpp)
        self.store_rns_bytes(data, bpp, GPU_POLY_FORMAT_EVAL if self.is_ntt else GPU_POLY_FORMAT_COEFF)
        return GpuDCRTMatrixRnsSnapshot(self.nrow, self.ncol, self.level, self.is_ntt, bpp, data)

    @classmethod
    def from_rns_snapshot(cls, params, snapshot: "GpuDCRTMatrixRnsSnapshot") -> "GpuDCRTPolyMatrix":
        snapshot.validate_for_params(params)
        out = cls(params, snapshot.nrow(), snapshot.ncol(), snapshot.level(), snapshot.is_ntt())
        if snapshot.bytes():
            out.load_rns_bytes(snapshot.bytes(), snapshot.bytes_per_poly(),
                               GPU_POLY_FORMAT_EVAL if snapshot.is_ntt() else GPU_POLY_FORMAT_COEFF)
        return out

    def load_rns_snapshot(self, snapshot: "GpuDCRTMatrixRnsSnapshot") -> None:
        snapshot.validate_for_params(self.params)
        assert self.nrow == snapshot.nrow(), "RNS snapshot row count mismatch"
        assert self.ncol == snapshot.ncol(), "RNS snapshot column count mismatch"
        assert self.level == snapshot.level(), "RNS snapshot level mismatch"
        assert self.is_ntt == snapshot.is_ntt(), "RNS snapshot format mismatch"
        if not snapshot.bytes():
            return
        self.load_rns_bytes(snapshot.bytes(), snapshot.bytes_per_poly(),
                            GPU_POLY_FORMAT_EVAL if snapshot.is_ntt() else GPU_POLY_FORMAT_COEFF)

    def to_cpu_matrix(self) -> np.ndarray:
        """`to_cpu_matrix` (gpu_dcrt_poly.rs:722-767): the CPU side receives EVAL residues, (rows, cols, L, n) u64."""
        return self.to_eval_rns()

    @classmethod
    def read_from_files(cls, params, nrow: int, ncol: int, dir_path, ident: str) -> "GpuDCRTPolyMatrix":
        """`read_from_files` (gpu_dcrt_poly.rs:1594-1641): blocks of `BLOCK_SIZE` x `BLOCK_SIZE` entries, one file
        `{id}_{bsize}_{r0}.{r1}_{c0}.{c1}.matrix` each, holding bincode(Vec<Vec<Vec<u8>>>) of EVAL wire bytes per entry;
        short or missing entries are zero-padded, as there."""
        bsize = min(block_size(), max(nrow, 1), max(ncol, 1))
        out = cls.new_empty(params, nrow, ncol)
        bpp = rns_bytes_len(params)
        rows_off, cols_off = block_offsets(range(0, nrow), bsize), block_offsets(range(0, ncol), bsize)
        for r0, r1 in zip(rows_off, rows_off[1:]):
            for c0, c1 in zip(cols_off, cols_off[1:]):
                path = os.path.join(os.fspath(dir_path), f"{ident}_{bsize}_{r0}.{r1}_{c0}.{c1}.matrix")
                try:
                    with open(path, "rb") as fh:
                        entries = _bincode_read_nested_bytes(fh.read())
                except OSError as e:
                    raise RuntimeError(f"Failed to read matrix file {path!r}") from e
                rl, cl = r1 - r0, c1 - c0
                flat = bytearray(rl * cl * bpp)
                for i in range(rl):
                    for j in range(cl):
                        if i < len(entries) and j < len(entries[i]):
                            src = entries[i][j][:bpp]
                            start = (i * cl + j) * bpp
                            flat[start : start + len(src)] = src
                block = cls.new_empty(params, rl, cl)
                block.load_rns_bytes(flat, bpp, GPU_POLY_FORMAT_EVAL)
                out.copy_block_from(block, r0, c0, 0, 0, rl, cl)
        return out

    def to_coeff_rns(self) -> np.ndarray:
        return self.ensure_coeff().to_rns()

    def to_eval_rns(self) -> np.ndarray:
        return self.ensure_eval().to_rns()

    def store_const_coeff_words(self) -> np.ndarray:
        """`store_const_coeff_words` (gpu_dcrt_poly.rs:598-627); COEFF format required."""
        L = self.level + 1
        out = np.zeros((self.nrow, self.ncol, L), dtype=np.uint64)
        if out.size == 0:
            return out
        events = C.c_void_p()
        st = _ffi.lib().gpu_matrix_store_const_coeff_batch(self.raw, out.ctypes.data, L, C.byref(events))
        check_status(st, "gpu_matrix_store_const_coeff_batch")
        _ffi.wait_and_destroy_events(events)
        return out

    def coeffs(self) -> list:
        """CRT-reconstructed coefficients as python ints in [0, Q_level), [row][col][i] (gpu.rs:959-994).  The device
        rebuilds every coefficient as little-endian 64-bit words (gpupoly_matrix_store_coeff_words, the matrix left as
        it is); the host makes one int per coefficient from its words, in one pass over the buffer."""
        n = self.params.ring_dimension()
        if self.nrow == 0 or self.ncol == 0:
            return [[] for _ in range(self.nrow)]
        Q = 1
        for q in self.params.moduli()[: self.level + 1]:
            Q *= q
        wpc = -(-Q.bit_length() // 64)
        words = np.empty((self.nrow, self.ncol, n, wpc), dtype=np.uint64)
        st = _ffi.lib().gpupoly_matrix_store_coeff_words(self.raw, words.ctypes.data_as(C.POINTER(C.c_uint64)), wpc)
        check_status(st, "gpupoly_matrix_store_coeff_words")
        if wpc == 1:
            return words[..., 0].tolist()
        mv, step = memoryview(words).cast("B"), 8 * wpc
        flat = [int.from_bytes(mv[i : i + step], "little") for i in range(0, len(mv), step)]
        return [[flat[(r * self.ncol + c) * n : (r * self.ncol + c + 1) * n] for c in range(self.ncol)] for r in range(self.nrow)]

    def _coeffs_host(self) -> list:
        """coeffs() as a host CRT over the residues: the form before the device store (kept for comparison)."""
        res = self.to_coeff_rns()
        moduli = self.params.moduli()[: self.level + 1]
        Q = 1
        for q in moduli:
            Q *= q
        weights = []
        for q in moduli:
            Qi = Q // q
            weights.append(Qi * pow(Qi, -1, q))
        out = []
        for r in range(self.nrow):
            row = []
            for c in range(self.ncol):
                vals = [0] * res.shape[-1]
                for l, w in enumerate(weights):
                    limb = res[r, c, l]
                    for i in range(len(vals)):
                        vals[i] += int(limb[i]) * w
                row.append([v % Q for v in vals])
            out.append(row)
        return out

    def centered_max_abs(self, axis=None):
        """Exact centred infinity norm: max |x| over the coefficients x of an entry, each taken in
        (-Q_level/2, Q_level/2] (= min(v, Q_level - v) for v in [0, Q_level)), Q_level the product of the matrix's own
        limbs.  One device call (gpupoly_matrix_centered_max_abs, the matrix left as it is) replaces coeffs() and a host
        pass.  axis=None: an int over the whole matrix; axis=1: a list per row; axis=0: a list per column;
        axis="entries": the [row][col] nested list.  Empty rows / columns contribute 0."""
        return _max_along(self._centered_max_abs_entries(), axis, self.nrow, self.ncol)

    def _centered_max_abs_entries(self) -> list:
        if self.nrow == 0 or self.ncol == 0:
            return [[] for _ in range(self.nrow)]
        Q = 1
        for q in self.params.moduli()[: self.level + 1]:
            Q *= q
        wpv = -(-Q.bit_length() // 64)
        words = np.empty((self.nrow, self.ncol, wpv), dtype=np.uint64)
        st = _ffi.lib().gpupoly_matrix_centered_max_abs(self.raw, words.ctypes.data_as(C.POINTER(C.c_uint64)), wpv)
        check_status(st, "gpupoly_matrix_centered_max_abs")
        if wpv == 1:
            return words[..., 0].tolist()
        mv, step = memoryview(words).cast("B"), 8 * wpv
        flat = [int.from_bytes(mv[i : i + step], "little") for i in range(0, len(mv), step)]
        return [flat[r * self.ncol : (r + 1) * self.ncol] for r in range(self.nrow)]

    def _centered_max_abs_host(self, axis=None):
        """centered_max_abs as the callers run it on the host: coeffs(), then min(v, Q - v) and a max (kept for
        comparison)."""
        Q = 1
        for q in self.params.moduli()[: self.level + 1]:
            Q *= q
        entries = [[max((min(v, Q - v) for v in poly), default=0) for poly in row] for row in self.coeffs()]
        return _max_along(entries, axis, self.nrow, self.ncol)

    # ------------------------------------------------------------------ bits and machine integers
    def _level_modulus(self) -> int:
        Q = 1
        for q in self.params.moduli()[: self.level + 1]:
            Q *= q
        return Q

    def extract_bits(self, lo: int, hi: int) -> np.ndarray:
        """A bool array (rows, cols, n): coefficient c in [0, Q_level) -> whether it lies in [lo, hi), or for lo > hi in
        the wrap-around set [lo, Q_level) u [0, hi) (|x| <= B in the centred representative: lo = Q_level - B,
        hi = B + 1).  0 <= lo, hi <= Q_level.  One device call (gpupoly_matrix_extract_bits, the matrix left as it is):
        no big integer is built on either side."""
        n = self.params.ring_dimension()
        Q = self._level_modulus()
        if not (0 <= lo <= Q and 0 <= hi <= Q):
            raise ValueError(f"extract_bits: bounds must lie in [0, Q_level] (got {lo}, {hi})")
        if self.nrow == 0 or self.ncol == 0:
            return np.zeros((self.nrow, self.ncol, n), dtype=bool)
        wpb = -(-Q.bit_length() // 64)
        bounds = np.array([[(b >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(wpb)] for b in (lo, hi)], dtype=np.uint64)
        bpp = -(-n // 8)
        out = np.empty((self.nrow, self.ncol, bpp), dtype=np.uint8)
        u64p = C.POINTER(C.c_uint64)
        st = _ffi.lib().gpupoly_matrix_extract_bits(self.raw, bounds[0].ctypes.data_as(u64p), bounds[1].ctypes.data_as(u64p), wpb,
                                                    out.ctypes.data_as(C.POINTER(C.c_uint8)), bpp)
        check_status(st, "gpupoly_matrix_extract_bits")
        return np.unpackbits(out, axis=-1, bitorder="little")[..., :n].astype(bool)

    def extract_bits_with_threshold(self) -> np.ndarray:
        """`extract_bits_with_threshold` (src/poly/dcrt/gpu.rs:1070-1081) of every entry: c in [quarter, 3 quarter),
        quarter = (Q_level // 2) >> 1."""
        quarter = (self._level_modulus() // 2) >> 1
        return self.extract_bits(quarter, 3 * quarter)

    def decode_bits(self) -> np.ndarray:
        """The boolean centred decode (decode_centered_masked_boolean_coeff, src/decoder/masked_high_bit.rs:31-35):
        floor((2 c + floor(Q/2)) / Q) mod 2 per coefficient, as a bool array (rows, cols, n).  For odd Q that is 1 exactly
        when ceil((Q + 1) / 4) <= c < ceil((3 Q + 1) / 4): 2 c + floor(Q/2) reaches Q at the first and 2 Q at the second."""
        Q = self._level_modulus()
        return self.extract_bits(-(-(Q + 1) // 4), -(-(3 * Q + 1) // 4))

    def coeffs_ints_misfits(self, dtype, coeffs_per_poly=None):
        """(array, misfit count, first misfit): the first coeffs_per_poly (default n) coefficients of every entry as a
        (rows, cols, coeffs_per_poly) array of np.uint32 / np.uint64 (c mod 2^b, c in [0, Q_level)) or np.int32 /
        np.int64 (the representative in (-Q_level/2, Q_level/2], two's complement); coefficients that do not fit are
        truncated and counted, `first` is the (row, col, k) of the first of them or None.  One device call
        (gpupoly_matrix_store_coeff_ints, the matrix left as it is)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint32), np.dtype(np.uint64), np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError(f"coeffs_ints: dtype must be uint32, uint64, int32 or int64 (got {dt})")
        n = self.params.ring_dimension()
        cpp = n if coeffs_per_poly is None else int(coeffs_per_poly)
        if not 0 <= cpp <= n:
            raise ValueError(f"coeffs_ints: coeffs_per_poly must lie in [0, {n}] (got {cpp})")
        out = np.zeros((self.nrow, self.ncol, cpp), dtype=dt)
        if out.size == 0:
            return out, 0, None
        count, first = C.c_uint64(0), C.c_uint64(0)
        st = _ffi.lib().gpupoly_matrix_store_coeff_ints(self.raw, C.c_void_p(out.ctypes.data), dt.itemsize, 1 if dt.kind == "i" else 0,
                                                        cpp, C.byref(count), C.byref(first))
        check_status(st, "gpupoly_matrix_store_coeff_ints")
        if count.value == 0:
            return out, 0, None
        poly, k = divmod(first.value, cpp)
        return out, count.value, (poly // self.ncol, poly % self.ncol, k)

    def coeffs_ints(self, dtype, coeffs_per_poly=None, strict=True) -> np.ndarray:
        """coeffs_ints_misfits' array.  strict: an OverflowError naming the first coefficient that does not fit the
        dtype; otherwise such coefficients are truncated (two's complement for the signed dtypes)."""
        out, count, first = self.coeffs_ints_misfits(dtype, coeffs_per_poly)
        if strict and count:
            raise OverflowError(f"coeffs_ints: {count} coefficient(s) do not fit {np.dtype(dtype).name}, the first at "
                                f"(row, col, k) = {first}")
        return out

    def const_coeffs_u64(self, strict=True) -> np.ndarray:
        """The constant coefficient of every entry as np.uint64, (rows, cols) (`const_coeff_u64`,
        src/poly/dcrt/gpu.rs:1103-1120, for a whole matrix in one call)."""
        return self.coeffs_ints(np.uint64, 1, strict)[..., 0]

    # ------------------------------------------------------------------ compact wire format
    def to_compact_bytes(self) -> bytes:
        """`into_compact_bytes` (gpu_dcrt_poly.rs:956-1002): bincode(standard) tuple
        (1u8, format u8, level u32, nrow usize, ncol usize, max_coeff_bits u16, bytes_per_coeff u16, payload)."""
        return self.clone().into_compact_bytes()

    def into_compact_bytes(self) -> bytes:
        """`into_compact_bytes` (gpu_dcrt_poly.rs:956-1002) as an immutable `bytes`: the framed payload of
        `into_compact_view`, copied once."""
        return bytes(self.into_compact_view())

    def into_compact_view(self) -> memoryview:
        """The same bytes WITHOUT a host copy: a memoryview of this thread's pinned staging buffer, valid until the thread's
        next `into_compact_view` / `into_compact_bytes` call - for a consumer that writes them out at once (a file, a
        socket).  The ABI call copies the payload device -> pinned host memory (PCIe rate; a pageable destination - what
        round 2's mirror handed over - goes through the runtime's bounce buffer and first-touch faults: 15.7 of that
        call's 20.6 ms at the M3A preimage).  The worst-case capacity the ABI wants (the Rust side's `vec![0u8; cap]`) is
        only reserved address space here: pinned memory is grown to the largest payload seen, and a payload that does
        not fit the current buffer is retried once with the exact size the first call reported."""
        fmt = GPU_POLY_FORMAT_EVAL if self.is_ntt else GPU_POLY_FORMAT_COEFF
        coeff_count = self.nrow * self.ncol * self.params.ring_dimension()
        bits_upper = sum(q.bit_length() for q in self.params.moduli()[: self.level + 1])
        cap = (coeff_count * bits_upper + 7) // 8
        head_room = 64  # the bincode header (6 varints) is written in front of the payload afterwards
        max_bits, bpc, plen = C.c_uint16(0), C.c_uint16(0), C.c_size_t(0)
        self._touch()  # an EVAL matrix is taken to the coefficient domain in place
        # first try: whatever this thread already holds (at least 1/8 of the worst case: Gaussian-sized entries need far less)
        want = min(max(cap, 1), max(_pinned_capacity() - head_room, (cap + 7) // 8, 1 << 16))
        for attempt in range(2):
            base = _pinned_buffer(head_room + want)
            st = _ffi.lib().gpu_matrix_store_compact_bytes(
                self.raw, C.c_void_p(base + head_room), want, C.byref(max_bits), C.byref(bpc), C.byref(plen)
            )
            if st != 0 and attempt == 0 and want < cap and "payload buffer too small" in _ffi.last_error_string():
                want = min(cap, plen.value if plen.value > want else cap)  # the library reports the length it needs
                continue
            break
        check_status(st, "gpu_matrix_store_compact_bytes")
        self.is_ntt = False  # the store converts in place (MatrixSerde.cu:1108-1118)
        header = b"".join(
            [
                bytes([1, fmt]),
                _bincode_varint(self.level),
                _bincode_varint(self.nrow),
                _bincode_varint(self.ncol),
                _bincode_varint(max_bits.value),
                _bincode_varint(bpc.value),
                _bincode_varint(plen.value),
            ]
        )
        start = head_room - len(header)
        C.memmove(base + start, header, len(header))
        total = len(header) + plen.value
        return memoryview((C.c_ubyte * total).from_address(base + start)).cast("B")

    def _compact_header(self, fmt, max_bits, bpc, plen) -> bytes:
        return b"".join([bytes([1, fmt]), _bincode_varint(self.level), _bincode_varint(self.nrow), _bincode_varint(self.ncol),
                         _bincode_varint(max_bits), _bincode_varint(bpc), _bincode_varint(plen)])

    @staticmethod
    def to_compact_bytes_many(mats) -> list:
        """`to_compact_bytes` of every matrix (the operands stay as they are), through ONE batched store per context."""
        return GpuDCRTPolyMatrix.into_compact_bytes_many([m.clone() for m in mats])

    @staticmethod
    def into_compact_bytes_many(mats) -> list:
        """[m.into_compact_bytes() for m in mats] - the same framed bytes per matrix - with the device work of all
        matrices of a context in ONE gpupoly_matrix_store_compact_bytes_many call (what `get_lookup_buffer`,
        src/storage/write.rs:724-793, does with a to_compact_bytes per matrix).  Every matrix ends in the coefficient
        domain, like after `into_compact_bytes`.  The payloads land in this thread's pinned staging buffer; a buffer
        that is too small is retried once with the total the first call reported."""
        mats = list(mats)
        out = [None] * len(mats)
        by_ctx = {}
        for j, m in enumerate(mats):
            by_ctx.setdefault(m.params.ctx_raw().value, []).append(j)
        for idx in by_ctx.values():
            n = len(idx)
            fmts = [GPU_POLY_FORMAT_EVAL if mats[j].is_ntt else GPU_POLY_FORMAT_COEFF for j in idx]
            cap = 0
            for j in idx:
                m = mats[j]
                bits_upper = sum(q.bit_length() for q in m.params.moduli()[: m.level + 1])
                cap += ((m.nrow * m.ncol * m.params.ring_dimension() * bits_upper + 7) // 8 + 7) // 8 * 8
                m._touch()  # an EVAL matrix is taken to the coefficient domain in place
            raws = (C.c_void_p * n)(*[mats[j].raw for j in idx])
            bits, bpcs = (C.c_uint16 * n)(), (C.c_uint16 * n)()
            offs, lens, total = (C.c_size_t * n)(), (C.c_size_t * n)(), C.c_size_t(0)
            want = min(max(cap, 1), max(_pinned_capacity(), (cap + 7) // 8, 1 << 16))
            for attempt in range(2):
                base = _pinned_buffer(want)
                st = _ffi.lib().gpupoly_matrix_store_compact_bytes_many(raws, n, C.c_void_p(base), want, bits, bpcs, offs, lens, C.byref(total))
                if st != 0 and attempt == 0 and want < cap and "payload buffer too small" in _ffi.last_error_string():
                    want = min(cap, total.value if total.value > want else cap)
                    continue
                break
            check_status(st, "gpupoly_matrix_store_compact_bytes_many")
            for k, j in enumerate(idx):
                mats[j].is_ntt = False
                out[j] = mats[j]._compact_header(fmts[k], bits[k], bpcs[k], lens[k]) + C.string_at(base + offs[k], lens[k])
        return out

    @classmethod
    def from_compact_bytes_many(cls, params, blobs) -> list:
        """[from_compact_bytes(params, b) for b in blobs] with the device work in ONE
        gpupoly_matrix_load_compact_bytes_many call.  Bytes after a frame are ignored, as `bincode::decode_from_slice`
        ignores them (gpu_dcrt_poly.rs:1004-1017): a slot of a lookup buffer is padded to the longest matrix."""
        blobs = list(blobs)
        n = len(blobs)
        if n == 0:
            return []
        outs, fmts, keep = [], [], []
        ptrs, lens, widths = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_uint16 * n)()
        for j, data in enumerate(blobs):
            version, fmt = data[0], data[1]
            assert version == 1, f"Unsupported compact matrix version: {version}"
            assert fmt in (GPU_POLY_FORMAT_COEFF, GPU_POLY_FORMAT_EVAL), f"Invalid compact matrix format tag: {fmt}"
            pos = 2
            level, pos = _bincode_read_varint(data, pos)
            nrow, pos = _bincode_read_varint(data, pos)
            ncol, pos = _bincode_read_varint(data, pos)
            max_bits, pos = _bincode_read_varint(data, pos)
            bpc, pos = _bincode_read_varint(data, pos)
            plen, pos = _bincode_read_varint(data, pos)
            assert pos + plen <= len(data), "truncated compact bytes"
            assert level < params.crt_depth(), f"invalid compact matrix level: {level}"
            assert bpc == (max_bits + 7) // 8, "compact bytes_per_coeff mismatch"
            payload = bytes(data[pos : pos + plen]) if plen else b"\0"
            keep.append(payload)  # the pointers below must outlive the call
            ptrs[j] = C.cast(C.c_char_p(payload), C.c_void_p)
            lens[j], widths[j] = plen, max_bits
            outs.append(cls(params, nrow, ncol, level, False))
            fmts.append(fmt)
        raws = (C.c_void_p * n)(*[m.raw for m in outs])
        st = _ffi.lib().gpupoly_matrix_load_compact_bytes_many(raws, n, ptrs, lens, widths)
        check_status(st, "gpupoly_matrix_load_compact_bytes_many")
        for m, fmt in zip(outs, fmts):
            m.is_ntt = False
            if fmt == GPU_POLY_FORMAT_EVAL:
                m.ntt_all_in_place()
        return outs

    @classmethod
    def zero_compact_bytes(cls, params, nrow, ncol, level, is_ntt, max_coeff_bits) -> bytes:
        """Compact bytes of a zero matrix without touching the device (gpu_dcrt_poly.rs:1681-1710)."""
        assert level < params.crt_depth(), "invalid level for compact zero matrix"
        max_coeff_bits = max(int(max_coeff_bits), 1)
        bytes_per_coeff = -(-max_coeff_bits // 8)
        coeff_count = nrow * ncol * params.ring_dimension()
        payload_len = -(-coeff_count * max_coeff_bits // 8)
        fmt = GPU_POLY_FORMAT_EVAL if is_ntt else GPU_POLY_FORMAT_COEFF
        header = b"".join([bytes([1, fmt]), _bincode_varint(level), _bincode_varint(nrow), _bincode_varint(ncol),
                           _bincode_varint(max_coeff_bits), _bincode_varint(bytes_per_coeff), _bincode_varint(payload_len)])
        return header + bytes(payload_len)

    @classmethod
    def from_poly_vec(cls, params, rows) -> "GpuDCRTPolyMatrix":
        """`from_poly_vec` (gpu_dcrt_poly.rs:1092-1115): entries are transformed to EVAL and copied in."""
        if not rows:
            return cls.new_empty(params, 0, 0)
        nrow, ncol = len(rows), len(rows[0])
        if ncol == 0:
            return cls.new_empty(params, nrow, 0)
        first = rows[0][0].inner if hasattr(rows[0][0], "inner") else rows[0][0]
        out = cls(params, nrow, ncol, first.level, True)
        for i, row in enumerate(rows):
            assert len(row) == ncol, "row length mismatch in from_poly_vec"
            for j, poly in enumerate(row):
                m = poly.inner if hasattr(poly, "inner") else poly
                assert m.params == params, "params mismatch in from_poly_vec entry"
                assert m.level == first.level, "level mismatch in from_poly_vec entry"
                out.copy_block_from(m.ensure_eval(), i, j, 0, 0, 1, 1)
        return out

    def modulus_switch(self, new_modulus: int) -> "GpuDCRTPolyMatrix":
        """`modulus_switch` (gpu_dcrt_poly.rs:1352-1372): every coefficient c becomes floor(c * new_modulus / Q) mod
        new_modulus (src/element/finite_ring.rs:22-26), Q = params.modulus(); params are unchanged, the result is EVAL at
        full level.  One device call (gpupoly_matrix_scale_round); the host round trip of the reference where the entry
        reports "unsupported" (an input below full level, new_modulus >= 2^64 - 59) or new_modulus is not a 64-bit word."""
        out = self._scale_round(new_modulus, False)
        return out if out is not None else self._modulus_switch_host(new_modulus)

    def _modulus_switch_host(self, new_modulus: int) -> "GpuDCRTPolyMatrix":
        """modulus_switch as the reference runs it, coeffs() -> big-integer rescale -> from_coeffs -> from_poly_vec, the
        last two as one from_coeffs of the whole matrix."""
        Q = self.params.modulus()
        rows = [[[(c * new_modulus // Q) % new_modulus for c in poly] for poly in row] for row in self.coeffs()]
        return GpuDCRTPolyMatrix.from_coeffs(self.params, rows)

    def decode_centered(self, plaintext_modulus: int) -> "GpuDCRTPolyMatrix":
        """Extension: `decode_centered_masked_matrix` (src/decoder/masked_high_bit.rs:39-70) on the device - every
        coefficient c becomes floor((t c + floor(Q/2)) / Q) mod t, t = plaintext_modulus >= 2, Q = params.modulus(); the
        result is EVAL at full level, as from_biguints + set_entry give.  The host loop where the entry reports
        "unsupported" or t is not a 64-bit word."""
        assert plaintext_modulus > 1, "plaintext modulus must be at least two"
        out = self._scale_round(plaintext_modulus, True)
        return out if out is not None else self._decode_centered_host(plaintext_modulus)

    def _decode_centered_host(self, plaintext_modulus: int) -> "GpuDCRTPolyMatrix":
        """decode_centered as the reference runs it, coeffs -> big-integer rounding -> from_biguints -> set_entry, the
        last two as one from_coeffs of the whole matrix."""
        Q = self.params.modulus()
        half = Q // 2
        rows = [[[((plaintext_modulus * c + half) // Q) % plaintext_modulus for c in poly] for poly in row] for row in self.coeffs()]
        return GpuDCRTPolyMatrix.from_coeffs(self.params, rows)

    def _scale_round(self, t: int, round_half: bool):
        """gpupoly_matrix_scale_round into a new full-level matrix, brought to EVAL; None where the host path applies."""
        if self.nrow == 0 or self.ncol == 0 or not (1 <= t < 1 << 64):
            return None
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.params.crt_depth() - 1, False)
        st = _ffi.lib().gpupoly_matrix_scale_round(out.raw, self.raw, t, 1 if round_half else 0)
        if st != 0 and "unsupported" in _ffi.last_error_string():
            return None
        check_status(st, "gpupoly_matrix_scale_round")
        out.ntt_all_in_place()
        return out

    @staticmethod
    def _check_crt_levels(params, firsts, num_slots) -> int:
        """the reference's assertions on the level vectors (naive_vec.rs:2090-2099); returns the column count"""
        _, _, crt_depth = params.to_crt()
        assert len(firsts) == num_slots * crt_depth, "level vector count must equal num_slots * crt_depth"
        assert len(firsts) > 0, "CRT recomposition requires at least one level vector"
        output_cols = firsts[0].col_size()
        assert all(v.row_size() == 1 and v.col_size() == output_cols for v in firsts), \
            "CRT recomposition level vectors must be one-row matrices with a consistent column count"
        return output_cols

    @staticmethod
    def crt_recompose_rows(params, crt_values, num_slots) -> "GpuDCRTPolyMatrix":
        """`crt_recompose_rows` (src/noise_refresh/naive_vec.rs:2086-2118): crt_values[slot * crt_depth + i] is the 1 x c
        level vector of (slot, limb i); row `slot` of the num_slots x c result is sum_i decode_centered(level_i, q_i) *
        reconst_coeffs[i].  One device call (gpupoly_matrix_crt_recompose_rounded): limb i of the row is the decode of
        level i alone.  The reference's loop over the per-level calls where the entry reports "unsupported" (a level vector
        below full level).  EVAL at full level; the level vectors are left as they were."""
        crt_values = list(crt_values)
        return GpuDCRTPolyMatrix.crt_recompose_rows_terms(params, [[v] for v in crt_values], [1], num_slots)

    @staticmethod
    def crt_recompose_rows_terms(params, terms, signs, num_slots) -> "GpuDCRTPolyMatrix":
        """Extension: crt_recompose_rows of the levels sum_t signs[t] * terms[level][t] without forming them - terms[level]
        is a list of T <= 8 one-row matrices, signs[t] is +1 or -1 for every level (the online path's
        `input_term + refresh_term - one_term - decoder`, naive_vec.rs:1687, is T = 4 with signs (+, +, -, -)).  Terms in
        mixed domains are brought to EVAL on copies: the caller's matrices are never changed."""
        terms = [list(level) for level in terms]
        signs = [int(s) for s in signs]
        T = len(signs)
        assert 1 <= T <= 8, "1 to 8 terms per level"
        assert all(s in (1, -1) for s in signs), "signs are +1 or -1"
        assert all(len(level) == T for level in terms), "every level has one term per sign"
        flat = [m for level in terms for m in level]
        output_cols = GpuDCRTPolyMatrix._check_crt_levels(params, [level[0] for level in terms], num_slots)
        for m in flat:
            assert m.params == params, "CRT recomposition requires the level vectors' params"
            assert m.row_size() == 1 and m.col_size() == output_cols, "terms of a level share its shape"
        if len({m.is_ntt for m in flat}) > 1:
            flat = [m.ensure_eval() for m in flat]
        out = GpuDCRTPolyMatrix(params, num_slots, output_cols, params.crt_depth() - 1, True)
        tarr = (C.c_void_p * len(flat))(*[m.raw.value for m in flat])
        sarr = (C.c_int * T)(*signs)
        st = _ffi.lib().gpupoly_matrix_crt_recompose_rounded(out.raw, tarr, sarr, T, num_slots)
        if st != 0 and "unsupported" in _ffi.last_error_string():
            levels = []
            for j in range(len(terms)):
                acc = None
                for m, s in zip(flat[j * T:(j + 1) * T], signs):
                    acc = (m if s > 0 else -m) if acc is None else (acc + m if s > 0 else acc - m)
                levels.append(acc)
            return GpuDCRTPolyMatrix._crt_recompose_rows_loop(params, levels, num_slots)
        check_status(st, "gpupoly_matrix_crt_recompose_rounded")
        out.is_ntt = True
        return out

    @staticmethod
    def _crt_recompose_rows_loop(params, crt_values, num_slots) -> "GpuDCRTPolyMatrix":
        """crt_recompose_rows as the reference runs it (naive_vec.rs:2100-2117), over the per-level device calls: for every
        slot a zero row, for every limb decode_centered(level, q_i) * constant_poly(reconst_coeffs[i]) added in place, the
        rows concatenated."""
        from .poly import GpuDCRTPoly

        crt_values = list(crt_values)
        q_moduli, _, crt_depth = params.to_crt()
        output_cols = GpuDCRTPolyMatrix._check_crt_levels(params, crt_values, num_slots)
        reconst_coeffs = params.reconst_coeffs()
        rows = []
        for slot_idx in range(num_slots):
            row = GpuDCRTPolyMatrix.zero(params, 1, output_cols)
            for crt_idx in range(crt_depth):
                level = crt_values[slot_idx * crt_depth + crt_idx]
                rounded = level.decode_centered(q_moduli[crt_idx])
                row.add_in_place(rounded.mul_scalar(GpuDCRTPoly.from_biguint_to_constant(params, reconst_coeffs[crt_idx])))
            rows.append(row)
        return rows[0].concat_rows(rows[1:])

    # ---- the nested-RNS gadget (extension; NestedRnsContext in nested_rns.py sits on these) ----
    @staticmethod
    def _p_moduli_arg(p_moduli):
        ps = [int(p) for p in p_moduli]
        if any(not (0 <= p < 1 << 64) for p in ps):
            raise ValueError("p moduli must fit 64 bits")
        return (C.c_uint64 * max(1, len(ps)))(*ps), len(ps)

    def nested_rns_decompose(self, p_moduli, scale: int, level_offset: int, active_levels: int,
                             eval_format: bool = True) -> "GpuDCRTPolyMatrix":
        """`nested_rns_gadget_decomposed` (src/gadgets/arith/nested_rns/encoding.rs:273-338) of this matrix against the
        window [level_offset, level_offset + active_levels) of its limbs: rows * active_levels * (len(p_moduli) + 1) x
        cols, one device call (gpupoly_matrix_nested_rns_decompose).  This matrix is left as it was."""
        parr, D = self._p_moduli_arg(p_moduli)
        out = GpuDCRTPolyMatrix(self.params, self.nrow * active_levels * (D + 1), self.ncol, self.level, eval_format)
        fmt = GPU_POLY_FORMAT_EVAL if eval_format else GPU_POLY_FORMAT_COEFF
        st = _ffi.lib().gpupoly_matrix_nested_rns_decompose(out.raw, self.raw, parr, D, scale, level_offset, active_levels, fmt)
        check_status(st, "gpupoly_matrix_nested_rns_decompose")
        return out

    @classmethod
    def nested_rns_gadget_vector(cls, params, p_moduli, scale: int, level_offset: int, active_levels: int,
                                 eval_format: bool = True, level=None) -> "GpuDCRTPolyMatrix":
        """`nested_rns_gadget_vector` (encoding.rs:240-271): 1 x active_levels * (len(p_moduli) + 1), written on the device
        (gpupoly_matrix_fill_nested_rns_gadget)."""
        parr, D = cls._p_moduli_arg(p_moduli)
        out = cls(params, 1, active_levels * (D + 1), params.crt_depth() - 1 if level is None else level, eval_format)
        fmt = GPU_POLY_FORMAT_EVAL if eval_format else GPU_POLY_FORMAT_COEFF
        st = _ffi.lib().gpupoly_matrix_fill_nested_rns_gadget(out.raw, parr, D, scale, level_offset, active_levels, fmt)
        check_status(st, "gpupoly_matrix_fill_nested_rns_gadget")
        return out

    def nested_rns_residues(self, p_moduli, level_offset: int, active_levels: int) -> "GpuDCRTPolyMatrix":
        """Row (row * active_levels + a) * D + j holds, coefficient by coefficient, (residue in limb level_offset + a)
        mod p_j as a small integer in every limb (gpupoly_matrix_nested_rns_residues): the slot-wise form of
        `encode_nested_rns_poly_with_offset` (encoding.rs:401-420).  COEFF; this matrix is left as it was."""
        parr, D = self._p_moduli_arg(p_moduli)
        out = GpuDCRTPolyMatrix(self.params, self.nrow * active_levels * D, self.ncol, self.level, False)
        st = _ffi.lib().gpupoly_matrix_nested_rns_residues(out.raw, self.raw, parr, D, level_offset, active_levels)
        check_status(st, "gpupoly_matrix_nested_rns_residues")
        return out

    @classmethod
    def from_compact_bytes(cls, params, data: bytes) -> "GpuDCRTPolyMatrix":
        """gpu_dcrt_poly.rs:1004-1044."""
        version, fmt = data[0], data[1]
        assert version == 1, f"Unsupported compact matrix version: {version}"
        assert fmt in (GPU_POLY_FORMAT_COEFF, GPU_POLY_FORMAT_EVAL), f"Invalid compact matrix format tag: {fmt}"
        pos = 2
        level, pos = _bincode_read_varint(data, pos)
        nrow, pos = _bincode_read_varint(data, pos)
        ncol, pos = _bincode_read_varint(data, pos)
        max_bits, pos = _bincode_read_varint(data, pos)
        bpc, pos = _bincode_read_varint(data, pos)
        plen, pos = _bincode_read_varint(data, pos)
        payload = data[pos : pos + plen]
        assert len(payload) == plen and pos + plen == len(data), "truncated compact bytes"
        assert level < params.crt_depth(), f"invalid compact matrix level: {level}"
        assert bpc == (max_bits + 7) // 8, "compact bytes_per_coeff mismatch"
        out = cls(params, nrow, ncol, level, False)
        buf = C.cast(C.c_char_p(payload if plen else b"\0"), C.POINTER(C.c_uint8))  # no copy: the call is synchronous
        st = _ffi.lib().gpu_matrix_load_compact_bytes(out.raw, buf, plen, max_bits)
        check_status(st, "gpu_matrix_load_compact_bytes")
        out.is_ntt = False
        if fmt == GPU_POLY_FORMAT_EVAL:
            out.ntt_all_in_place()
        return out

    def to_cpu_staging_bytes(self) -> bytes:
        """RNS snapshot framing (gpu_dcrt_poly.rs:1046-1061): (1u8, nrow, ncol, level, is_ntt, bytes_per_poly, bytes)."""
        raw = memoryview(self.to_rns()).cast("B")  # joined below without an intermediate copy
        return b"".join(
            [
                bytes([1]),
                _bincode_varint(self.nrow),
                _bincode_varint(self.ncol),
                _bincode_varint(self.level),
                bytes([1 if self.is_ntt else 0]),
                _bincode_varint(self._bytes_per_poly()),
                _bincode_varint(len(raw)),
                raw,
            ]
        )

    into_cpu_staging_bytes = to_cpu_staging_bytes  # the consuming form (gpu_dcrt_poly.rs:1046)

    @classmethod
    def from_cpu_staging_bytes(cls, params, data: bytes) -> "GpuDCRTPolyMatrix":
        assert data[0] == 1, "Unsupported GPU matrix RNS staging version"
        pos = 1
        nrow, pos = _bincode_read_varint(data, pos)
        ncol, pos = _bincode_read_varint(data, pos)
        level, pos = _bincode_read_varint(data, pos)
        is_ntt = bool(data[pos])
        pos += 1
        bpp, pos = _bincode_read_varint(data, pos)
        blen, pos = _bincode_read_varint(data, pos)
        n = params.ring_dimension()
        assert bpp == (level + 1) * n * 8 and blen == nrow * ncol * bpp
        arr = np.frombuffer(data, dtype="<u8", count=blen // 8, offset=pos).reshape(nrow, ncol, level + 1, n)
        return cls.from_rns(params, arr, is_ntt)

    # ------------------------------------------------------------------ domain
    def ntt_all_in_place(self) -> None:
        if self.nrow == 0 or self.ncol == 0 or self.is_ntt:
            self.is_ntt = True
            return
        self._touch()
        check_status(_ffi.lib().gpu_matrix_ntt_all(self.raw), "gpu_matrix_ntt_all")
        self.is_ntt = True

    def intt_all_in_place(self) -> None:
        if self.nrow == 0 or self.ncol == 0 or not self.is_ntt:
            return
        self._touch()
        check_status(_ffi.lib().gpu_matrix_intt_all(self.raw), "gpu_matrix_intt_all")
        self.is_ntt = False

    def into_coeff_domain(self) -> "GpuDCRTPolyMatrix":
        self.intt_all_in_place()
        return self

    def ensure_coeff(self) -> "GpuDCRTPolyMatrix":
        if not self.is_ntt:
            return self
        return self.clone().into_coeff_domain()

    def ensure_eval(self) -> "GpuDCRTPolyMatrix":
        if self.is_ntt:
            return self
        out = self.clone()
        out.ntt_all_in_place()
        return out

    # ------------------------------------------------------------------ structure
    def clone(self) -> "GpuDCRTPolyMatrix":
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, self.is_ntt)
        if self.nrow and self.ncol:
            check_status(_ffi.lib().gpu_matrix_copy(out.raw, self.raw), "gpu_matrix_copy")
        return out

    def to_params(self, params) -> "GpuDCRTPolyMatrix":
        """Replica of this matrix in the context of `params` (another device's, usually): one peer copy over
        xGMI instead of the reference's `to_cpu_staging_bytes` -> `from_cpu_staging_bytes` host round trip
        (src/lookup/ggh15/pubkey_gpu.rs:153-196)."""
        if params.ctx_raw().value == self.params.ctx_raw().value:
            return self.clone()
        out = object.__new__(GpuDCRTPolyMatrix)
        raw = C.c_void_p()
        check_status(_ffi.lib().gpupoly_matrix_copy_to_context(params.ctx_raw(), self.raw, C.byref(raw)),
                     "gpupoly_matrix_copy_to_context")
        out.params, out.nrow, out.ncol, out.level, out.is_ntt, out.raw = params, self.nrow, self.ncol, self.level, self.is_ntt, raw
        out._parent, out._version = None, 0
        out._finalizer = weakref.finalize(out, _ffi.lib().gpu_matrix_destroy, raw)
        return out

    def size(self):
        return self.nrow, self.ncol

    def row_size(self) -> int:
        return self.nrow

    def col_size(self) -> int:
        return self.ncol

    def copy_block_from(self, src, dst_row, dst_col, src_row, src_col, rows, cols) -> None:
        if rows == 0 or cols == 0:
            return
        self._touch()
        st = _ffi.lib().gpu_matrix_copy_block(self.raw, src.raw, dst_row, dst_col, src_row, src_col, rows, cols)
        check_status(st, "gpu_matrix_copy_block")

    def add_block_from(self, src, dst_row, dst_col, src_row, src_col, rows, cols) -> None:
        assert self.params == src.params and self.level == src.level and self.is_ntt == src.is_ntt
        if rows == 0 or cols == 0:
            return
        self._touch()
        st = _ffi.lib().gpu_matrix_add_block(self.raw, src.raw, dst_row, dst_col, src_row, src_col, rows, cols)
        check_status(st, "gpu_matrix_add_block")
        self.is_ntt = src.is_ntt

    def add_rows_from(self, dst_row, lhs, rhs) -> None:
        """self[dst_row : dst_row + lhs.nrow] = lhs + rhs in one pass (gpupoly_matrix_add_rows)."""
        assert lhs.size() == rhs.size() and lhs.ncol == self.ncol and dst_row + lhs.nrow <= self.nrow
        if lhs.is_ntt != rhs.is_ntt:
            rhs = rhs.ensure_eval() if lhs.is_ntt else rhs.ensure_coeff()
        self._touch()
        check_status(_ffi.lib().gpupoly_matrix_add_rows(self.raw, dst_row, lhs.raw, rhs.raw), "gpupoly_matrix_add_rows")
        self.is_ntt = lhs.is_ntt

    def row_view(self, row_start, row_end) -> "GpuDCRTPolyMatrix":
        """Rows [row_start, row_end) as a matrix that shares this one's storage (gpupoly_matrix_row_view): an operand
        without the slice's copy.  The view keeps its parent alive; writes through either are seen by both."""
        assert 0 <= row_start <= row_end <= self.nrow
        raw = C.c_void_p()
        check_status(_ffi.lib().gpupoly_matrix_row_view(self.raw, row_start, row_end - row_start, C.byref(raw)), "gpupoly_matrix_row_view")
        v = object.__new__(GpuDCRTPolyMatrix)
        v.params, v.nrow, v.ncol, v.level, v.is_ntt, v.raw = self.params, row_end - row_start, self.ncol, self.level, self.is_ntt, raw
        v._parent = self
        v._version = 0
        v._finalizer = weakref.finalize(v, _ffi.lib().gpu_matrix_destroy, raw)
        return v

    def reshape_view(self, nrow, ncol) -> "GpuDCRTPolyMatrix":
        """The whole matrix as nrow x ncol (nrow * ncol polynomials, as here) over the same storage, entry (i, j) =
        polynomial i * ncol + j of the row-major order (gpupoly_matrix_reshape_view): no copy.  A row view in every
        other respect - it keeps its parent alive, writes through either are seen by both, and the overlap rule treats
        it as the parent's block.  Another polynomial count raises GpuPolyError."""
        raw = C.c_void_p()
        check_status(_ffi.lib().gpupoly_matrix_reshape_view(self.raw, nrow, ncol, C.byref(raw)), "gpupoly_matrix_reshape_view")
        v = object.__new__(GpuDCRTPolyMatrix)
        v.params, v.nrow, v.ncol, v.level, v.is_ntt, v.raw = self.params, nrow, ncol, self.level, self.is_ntt, raw
        v._parent = self
        v._version = 0
        v._finalizer = weakref.finalize(v, _ffi.lib().gpu_matrix_destroy, raw)
        return v

    def ntt_add_rows_from(self, dst_row, coeff, addend, consume: bool = False) -> None:
        """self[dst_row : dst_row + coeff.nrow] = NTT(coeff) + addend (gpupoly_matrix_ntt_add_rows): `coeff` holds
        coefficients, `addend` is EVAL; one pass where the fused kernel exists.  consume: the caller gives `coeff` up
        (do not use it afterwards) - where no fused kernel exists it is then transformed in place instead of copied."""
        assert coeff.size() == addend.size() and coeff.ncol == self.ncol and dst_row + coeff.nrow <= self.nrow
        assert not coeff.is_ntt, "ntt_add_rows_from takes a coefficient-domain matrix"
        addend = addend.ensure_eval()
        self._touch()
        st = _ffi.lib().gpupoly_matrix_ntt_add_rows(self.raw, dst_row, coeff.raw, addend.raw, 1 if consume else 0)
        check_status(st, "gpupoly_matrix_ntt_add_rows")
        self.is_ntt = True

    def slice(self, row_start, row_end, col_start, col_end) -> "GpuDCRTPolyMatrix":
        nrow, ncol = row_end - row_start, col_end - col_start
        out = GpuDCRTPolyMatrix(self.params, nrow, ncol, self.level, self.is_ntt)
        out.copy_block_from(self, 0, 0, row_start, col_start, nrow, ncol)
        return out

    def slice_rows(self, start, end):
        return self.slice(start, end, 0, self.ncol)

    def slice_columns(self, start, end):
        return self.slice(0, self.nrow, start, end)

    def entry(self, i, j):
        from .poly import GpuDCRTPoly

        return GpuDCRTPoly(self.slice(i, i + 1, j, j + 1))

    def set_entry(self, i, j, elem) -> None:
        src = elem.inner if hasattr(elem, "inner") else elem
        # convert domains first so the whole-matrix retag of copy_block stays harmless
        # (gpu_dcrt_poly.rs:1122-1132)
        src = src.ensure_eval() if self.is_ntt else src.ensure_coeff()
        self.copy_block_from(src, i, j, 0, 0, 1, 1)

    def get_row(self, i):
        return [self.entry(i, j) for j in range(self.ncol)]

    def get_column(self, j):
        return [self.entry(i, j) for i in range(self.nrow)]

    def transpose(self) -> "GpuDCRTPolyMatrix":
        """One launch (gpupoly_matrix_transpose); the reference loops nrow*ncol single-entry copy_block calls
        (gpu_dcrt_poly.rs:1190-1199)."""
        out = GpuDCRTPolyMatrix(self.params, self.ncol, self.nrow, self.level, self.is_ntt)
        if self.nrow and self.ncol:
            check_status(_ffi.lib().gpupoly_matrix_transpose(out.raw, self.raw), "gpupoly_matrix_transpose")
        return out

    def _same_domain(self, others):
        for o in others:
            assert o.params == self.params and o.level == self.level, "concat requires same params/level"
        return [o.ensure_eval() if self.is_ntt else o.ensure_coeff() for o in others]

    def concat_columns(self, others) -> "GpuDCRTPolyMatrix":
        others = self._same_domain(others)
        for o in others:
            assert o.nrow == self.nrow, "concat_columns requires same row count"
        ncol = self.ncol + sum(o.ncol for o in others)
        out = GpuDCRTPolyMatrix(self.params, self.nrow, ncol, self.level, self.is_ntt)
        off = 0
        for m in [self] + others:
            out.copy_block_from(m, 0, off, 0, 0, m.nrow, m.ncol)
            off += m.ncol
        out.is_ntt = self.is_ntt
        return out

    def concat_rows(self, others) -> "GpuDCRTPolyMatrix":
        others = self._same_domain(others)
        for o in others:
            assert o.ncol == self.ncol, "concat_rows requires same column count"
        nrow = self.nrow + sum(o.nrow for o in others)
        out = GpuDCRTPolyMatrix(self.params, nrow, self.ncol, self.level, self.is_ntt)
        off = 0
        for m in [self] + others:
            out.copy_block_from(m, off, 0, 0, 0, m.nrow, m.ncol)
            off += m.nrow
        out.is_ntt = self.is_ntt
        return out

    def concat_diag(self, others) -> "GpuDCRTPolyMatrix":
        others = self._same_domain(others)
        nrow = self.nrow + sum(o.nrow for o in others)
        ncol = self.ncol + sum(o.ncol for o in others)
        out = GpuDCRTPolyMatrix._new_zero_with_state(self.params, nrow, ncol, self.level, self.is_ntt)
        ro = co = 0
        for m in [self] + others:
            out.copy_block_from(m, ro, co, 0, 0, m.nrow, m.ncol)
            ro += m.nrow
            co += m.ncol
        out.is_ntt = self.is_ntt
        return out

    def tensor(self, other) -> "GpuDCRTPolyMatrix":
        """Kronecker product (gpu_dcrt_poly.rs:1225-1252: entry, mul_scalar, copy_block per entry there); one launch
        here.  As in the reference the blocks come out of mul_scalar, i.e. the result is EVAL."""
        assert self.params == other.params and self.level == other.level and self.is_ntt == other.is_ntt
        out = GpuDCRTPolyMatrix(self.params, self.nrow * other.nrow, self.ncol * other.ncol, self.level, self.is_ntt)
        if 0 in (self.nrow, self.ncol, other.nrow, other.ncol):
            return out
        lhs, rhs = self.ensure_eval(), other.ensure_eval()
        st = _ffi.lib().gpupoly_matrix_tensor(out.raw, lhs.raw, rhs.raw)
        check_status(st, "gpupoly_matrix_tensor")
        out.is_ntt = True
        return out

    def vectorize_columns(self) -> "GpuDCRTPolyMatrix":
        out = GpuDCRTPolyMatrix(self.params, self.nrow * self.ncol, 1, self.level, self.is_ntt)
        for j in range(self.ncol):
            out.copy_block_from(self, j * self.nrow, 0, 0, j, self.nrow, 1)
        return out

    # ------------------------------------------------------------------ arithmetic
    def _check_binop(self, rhs, what):
        assert self.params == rhs.params, f"{what} requires same params"
        assert self.level == rhs.level, f"{what} requires same level"
        assert self.is_ntt == rhs.is_ntt, f"{what} requires same domain"
        assert (self.nrow, self.ncol) == (rhs.nrow, rhs.ncol), f"{what} requires same dimensions"

    def add_in_place(self, rhs) -> None:
        self._check_binop(rhs, "add_in_place")
        if self.nrow == 0 or self.ncol == 0:
            return
        self._touch()
        check_status(_ffi.lib().gpu_matrix_add(self.raw, self.raw, rhs.raw), "gpu_matrix_add")
        self.is_ntt = rhs.is_ntt

    def sub_in_place(self, rhs) -> None:
        self._check_binop(rhs, "sub_in_place")
        if self.nrow == 0 or self.ncol == 0:
            return
        self._touch()
        check_status(_ffi.lib().gpu_matrix_sub(self.raw, self.raw, rhs.raw), "gpu_matrix_sub")
        self.is_ntt = rhs.is_ntt

    def _binop(self, rhs, fn, what):
        """out = self (+|-) rhs through the three-operand ABI call into a fresh matrix: three passes over memory.  The
        reference's `&a + &b` clones a and adds in place (gpu_dcrt_poly.rs:1731-1739): five passes."""
        self._check_binop(rhs, what)
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, self.is_ntt)
        if self.nrow == 0 or self.ncol == 0:
            return out
        check_status(fn(out.raw, self.raw, rhs.raw), what)
        out.is_ntt = rhs.is_ntt
        return out

    def __add__(self, rhs):
        return self._binop(rhs, _ffi.lib().gpu_matrix_add, "gpu_matrix_add")

    def __sub__(self, rhs):
        return self._binop(rhs, _ffi.lib().gpu_matrix_sub, "gpu_matrix_sub")

    def __neg__(self):
        """one pass (gpupoly_matrix_neg); the reference uploads zeros, clones and subtracts (gpu_dcrt_poly.rs:1890-1897)"""
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, self.is_ntt)
        if self.nrow == 0 or self.ncol == 0:
            return out
        check_status(_ffi.lib().gpupoly_matrix_neg(out.raw, self.raw), "gpupoly_matrix_neg")
        return out

    def mul_scalar(self, scalar) -> "GpuDCRTPolyMatrix":
        """`mul_scalar` (gpu_dcrt_poly.rs:1770-1790)."""
        s = scalar.inner if hasattr(scalar, "inner") else scalar
        lhs = self.ensure_eval()
        s = s.ensure_eval()
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, True)
        if self.nrow == 0 or self.ncol == 0:
            return out
        check_status(_ffi.lib().gpu_matrix_mul_scalar(out.raw, lhs.raw, s.raw), "gpu_matrix_mul_scalar")
        return out

    @classmethod
    def monomial(cls, params, nrow, ncol, shift, eval_format: bool = True, level=None) -> "GpuDCRTPolyMatrix":
        """Extension: every entry x^shift (shift mod 2N, x^N = -1), written on the device directly in the wanted form
        (gpupoly_matrix_fill_monomial): no one-hot host vector, no upload, no transform."""
        out = cls(params, nrow, ncol, params.crt_depth() - 1 if level is None else level, eval_format)
        fmt = GPU_POLY_FORMAT_EVAL if eval_format else GPU_POLY_FORMAT_COEFF
        shift = int(shift) % (2 * params.ring_dimension())
        check_status(_ffi.lib().gpupoly_matrix_fill_monomial(out.raw, shift, fmt), "gpupoly_matrix_fill_monomial")
        return out

    def mul_monomial(self, shift) -> "GpuDCRTPolyMatrix":
        """self * x^shift in one pass, in the domain self is in (gpupoly_matrix_mul_monomial): a twiddle-table look-up per
        slot in EVAL, a signed rotation in COEFF.  rotate_gate / monomial_scalar of the reference
        (src/circuit/poly_circuit/construction.rs:352-357) build the monomial on the host and multiply."""
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, self.is_ntt)
        shift = int(shift) % (2 * self.params.ring_dimension())
        check_status(_ffi.lib().gpupoly_matrix_mul_monomial(out.raw, self.raw, shift), "gpupoly_matrix_mul_monomial")
        return out

    @staticmethod
    def monomial_sum(mats, shifts, addend=None, negate: bool = False, out=None) -> "GpuDCRTPolyMatrix":
        """addend +- sum_j mats[j] * x^shifts[j] in ceil(n / 64) launches (gpupoly_matrix_monomial_sum): the slot-packing
        sums of collapse_slot_matrices (src/noise_refresh/naive_vec.rs:1983-1998) and the slot-transfer reduce steps
        (src/slot_transfer/bgg_poly_encoding.rs:362-380, src/slot_transfer/bgg_pubkey_gpu.rs:448-464).  All operands share
        one shape, level and domain, which the result takes.  `out`: write there (it may be `addend`: accumulate in place;
        never one of `mats`); a fresh matrix otherwise."""
        mats, shifts = list(mats), list(shifts)
        n = len(mats)
        assert len(shifts) == n, "monomial_sum: one shift per matrix"
        first = addend if addend is not None else (mats[0] if n else out)
        if first is None:
            raise ValueError("monomial_sum: no operand to take the shape from")
        for m in mats + ([addend] if addend is not None else []):
            first._check_binop(m, "monomial_sum")
        if out is None:
            out = GpuDCRTPolyMatrix(first.params, first.nrow, first.ncol, first.level, first.is_ntt)
        else:
            out._touch()
        two_n = 2 * first.params.ring_dimension()
        marr = (C.c_void_p * max(n, 1))(*[m.raw.value for m in mats])
        sarr = (C.c_uint64 * max(n, 1))(*[int(s) % two_n for s in shifts])
        st = _ffi.lib().gpupoly_matrix_monomial_sum(out.raw, None if addend is None else addend.raw, marr, sarr, n, 1 if negate else 0)
        check_status(st, "gpupoly_matrix_monomial_sum")
        if n or addend is not None:
            out.is_ntt = first.is_ntt
        return out

    @staticmethod
    def mul_sum(lhss, rhss, addend=None, negate: bool = False, out=None, dst_col: int = 0) -> "GpuDCRTPolyMatrix":
        """addend +- sum_t lhss[t] * rhss[t] in one call (gpupoly_matrix_mul_sum), written into columns
        [dst_col, dst_col + cols) of `out`: the `add_in_place(&(a * &b))` / `x - (a * &b)` chains and the chunk-by-chunk
        concatenation of src/lookup/ggh15/encoding.rs:205-298, src/lookup/ggh15/pubkey_gpu.rs:408,494-505 and
        src/lookup/lwe/encoding_gpu.rs:142-223.  All operands are in the NTT domain; lhss[t] is r x k_t, rhss[t] k_t x cols.
        `out` None: a fresh r x cols matrix (`addend`, if any, has that shape; dst_col = 0).  Otherwise `out` is r x C,
        `addend` None or r x C (it may be `out`: accumulate in place), and columns outside the block keep their contents."""
        lhss, rhss = list(lhss), list(rhss)
        n = len(lhss)
        assert len(rhss) == n, "mul_sum: one right operand per left operand"
        first = out if out is not None else (addend if addend is not None else (lhss[0] if n else None))
        if first is None:
            raise ValueError("mul_sum: no operand to take the shape from")
        cols = rhss[0].ncol if n else first.ncol - dst_col
        for l_, r_ in zip(lhss, rhss):
            assert l_.params == first.params and r_.params == first.params, "mul_sum requires same params"
            assert l_.level == first.level and r_.level == first.level, "mul_sum requires same level"
            assert l_.is_ntt and r_.is_ntt, "mul_sum requires NTT domain"
            assert l_.ncol == r_.nrow and l_.nrow == first.nrow and r_.ncol == cols, "mul_sum: term shape mismatch"
        if out is None:
            assert dst_col == 0, "mul_sum: dst_col needs an `out` to place the block in"
            out = GpuDCRTPolyMatrix(first.params, first.nrow, cols, first.level, True)
        else:
            out._touch()
        if addend is not None:
            assert addend.is_ntt and (addend.nrow, addend.ncol) == (out.nrow, out.ncol), "mul_sum: the addend has out's shape, NTT domain"
        larr = (C.c_void_p * max(n, 1))(*[m.raw.value for m in lhss])
        rarr = (C.c_void_p * max(n, 1))(*[m.raw.value for m in rhss])
        st = _ffi.lib().gpupoly_matrix_mul_sum(out.raw, dst_col, cols, None if addend is None else addend.raw, larr, rarr, n, 1 if negate else 0)
        check_status(st, "gpupoly_matrix_mul_sum")
        out.is_ntt = True
        return out

    def _mul_acc(self, lhs, rhs, negate: bool) -> None:
        assert self.params == lhs.params == rhs.params, "mul_acc requires same params"
        assert self.level == lhs.level == rhs.level, "mul_acc requires same level"
        assert self.is_ntt and lhs.is_ntt and rhs.is_ntt, "mul_acc requires NTT domain"
        assert lhs.ncol == rhs.nrow and (lhs.nrow, rhs.ncol) == (self.nrow, self.ncol), "mul_acc: shape mismatch"
        self._touch()
        check_status(_ffi.lib().gpupoly_matrix_mul_acc(self.raw, lhs.raw, rhs.raw, 1 if negate else 0), "gpupoly_matrix_mul_acc")

    def mul_add_in_place(self, lhs, rhs) -> None:
        """self += lhs * rhs in one call (gpupoly_matrix_mul_acc): `x.add_in_place(&(a * &b))` without the temporary."""
        self._mul_acc(lhs, rhs, False)

    def mul_sub_in_place(self, lhs, rhs) -> None:
        """self -= lhs * rhs in one call (gpupoly_matrix_mul_acc)."""
        self._mul_acc(lhs, rhs, True)

    # ---- products with the gadget matrix that never build it (gpupoly_matrix_mul_gadget / _gadget_mul) ----
    @staticmethod
    def _gadget_digits(params, level, small: bool) -> int:
        """columns of g at `level`: digits per tower, times the towers unless `small`"""
        dpt = -(-params.crt_bits() // params.base_bits())
        return dpt if small else dpt * (level + 1)

    @staticmethod
    def _scalar_raw(scalar):
        if scalar is None:
            return None, None
        s = scalar.inner if hasattr(scalar, "inner") else scalar
        s = s.ensure_eval()
        return s, s.raw

    def mul_gadget(self, scalar=None, col_start: int = 0, col_end=None, addend=None, negate: bool = False, out=None, dst_col: int = 0,
                   small: bool = False) -> "GpuDCRTPolyMatrix":
        """addend +- (self * G[:, col_start:col_end]) o scalar in one launch, G = I_d (x) g with d = self.ncol, never built
        (gpupoly_matrix_mul_gadget): `s * G` and `s * (G * y)` of src/bgg/sampler_gpu.rs:149 and src/bgg/sampler.rs:165.
        `out` None: a fresh r x (col_end - col_start) matrix (`addend`, if any, has that shape; dst_col = 0).  Otherwise the
        block goes to columns [dst_col, dst_col + col_end - col_start) of `out`, `addend` is None or has out's shape (it may
        be `out`), and the other columns keep their contents."""
        assert self.is_ntt, "mul_gadget requires NTT domain"
        k = self._gadget_digits(self.params, self.level, small)
        col_end = self.ncol * k if col_end is None else col_end
        cols = col_end - col_start
        assert 0 <= col_start <= col_end <= self.ncol * k, "mul_gadget: gadget window out of range"
        s, s_raw = self._scalar_raw(scalar)
        if out is None:
            assert dst_col == 0, "mul_gadget: dst_col needs an `out` to place the block in"
            out = GpuDCRTPolyMatrix(self.params, self.nrow, cols, self.level, True)
        else:
            out._touch()
        if addend is not None:
            assert addend.is_ntt and (addend.nrow, addend.ncol) == (out.nrow, out.ncol), "mul_gadget: the addend has out's shape, NTT domain"
        st = _ffi.lib().gpupoly_matrix_mul_gadget(out.raw, dst_col, self.raw, s_raw, col_start, cols, None if addend is None else addend.raw,
                                                  1 if negate else 0, self.params.base_bits(), 1 if small else 0)
        check_status(st, "gpupoly_matrix_mul_gadget")
        out.is_ntt = True
        return out

    def add_scaled_gadget(self, scalar=None, negate: bool = False, gadget_col: int = 0, small: bool = False) -> None:
        """self +- G[:, gadget_col : gadget_col + self.ncol] o scalar in place, G = I_d (x) g with d = self.nrow: the
        `A - G * x` idiom (src/lookup/lwe/pubkey_gpu.rs:205-210, src/io/diamond_io/utils.rs:612-616).  Only the limb
        vectors G makes non-zero are read and written."""
        assert self.is_ntt, "add_scaled_gadget requires NTT domain"
        s, s_raw = self._scalar_raw(scalar)
        self._touch()
        st = _ffi.lib().gpupoly_matrix_mul_gadget(self.raw, 0, None, s_raw, gadget_col, self.ncol, self.raw, 1 if negate else 0,
                                                  self.params.base_bits(), 1 if small else 0)
        check_status(st, "gpupoly_matrix_mul_gadget")

    @classmethod
    def gadget_block(cls, params, size, col_start, col_end, scalar=None, negate: bool = False, small: bool = False, level=None) -> "GpuDCRTPolyMatrix":
        """+-G[:, col_start:col_end] o scalar for G = I_size (x) g without the full matrix (gpupoly_matrix_mul_gadget):
        `gadget_matrix.slice(0, d, col_start, col_end)` and `-G[:, chunk]` of the reference's callers."""
        level = params.crt_depth() - 1 if level is None else level
        out = cls(params, size, col_end - col_start, level, True)
        s, s_raw = cls._scalar_raw(scalar)
        st = _ffi.lib().gpupoly_matrix_mul_gadget(out.raw, 0, None, s_raw, col_start, col_end - col_start, None, 1 if negate else 0,
                                                  params.base_bits(), 1 if small else 0)
        check_status(st, "gpupoly_matrix_mul_gadget")
        return out

    @staticmethod
    def gadget_mul(rhs, addend=None, negate: bool = False, small: bool = False) -> "GpuDCRTPolyMatrix":
        """addend +- G * rhs in one launch, G = I_d (x) g with d = rhs.nrow / k, never built (gpupoly_matrix_gadget_mul): the
        recomposition of digit rows (src/lookup/ggh15/pubkey_gpu.rs:505, src/commit/wee25.rs:718).  rhs and addend share one
        domain, which the result takes."""
        k = GpuDCRTPolyMatrix._gadget_digits(rhs.params, rhs.level, small)
        assert rhs.nrow % k == 0, "gadget_mul: rhs rows must be a multiple of the digit count"
        out = GpuDCRTPolyMatrix(rhs.params, rhs.nrow // k, rhs.ncol, rhs.level, rhs.is_ntt)
        if addend is not None:
            assert addend.is_ntt == rhs.is_ntt and (addend.nrow, addend.ncol) == (out.nrow, out.ncol), "gadget_mul: addend shape / domain mismatch"
        st = _ffi.lib().gpupoly_matrix_gadget_mul(out.raw, rhs.raw, None if addend is None else addend.raw, 1 if negate else 0,
                                                  rhs.params.base_bits(), 1 if small else 0)
        check_status(st, "gpupoly_matrix_gadget_mul")
        return out

    def mul_scalar_intt(self, scalar) -> "GpuDCRTPolyMatrix":
        """INTT(self o scalar) in one kernel (extension: the product rides in the inverse transform's load)."""
        s = scalar.inner if hasattr(scalar, "inner") else scalar
        lhs = self.ensure_eval()
        s = s.ensure_eval()
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, False)
        if self.nrow == 0 or self.ncol == 0:
            return out
        check_status(_ffi.lib().gpupoly_matrix_mul_scalar_intt(out.raw, lhs.raw, s.raw), "gpupoly_matrix_mul_scalar_intt")
        return out

    def __mul__(self, rhs):
        from .poly import GpuDCRTPoly

        if isinstance(rhs, GpuDCRTPoly):
            return self.mul_scalar(rhs)
        return self._mul_internal(rhs)

    __matmul__ = __mul__

    def _mul_internal(self, rhs) -> "GpuDCRTPolyMatrix":
        """`mul_internal` (gpu_dcrt_poly.rs:1792-1815)."""
        assert self.ncol == rhs.nrow, f"matrix multiply shape mismatch: ({self.nrow},{self.ncol}) x ({rhs.nrow},{rhs.ncol})"
        assert self.params == rhs.params, "mul requires same params"
        assert self.level == rhs.level, "mul requires same level"
        assert self.is_ntt and rhs.is_ntt, "mul requires NTT domain"
        out = GpuDCRTPolyMatrix(self.params, self.nrow, rhs.ncol, self.level, True)
        if self.nrow == 0 or rhs.ncol == 0:
            return out
        check_status(_ffi.lib().gpu_matrix_mul(out.raw, self.raw, rhs.raw), "gpu_matrix_mul")
        return out

    def __eq__(self, other):
        if not isinstance(other, GpuDCRTPolyMatrix):
            return NotImplemented
        if (
            self.params != other.params
            or (self.nrow, self.ncol) != (other.nrow, other.ncol)
            or self.level != other.level
            or self.is_ntt != other.is_ntt
        ):
            return False
        if self.raw.value == other.raw.value:
            return True
        eq = C.c_int(0)
        check_status(_ffi.lib().gpu_matrix_equal(self.raw, other.raw, C.byref(eq)), "gpu_matrix_equal")
        return eq.value != 0

    __hash__ = None

    # ------------------------------------------------------------------ decomposition
    def _decompose_from(self, src, out_nrow, small) -> "GpuDCRTPolyMatrix":
        out = GpuDCRTPolyMatrix.new_empty(self.params, out_nrow, self.ncol)
        fn = _ffi.lib().gpu_matrix_decompose_base_small if small else _ffi.lib().gpu_matrix_decompose_base
        check_status(fn(src.raw, self.params.base_bits(), out.raw), "gpu_matrix_decompose_base")
        return out

    def decompose(self) -> "GpuDCRTPolyMatrix":
        # an EVAL source goes to the library as it is: its coefficients are produced by an out-of-place inverse
        # transform into a scratch block (decompose.hip), not by clone() + in-place INTT (gpu_dcrt_poly.rs:1227-1233)
        return self._decompose_from(self, self.nrow * self.params.modulus_digits(), False)

    def decompose_owned(self) -> "GpuDCRTPolyMatrix":
        self.intt_all_in_place()
        return self._decompose_from(self, self.nrow * self.params.modulus_digits(), False)

    def small_decompose(self) -> "GpuDCRTPolyMatrix":
        k = -(-self.params.crt_bits() // self.params.base_bits())
        return self._decompose_from(self, self.nrow * k, True)

    def small_decompose_owned(self) -> "GpuDCRTPolyMatrix":
        self.intt_all_in_place()
        k = -(-self.params.crt_bits() // self.params.base_bits())
        return self._decompose_from(self, self.nrow * k, True)

    @classmethod
    def small_decomposed_identity_chunk(cls, params, size, chunk_idx, chunk_count, scalar_by_digit):
        """gpu_dcrt_poly.rs:1296-1326."""
        assert chunk_count > 0 and len(scalar_by_digit) == chunk_count
        assert chunk_idx < chunk_count
        polys = [p.inner.ensure_eval() if hasattr(p, "inner") else p.ensure_eval() for p in scalar_by_digit]
        row = polys[0].concat_columns(polys[1:]) if len(polys) > 1 else polys[0]
        out = cls.new_empty(params, size, size)
        st = _ffi.lib().gpu_matrix_fill_small_decomposed_identity_chunk(out.raw, row.raw, chunk_idx)
        check_status(st, "gpu_matrix_fill_small_decomposed_identity_chunk")
        return out

    @staticmethod
    def mul_batch(lhss, rhss) -> list:
        """[l * r for l, r in zip(lhss, rhss)] through `gpupoly_matrix_mul_batch`: the independent products of one
        circuit level in one call (small ones in one launch; src/circuit/poly_circuit/eval.rs:269 issues one per gate)."""
        assert len(lhss) == len(rhss)
        if not lhss:
            return []
        ls = [m.ensure_eval() for m in lhss]  # converted copies stay referenced until the call returns
        rs = [m.ensure_eval() for m in rhss]
        outs = []
        for l_, r_ in zip(ls, rs):
            assert l_.params == r_.params and l_.level == r_.level and l_.ncol == r_.nrow, "mul_batch: operand mismatch"
            outs.append(GpuDCRTPolyMatrix(l_.params, l_.nrow, r_.ncol, l_.level, True))
        arr = lambda ms: (C.c_void_p * len(ms))(*[m.raw.value if hasattr(m.raw, "value") else m.raw for m in ms])
        st = _ffi.lib().gpupoly_matrix_mul_batch(arr(outs), arr(ls), arr(rs), len(outs))
        check_status(st, "gpupoly_matrix_mul_batch")
        return outs

    @staticmethod
    def eval_gates(gates) -> list:
        """One level of independent circuit gates through `gpupoly_batch` (src/circuit/poly_circuit/eval.rs:269-345
        issues one ABI call per gate).  `gates` = [(kind, lhs, rhs_or_None), ...] with kind in {"mul", "add", "sub",
        "mul_scalar", "neg", "decompose", "mul_decompose"}; returns the gate outputs in order."""
        if not gates:
            return []
        kinds = {"mul": _ffi.GPUPOLY_OP_MUL, "add": _ffi.GPUPOLY_OP_ADD, "sub": _ffi.GPUPOLY_OP_SUB,
                 "mul_scalar": _ffi.GPUPOLY_OP_MUL_SCALAR, "neg": _ffi.GPUPOLY_OP_NEG,
                 "decompose": _ffi.GPUPOLY_OP_DECOMPOSE, "mul_decompose": _ffi.GPUPOLY_OP_MUL_DECOMPOSE}
        params = gates[0][1].params
        k = params.modulus_digits()
        ops = (_ffi.GpuBatchOp * len(gates))()
        outs, keep = [], []
        for i, (kind, lhs, rhs) in enumerate(gates):
            code = kinds[kind]
            if kind in ("mul", "mul_scalar", "mul_decompose"):
                lhs = lhs.ensure_eval()
                if kind != "mul_decompose":
                    rhs = rhs.ensure_eval()
            elif kind in ("add", "sub"):
                assert lhs.is_ntt == rhs.is_ntt, "add / sub gates need operands in one domain"
            if kind == "mul":
                out = GpuDCRTPolyMatrix(params, lhs.nrow, rhs.ncol, lhs.level, True)
            elif kind == "decompose":
                out = GpuDCRTPolyMatrix(params, lhs.nrow * k, lhs.ncol, lhs.level, True)
            elif kind == "mul_decompose":
                out = GpuDCRTPolyMatrix(params, lhs.nrow, rhs.ncol, lhs.level, True)
            else:
                out = GpuDCRTPolyMatrix(params, lhs.nrow, lhs.ncol, lhs.level, lhs.is_ntt)
            keep.append((lhs, rhs))
            ops[i].kind, ops[i].out, ops[i].lhs = code, out.raw, lhs.raw
            ops[i].rhs = rhs.raw if rhs is not None else None
            outs.append(out)
        check_status(_ffi.lib().gpupoly_batch(ops, len(gates), params.base_bits()), "gpupoly_batch")
        for (kind, lhs, rhs), out in zip(gates, outs):
            out.is_ntt = True if kind in ("mul", "mul_scalar", "decompose", "mul_decompose") else (rhs if rhs is not None else lhs).is_ntt
        return outs

    def _digit_count(self, small) -> int:
        """digit rows per source row at this matrix's level: k of include/gpupoly.h"""
        dpt = -(-self.params.crt_bits() // self.params.base_bits())
        return dpt if small else dpt * (self.level + 1)

    def decompose_rows(self, row_start, row_end, small=False, is_ntt=True) -> "GpuDCRTPolyMatrix":
        """Rows [row_start, row_end) of `decompose()` (small: of `small_decompose()`) through
        `gpupoly_matrix_decompose_rows`: the digit transforms run for those rows only, and of an EVAL source only the
        source rows they are digits of are inverse-transformed.  The window may start and end anywhere."""
        total = self.nrow * self._digit_count(small)
        assert 0 <= row_start <= row_end <= total, f"decompose_rows window [{row_start}, {row_end}) out of range: {total} digit rows"
        out = GpuDCRTPolyMatrix(self.params, row_end - row_start, self.ncol, self.level, is_ntt)
        st = _ffi.lib().gpupoly_matrix_decompose_rows(self.raw, self.params.base_bits(), 1 if small else 0, row_start, out.raw)
        check_status(st, "gpupoly_matrix_decompose_rows")
        if row_end == row_start or self.ncol == 0:
            out.is_ntt = True  # an empty result is tagged EVAL, as by gpu_matrix_decompose_base
        return out

    # ---- PolyMatrix trait defaults the GPU wrapper inherits (src/matrix/mod.rs:185-345) ------------------------
    # the defaults build all nrow * chunk_count digit rows and slice nrow of them; here only the kept rows are built
    def decompose_chunk(self, chunk_idx, chunk_count) -> "GpuDCRTPolyMatrix":
        assert chunk_count > 0, "decompose_chunk chunk_count must be > 0"
        assert chunk_idx < chunk_count, f"decompose_chunk chunk_idx out of range: chunk_idx={chunk_idx}, chunk_count={chunk_count}"
        rows = self.nrow * self._digit_count(False)
        assert rows == self.nrow * chunk_count, f"decompose_chunk expected decomposed row count {self.nrow * chunk_count} but got {rows}"
        return self.decompose_rows(chunk_idx * self.nrow, (chunk_idx + 1) * self.nrow, False)

    def small_decompose_chunk(self, chunk_idx, chunk_count) -> "GpuDCRTPolyMatrix":
        assert chunk_count > 0, "small_decompose_chunk chunk_count must be > 0"
        assert chunk_idx < chunk_count, f"small_decompose_chunk chunk_idx out of range: chunk_idx={chunk_idx}, chunk_count={chunk_count}"
        rows = self.nrow * self._digit_count(True)
        assert rows == self.nrow * chunk_count, f"small_decompose_chunk expected decomposed row count {self.nrow * chunk_count} but got {rows}"
        return self.decompose_rows(chunk_idx * self.nrow, (chunk_idx + 1) * self.nrow, True)

    @classmethod
    def small_decomposed_identity_chunk_from_scalar(cls, params, size, scalar, chunk_idx, chunk_count):
        """gpu_dcrt_poly.rs:1328-1350: the scalar's small digits, then one fill per chunk."""
        dec = cls.identity(params, 1, scalar).small_decompose()
        assert dec.size() == (chunk_count, 1), "scalar small decomposition shape mismatch in small_decomposed_identity_chunk_from_scalar"
        by_digit = [dec.entry(d, 0) for d in range(chunk_count)]
        return cls.small_decomposed_identity_chunk(params, size, chunk_idx, chunk_count, by_digit)

    @classmethod
    def unit_column_vector(cls, params, size, index) -> "GpuDCRTPolyMatrix":
        from .poly import GpuDCRTPoly

        assert index < size, "unit column index must be in range"
        col = [[GpuDCRTPoly.const_one(params) if i == index else GpuDCRTPoly.const_zero(params)] for i in range(size)]
        return cls.from_poly_vec(params, col)

    @classmethod
    def unit_row_vector(cls, params, size, index) -> "GpuDCRTPolyMatrix":
        from .poly import GpuDCRTPoly

        row = [GpuDCRTPoly.const_one(params) if j == index else GpuDCRTPoly.const_zero(params) for j in range(size)]
        return cls.from_poly_vec(params, [row])

    def block_entries(self, rows: range, cols: range) -> list:
        assert rows.start <= rows.stop <= self.nrow and cols.start <= cols.stop <= self.ncol, "block range out of bounds"
        return [[self.entry(i, j) for j in cols] for i in rows]

    def concat_rows_owned(self, others) -> "GpuDCRTPolyMatrix":
        return self.concat_rows(others)

    def concat_columns_owned(self, others) -> "GpuDCRTPolyMatrix":
        return self.concat_columns(others)

    def concat_diag_owned(self, others) -> "GpuDCRTPolyMatrix":
        return self.concat_diag(others)

    def mul_tensor_identity(self, other, identity_size) -> "GpuDCRTPolyMatrix":
        """self * (I (x) other) (gpu_dcrt_poly.rs:1374-1390): one extension call, products written in place."""
        assert self.ncol == other.nrow * identity_size
        if not mul_decompose_column_chunk_width_is_set():
            out = GpuDCRTPolyMatrix.new_empty(self.params, self.nrow, other.ncol * identity_size)
            if self.nrow == 0 or out.ncol == 0:
                return out
            lhs, rhs = self.ensure_eval(), other.ensure_eval()  # held: a converted copy must outlive the call
            st = _ffi.lib().gpupoly_matrix_mul_tensor_identity(out.raw, lhs.raw, rhs.raw, identity_size)
            check_status(st, "gpupoly_matrix_mul_tensor_identity")
            return out
        w = other.nrow
        slices = [self.slice(0, self.nrow, i * w, (i + 1) * w)._mul_internal(other) for i in range(identity_size)]
        return slices[0].concat_columns(slices[1:])

    def get_column_matrix_decompose(self, j) -> "GpuDCRTPolyMatrix":
        return self.slice(0, self.nrow, j, j + 1).decompose_owned()

    def mul_tensor_identity_decompose(self, other, identity_size) -> "GpuDCRTPolyMatrix":
        """self * (I (x) G^-1(other)) (gpu_dcrt_poly.rs:1392-1412).  The extension builds G^-1(other) once for all
        identity blocks; the reference's per-block, per-column loop runs when its chunk switch is set."""
        k = self.params.modulus_digits()
        assert self.ncol == other.nrow * identity_size * k
        if not mul_decompose_column_chunk_width_is_set():
            out = GpuDCRTPolyMatrix.new_empty(self.params, self.nrow, other.ncol * identity_size)
            if self.nrow == 0 or out.ncol == 0:
                return out
            lhs = self.ensure_eval()
            st = _ffi.lib().gpupoly_matrix_mul_tensor_identity_decompose(
                out.raw, lhs.raw, other.raw, identity_size, self.params.base_bits()
            )
            check_status(st, "gpupoly_matrix_mul_tensor_identity_decompose")
            return out
        w = other.nrow * k
        outs = []
        for i in range(identity_size):
            sl = self.slice(0, self.nrow, i * w, (i + 1) * w)
            for j in range(other.ncol):
                outs.append(sl._mul_internal(other.get_column_matrix_decompose(j)))
        return outs[0].concat_columns(outs[1:])

    def mul_decompose(self, other) -> "GpuDCRTPolyMatrix":
        """S * G^-1(B), column-chunked (gpu_dcrt_poly.rs:1414-1493)."""
        k = self.params.modulus_digits()
        assert self.ncol == other.nrow * k
        assert self.params == other.params
        ncol = other.ncol
        out = GpuDCRTPolyMatrix.new_empty(self.params, self.nrow, ncol)
        if self.nrow == 0 or ncol == 0:
            return out
        if not mul_decompose_column_chunk_width_is_set():
            # one ABI call: digits generated inside the forward transform, all columns at once, S read once
            # (gpupoly_matrix_mul_decompose).  The reference's column-chunk loop below (chunk
            # width 1 by default, re-reading S per chunk) runs only when its env switch is set explicitly.
            lhs = self.ensure_eval()
            st = _ffi.lib().gpupoly_matrix_mul_decompose(out.raw, lhs.raw, other.raw, self.params.base_bits())
            check_status(st, "gpupoly_matrix_mul_decompose")
            return out
        width = min(mul_decompose_column_chunk_width(), ncol)
        for c0 in range(0, ncol, width):
            c1 = min(c0 + width, ncol)
            dec = other.slice(0, other.nrow, c0, c1).decompose_owned()
            prod = self._mul_internal(dec)
            out.copy_block_from(prod, 0, c0, 0, 0, self.nrow, c1 - c0)
        return out

    @staticmethod
    def mul_decompose_many(lhss, rhs, addends=None, scalars=None) -> list:
        """[l.mul_decompose(rhs) + a.mul_scalar(s) for l, a, s in zip(lhss, addends, scalars)] through
        `gpupoly_matrix_mul_decompose_many`: G^-1(rhs) is built once for all operands and the addend term rides in the
        product's epilogue (the BGG multiplication gates: src/bgg/encoding.rs:125-145,191-219,
        src/bgg/poly_encoding.rs:327-357).  `addends` / `scalars` may be None or hold None entries: no addend / the
        addend as it is.  The reference's per-operand sequence runs when its chunk switch is set."""
        n = len(lhss)
        addends = [None] * n if addends is None else list(addends)
        scalars = [None] * n if scalars is None else list(scalars)
        assert len(addends) == n and len(scalars) == n, "mul_decompose_many: one addend / scalar slot per operand"
        if n == 0:
            return []
        scalars = [s.inner if hasattr(s, "inner") else s for s in scalars]
        k = rhs.params.modulus_digits()
        for l_, a_, s_ in zip(lhss, addends, scalars):
            assert l_.params == rhs.params and l_.ncol == rhs.nrow * k, "mul_decompose_many: operand mismatch"
            assert a_ is None or (a_.nrow, a_.ncol) == (l_.nrow, rhs.ncol), "mul_decompose_many: addend shape"
            assert s_ is None or a_ is not None, "mul_decompose_many: a scalar needs an addend"
        if mul_decompose_column_chunk_width_is_set():
            outs = []
            for l_, a_, s_ in zip(lhss, addends, scalars):
                out = l_.mul_decompose(rhs)
                if a_ is not None:
                    out = out + (a_.mul_scalar(s_) if s_ is not None else a_.ensure_eval())
                outs.append(out)
            return outs
        # converted copies stay referenced until the call returns
        ls = [m.ensure_eval() for m in lhss]
        ads = [None if m is None else m.ensure_eval() for m in addends]
        scs = [None if m is None else m.ensure_eval() for m in scalars]
        outs = [GpuDCRTPolyMatrix(rhs.params, l_.nrow, rhs.ncol, l_.level, True) for l_ in ls]
        raw = lambda m: None if m is None else (m.raw.value if hasattr(m.raw, "value") else m.raw)
        arr = lambda ms: (C.c_void_p * n)(*[raw(m) for m in ms])
        st = _ffi.lib().gpupoly_matrix_mul_decompose_many(arr(outs), arr(ls), arr(ads), arr(scs), n, rhs.raw, rhs.params.base_bits())
        check_status(st, "gpupoly_matrix_mul_decompose_many")
        return outs

    @staticmethod
    def mul_decompose_pairs(lhss, rhss, col_start, col_len, scalars=None, addends=None, negate: bool = False, outs=None) -> list:
        """[a +- (l * r.slice_columns(col_start, col_start + col_len).decompose()) * s for l, r, s, a in ...] through
        `gpupoly_matrix_mul_decompose_pairs`: every operand has its OWN right operand, the windows of all of them go through
        one gather and one digit transform, and scalar, sign and addend ride in the product's epilogue (the slot-transfer gate
        targets: src/slot_transfer/bgg_pubkey_gpu.rs:371-407,409-471).  `scalars` / `addends` may be None or hold None
        entries: the product as it is / no addend.  The scalar multiplies the product (in `mul_decompose_many` it multiplies
        the addend).  `outs`: write there (outs[j] may be addends[j] itself, or a row view of the same rows); fresh matrices
        otherwise.  The right operands may be in either domain and are left as they are."""
        lhss, rhss = list(lhss), list(rhss)
        n = len(lhss)
        assert len(rhss) == n, "mul_decompose_pairs: one right operand per left operand"
        scalars = [None] * n if scalars is None else list(scalars)
        addends = [None] * n if addends is None else list(addends)
        assert len(addends) == n and len(scalars) == n, "mul_decompose_pairs: one addend / scalar slot per operand"
        assert outs is None or len(outs) == n, "mul_decompose_pairs: one output per operand"
        if n == 0:
            return []
        scalars = [s.inner if hasattr(s, "inner") else s for s in scalars]
        p = rhss[0].params
        k = p.modulus_digits()
        for l_, r_, a_ in zip(lhss, rhss, addends):
            assert l_.params == p and r_.params == p and l_.ncol == r_.nrow * k, "mul_decompose_pairs: operand mismatch"
            assert col_start + col_len <= r_.ncol, "mul_decompose_pairs: column window past the right operand"
            assert a_ is None or (a_.nrow, a_.ncol) == (l_.nrow, col_len), "mul_decompose_pairs: addend shape"
        # converted copies stay referenced until the call returns
        ls = [m.ensure_eval() for m in lhss]
        ads = [None if m is None else m.ensure_eval() for m in addends]
        scs = [None if m is None else m.ensure_eval() for m in scalars]
        if outs is None:
            outs = [GpuDCRTPolyMatrix(p, l_.nrow, col_len, l_.level, True) for l_ in ls]
        else:
            outs = list(outs)
            for o in outs:
                o._touch()
        raw = lambda m: None if m is None else (m.raw.value if hasattr(m.raw, "value") else m.raw)
        arr = lambda ms: (C.c_void_p * n)(*[raw(m) for m in ms])
        st = _ffi.lib().gpupoly_matrix_mul_decompose_pairs(arr(outs), arr(ads), arr(ls), arr(rhss), arr(scs), n, col_start,
                                                           p.base_bits(), 1 if negate else 0)
        check_status(st, "gpupoly_matrix_mul_decompose_pairs")
        for o in outs:
            o.is_ntt = True
        return outs

    # ---- the LargeScalarMul gate: lhs * G^-1(G o c) without G or its digit matrix ----
    @staticmethod
    def _int_words(value: int) -> np.ndarray:
        value = int(value)
        if value < 0:
            raise ValueError("large_scalar_mul: negative constant (constants are unsigned)")
        wpc = max(1, -(-value.bit_length() // 64))
        return np.frombuffer(value.to_bytes(8 * wpc, "little"), dtype=np.uint64).copy()

    @staticmethod
    def _large_scalar(first, scalar):
        """-> (constant as an int, None) or (None, 1 x 1 matrix at first's level)"""
        if isinstance(scalar, (int, np.integer)):
            return int(scalar), None
        if isinstance(scalar, (list, tuple)):
            if len(scalar) == 1:
                return int(scalar[0]), None
            assert len(scalar) <= first.params.ring_dimension(), "more coefficients than the ring dimension"
            words = [GpuDCRTPolyMatrix._int_words(c) for c in scalar]
            wpc = max((len(w) for w in words), default=1)
            arr = np.zeros((1, 1, max(len(words), 1), wpc), dtype=np.uint64)
            for i, w in enumerate(words):
                arr[0, 0, i, : len(w)] = w
            return None, GpuDCRTPolyMatrix.from_coeff_words(first.params, arr, True, level=first.level)
        s = scalar.inner if hasattr(scalar, "inner") else scalar
        assert s.size() == (1, 1), "large_scalar_mul: the scalar is a polynomial or a 1 x 1 matrix"
        return None, s

    def large_scalar_mul(self, scalar) -> "GpuDCRTPolyMatrix":
        """self * G^-1(G_d o scalar), d = self.ncol / k: the LargeScalarMul gate of the reference's Evaluables
        (src/bgg/public_key.rs:134-140, src/bgg/encoding.rs:191-200).  See large_scalar_mul_many."""
        return GpuDCRTPolyMatrix.large_scalar_mul_many([self], scalar)[0]

    @staticmethod
    def large_scalar_mul_many(lhss, scalar, addends=None, negate: bool = False) -> list:
        """[a +- l * G^-1(G o scalar) for l, a in zip(lhss, addends)] without G or its digit matrix
        (gpupoly_matrix_mul_decompose_gadget_const_many / _scalar_many).  `scalar`: an int or a one-element list (the
        constant entry: no transform at all), a longer coefficient list, a GpuDCRTPoly or a 1 x 1 matrix in either domain.
        lhss[j] is rows_j x (d_j k) in the NTT domain; `addends` may be None or hold None entries.  The reference's sequence
        (_large_scalar_mul_host) runs when its chunk switch is set."""
        lhss = list(lhss)
        n = len(lhss)
        addends = [None] * n if addends is None else list(addends)
        assert len(addends) == n, "large_scalar_mul_many: one addend slot per operand"
        if n == 0:
            return []
        first = lhss[0]
        k = GpuDCRTPolyMatrix._gadget_digits(first.params, first.level, False)
        for l_, a_ in zip(lhss, addends):
            assert l_.params == first.params and l_.level == first.level, "large_scalar_mul_many: one context and level per call"
            assert l_.ncol % k == 0, "large_scalar_mul_many: lhs columns must be a multiple of the digit count"
            assert a_ is None or (a_.nrow, a_.ncol) == (l_.nrow, l_.ncol), "large_scalar_mul_many: addend shape"
        const, sc = GpuDCRTPolyMatrix._large_scalar(first, scalar)
        if mul_decompose_column_chunk_width_is_set():
            outs = []
            for l_, a_ in zip(lhss, addends):
                prod = l_._large_scalar_mul_host(const if sc is None else sc)
                if a_ is None:
                    outs.append(-prod if negate else prod)
                else:
                    outs.append(a_.ensure_eval() - prod if negate else a_.ensure_eval() + prod)
            return outs
        ls = [m.ensure_eval() for m in lhss]  # converted copies stay referenced until the call returns
        ads = [None if m is None else m.ensure_eval() for m in addends]
        outs = [GpuDCRTPolyMatrix(first.params, l_.nrow, l_.ncol, l_.level, True) for l_ in ls]
        raw = lambda m: None if m is None else (m.raw.value if hasattr(m.raw, "value") else m.raw)
        arr = lambda ms: (C.c_void_p * n)(*[raw(m) for m in ms])
        base = first.params.base_bits()
        if sc is None:
            words = GpuDCRTPolyMatrix._int_words(const)
            st = _ffi.lib().gpupoly_matrix_mul_decompose_gadget_const_many(
                arr(outs), arr(ls), arr(ads), n, words.ctypes.data_as(C.POINTER(C.c_uint64)), len(words), 1 if negate else 0, base)
            check_status(st, "gpupoly_matrix_mul_decompose_gadget_const_many")
        else:
            st = _ffi.lib().gpupoly_matrix_mul_decompose_gadget_scalar_many(arr(outs), arr(ls), arr(ads), n, sc.raw, 1 if negate else 0, base)
            check_status(st, "gpupoly_matrix_mul_decompose_gadget_scalar_many")
        return outs

    def _large_scalar_mul_host(self, scalar) -> "GpuDCRTPolyMatrix":
        """The reference's sequence, kept for comparison: G_d (gpu_matrix_fill_gadget), G_d o scalar (gpu_matrix_mul_scalar),
        self * G^-1(.) (gpupoly_matrix_mul_decompose).  `scalar`: an int or a 1 x 1 matrix / polynomial."""
        k = self._gadget_digits(self.params, self.level, False)
        assert self.ncol % k == 0
        d = self.ncol // k
        out = GpuDCRTPolyMatrix(self.params, self.nrow, self.ncol, self.level, True)
        if self.nrow == 0 or d == 0:
            return out
        if isinstance(scalar, (int, np.integer)):
            words = self._int_words(scalar).reshape(1, 1, 1, -1)
            scalar = GpuDCRTPolyMatrix.from_coeff_words(self.params, words, True, level=self.level)
        s = (scalar.inner if hasattr(scalar, "inner") else scalar).ensure_eval()
        g = GpuDCRTPolyMatrix(self.params, d, d * k, self.level, True)
        check_status(_ffi.lib().gpu_matrix_fill_gadget(g.raw, self.params.base_bits()), "gpu_matrix_fill_gadget")
        gs = GpuDCRTPolyMatrix(self.params, d, d * k, self.level, True)
        check_status(_ffi.lib().gpu_matrix_mul_scalar(gs.raw, g.raw, s.raw), "gpu_matrix_mul_scalar")
        lhs = self.ensure_eval()
        st = _ffi.lib().gpupoly_matrix_mul_decompose(out.raw, lhs.raw, gs.raw, self.params.base_bits())
        check_status(st, "gpupoly_matrix_mul_decompose")
        return out

    def mul_decompose_small(self, other) -> "GpuDCRTPolyMatrix":
        k = -(-self.params.crt_bits() // self.params.base_bits())
        assert self.ncol == other.nrow * k
        ncol = other.ncol
        out = GpuDCRTPolyMatrix.new_empty(self.params, self.nrow, ncol)
        if self.nrow == 0 or ncol == 0:
            return out
        if not mul_decompose_column_chunk_width_is_set():
            lhs = self.ensure_eval()
            st = _ffi.lib().gpupoly_matrix_mul_decompose_small(out.raw, lhs.raw, other.raw, self.params.base_bits())
            check_status(st, "gpupoly_matrix_mul_decompose_small")
            return out
        width = min(mul_decompose_column_chunk_width(), ncol)
        for c0 in range(0, ncol, width):
            c1 = min(c0 + width, ncol)
            dec = other.slice(0, other.nrow, c0, c1).small_decompose_owned()
            prod = self._mul_internal(dec)
            out.copy_block_from(prod, 0, c0, 0, 0, self.nrow, c1 - c0)
        return out

    # ------------------------------------------------------------------ sampling entry points
    @classmethod
    def sample_distribution(cls, params, nrow, ncol, dist: int, sigma: float, seed: GpuRngSeed):
        out = cls.new_empty(params, nrow, ncol)
        if nrow == 0 or ncol == 0:
            return out
        check_status(_ffi.lib().gpu_matrix_sample_distribution(out.raw, dist, sigma, seed), "gpu_matrix_sample_distribution")
        return out

    @classmethod
    def sample_distribution_columns(cls, params, nrow, total_ncol, col_start, col_len, dist, sigma, seed):
        assert col_start + col_len <= total_ncol, "sample_distribution_columns range out of bounds"
        out = cls.new_empty(params, nrow, col_len)
        if nrow == 0 or col_len == 0:
            return out
        st = _ffi.lib().gpu_matrix_sample_distribution_columns(out.raw, dist, sigma, seed, total_ncol, col_start)
        check_status(st, "gpu_matrix_sample_distribution_columns")
        return out

    @classmethod
    def sample_distribution_decomposed(cls, params, nrow, ncol, dist: int, sigma: float, seed: GpuRngSeed, small=False):
        """G^-1 (or the small G^-1) of `sample_distribution(params, nrow, ncol, ...)` through the
        `gpupoly_matrix_sample_decomposed` extension: the samples never leave the coefficient domain."""
        k = -(-params.crt_bits() // params.base_bits()) if small else params.modulus_digits()
        out = cls.new_empty(params, nrow * k, ncol)
        if nrow == 0 or ncol == 0:
            return out
        st = _ffi.lib().gpupoly_matrix_sample_decomposed(out.raw, dist, sigma, seed, params.base_bits(), 1 if small else 0)
        check_status(st, "gpupoly_matrix_sample_decomposed")
        return out

    @classmethod
    def sample_distribution_decomposed_window(cls, params, nrow, total_ncol, col_start, col_len, dist: int, sigma: float,
                                              seed: GpuRngSeed, small=False, row_start=0, row_end=None, is_ntt=True,
                                              level=None):
        """Rows [row_start, row_end) (all of them by default) of G^-1 (or the small G^-1) of
        `sample_distribution_columns(params, nrow, total_ncol, col_start, col_len, ...)` (at `level`, the top one by default) through
        `gpupoly_matrix_sample_decomposed_window`: only the source rows (uniform: and towers) the window touches are
        sampled, the samples never leave the coefficient domain, and only the window's digit transforms run."""
        assert col_start + col_len <= total_ncol, "sample_distribution_decomposed_window column range out of bounds"
        level = params.crt_depth() - 1 if level is None else level
        dpt = -(-params.crt_bits() // params.base_bits())
        k = dpt if small else dpt * (level + 1)
        if row_end is None:
            row_end = nrow * k
        assert 0 <= row_start <= row_end <= nrow * k, f"sample_distribution_decomposed_window rows [{row_start}, {row_end}) out of range: {nrow * k} digit rows"
        out = cls(params, row_end - row_start, col_len, level, is_ntt)
        st = _ffi.lib().gpupoly_matrix_sample_decomposed_window(out.raw, dist, sigma, seed, params.base_bits(), 1 if small else 0,
                                                                nrow, total_ncol, col_start, row_start)
        check_status(st, "gpupoly_matrix_sample_decomposed_window")
        if row_end == row_start or col_len == 0:
            out.is_ntt = True  # an empty result is tagged EVAL, as by gpu_matrix_decompose_base
        return out

    def gauss_samp_gq_arb_base(self, c: float, dgg_stddev: float, seed: GpuRngSeed, coeff_out: bool = False) -> "GpuDCRTPolyMatrix":
        """Consumes self (gpu_dcrt_poly.rs:509-528).  coeff_out: leave the digits as coefficients (the entry point
        finishes in whatever format the output matrix is tagged with) for a caller that transforms them itself
        (`ntt_add_rows_from`)."""
        out = GpuDCRTPolyMatrix(self.params, self.nrow * self.params.modulus_digits(), self.ncol, self.params.crt_depth() - 1,
                                not coeff_out)
        self.intt_all_in_place()
        self._touch()
        st = _ffi.lib().gpu_matrix_gauss_samp_gq_arb_base(self.raw, self.params.base_bits(), c, dgg_stddev, seed, out.raw)
        check_status(st, "gpu_matrix_gauss_samp_gq_arb_base")
        return out

    @staticmethod
    def create_p1_covariance_cache(a_mat, b_mat, d_mat, sigma, s, dgg_stddev) -> GpuP1CovarianceCache:
        raw = C.c_void_p()
        st = _ffi.lib().gpu_matrix_create_p1_covariance_cache(a_mat.raw, b_mat.raw, d_mat.raw, sigma, s, dgg_stddev, C.byref(raw))
        check_status(st, "gpu_matrix_create_p1_covariance_cache")
        return GpuP1CovarianceCache(raw, a_mat.params)

    @staticmethod
    def sample_p1_full_cached(cache: GpuP1CovarianceCache, tp2, seed: GpuRngSeed) -> "GpuDCRTPolyMatrix":
        out = GpuDCRTPolyMatrix.new_empty(tp2.params, tp2.nrow, tp2.ncol)
        if tp2.nrow == 0 or tp2.ncol == 0:
            return out
        tp2.intt_all_in_place()
        check_status(_ffi.lib().gpu_matrix_sample_p1_full_cached(cache.raw, tp2.raw, seed, out.raw), "gpu_matrix_sample_p1_full_cached")
        return out

    # ---- several independently seeded requests in one launch (gpupoly_*_segments; include/gpupoly.h) ------------------
    @staticmethod
    def _segment_args(seeds, seg_cols):
        assert len(seeds) == len(seg_cols) and seeds, "one seed per segment"
        return (GpuRngSeed * len(seeds))(*seeds), (C.c_size_t * len(seg_cols))(*seg_cols), len(seeds)

    @classmethod
    def sample_distribution_segments(cls, params, nrow, seg_cols, dist: int, sigma: float, seeds) -> "GpuDCRTPolyMatrix":
        """[S_0 | S_1 | ...] with S_j == sample_distribution(params, nrow, seg_cols[j], dist, sigma, seeds[j]), one launch.
        Raises GpuPolyError (text contains "unsupported") where the library has no segmented form."""
        out = cls.new_empty(params, nrow, sum(seg_cols))
        arr, cols, n = cls._segment_args(seeds, seg_cols)
        check_status(_ffi.lib().gpupoly_matrix_sample_distribution_segments(out.raw, dist, sigma, arr, cols, n),
                     "gpupoly_matrix_sample_distribution_segments")
        return out

    @classmethod
    def sample_distribution_blocks(cls, params, seeds, dist: int, *, block_polys=None, nrow=None, seg_cols=None) -> "GpuDCRTPolyMatrix":
        """Uniform / bit / ternary samples of len(seeds) independently seeded blocks in one call
        (gpupoly_matrix_sample_distribution_blocks), any number of blocks up to 2^20, the launches not depending on it.
        Stacked layout, `block_polys=P`: the len(seeds) x P matrix whose row t holds the P polynomials of
        `sample_distribution(params, r, c, dist, 0, seeds[t])`, r * c == P, in row-major order.
        Columns layout, `nrow=r, seg_cols=[c_0, ...]`: [S_0 | S_1 | ...] with S_j == sample_distribution(params, r, c_j,
        dist, 0, seeds[j]).  Raises GpuPolyError (text contains "unsupported") for the
        Gaussian distribution - `sample_gauss_blocks` is its entry - and under MXX_HIP_RNG_COMPAT=reference."""
        seeds = list(seeds)
        level = params.crt_depth() - 1
        arr = (GpuRngSeed * max(len(seeds), 1))(*seeds)
        if seg_cols is None:
            assert block_polys is not None and nrow is None, "sample_distribution_blocks: block_polys (stacked) or nrow and seg_cols (columns)"
            out = cls(params, len(seeds), block_polys, level, True)
            layout, cols = _ffi.GPUPOLY_BLOCKS_STACKED, None
        else:
            assert block_polys is None and nrow is not None, "sample_distribution_blocks: block_polys (stacked) or nrow and seg_cols (columns)"
            seg_cols = list(seg_cols)
            assert len(seg_cols) == len(seeds), "sample_distribution_blocks: one seed per block"
            out = cls(params, nrow, sum(seg_cols), level, True)
            layout, cols = _ffi.GPUPOLY_BLOCKS_COLUMNS, (C.c_size_t * max(len(seg_cols), 1))(*seg_cols)
        check_status(_ffi.lib().gpupoly_matrix_sample_distribution_blocks(out.raw, dist, arr, len(seeds), layout, cols),
                     "gpupoly_matrix_sample_distribution_blocks")
        return out

    @classmethod
    def sample_hash_blocks(cls, params, key: bytes, tags, dist: int, *, hash_name: str = "keccak256", block_polys=None, nrow=None,
                           seg_cols=None) -> "GpuDCRTPolyMatrix":
        """`sample_distribution_blocks` with seeds[t] = hash_seed_for_matrix(key, tags[t], hash_name) derived on the device
        (gpupoly_matrix_sample_hash_blocks): tags in, no seeds on the host.  `tags` is an `IndexedTags`
        (generated on the device: nothing is uploaded for them) or any sequence of byte strings (uploaded as one table);
        `hash_name` is keccak256 / keccak_256 or sha3_256.  Layouts, result and the "unsupported" answers are those of
        `sample_distribution_blocks`."""
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        level = params.crt_depth() - 1
        if seg_cols is None:
            assert block_polys is not None and nrow is None, "sample_hash_blocks: block_polys (stacked) or nrow and seg_cols (columns)"
            out = cls(params, count, block_polys, level, True)
            layout, cols = _ffi.GPUPOLY_BLOCKS_STACKED, None
        else:
            assert block_polys is None and nrow is not None, "sample_hash_blocks: block_polys (stacked) or nrow and seg_cols (columns)"
            seg_cols = list(seg_cols)
            assert len(seg_cols) == count, "sample_hash_blocks: one tag per block"
            out = cls(params, nrow, sum(seg_cols), level, True)
            layout, cols = _ffi.GPUPOLY_BLOCKS_COLUMNS, (C.c_size_t * max(len(seg_cols), 1))(*seg_cols)
        check_status(_ffi.lib().gpupoly_matrix_sample_hash_blocks(out.raw, dist, C.byref(arg), count, layout, cols),
                     "gpupoly_matrix_sample_hash_blocks")
        del keep
        return out

    @classmethod
    def _blocks_out(cls, who, params, count, block_polys, nrow, seg_cols):
        """(out, layout, seg_cols array) of a block sample: block_polys (stacked) or nrow and seg_cols (columns)"""
        level = params.crt_depth() - 1
        if seg_cols is None:
            assert block_polys is not None and nrow is None, f"{who}: block_polys (stacked) or nrow and seg_cols (columns)"
            return cls(params, count, block_polys, level, True), _ffi.GPUPOLY_BLOCKS_STACKED, None
        assert block_polys is None and nrow is not None, f"{who}: block_polys (stacked) or nrow and seg_cols (columns)"
        seg_cols = list(seg_cols)
        assert len(seg_cols) == count, f"{who}: one seed or tag per block"
        return cls(params, nrow, sum(seg_cols), level, True), _ffi.GPUPOLY_BLOCKS_COLUMNS, (C.c_size_t * max(len(seg_cols), 1))(*seg_cols)

    @classmethod
    def sample_gauss_blocks(cls, params, seeds, sigma: float, *, block_polys=None, nrow=None, seg_cols=None) -> "GpuDCRTPolyMatrix":
        """Gaussian samples of len(seeds) independently seeded blocks in one call (gpupoly_matrix_sample_gauss_blocks; DESIGN.md
        section 5s), any number of blocks up to 2^20 in four launches: `sample_distribution_blocks`' layouts with block t ==
        sample_distribution(params, r, c, GAUSS, sigma, seeds[t]).  Raises GpuPolyError (text contains "unsupported") for rings
        below n = 128 and under MXX_HIP_RNG_COMPAT=reference."""
        seeds = list(seeds)
        arr = (GpuRngSeed * max(len(seeds), 1))(*seeds)
        out, layout, cols = cls._blocks_out("sample_gauss_blocks", params, len(seeds), block_polys, nrow, seg_cols)
        check_status(_ffi.lib().gpupoly_matrix_sample_gauss_blocks(out.raw, float(sigma), arr, len(seeds), layout, cols),
                     "gpupoly_matrix_sample_gauss_blocks")
        return out

    @classmethod
    def sample_hash_gauss_blocks(cls, params, key: bytes, tags, sigma: float, *, hash_name: str = "keccak256", block_polys=None,
                                 nrow=None, seg_cols=None) -> "GpuDCRTPolyMatrix":
        """`sample_gauss_blocks` with seeds[t] = hash_seed_for_matrix(key, tags[t], hash_name) derived on the device
        (gpupoly_matrix_sample_hash_gauss_blocks): `key`, `tags` and `hash_name` as `sample_hash_blocks` takes them."""
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        out, layout, cols = cls._blocks_out("sample_hash_gauss_blocks", params, count, block_polys, nrow, seg_cols)
        check_status(_ffi.lib().gpupoly_matrix_sample_hash_gauss_blocks(out.raw, float(sigma), C.byref(arg), count, layout, cols),
                     "gpupoly_matrix_sample_hash_gauss_blocks")
        del keep
        return out

    @classmethod
    def _decomposed_blocks_out(cls, params, nblk, nrow, col_len, small, is_ntt, level):
        level = params.crt_depth() - 1 if level is None else level
        dpt = -(-params.crt_bits() // params.base_bits())
        k = dpt if small else dpt * (level + 1)
        return cls(params, nrow * k, nblk * col_len, level, is_ntt)

    @classmethod
    def sample_decomposed_blocks(cls, params, seeds, nrow, total_ncol, col_start, col_len, dist: int, small=False, is_ntt=True,
                                 level=None) -> "GpuDCRTPolyMatrix":
        """[D_0 | D_1 | ...] with D_t == sample_distribution_decomposed_window(params, nrow, total_ncol, col_start, col_len, dist,
        0, seeds[t], small, is_ntt=is_ntt, level=level): G^-1 of the same column window of len(seeds) independently seeded
        nrow x total_ncol matrices in one call (gpupoly_matrix_sample_decomposed_blocks), the launches
        not depending on len(seeds).  Uniform / bit / ternary; raises GpuPolyError (text contains "unsupported") for the
        Gaussian distribution and under MXX_HIP_RNG_COMPAT=reference."""
        seeds = list(seeds)
        out = cls._decomposed_blocks_out(params, len(seeds), nrow, col_len, small, is_ntt, level)
        arr = (GpuRngSeed * max(len(seeds), 1))(*seeds)
        st = _ffi.lib().gpupoly_matrix_sample_decomposed_blocks(out.raw, dist, arr, len(seeds), params.base_bits(), 1 if small else 0, nrow,
                                                                total_ncol, col_start)
        check_status(st, "gpupoly_matrix_sample_decomposed_blocks")
        if out.nrow == 0 or out.ncol == 0:
            out.is_ntt = True  # an empty result is tagged EVAL
        return out

    @classmethod
    def sample_hash_decomposed_blocks(cls, params, key: bytes, tags, nrow, total_ncol, col_start, col_len, dist: int, small=False,
                                      is_ntt=True, level=None, hash_name: str = "keccak256") -> "GpuDCRTPolyMatrix":
        """`sample_decomposed_blocks` with seeds[t] = hash_seed_for_matrix(key, tags[t], hash_name) derived on the device
        (gpupoly_matrix_sample_hash_decomposed_blocks): tags in (an `IndexedTags` or byte strings, as `sample_hash_blocks`
        takes them), no seeds on the host."""
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        out = cls._decomposed_blocks_out(params, count, nrow, col_len, small, is_ntt, level)
        st = _ffi.lib().gpupoly_matrix_sample_hash_decomposed_blocks(out.raw, dist, C.byref(arg), count, params.base_bits(), 1 if small else 0,
                                                                     nrow, total_ncol, col_start)
        check_status(st, "gpupoly_matrix_sample_hash_decomposed_blocks")
        del keep
        if out.nrow == 0 or out.ncol == 0:
            out.is_ntt = True
        return out

    @staticmethod
    def _int_rows(values):
        """The non-negative integers `values` (one at least) as a (count, words) little-endian uint64 array, and `words`."""
        words = [GpuDCRTPolyMatrix._int_words(v) for v in values]
        arr = np.zeros((len(words), max(len(w) for w in words)), dtype=np.uint64)
        for t, w in enumerate(words):
            arr[t, : len(w)] = w
        return arr, arr.shape[1]

    @staticmethod
    def _wee25_call(entry: str, t_bottom, nparts, secret_size, idxs, args) -> list:
        """len(idxs) x nparts fresh secret_size x m_b outputs, `entry(outs, len(idxs), nparts, *args(idx array))` when there is
        any, and the outputs regrouped by block."""
        p = t_bottom.params
        outs = [GpuDCRTPolyMatrix(p, secret_size, t_bottom.nrow, t_bottom.level, True) for _ in range(len(idxs) * nparts)]
        if outs:
            i_arr = np.array(idxs, dtype=np.uint64)
            st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), len(idxs), nparts, *args(i_arr.ctypes.data_as(C.POINTER(C.c_uint64))))
            check_status(st, entry)
        return [outs[t * nparts:(t + 1) * nparts] for t in range(len(idxs))]

    @staticmethod
    def lut_targets(w_identity, w_gy, w_v, w_vx, col_start, col_len, ys, idxs, key: bytes, tags, hash_name: str = "keccak256") -> list:
        """The preimage targets of len(ys) LUT rows of the column chunk [col_start, col_start + col_len) in one call
        (gpupoly_matrix_lut_targets):
            W_id[:, chunk] + W_gy G^-1(G_d[:, chunk] o ys[t]) + (W_v + idxs[t] W_vx) G^-1(U_t[:, chunk]),
        U_t the d x m uniform matrix under hash_seed_for_matrix(key, tags[t]); ys[t], idxs[t] non-negative integers (ys of any
        size, idxs below 2^64).  The four operands are d x m EVAL matrices of one level."""
        ys, idxs = [int(y) for y in ys], [int(i) for i in idxs]
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert len(ys) == len(idxs) == count, "lut_targets: one y, one index and one tag per row"
        p = w_identity.params
        outs = [GpuDCRTPolyMatrix(p, w_identity.nrow, col_len, w_identity.level, True) for _ in range(count)]
        if count == 0:
            return outs
        y_arr, wpy = GpuDCRTPolyMatrix._int_rows(ys)
        i_arr = np.array(idxs, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        st = _ffi.lib().gpupoly_matrix_lut_targets(GpuDCRTPolyMatrix._raw_array(outs), count, w_identity.raw, w_gy.raw, w_v.raw, w_vx.raw,
                                                   col_start, p.base_bits(), y_arr.ctypes.data_as(u64p), wpy, i_arr.ctypes.data_as(u64p),
                                                   C.byref(arg))
        check_status(st, "gpupoly_matrix_lut_targets")
        del keep
        return outs

    @staticmethod
    def lwe_targets(a_z, a_lt, col_start, col_len, ys, xs, key: bytes, tags, hash_name: str = "keccak256") -> list:
        """The preimage targets of len(ys) LUT rows of the column chunk [col_start, col_start + col_len) of the LWE public
        lookup in one call (gpupoly_matrix_lwe_targets):
            A_lt[:, chunk] - G_d[:, chunk] o ys[t] - (A_z - G_d o xs[t]) G^-1(U_t[:, chunk]),
        U_t the d x m uniform matrix under hash_seed_for_matrix(key, tags[t]); ys[t], xs[t] non-negative integers (ys of any
        size, xs below 2^64).  The two operands are d x m EVAL matrices of one level."""
        ys, xs = [int(y) for y in ys], [int(x) for x in xs]
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert len(ys) == len(xs) == count, "lwe_targets: one y, one x and one tag per row"
        p = a_lt.params
        outs = [GpuDCRTPolyMatrix(p, a_lt.nrow, col_len, a_lt.level, True) for _ in range(count)]
        if count == 0:
            return outs
        y_arr, wpy = GpuDCRTPolyMatrix._int_rows(ys)
        x_arr = np.array(xs, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        st = _ffi.lib().gpupoly_matrix_lwe_targets(GpuDCRTPolyMatrix._raw_array(outs), count, a_z.raw, a_lt.raw, col_start, p.base_bits(),
                                                   y_arr.ctypes.data_as(u64p), wpy, x_arr.ctypes.data_as(u64p), C.byref(arg))
        check_status(st, "gpupoly_matrix_lwe_targets")
        del keep
        return outs

    @staticmethod
    def wee25_targets(t_bottom, part_start, nparts, secret_size, idxs, key: bytes, tags, hash_name: str = "keccak256") -> list:
        """The preimage targets of len(idxs) public-parameter indices x `nparts` column parts of the Wee25 commitment in one
        call (gpupoly_matrix_wee25_targets): result[t][p] is the secret_size x m_b matrix
            G_s J(idxs[t], part_start + p) - W_t T_bottom[:, part part_start + p],
        W_t the secret_size x m_b uniform matrix under hash_seed_for_matrix(key, tags[t]), m_b = t_bottom.nrow.  `t_bottom` is
        an m_b x (a multiple of m_b) EVAL matrix; idxs[t] are integers below 2^64."""
        idxs = [int(i) for i in idxs]
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert len(idxs) == count, "wee25_targets: one index and one tag per block"
        base = t_bottom.params.base_bits()
        out = GpuDCRTPolyMatrix._wee25_call("gpupoly_matrix_wee25_targets", t_bottom, nparts, secret_size, idxs,
                                            lambda i_ptr: (t_bottom.raw, part_start, secret_size, base, i_ptr, C.byref(arg)))
        del keep
        return out

    @staticmethod
    def wee25_targets_product(w_stacked, t_bottom, part_start, nparts, secret_size, idxs) -> list:
        """Test instrument (gpupoly_matrix_wee25_targets_product): `wee25_targets` with the stacked [W_0; W_1; ...] given as
        the (len(idxs) * secret_size) x m_b EVAL matrix `w_stacked` instead of sampled."""
        idxs = [int(i) for i in idxs]
        base = t_bottom.params.base_bits()
        return GpuDCRTPolyMatrix._wee25_call("gpupoly_matrix_wee25_targets_product", t_bottom, nparts, secret_size, idxs,
                                             lambda i_ptr: (w_stacked.raw, t_bottom.raw, part_start, secret_size, base, i_ptr))

    @staticmethod
    def _commit_lut_call(entry: str, outs, count, pubkey_sums, a_outs, gate_of_row, ys, head, tail) -> list:
        """`entry(outs, T, *head, P array, A_out array, ngates, gate array, base, y words, words, *tail(arrays kept alive))`;
        `outs` None: T fresh d x m_b outputs, m_b = m_g + 2 d"""
        pubkey_sums, a_outs, ys = list(pubkey_sums), list(a_outs), [int(y) for y in ys]
        gate_of_row = [int(g) for g in gate_of_row]
        assert len(pubkey_sums) == len(a_outs), "commit_lut_messages: one pubkey sum and one A_out per gate"
        assert len(ys) == len(gate_of_row) == count, "commit_lut_messages: one y and one gate per row"
        if outs is None:
            first = a_outs[0]
            outs = [GpuDCRTPolyMatrix(first.params, first.nrow, first.ncol + 2 * first.nrow, first.level, True) for _ in range(count)]
        else:
            outs = list(outs)
            assert len(outs) == count, "commit_lut_messages: one output per row"
        if count == 0:
            return outs
        y_arr, wpy = GpuDCRTPolyMatrix._int_rows(ys)
        g_arr = np.array(gate_of_row, dtype=np.uint32)
        for out in outs:
            out._touch()
        st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), count, *head, GpuDCRTPolyMatrix._raw_array(pubkey_sums),
                                        GpuDCRTPolyMatrix._raw_array(a_outs), len(a_outs), g_arr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        a_outs[0].params.base_bits(), y_arr.ctypes.data_as(C.POINTER(C.c_uint64)), wpy, *tail)
        check_status(st, entry)
        for out in outs:
            out.is_ntt = True
        return outs

    @staticmethod
    def commit_lut_messages(b_1, verifier, vslots, pubkey_sums, a_outs, gate_of_row, ys, idxs, key: bytes, tags, hash_name: str = "keccak256",
                            outs=None) -> list:
        """The message blocks of len(ys) LUT rows of the commitment-based public lookup in one call
        (gpupoly_matrix_commit_lut_messages), g = gate_of_row[t]:
            [a_outs[g] - G_d o ys[t] | 0] + R_t - pubkey_sums[g] G^-1((b_1 V_t + R_t) o (idxs[t] + 1)^-1),
        R_t the d x m_b uniform matrix under hash_seed_for_matrix(key, tags[t]), V_t the block vslots[t] of the
        m_b x (nV m_b) EVAL matrix `verifier`; ys[t] non-negative integers of any size, idxs[t] below 2^64.  b_1 is d x m_b,
        pubkey_sums[g] and a_outs[g] are d x m_g, EVAL, of one level.  Returns the rows' d x m_b matrices."""
        vslots, idxs = [int(v) for v in vslots], [int(i) for i in idxs]
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert len(vslots) == len(idxs) == count, "commit_lut_messages: one verifier slot, one index and one tag per row"
        u64p = C.POINTER(C.c_uint64)
        v_arr, i_arr = np.array(vslots, dtype=np.uint64), np.array(idxs, dtype=np.uint64)
        out = GpuDCRTPolyMatrix._commit_lut_call("gpupoly_matrix_commit_lut_messages", outs, count, pubkey_sums, a_outs, gate_of_row, ys,
                                                 (b_1.raw, verifier.raw, v_arr.ctypes.data_as(u64p)), (i_arr.ctypes.data_as(u64p), C.byref(arg)))
        del keep
        return out

    @staticmethod
    def commit_lut_messages_combine(r_stacked, digits, pubkey_sums, a_outs, gate_of_row, ys, outs=None) -> list:
        """Test instrument (gpupoly_matrix_commit_lut_messages_combine): `commit_lut_messages` with [R_0 | R_1 | ...] given
        as the d x (len(ys) * m_b) EVAL matrix `r_stacked` and the digits of the cancelers as the m_g x (len(ys) * m_b) EVAL
        matrix `digits`, instead of sampled, multiplied and decomposed."""
        ys = list(ys)
        return GpuDCRTPolyMatrix._commit_lut_call("gpupoly_matrix_commit_lut_messages_combine", outs, len(ys), pubkey_sums, a_outs,
                                                  gate_of_row, ys, (r_stacked.raw, digits.raw), ())

    @staticmethod
    def _ggh15_lookup_call(entry: str, mids, lut_preimages, xs, col_start, col_len, ys, last) -> list:
        """len(ys) fresh r x col_len outputs and `entry(outs, S, *mids, K array, x array, col_start, base, y words, words, last)`"""
        mids, lut_preimages, xs, ys = list(mids), list(lut_preimages), list(xs), [int(y) for y in ys]
        count = len(ys)
        assert len(mids) == 6 and len(lut_preimages) == len(xs) == count, "ggh15_lookup: six stage-1 products; one K, x and y per slot"
        first = mids[0]
        outs = [GpuDCRTPolyMatrix(first.params, first.nrow // max(count, 1), col_len, first.level, True) for _ in range(count)]
        if count == 0:
            return outs
        y_arr, wpy = GpuDCRTPolyMatrix._int_rows(ys)
        st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), count, *[m.raw for m in mids], GpuDCRTPolyMatrix._raw_array(lut_preimages),
                                        GpuDCRTPolyMatrix._raw_array(xs), col_start, first.params.base_bits(),
                                        y_arr.ctypes.data_as(C.POINTER(C.c_uint64)), wpy, last)
        check_status(st, entry)
        return outs

    @staticmethod
    def ggh15_lookup(mids, lut_preimages, xs, col_start, col_len, ys, key: bytes, tags, hash_name: str = "keccak256") -> list:
        """Stage 2 of the GGH15 public lookup for len(ys) slots of one gate and the output column chunk
        [col_start, col_start + col_len) in one call (gpupoly_matrix_ggh15_lookup):
            mid_id_s[:, chunk] + mid_gy_s G^-1(G_d[:, chunk] o ys[s]) + (mid_v_s + xs[s] o mid_vx_s + mid_rand_s) V_s - mid_g1_s K_s,
        `mids` = (mid_identity, mid_gy, mid_v, mid_vx, mid_rand, mid_gate1), the stage-1 products with slot s in rows
        [s r, (s + 1) r); lut_preimages[s] = K_s (w x col_len; one matrix may serve several slots), xs[s] the slot's plaintext
        as a 1 x 1 EVAL matrix, V_s = G^-1(U_s[:, chunk]) with U_s the d x m_g uniform matrix under
        hash_seed_for_matrix(key, tags[s]).  Returns the slots' r x col_len matrices."""
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert count == len(ys), "ggh15_lookup: one tag per slot"
        out = GpuDCRTPolyMatrix._ggh15_lookup_call("gpupoly_matrix_ggh15_lookup", mids, lut_preimages, xs, col_start, col_len, ys, C.byref(arg))
        del keep
        return out

    @staticmethod
    def ggh15_lookup_combine(mids, lut_preimages, xs, digits, col_start, col_len, ys) -> list:
        """Test instrument (gpupoly_matrix_ggh15_lookup_combine): `ggh15_lookup` with [V_0 | V_1 | ...] given as the
        m_g x (len(ys) * col_len) EVAL matrix `digits` instead of sampled."""
        return GpuDCRTPolyMatrix._ggh15_lookup_call("gpupoly_matrix_ggh15_lookup_combine", mids, lut_preimages, xs, col_start, col_len, ys, digits.raw)

    @staticmethod
    def _lwe_lookup_call(entry: str, outs, c_bs, k_highs, c_zs, col_start, dst_col, last) -> list:
        """`entry(outs, S, dst_col, c_b array, K_high array, c_z array, col_start, base, last)`; `outs` None: S fresh
        r x chunk-column outputs (dst_col = 0)"""
        c_bs, k_highs, c_zs = list(c_bs), list(k_highs), list(c_zs)
        count = len(c_zs)
        assert len(c_bs) == len(k_highs) == count, "lwe_lookup: one c_b, K_high chunk and input vector per slot"
        if outs is None:
            assert dst_col == 0, "lwe_lookup: dst_col needs `outs` to place the block in"
            outs = [GpuDCRTPolyMatrix(z.params, z.nrow, kh.ncol, z.level, True) for z, kh in zip(c_zs, k_highs)]
        else:
            outs = list(outs)
            assert len(outs) == count, "lwe_lookup: one output per slot"
        if count == 0:
            return outs
        for out in outs:
            out._touch()
        st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), count, dst_col, GpuDCRTPolyMatrix._raw_array(c_bs),
                                        GpuDCRTPolyMatrix._raw_array(k_highs), GpuDCRTPolyMatrix._raw_array(c_zs), col_start,
                                        c_zs[0].params.base_bits(), last)
        check_status(st, entry)
        for out in outs:
            out.is_ntt = True
        return outs

    @staticmethod
    def lwe_lookup(outs, c_bs, k_highs, c_zs, col_start, key: bytes, tags, hash_name: str = "keccak256", dst_col: int = 0) -> list:
        """The online side of the LWE public lookup for len(c_zs) slots of one gate and the output column chunk
        [col_start, col_start + c), c = k_highs[0].ncol, in one call (gpupoly_matrix_lwe_lookup):
            outs[s][:, dst_col .. dst_col + c) = c_bs[s] k_highs[s] + c_zs[s] G^-1(U_s[:, col_start .. col_start + c)),
        c_bs[s] r x w, k_highs[s] w x c, c_zs[s] r x m_g, U_s the d x m_g uniform matrix under
        hash_seed_for_matrix(key, tags[s]); one matrix may serve several slots.  `outs` None: fresh r x c matrices; otherwise
        the slots' r x C matrices, whose columns outside the block keep their contents.  Returns the outputs."""
        c_zs = list(c_zs)
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert count == len(c_zs), "lwe_lookup: one tag per slot"
        out = GpuDCRTPolyMatrix._lwe_lookup_call("gpupoly_matrix_lwe_lookup", outs, c_bs, k_highs, c_zs, col_start, dst_col, C.byref(arg))
        del keep
        return out

    @staticmethod
    def lwe_lookup_combine(outs, c_bs, k_highs, c_zs, digits, col_start, dst_col: int = 0) -> list:
        """Test instrument (gpupoly_matrix_lwe_lookup_combine): `lwe_lookup` with [D_0 | D_1 | ...] given as the
        m_g x (len(c_zs) * c) EVAL matrix `digits` instead of sampled."""
        return GpuDCRTPolyMatrix._lwe_lookup_call("gpupoly_matrix_lwe_lookup_combine", outs, c_bs, k_highs, c_zs, col_start, dst_col, digits.raw)

    @staticmethod
    def _slot_transfer_eval_call(entry: str, outs, c_b0, gate_preimages, b1_preimages, terms_by_out, col_start, dst_col, last) -> list:
        """`entry(outs, S, dst_col, c_b0, Pg array, P1 array, terms, term offsets, mu words, words per mu, col_start, base,
        last)`; terms_by_out[s] lists output s's terms (c_in, mid, shift, scalar, mu); `outs` None: S fresh r x chunk-column
        outputs (dst_col = 0)"""
        gate_preimages, b1_preimages = list(gate_preimages), list(b1_preimages)
        terms_by_out = [list(ts) for ts in terms_by_out]
        count = len(terms_by_out)
        assert len(gate_preimages) == len(b1_preimages) == count, "slot_transfer_eval: one gate preimage chunk, P1 chunk and term list per output"
        if outs is None:
            assert dst_col == 0, "slot_transfer_eval: dst_col needs `outs` to place the block in"
            outs = [GpuDCRTPolyMatrix(c_b0.params, c_b0.nrow, pg.ncol, c_b0.level, True) for pg in gate_preimages]
        else:
            outs = list(outs)
            assert len(outs) == count, "slot_transfer_eval: one output per term list"
        if count == 0:
            return outs
        flat = [t for ts in terms_by_out for t in ts]
        terms = (_ffi.GpuSlotTerm * max(len(flat), 1))()
        for j, (c_in, mid, shift, scalar, _) in enumerate(flat):
            terms[j].c_in, terms[j].mid = GpuDCRTPolyMatrix._raw_array([c_in, mid])
            terms[j].shift, terms[j].scalar = int(shift), int(scalar)
        offsets = (C.c_size_t * (count + 1))()
        for s, ts in enumerate(terms_by_out):
            offsets[s + 1] = offsets[s] + len(ts)
        mu_arr, wpm = GpuDCRTPolyMatrix._int_rows([int(t[4]) for t in flat] or [0])
        for out in outs:
            out._touch()
        st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), count, dst_col, c_b0.raw, GpuDCRTPolyMatrix._raw_array(gate_preimages),
                                        GpuDCRTPolyMatrix._raw_array(b1_preimages), terms, offsets, mu_arr.ctypes.data_as(C.POINTER(C.c_uint64)), wpm,
                                        col_start, c_b0.params.base_bits(), last)
        check_status(st, entry)
        for out in outs:
            out.is_ntt = True
        return outs

    @staticmethod
    def slot_transfer_eval(outs, c_b0, gate_preimages, b1_preimages, terms_by_out, col_start, key: bytes, tags, hash_name: str = "keccak256",
                           dst_col: int = 0) -> list:
        """Stage 2 of the slot-transfer online evaluation for len(terms_by_out) outputs of one gate and the output column chunk
        [col_start, col_start + c), c = gate_preimages[0].ncol, in one call (gpupoly_matrix_slot_transfer_eval; DESIGN.md
        section 5y):
            outs[s][:, dst_col .. dst_col + c) = c_b0 Pg_s + sum_t (kappa_t x^shift_t) o (c_in_t G^-1(A_s[:, chunk]) + mu_t o (mid_t P1_s)),
        c_b0 r x w0, gate_preimages[s] = Pg_s w0 x c, b1_preimages[s] = P1_s w1 x c, terms_by_out[s] the output's terms as
        (c_in r x m_g, mid = c_b0 P0_src r x w1, shift, scalar kappa, integer mu), A_s the d x m_g uniform matrix under
        hash_seed_for_matrix(key, tags[s]); one matrix may serve several outputs or terms.  `outs` None: fresh r x c matrices;
        otherwise the outputs' r x C matrices, whose columns outside the block keep their contents.  Returns the outputs."""
        terms_by_out = [list(ts) for ts in terms_by_out]
        arg, keep, count = hash_tags_arg(key, tags, hash_name)
        assert count == len(terms_by_out), "slot_transfer_eval: one tag per output"
        out = GpuDCRTPolyMatrix._slot_transfer_eval_call("gpupoly_matrix_slot_transfer_eval", outs, c_b0, gate_preimages, b1_preimages, terms_by_out,
                                                         col_start, dst_col, C.byref(arg))
        del keep
        return out

    @staticmethod
    def slot_transfer_eval_combine(outs, c_b0, gate_preimages, b1_preimages, terms_by_out, digits, col_start, dst_col: int = 0) -> list:
        """Test instrument (gpupoly_matrix_slot_transfer_eval_combine): `slot_transfer_eval` with [D_0 | D_1 | ...] given as
        the m_g x (outputs * c) EVAL matrix `digits` instead of sampled."""
        return GpuDCRTPolyMatrix._slot_transfer_eval_call("gpupoly_matrix_slot_transfer_eval_combine", outs, c_b0, gate_preimages, b1_preimages,
                                                          terms_by_out, col_start, dst_col, digits.raw)

    @staticmethod
    def _bgg_encode_call(entry: str, outs, secrets, pubkeys, plaintexts, *last) -> list:
        """`entry(outs, P, secrets, pubkey array, plaintexts, base, *last)`; `outs` None: P fresh S x m outputs"""
        pubkeys = list(pubkeys)
        count = len(pubkeys)
        if outs is None:
            outs = [GpuDCRTPolyMatrix(secrets.params, secrets.nrow, pk.ncol, secrets.level, True) for pk in pubkeys]
        else:
            outs = list(outs)
            assert len(outs) == count, "bgg_encode_slots: one output per public key"
        if count == 0:
            return outs
        for out in outs:
            out._touch()
        st = getattr(_ffi.lib(), entry)(GpuDCRTPolyMatrix._raw_array(outs), count, secrets.raw, GpuDCRTPolyMatrix._raw_array(pubkeys),
                                        None if plaintexts is None else plaintexts.raw, secrets.params.base_bits(), *last)
        check_status(st, entry)
        for out in outs:
            out.is_ntt = True
        return outs

    @staticmethod
    def bgg_encode_slots(secrets, pubkeys, plaintexts, sigma: float, seeds, outs=None) -> list:
        """The BGG+ encoding vectors of len(pubkeys) inputs in S = secrets.nrow slots in one call
        (gpupoly_matrix_bgg_encode_slots):
            outs[i][s, :] = secrets[s, :] pubkeys[i] - plaintexts[s, i - 1] o (secrets[s, :] G) + e_s[:, i m .. (i + 1) m),
        secrets S x d (row s is the slot's secret t_s), pubkeys[i] d x m, plaintexts S x (len(pubkeys) - 1) or None with one
        input (input 0's plaintext is the constant 1), e_s = sample_distribution(params, 1, len(pubkeys) * m, GAUSS, sigma,
        seeds[s]); sigma == 0: no error and `seeds` is not read.  `outs` None: fresh S x m matrices.  Raises GpuPolyError
        (text contains "unsupported") with sigma > 0 for rings below n = 128 and under MXX_HIP_RNG_COMPAT=reference."""
        arr = None
        if sigma > 0:
            seeds = list(seeds)
            assert len(seeds) == secrets.nrow, "bgg_encode_slots: one seed per slot"
            arr = (GpuRngSeed * max(len(seeds), 1))(*seeds)
        return GpuDCRTPolyMatrix._bgg_encode_call("gpupoly_matrix_bgg_encode_slots", outs, secrets, pubkeys, plaintexts, float(sigma), arr)

    @staticmethod
    def bgg_encode_slots_combine(secrets, pubkeys, plaintexts, errors, outs=None) -> list:
        """`bgg_encode_slots` with the errors given as the S x (len(pubkeys) * m) EVAL matrix `errors`, or None for none
        (gpupoly_matrix_bgg_encode_slots_combine): a test instrument, and the path for errors of the plain sampler."""
        return GpuDCRTPolyMatrix._bgg_encode_call("gpupoly_matrix_bgg_encode_slots_combine", outs, secrets, pubkeys, plaintexts,
                                                  None if errors is None else errors.raw)

    @staticmethod
    def sample_p1_full_cached_segments(cache: GpuP1CovarianceCache, tp2, seeds, seg_cols) -> "GpuDCRTPolyMatrix":
        """`sample_p1_full_cached` over column segments with a seed each (tp2 is taken to the coefficient domain in place)."""
        out = GpuDCRTPolyMatrix.new_empty(tp2.params, tp2.nrow, tp2.ncol)
        arr, cols, n = GpuDCRTPolyMatrix._segment_args(seeds, seg_cols)
        tp2.intt_all_in_place()
        check_status(_ffi.lib().gpupoly_matrix_sample_p1_full_cached_segments(cache.raw, tp2.raw, arr, cols, n, out.raw),
                     "gpupoly_matrix_sample_p1_full_cached_segments")
        return out

    def gauss_samp_gq_arb_base_segments(self, c: float, dgg_stddev: float, seeds, seg_cols, coeff_out: bool = False) -> "GpuDCRTPolyMatrix":
        """`gauss_samp_gq_arb_base` over column segments with a seed each; consumes self."""
        out = GpuDCRTPolyMatrix(self.params, self.nrow * self.params.modulus_digits(), self.ncol, self.params.crt_depth() - 1,
                                not coeff_out)
        arr, cols, n = self._segment_args(seeds, seg_cols)
        self.intt_all_in_place()
        self._touch()
        st = _ffi.lib().gpupoly_matrix_gauss_samp_gq_arb_base_segments(self.raw, self.params.base_bits(), c, dgg_stddev, arr, cols, n, out.raw)
        check_status(st, "gpupoly_matrix_gauss_samp_gq_arb_base_segments")
        return out

    @staticmethod
    def _raw_array(ms):
        return (C.c_void_p * len(ms))(*[m.raw.value if hasattr(m.raw, "value") else m.raw for m in ms])

    @classmethod
    def concat_columns_of(cls, blocks) -> "GpuDCRTPolyMatrix":
        """[blocks[0] | blocks[1] | ...] in one launch per 64 blocks (`gpupoly_matrix_concat_columns`); the blocks share one
        domain (converted copies are made like `concat_columns` does)."""
        blocks = [blocks[0]] + blocks[0]._same_domain(blocks[1:])
        first = blocks[0]
        for b in blocks:
            assert b.nrow == first.nrow and b.level == first.level and b.params == first.params, "concat_columns_of: block mismatch"
        out = cls(first.params, first.nrow, sum(b.ncol for b in blocks), first.level, first.is_ntt)
        check_status(_ffi.lib().gpupoly_matrix_concat_columns(out.raw, cls._raw_array(blocks), len(blocks)), "gpupoly_matrix_concat_columns")
        return out

    def split_columns(self, widths) -> list:
        """the column blocks of the given widths, in order, in one launch per 64 blocks (`gpupoly_matrix_split_columns`)"""
        assert sum(widths) == self.ncol, "split_columns: widths must add up to the column count"
        outs = [GpuDCRTPolyMatrix(self.params, self.nrow, w, self.level, self.is_ntt) for w in widths]
        check_status(_ffi.lib().gpupoly_matrix_split_columns(self.raw, self._raw_array(outs), len(outs)), "gpupoly_matrix_split_columns")
        return outs

    def __repr__(self):
        return f"GpuDCRTPolyMatrix({self.nrow}x{self.ncol}, level={self.level}, is_ntt={self.is_ntt})"
