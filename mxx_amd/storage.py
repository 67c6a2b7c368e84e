"""The lookup buffer of src/storage/write.rs:724-793 (`get_lookup_buffer`) and the reading of its slots
(src/storage/read.rs:129-149), with the matrices serialised and loaded through the batched compact-bytes entries: one
device call per buffer instead of one per matrix.  Nothing else of src/storage/ (files, the global index) is mirrored.

Layout (write.rs:757-775), every integer a little-endian u64:
    count | bytes per matrix = longest blob + 16 | count indices | count slots of `bytes per matrix` bytes, zero padded
"""
import struct

from .matrix import GpuDCRTPolyMatrix

SLOT_SLACK = 16  # write.rs:757


def lookup_buffer_from_blobs(indices, blobs) -> bytes:
    """The buffer for blobs that are already in slot order (pure host)."""
    indices, blobs = list(indices), list(blobs)
    assert len(indices) == len(blobs), "one index per blob"
    count = len(blobs)
    slot = max((len(b) for b in blobs), default=0) + SLOT_SLACK
    header = 16 + 8 * count
    out = bytearray(header + slot * count)
    struct.pack_into(f"<QQ{count}Q", out, 0, count, slot, *indices)
    for i, b in enumerate(blobs):
        at = header + i * slot
        out[at : at + len(b)] = b
    return bytes(out)


def parse_lookup_buffer(data):
    """(indices, slots): every slot with its padding, as the reading side hands it to `from_compact_bytes`."""
    assert len(data) >= 16, "truncated lookup buffer"
    count, slot = struct.unpack_from("<QQ", data, 0)
    header = 16 + 8 * count
    assert len(data) == header + slot * count, "lookup buffer length mismatch"
    indices = list(struct.unpack_from(f"<{count}Q", data, 16))
    return indices, [bytes(data[header + i * slot : header + (i + 1) * slot]) for i in range(count)]


def get_lookup_buffer(preimages) -> bytes:
    """`get_lookup_buffer` for (index, matrix) pairs: sorted by index, serialised by one batched store (the matrices are
    left as they are), laid out as above."""
    pairs = sorted(preimages, key=lambda kv: kv[0])
    blobs = GpuDCRTPolyMatrix.to_compact_bytes_many([m for _, m in pairs])
    return lookup_buffer_from_blobs([k for k, _ in pairs], blobs)


def matrices_from_lookup_buffer(params, data) -> list:
    """[(index, matrix)] of a whole buffer, loaded by one batched call."""
    indices, slots = parse_lookup_buffer(data)
    return list(zip(indices, GpuDCRTPolyMatrix.from_compact_bytes_many(params, slots)))
