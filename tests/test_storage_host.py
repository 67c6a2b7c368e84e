"""CPU-only: the lookup-buffer layout of mxx_amd/storage.py (src/storage/write.rs:757-775) against bytes built by hand."""
import struct


def test_lookup_buffer_layout_and_parser():
    from mxx_amd import storage

    blobs = [b"\x01\x02\x03", b"\xaa" * 21, b"\x7f" * 8]
    indices = [9, 2, 40]  # the caller's order is kept as it is: sorting is get_lookup_buffer's job
    buf = storage.lookup_buffer_from_blobs(indices, blobs)
    slot = 21 + 16
    want = struct.pack("<Q", 3) + struct.pack("<Q", slot)
    for k in indices:
        want += struct.pack("<Q", k)
    for b in blobs:
        want += b + bytes(slot - len(b))
    assert buf == want
    assert len(buf) == 16 + 8 * 3 + 3 * slot
    got_indices, slots = storage.parse_lookup_buffer(buf)
    assert got_indices == indices
    assert slots == [b + bytes(slot - len(b)) for b in blobs]
    assert all(len(s) == slot for s in slots)


def test_empty_lookup_buffer():
    from mxx_amd import storage

    buf = storage.lookup_buffer_from_blobs([], [])
    assert buf == struct.pack("<QQ", 0, 16)
    assert storage.parse_lookup_buffer(buf) == ([], [])
