"""CPU-only: mxx_amd/csrc/keccak.h - the sponge hash_seed.hip runs on the device - compiled as plain C++17 into a stand-alone
program (tests/cpp/keccak_check.cpp, its own main, the header its only include) under AddressSanitizer and
UndefinedBehaviorSanitizer, and run in its own process against the committed known answers, hashlib's SHA3-256 and the mirror's
keccak256; and the pure-Python side of the tagged entries: IndexedTags and the binding of the two new symbols."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_KECCAK, PAD_SHA3 = 0x01, 0x06


@pytest.fixture(scope="module")
def keccak_check(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/keccak_check.cpp"
    exe = tmp_path_factory.mktemp("keccak") / "keccak_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "keccak_check.cpp"), "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]

    def digests(pad, messages):
        text = "".join(f"{pad:02x} {m.hex() or '-'}\n" for m in messages)
        run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]  # a sanitizer report ends the program with a message
        lines = run.stdout.split()
        assert len(lines) == len(messages)
        return lines

    return digests


def message(n):
    return bytes((7 * n + 13 * j + 1) & 0xFF for j in range(n))


def test_known_answers_of_keccak256(keccak_check):
    """the answers committed in tests/test_host_logic.py"""
    want = {b"": "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
            b"abc": "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45",
            b"a" * 135: "34367dc248bbd832f4e3e69dfaac2f92638bd0bbd18f2912ba4ef454919cf446"}
    assert keccak_check(PAD_KECCAK, list(want)) == list(want.values())


def test_sha3_256_against_hashlib(keccak_check):
    msgs = [message(n) for n in range(301)] + [b"", b"abc", b"a" * 135, bytes(1000)]
    assert keccak_check(PAD_SHA3, msgs) == [hashlib.sha3_256(m).hexdigest() for m in msgs]


def test_keccak256_against_the_mirror_at_every_length(keccak_check):
    """0..300 bytes: one, two and three rate blocks, with the padding byte and the closing bit in one byte at 135 and 271,
    a block of padding alone at 136 and 272"""
    from mxx_amd.sampler import keccak256

    msgs = [message(n) for n in range(301)]
    got = keccak_check(PAD_KECCAK, msgs)
    for n, m in enumerate(msgs):
        assert got[n] == keccak256(m).hex(), n
    assert len(set(got)) == 301


# ---- the mirror's side ------------------------------------------------------------------------------------------------
def test_indexed_tags_expand_to_the_literal_tags():
    from mxx_amd import IndexedTags

    top = (1 << 64) - 1
    for first in (0, 9, 10, top):
        le, dec = IndexedTags(b"wee25_w_block_", first, 1), IndexedTags(b"ggh15_lut_v_idx_3_", first, 1, decimal=True)
        assert list(le) == [b"wee25_w_block_" + first.to_bytes(8, "little")] and len(le) == 1
        assert list(dec) == [b"ggh15_lut_v_idx_3_" + str(first).encode()] and dec[0] == dec[-1] == list(dec)[0]
    assert list(IndexedTags(b"ggh15_lut_v_idx_3_", top, 1, decimal=True))[0].endswith(b"_18446744073709551615")
    grow = IndexedTags(b"t_", 98, 4, decimal=True)  # 99 -> 100: a digit more inside the range
    assert list(grow) == [b"t_98", b"t_99", b"t_100", b"t_101"] and len(grow) == 4
    assert list(IndexedTags(b"wee25_w_block_", 98, 4)) == [b"wee25_w_block_" + i.to_bytes(8, "little") for i in range(98, 102)]
    # slicing: a step of one stays indexed, and every slice holds the literal tags
    part = grow[1:3]
    assert isinstance(part, IndexedTags) and (part.first, len(part), part.decimal) == (99, 2, True) and list(part) == [b"t_99", b"t_100"]
    assert list(grow[2:100]) == [b"t_100", b"t_101"] and list(grow[4:]) == [] and grow[::2] == [b"t_98", b"t_100"]
    assert grow[3] == b"t_101" and grow[-4] == b"t_98"
    with pytest.raises(IndexError):
        grow[4]
    assert list(IndexedTags(b"", 5, 0)) == [] and len(IndexedTags(b"", 5, 0)) == 0
    assert list(IndexedTags(b"", top - 1, 2)) == [(top - 1).to_bytes(8, "little"), top.to_bytes(8, "little")]
    with pytest.raises(ValueError):
        IndexedTags(b"x", top, 2)  # the range wraps


def test_the_tags_argument_of_the_entries():
    import ctypes as C

    from mxx_amd import IndexedTags, _ffi
    from mxx_amd.matrix import hash_tags_arg

    key = bytes(range(32))
    arg, keep, count = hash_tags_arg(key, IndexedTags(b"wee25_w_block_", 7, 5), "keccak256")
    assert (arg.hash, arg.form, count) == (_ffi.GPUPOLY_HASH_KECCAK256, _ffi.GPUPOLY_TAGS_INDEXED_LE64, 5)
    assert (arg.prefix_len, arg.first_index, bytes(arg.key)) == (14, 7, key) and not arg.tag_offsets
    assert C.string_at(arg.tags, 14) == b"wee25_w_block_"
    arg, keep, count = hash_tags_arg(key, IndexedTags(b"i_", 7, 5, decimal=True), "sha3_256")
    assert (arg.hash, arg.form) == (_ffi.GPUPOLY_HASH_SHA3_256, _ffi.GPUPOLY_TAGS_INDEXED_DECIMAL)
    arg, keep, count = hash_tags_arg(key, [b"ab", b"", b"cde"], "keccak_256")
    assert (arg.form, count) == (_ffi.GPUPOLY_TAGS_TABLE, 3) and [arg.tag_offsets[i] for i in range(4)] == [0, 2, 2, 5]
    assert C.string_at(arg.tags, 5) == b"abcde"
    # a prefix the indexed forms do not take goes up as a table of the literal tags
    long = IndexedTags(bytes(65), 0, 2)
    arg, keep, count = hash_tags_arg(key, long, "keccak256")
    assert arg.form == _ffi.GPUPOLY_TAGS_TABLE and arg.tag_offsets[2] == 2 * 73
    with pytest.raises(ValueError):
        hash_tags_arg(key, [b"x"], "blake2s")


def test_both_symbols_are_declared_and_bound():
    from mxx_amd import _ffi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpupoly.h")).read(), flags=re.S)
    for name in ("gpupoly_hash_seeds", "gpupoly_matrix_sample_hash_blocks"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _ffi.SIGNATURES
        assert hasattr(_ffi.lib(), name)
    assert "typedef struct GpuHashTags" in text
    for macro, value in (("GPUPOLY_HASH_KECCAK256", 0), ("GPUPOLY_HASH_SHA3_256", 1), ("GPUPOLY_TAGS_TABLE", 0),
                         ("GPUPOLY_TAGS_INDEXED_LE64", 1), ("GPUPOLY_TAGS_INDEXED_DECIMAL", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
        assert getattr(_ffi, macro) == value
    # the struct as C lays it out: two ints, the key, two pointers, a size and a 64-bit index
    import ctypes as C

    assert C.sizeof(_ffi.GpuHashTags) == 72 and _ffi.GpuHashTags.tags.offset == 40 and _ffi.GpuHashTags.first_index.offset == 64


def test_null_arguments_are_an_error_naming_the_entry():
    """no device needed: the argument checks come first"""
    import ctypes as C

    from mxx_amd import IndexedTags, _ffi
    from mxx_amd.matrix import hash_tags_arg

    lib = _ffi.lib()
    arg, keep, count = hash_tags_arg(bytes(32), IndexedTags(b"wee25_w_block_", 0, 2))
    seeds = (_ffi.GpuRngSeed * 2)()
    for args in ((None, 0, C.byref(arg), 2, _ffi.GPUPOLY_BLOCKS_STACKED, None), (None, 0, None, 2, _ffi.GPUPOLY_BLOCKS_STACKED, None)):
        assert lib.gpupoly_matrix_sample_hash_blocks(*args) != 0
        assert "gpupoly_matrix_sample_hash_blocks" in _ffi.last_error_string()
    for args in ((None, C.byref(arg), 2, seeds), (None, None, 0, None)):
        assert lib.gpupoly_hash_seeds(*args) != 0
        assert "gpupoly_hash_seeds" in _ffi.last_error_string()
    assert all(w == 0 for s in seeds for w in s.words)
