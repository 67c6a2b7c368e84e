"""GPU: tags to sampler seeds on the device (`gpupoly_hash_seeds`, `gpupoly_matrix_sample_hash_blocks`).

The bar: a device-hashed seed IS hash_seed_for_matrix(key, tag) of the mirror - the host definition, pure Python and hashlib -
bit for bit, and a tagged block call leaves `out` as the seeds-given call leaves it for those host seeds (gpu_matrix_equal and
the layout tag).  Rings: n = 256 with three 51-bit limbs (64-bit words) and n = 1024 with three 24-bit limbs (32-bit words, a
uniform sample finishes PACKED24).  The host hashes are computed once per (hash, tag) and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

HASH_ENTRY = "gpupoly_hash_seeds"
ENTRY = "gpupoly_matrix_sample_hash_blocks"
RINGS = {"n256_u64": (256, 3, 51, 17), "n1024_packed24": (1024, 3, 24, 12)}
KEY = bytes((11 * i + 3) & 0xFF for i in range(32))
WEE25 = b"wee25_w_block_"
GGH15 = b"ggh15_lut_v_idx_3_"
TOP = 1 << 64


def params_of(gpu, oracle, ring):
    return make_params(gpu, oracle, *RINGS[ring])


@functools.lru_cache(maxsize=None)
def host_seed_bytes(hash_name, tag):
    import mxx_amd

    return mxx_amd.hash_seed_for_matrix(KEY, tag, hash_name).to_bytes()


def host_seeds(gpu, hash_name, tags):
    return [gpu.GpuRngSeed.from_bytes(host_seed_bytes(hash_name, bytes(t))) for t in tags]


def device_seed_bytes(p, tags, hash_name="keccak256"):
    from mxx_amd.matrix import device_hash_seeds

    return [s.to_bytes() for s in device_hash_seeds(p, KEY, tags, hash_name)]


def table_tag(n):
    return bytes((5 * n + 3 * j + 1) & 0xFF for j in range(n))


# ---------------------------------------------------------------------------------------------------
# 1. gpupoly_hash_seeds against the host definition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_name", ["keccak256", "sha3_256"])
def test_table_form_equals_the_host_hash_at_every_tag_length(gpu, oracle, hash_name):
    """300 tags of 0..299 bytes behind the 57 bytes of domain and key and in front of the 4 counter bytes: the message ends one
    byte short of the rate at 74 (padding byte and closing bit in one byte), fills it at 75 (a block of padding alone), and
    likewise at 210 / 211 / 212 for two blocks"""
    p = params_of(gpu, oracle, "n256_u64")
    tags = [table_tag(n) for n in range(300)]
    got = device_seed_bytes(p, tags, hash_name)
    for n, tag in enumerate(tags):
        assert got[n] == host_seed_bytes(hash_name, tag), f"{hash_name}: tag of {n} bytes"


@pytest.mark.parametrize("decimal", [False, True], ids=["le64", "decimal"])
def test_indexed_forms_equal_their_literal_expansion(gpu, oracle, decimal):
    p = params_of(gpu, oracle, "n1024_packed24")
    prefix = GGH15 if decimal else WEE25
    # 95: the decimal form grows a digit inside the range; 2^32 - 3: the index crosses a word; 2^64 - 300: up to the last index
    for first, count in ((0, 12), (95, 12), ((1 << 32) - 3, 12), (TOP - 300, 300)):
        tags = gpu.IndexedTags(prefix, first, count, decimal)
        literal = list(tags)
        assert literal[0] == prefix + (str(first).encode() if decimal else first.to_bytes(8, "little"))
        got = device_seed_bytes(p, tags)
        assert got == [host_seed_bytes("keccak256", t) for t in literal], (decimal, first)
        assert got == device_seed_bytes(p, literal), (decimal, first)  # and the table form of the same tags
    sha = gpu.IndexedTags(prefix, 95, 12, decimal)
    assert device_seed_bytes(p, sha, "sha3_256") == [host_seed_bytes("sha3_256", t) for t in sha]


def test_counts_at_the_wave_and_workgroup_edges_and_the_prefix_lengths(gpu, oracle):
    p = params_of(gpu, oracle, "n256_u64")
    want = [host_seed_bytes("keccak256", t) for t in gpu.IndexedTags(WEE25, 0, 257)]
    for count in (1, 63, 64, 65, 256, 257):
        assert device_seed_bytes(p, gpu.IndexedTags(WEE25, 0, count)) == want[:count], count
        assert device_seed_bytes(p, list(gpu.IndexedTags(WEE25, 0, count))) == want[:count], count
    from mxx_amd import _ffi
    from mxx_amd.matrix import hash_tags_arg

    for prefix in (b"", bytes((9 * i + 200) & 0xFF for i in range(64))):
        for decimal in (False, True):
            tags = gpu.IndexedTags(prefix, 7, 5, decimal)
            assert hash_tags_arg(KEY, tags)[0].form != _ffi.GPUPOLY_TAGS_TABLE
            assert device_seed_bytes(p, tags) == [host_seed_bytes("keccak256", t) for t in tags], (len(prefix), decimal)


def test_a_second_context_of_the_device_gives_the_same_seeds(gpu, oracle):
    """no per-context state is involved"""
    a, b = params_of(gpu, oracle, "n256_u64"), params_of(gpu, oracle, "n1024_packed24")
    assert a.ctx().raw != b.ctx().raw
    for tags in (gpu.IndexedTags(WEE25, 40, 70), gpu.IndexedTags(GGH15, 40, 70, True), [table_tag(n) for n in range(60, 90)]):
        assert device_seed_bytes(a, tags) == device_seed_bytes(b, tags)
        assert device_seed_bytes(a, tags, "sha3_256") == device_seed_bytes(b, tags, "sha3_256")


# ---------------------------------------------------------------------------------------------------
# 2. the tagged block call against the seeds-given call
# ---------------------------------------------------------------------------------------------------
def tag_forms(gpu, count, first=97):
    return {"table": [table_tag(70 + n) for n in range(count)], "le64": gpu.IndexedTags(WEE25, first, count),
            "decimal": gpu.IndexedTags(GGH15, first, count, True)}


@pytest.mark.parametrize("dist", ["uniform", "bit", "ternary"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_hash_blocks_equal_the_blocks_of_host_derived_seeds(gpu, oracle, ring, dist):
    p = params_of(gpu, oracle, ring)
    M, code = gpu.GpuDCRTPolyMatrix, oracle.DIST[dist]
    widths = [1, 3, 2, 1, 2]
    layout = "packed24" if (ring, dist) == ("n1024_packed24", "uniform") else "words"  # read before the comparison unpacks
    for form, tags in tag_forms(gpu, len(widths)).items():
        seeds = host_seeds(gpu, "keccak256", tags)
        want = M.sample_distribution_blocks(p, seeds, code, block_polys=3)
        got = M.sample_hash_blocks(p, KEY, tags, code, block_polys=3)
        assert got.size() == (5, 3) and got.is_ntt and got.layout == want.layout == layout and got == want, ("stacked", form)
        want = M.sample_distribution_blocks(p, seeds, code, nrow=2, seg_cols=widths)
        got = M.sample_hash_blocks(p, KEY, tags, code, nrow=2, seg_cols=widths)
        assert got.size() == (2, 9) and got.is_ntt and got.layout == want.layout == layout and got == want, ("columns", form)
    # the other padding, and more blocks than a workgroup of the hash kernel has lanes
    tags = gpu.IndexedTags(WEE25, TOP - 300, 300)
    want = M.sample_distribution_blocks(p, host_seeds(gpu, "sha3_256", tags), code, block_polys=1)
    assert M.sample_hash_blocks(p, KEY, tags, code, hash_name="sha3_256", block_polys=1) == want


def host_path_sampler(gpu, hash_name):
    """a hash sampler forced to hash on the host"""

    class Forced(gpu.GpuDCRTPolyHashSampler):
        def _on_device(self):
            return False

    return Forced(hash_name)


@pytest.mark.parametrize("hash_name", ["keccak256", "sha3_256"])
def test_the_mirror_hashes_on_the_device_and_equals_its_host_path(gpu, oracle, hash_name, monkeypatch):
    import hashlib

    import mxx_amd.sampler as sampler_mod

    p = params_of(gpu, oracle, "n1024_packed24")
    M, moduli, n = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension()
    fin, bit = gpu.DistType.FinRingDist(), gpu.DistType.BitDist()
    host, dev = host_path_sampler(gpu, hash_name), gpu.GpuDCRTPolyHashSampler(hash_name)
    literal, indexed = [WEE25 + t.to_bytes(8, "little") for t in range(70)], gpu.IndexedTags(WEE25, 0, 70)
    weights = M.from_rns(p, oracle.random_matrix(31, 1, 70, moduli, n), True)
    want_many = host.sample_hash_many(p, KEY, literal, 1, 2, fin)
    want_bits = host.sample_hash_many(p, KEY, literal[:3], 2, 1, bit)
    want_stack = host.sample_hash_stacked(p, KEY, literal, 1, 2, fin)
    stack_layout = want_stack.layout  # read before a comparison unpacks it
    assert stack_layout == "packed24"
    want_sum = host.sample_hash_weighted_sum(p, KEY, literal, weights, 1, 2)
    want_one = host.sample_hash(p, KEY, literal[5], 1, 2, fin)
    # from here on the host definitions are out of reach: the device sampler must not miss them
    def no_host_hash(*a, **k):
        raise AssertionError("the mirror hashed on the host")

    monkeypatch.setattr(sampler_mod, "keccak256", no_host_hash)
    monkeypatch.setattr(sampler_mod, "hash_seed_for_matrix", no_host_hash)
    monkeypatch.setattr(hashlib, "new", no_host_hash)
    for tags in (literal, indexed):
        many = dev.sample_hash_many(p, KEY, tags, 1, 2, fin)
        assert len(many) == 70 and all(many[t] == want_many[t] for t in range(70))
        assert all(a == b for a, b in zip(dev.sample_hash_many(p, KEY, tags[:3], 2, 1, bit), want_bits))
        stack = dev.sample_hash_stacked(p, KEY, tags, 1, 2, fin)
        assert stack.layout == stack_layout and stack == want_stack
        assert dev.sample_hash_weighted_sum(p, KEY, tags, weights, 1, 2) == want_sum
        # three chunks of the stack: 32 + 32 + 6 tags
        poly_bytes = len(moduli) * n * p.ctx().word_bytes()
        assert dev.sample_hash_weighted_sum(p, KEY, tags, weights, 1, 2, max_stack_bytes=32 * 2 * poly_bytes) == want_sum
        assert dev.sample_hash(p, KEY, tags[5], 1, 2, fin) == want_one
    gauss = gpu.DistType.GaussDist(3.5)  # the Gaussian leg: seeds from the device, the Gaussian segments as before
    got = dev.sample_hash_many(p, KEY, indexed[:3], 1, 2, gauss)
    monkeypatch.undo()
    assert all(a == b for a, b in zip(got, host.sample_hash_many(p, KEY, literal[:3], 1, 2, gauss)))


def test_another_hashlib_name_still_goes_through_the_host(gpu, oracle):
    p = params_of(gpu, oracle, "n256_u64")
    M, fin = gpu.GpuDCRTPolyMatrix, gpu.DistType.FinRingDist()
    sampler = gpu.GpuDCRTPolyHashSampler("blake2s")
    tags = gpu.IndexedTags(GGH15, 8, 4, True)
    many = sampler.sample_hash_many(p, KEY, tags, 1, 2, fin)
    stack = sampler.sample_hash_stacked(p, KEY, tags, 1, 2, fin)
    for t, tag in enumerate(tags):
        alone = M.sample_distribution(p, 1, 2, fin.as_ffi(), 0.0, gpu.hash_seed_for_matrix(KEY, tag, "blake2s"))
        assert many[t] == alone and stack.row_view(t, t + 1) == alone
    assert not (many[0] == gpu.GpuDCRTPolyHashSampler().sample_hash_many(p, KEY, tags, 1, 2, fin)[0])


# ---------------------------------------------------------------------------------------------------
# 3. launches and copies
# ---------------------------------------------------------------------------------------------------
def test_one_launch_more_than_the_seeds_given_entry_and_no_upload_for_indexed_tags(gpu, oracle):
    from mxx_amd import _ffi

    lib = _ffi.lib()

    def launches(fn):
        c0 = lib.gpupoly_launch_count()
        fn()
        return lib.gpupoly_launch_count() - c0

    def traced(fn):
        _ffi.trace_begin()
        fn()
        return _ffi.trace_end()

    def copies(trace):
        return [e for e in trace if e["threads"] == 0 or "host to device" in e["kernel"]]

    for ring in RINGS:
        p = params_of(gpu, oracle, ring)
        M = gpu.GpuDCRTPolyMatrix
        given = {}
        for count in (1, 257):
            forms = tag_forms(gpu, count)
            seeds = host_seeds(gpu, "keccak256", forms["le64"])
            for layout, shape in (("stacked", dict(block_polys=2)), ("columns", dict(nrow=1, seg_cols=[1] * count))):
                given[count, layout] = launches(lambda: M.sample_distribution_blocks(p, seeds, 0, **shape))
                for form, tags in forms.items():
                    got = launches(lambda: M.sample_hash_blocks(p, KEY, tags, 0, **shape))
                    assert got == given[count, layout] + 1, (ring, count, form, layout)
        # the launch count does not depend on the block count
        one = launches(lambda: M.sample_hash_blocks(p, KEY, gpu.IndexedTags(WEE25, 0, 1), 0, block_polys=2))
        many = launches(lambda: M.sample_hash_blocks(p, KEY, gpu.IndexedTags(WEE25, 0, 257), 0, block_polys=2))
        assert one == many == given[257, "stacked"] + 1
        # what is copied: nothing for indexed tags in the stacked layout, the starts alone in the columns layout, one table
        # of offsets and bytes (and starts) in the table form
        forms = tag_forms(gpu, 257)
        for form in ("le64", "decimal"):
            trace = traced(lambda: M.sample_hash_blocks(p, KEY, forms[form], 0, block_polys=2))
            assert copies(trace) == [] and [e["kernel"] for e in trace][0] == "hash_seeds_kernel", (form, trace)
            assert len(trace) == many
            trace = traced(lambda: M.sample_hash_blocks(p, KEY, forms[form], 0, nrow=1, seg_cols=[1] * 257))
            assert [e["bytes"] for e in copies(trace)] == [8.0 * 258], (form, trace)
        table_bytes = sum(len(t) for t in forms["table"])
        trace = traced(lambda: M.sample_hash_blocks(p, KEY, forms["table"], 0, block_polys=2))
        assert [e["bytes"] for e in copies(trace)] == [8.0 * (258 + (table_bytes + 7) // 8)], trace
        trace = traced(lambda: M.sample_hash_blocks(p, KEY, forms["table"], 0, nrow=1, seg_cols=[1] * 257))
        assert [e["bytes"] for e in copies(trace)] == [8.0 * (258 + 258 + (table_bytes + 7) // 8)], trace


# ---------------------------------------------------------------------------------------------------
# 4. refusals: nothing launched, `out` (residues and tag) as it was, the message names the entry
# ---------------------------------------------------------------------------------------------------
def make_tags(form=1, hash_=0, tags=WEE25, offsets=None, prefix_len=None, first=0):
    from mxx_amd import _ffi

    arg = _ffi.GpuHashTags()
    arg.hash, arg.form = hash_, form
    arg.key[:] = KEY
    buf = None if tags is None else C.create_string_buffer(tags, max(len(tags), 1))
    arg.tags = None if buf is None else C.cast(buf, C.c_void_p)
    off = None if offsets is None else (C.c_size_t * len(offsets))(*offsets)
    arg.tag_offsets = off
    arg.prefix_len = (len(tags) if tags is not None and form != 0 else 0) if prefix_len is None else prefix_len
    arg.first_index = first
    arg._keep = (buf, off)
    return arg


# name -> (GpuHashTags for two tags, a word of the message); every one is refused by both entries
BAD_TAGS = {
    "unknown hash": (lambda: make_tags(hash_=2), "hash"),
    "negative hash": (lambda: make_tags(hash_=-1), "hash"),
    "unknown form": (lambda: make_tags(form=3), "form"),
    "negative form": (lambda: make_tags(form=-1), "form"),
    "table without offsets": (lambda: make_tags(form=0, tags=b"abcd"), "tag_offsets"),
    "table without bytes": (lambda: make_tags(form=0, tags=None, offsets=[0, 2, 4]), "null tag bytes"),
    "table offsets not from 0": (lambda: make_tags(form=0, tags=b"abcd", offsets=[1, 2, 4]), "start at 0"),
    "table offsets decreasing": (lambda: make_tags(form=0, tags=b"abcd", offsets=[0, 3, 2]), "decrease"),
    "indexed prefix of 65 bytes": (lambda: make_tags(tags=bytes(65)), "prefix_len"),
    "decimal prefix of 65 bytes": (lambda: make_tags(form=2, tags=bytes(65)), "prefix_len"),
    "indexed with offsets": (lambda: make_tags(offsets=[0, 1, 2]), "tag_offsets"),
    "decimal with offsets": (lambda: make_tags(form=2, offsets=[0, 1, 2]), "tag_offsets"),
    "indexed range wraps": (lambda: make_tags(first=TOP - 1), "wraps"),
    "decimal range wraps": (lambda: make_tags(form=2, first=TOP - 1), "wraps"),
}


def test_refusals_launch_nothing_and_leave_the_output_alone(gpu, oracle, hip_env):
    from mxx_amd import _ffi

    p = params_of(gpu, oracle, "n1024_packed24")
    M, moduli, n, lib = gpu.GpuDCRTPolyMatrix, p.moduli(), p.ring_dimension(), _ffi.lib()
    sentinel = oracle.random_matrix(91, 2, 3, moduli, n)
    STACKED, COLUMNS = _ffi.GPUPOLY_BLOCKS_STACKED, _ffi.GPUPOLY_BLOCKS_COLUMNS
    good = make_tags()

    def widths(*w):
        return (C.c_size_t * len(w))(*w)

    def call(out, dist=0, tags=good, nblk=2, layout=STACKED, seg_cols=None):
        return lib.gpupoly_matrix_sample_hash_blocks(None if out is None else out.raw, dist, None if tags is None else C.byref(tags), nblk, layout, seg_cols)

    cases = {  # what gpupoly_matrix_sample_distribution_blocks refuses
        "null out": (lambda out: call(None), ""),
        "null tags": (lambda out: call(out, tags=None), "null tags"),
        "no blocks": (lambda out: call(out, nblk=0), ""),
        "more than 2^20 blocks": (lambda out: call(out, nblk=(1 << 20) + 1), ""),
        "unknown layout": (lambda out: call(out, layout=2), "layout"),
        "negative layout": (lambda out: call(out, layout=-1), "layout"),
        "stacked with seg_cols": (lambda out: call(out, seg_cols=widths(1, 2)), "seg_cols"),
        "stacked rows": (lambda out: call(out, nblk=3), "row"),
        "columns without seg_cols": (lambda out: call(out, layout=COLUMNS), "seg_cols"),
        "zero width": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(3, 0)), "zero"),
        "widths short of the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 1)), "sum"),
        "widths past the columns": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(2, 2)), "sum"),
        "gaussian": (lambda out: call(out, dist=1), "unsupported"),
        "gaussian, columns": (lambda out: call(out, dist=1, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported"),
        "dist_type 4": (lambda out: call(out, dist=4), "dist_type"),
        "dist_type -1": (lambda out: call(out, dist=-1), "dist_type"),
        "a block of 2^48 polynomials": (lambda out: call(out, layout=COLUMNS, seg_cols=widths(1 << 47, 3)), "48-bit"),
    }
    for name, (make, word) in BAD_TAGS.items():
        cases[name] = (lambda out, make=make: call(out, tags=make()), word)
        cases[name + ", columns"] = (lambda out, make=make: call(out, tags=make(), layout=COLUMNS, seg_cols=widths(1, 2)), word)

    def check(name, fn, word):
        out = M.from_rns(p, sentinel, False)  # COEFF-tagged: a tag flipped to EVAL would change the COEFF read-out
        c0 = lib.gpupoly_launch_count()
        assert fn(out) != 0, name
        msg = _ffi.last_error_string()
        assert ENTRY in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0, name
        assert not out.is_ntt and np.array_equal(out.to_rns(), sentinel), name

    for name, (fn, word) in cases.items():
        check(name, fn, word)
    # gpupoly_hash_seeds: the same refusals of `tags`, and its own arguments
    ctx = p.ctx().raw
    seeds = (gpu.GpuRngSeed * 2)()
    canary = bytes(range(100, 164))
    C.memmove(seeds, canary, 64)
    own = {"null context": (lambda: lib.gpupoly_hash_seeds(None, C.byref(good), 2, seeds), "context"),
           "null tags": (lambda: lib.gpupoly_hash_seeds(ctx, None, 2, seeds), "null tags"),
           "null seeds_out": (lambda: lib.gpupoly_hash_seeds(ctx, C.byref(good), 2, None), "seeds_out"),
           "no tags": (lambda: lib.gpupoly_hash_seeds(ctx, C.byref(good), 0, seeds), "2^20"),
           "more than 2^20 tags": (lambda: lib.gpupoly_hash_seeds(ctx, C.byref(good), (1 << 20) + 1, seeds), "2^20")}
    for name, (make, word) in BAD_TAGS.items():
        own[name] = (lambda make=make: lib.gpupoly_hash_seeds(ctx, C.byref(make()), 2, seeds), word)
    for name, (fn, word) in own.items():
        c0 = lib.gpupoly_launch_count()
        assert fn() != 0, name
        msg = _ffi.last_error_string()
        assert HASH_ENTRY in msg and word in msg, (name, msg)
        assert lib.gpupoly_launch_count() == c0 and C.string_at(seeds, 64) == canary, name
    # the same calls succeed once the fault is gone; a table of empty tags needs no bytes; the last index is reachable
    out = M.from_rns(p, sentinel, False)
    assert call(out) == 0 and call(out, layout=COLUMNS, seg_cols=widths(1, 2)) == 0
    empty = make_tags(form=0, tags=None, offsets=[0, 0, 0])
    assert call(out, tags=empty) == 0, _ffi.last_error_string()
    assert lib.gpupoly_hash_seeds(ctx, C.byref(empty), 2, seeds) == 0, _ffi.last_error_string()
    assert [s.to_bytes() for s in seeds] == [host_seed_bytes("keccak256", b"")] * 2
    assert lib.gpupoly_hash_seeds(ctx, C.byref(make_tags(first=TOP - 2)), 2, seeds) == 0
    assert seeds[1].to_bytes() == host_seed_bytes("keccak256", WEE25 + (TOP - 1).to_bytes(8, "little"))
    for hollow, kw in ((M(p, 2, 0, 1, False), {}), (M(p, 0, 3, 1, False), dict(layout=COLUMNS, seg_cols=widths(1, 2)))):
        c0 = lib.gpupoly_launch_count()
        assert call(hollow, **kw) == 0 and lib.gpupoly_launch_count() == c0
    # the reference's own keying has no block form: refused, and the mirror falls back to the loop with the loop's matrices
    sampler = gpu.GpuDCRTPolyHashSampler()
    tags, fin = gpu.IndexedTags(WEE25, 0, 5), gpu.DistType.FinRingDist()
    default = sampler.sample_hash_many(p, KEY, tags, 1, 2, fin)
    hip_env.set("MXX_HIP_RNG_COMPAT", "reference")
    check("reference keying", lambda out: call(out), "unsupported")
    check("reference keying, columns", lambda out: call(out, layout=COLUMNS, seg_cols=widths(1, 2)), "unsupported")
    many = sampler.sample_hash_many(p, KEY, tags, 1, 2, fin)
    stacked = sampler.sample_hash_stacked(p, KEY, tags, 1, 2, fin)
    for t, tag in enumerate(tags):
        alone = sampler.sample_hash(p, KEY, tag, 1, 2, fin)
        assert many[t] == alone and stacked.row_view(t, t + 1) == alone
        assert not (alone == default[t])  # the other keying
    hip_env.unset("MXX_HIP_RNG_COMPAT")
    assert sampler.sample_hash_many(p, KEY, tags, 1, 2, fin)[4] == default[4]
