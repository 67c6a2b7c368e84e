"""CPU-only: `gpupoly_matrix_sample_gauss_blocks` and `gpupoly_matrix_sample_hash_gauss_blocks` are part of the plain C ABI -
declared in include/gpupoly.h, exported by libgpupoly, bound in `_ffi.SIGNATURES`; a C99 caller compiles against the header,
links, and gets an error code plus a message naming the function (never a crash) for null arguments, with its own arrays
left as they were."""
import os
import subprocess

SEEDED = "gpupoly_matrix_sample_gauss_blocks"
HASHED = "gpupoly_matrix_sample_hash_gauss_blocks"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, who) != NULL;
}

int main(void) {
    GpuRngSeed seeds[2] = {{{1, 2, 3, 4}}, {{5, 6, 7, 8}}};
    size_t cols[2] = {1, 2};
    static const uint8_t prefix[4] = {'t', 'a', 'g', '_'};
    GpuHashTags tags;
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.hash = GPUPOLY_HASH_KECCAK256;
    tags.form = GPUPOLY_TAGS_INDEXED_DECIMAL;
    tags.tags = prefix;
    tags.prefix_len = 4;
    tags.first_index = 9;
    ok = ok && refused(gpupoly_matrix_sample_gauss_blocks(NULL, 3.5, seeds, 2, GPUPOLY_BLOCKS_COLUMNS, cols), "gpupoly_matrix_sample_gauss_blocks");
    ok = ok && refused(gpupoly_matrix_sample_gauss_blocks(NULL, 3.5, seeds, 2, GPUPOLY_BLOCKS_STACKED, NULL), "gpupoly_matrix_sample_gauss_blocks");
    ok = ok && refused(gpupoly_matrix_sample_gauss_blocks(NULL, 0.0, NULL, 0, GPUPOLY_BLOCKS_STACKED, NULL), "gpupoly_matrix_sample_gauss_blocks");
    ok = ok && refused(gpupoly_matrix_sample_hash_gauss_blocks(NULL, 3.5, &tags, 2, GPUPOLY_BLOCKS_COLUMNS, cols),
                       "gpupoly_matrix_sample_hash_gauss_blocks");
    ok = ok && refused(gpupoly_matrix_sample_hash_gauss_blocks(NULL, 3.5, NULL, 2, GPUPOLY_BLOCKS_STACKED, NULL),
                       "gpupoly_matrix_sample_hash_gauss_blocks");
    ok = ok && cols[0] == 1 && cols[1] == 2 && tags.prefix_len == 4 && tags.first_index == 9 && tags.tags == prefix;
    ok = ok && seeds[0].words[0] == 1 && seeds[0].words[3] == 4 && seeds[1].words[0] == 5 && seeds[1].words[3] == 8;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (SEEDED, HASHED):
        assert f"int {name}(GpuMatrix *out, double sigma, " in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    # each prototype cites what it replaces
    doc = header[header.index("Gaussian seeded blocks"):header.index(f"int {HASHED}(")]
    for cited in ("sample_error_matrix", "pubkey.rs:227-239", "src/bgg/sampler_gpu.rs:125-135", "US::sample_uniform"):
        assert cited in doc, cited


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "gauss_blocks_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "gauss_blocks_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 5 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    seeds = (_ffi.GpuRngSeed * 2)(_ffi.GpuRngSeed.from_bytes(bytes(range(32))), _ffi.GpuRngSeed.from_bytes(bytes(range(32, 64))))
    before = [s.to_bytes() for s in seeds]
    cols = (C.c_size_t * 2)(1, 2)
    for args in ((None, 3.5, seeds, 2, _ffi.GPUPOLY_BLOCKS_COLUMNS, cols), (None, 3.5, seeds, 2, _ffi.GPUPOLY_BLOCKS_STACKED, None),
                 (None, float("nan"), None, 0, _ffi.GPUPOLY_BLOCKS_STACKED, None)):
        assert lib.gpupoly_matrix_sample_gauss_blocks(*args) != 0
        assert SEEDED in _ffi.last_error_string()
    for args in ((None, 3.5, None, 2, _ffi.GPUPOLY_BLOCKS_COLUMNS, cols), (None, -1.0, None, 0, _ffi.GPUPOLY_BLOCKS_STACKED, None)):
        assert lib.gpupoly_matrix_sample_hash_gauss_blocks(*args) != 0
        assert HASHED in _ffi.last_error_string()
    assert [s.to_bytes() for s in seeds] == before and list(cols) == [1, 2]
