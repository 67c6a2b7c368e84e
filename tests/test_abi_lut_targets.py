"""CPU-only: `gpupoly_matrix_sample_decomposed_blocks`, `gpupoly_matrix_sample_hash_decomposed_blocks` and
`gpupoly_matrix_lut_targets` (with its test instrument `gpupoly_matrix_lut_targets_combine`) are part of the plain C ABI -
declared in include/gpupoly.h, exported by libgpupoly, bound in `_ffi.SIGNATURES`; a C99 caller compiles against the header,
links, and gets an error code plus a message naming the function (never a crash) for null arguments, with its own arrays
left as they were."""
import os
import subprocess

BLOCKS = "gpupoly_matrix_sample_decomposed_blocks"
HASH_BLOCKS = "gpupoly_matrix_sample_hash_decomposed_blocks"
TARGETS = "gpupoly_matrix_lut_targets"
COMBINE = "gpupoly_matrix_lut_targets_combine"
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
    GpuHashTags tags;
    GpuMatrix *outs[2] = {NULL, NULL};
    uint64_t y[2] = {7, 9}, idx[2] = {0, 1};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_INDEXED_DECIMAL;
    ok = ok && refused(gpupoly_matrix_sample_decomposed_blocks(NULL, GPU_MATRIX_DIST_UNIFORM, seeds, 2, 12, 0, 1, 4, 0),
                       "gpupoly_matrix_sample_decomposed_blocks");
    ok = ok && refused(gpupoly_matrix_sample_decomposed_blocks(NULL, GPU_MATRIX_DIST_BIT, NULL, 0, 0, 1, 0, 0, 0),
                       "gpupoly_matrix_sample_decomposed_blocks");
    ok = ok && refused(gpupoly_matrix_sample_hash_decomposed_blocks(NULL, GPU_MATRIX_DIST_UNIFORM, &tags, 2, 12, 0, 1, 4, 0),
                       "gpupoly_matrix_sample_hash_decomposed_blocks");
    ok = ok && refused(gpupoly_matrix_sample_hash_decomposed_blocks(NULL, GPU_MATRIX_DIST_TERNARY, NULL, 2, 12, 0, 1, 4, 0),
                       "gpupoly_matrix_sample_hash_decomposed_blocks");
    ok = ok && refused(gpupoly_matrix_lut_targets(NULL, 2, NULL, NULL, NULL, NULL, 0, 12, y, 1, idx, &tags), "gpupoly_matrix_lut_targets");
    ok = ok && refused(gpupoly_matrix_lut_targets(outs, 2, NULL, NULL, NULL, NULL, 0, 12, y, 1, idx, &tags), "gpupoly_matrix_lut_targets");
    ok = ok && refused(gpupoly_matrix_lut_targets(outs, 2, NULL, NULL, NULL, NULL, 0, 12, NULL, 1, NULL, NULL), "gpupoly_matrix_lut_targets");
    ok = ok && refused(gpupoly_matrix_lut_targets_combine(outs, 2, NULL, NULL, NULL, 0, 12, y, 1, idx), "gpupoly_matrix_lut_targets_combine");
    /* no rows: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_lut_targets(NULL, 0, NULL, NULL, NULL, NULL, 0, 0, NULL, 0, NULL, NULL) == 0;
    ok = ok && gpupoly_matrix_lut_targets_combine(NULL, 0, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && y[0] == 7 && y[1] == 9 && idx[0] == 0 && idx[1] == 1;
    ok = ok && seeds[0].words[0] == 1 && seeds[0].words[3] == 4 && seeds[1].words[0] == 5 && seeds[1].words[3] == 8;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (BLOCKS, HASH_BLOCKS, TARGETS, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    import mxx_amd
    from mxx_amd import lookup

    assert mxx_amd.lookup is lookup
    for name in ("build_lut_preimage_target_chunk", "lut_preimage_target_chunks", "sample_lut_preimages"):
        assert callable(getattr(lookup, name))
    for name in ("sample_decomposed_blocks", "sample_hash_decomposed_blocks", "lut_targets"):
        assert callable(getattr(mxx_amd.GpuDCRTPolyMatrix, name))
    assert callable(mxx_amd.GpuDCRTPolyHashSampler.sample_hash_decomposed_columns_many)


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "lut_targets_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "lut_targets_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 8 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    seeds = (_ffi.GpuRngSeed * 2)(_ffi.GpuRngSeed.from_bytes(bytes(range(32))), _ffi.GpuRngSeed.from_bytes(bytes(range(32, 64))))
    before = [s.to_bytes() for s in seeds]
    for args in ((None, 0, seeds, 2, 12, 0, 1, 4, 0), (None, 3, None, 0, 0, 1, 0, 0, 0)):
        assert lib.gpupoly_matrix_sample_decomposed_blocks(*args) != 0
        assert BLOCKS in _ffi.last_error_string()
    assert [s.to_bytes() for s in seeds] == before
    tags = _ffi.GpuHashTags()
    for args in ((None, 0, C.byref(tags), 2, 12, 0, 1, 4, 0), (None, 0, None, 2, 12, 0, 1, 4, 0)):
        assert lib.gpupoly_matrix_sample_hash_decomposed_blocks(*args) != 0
        assert HASH_BLOCKS in _ffi.last_error_string()
    outs = (C.c_void_p * 2)()
    y, idx = (C.c_uint64 * 2)(7, 9), (C.c_uint64 * 2)(0, 1)
    for args in ((None, 2, None, None, None, None, 0, 12, y, 1, idx, C.byref(tags)), (outs, 2, None, None, None, None, 0, 12, y, 1, idx, C.byref(tags)),
                 (outs, 2, None, None, None, None, 0, 12, None, 1, None, None)):
        assert lib.gpupoly_matrix_lut_targets(*args) != 0
        assert TARGETS in _ffi.last_error_string()
    assert lib.gpupoly_matrix_lut_targets_combine(outs, 2, None, None, None, 0, 12, y, 1, idx) != 0
    assert COMBINE in _ffi.last_error_string()
    assert list(y) == [7, 9] and list(idx) == [0, 1] and outs[0] is None and outs[1] is None
    assert lib.gpupoly_matrix_lut_targets(None, 0, None, None, None, None, 0, 0, None, 0, None, None) == 0
