"""CPU-only: `gpupoly_matrix_lwe_targets` (with its test instrument `gpupoly_matrix_lwe_targets_combine`) is part of the plain
C ABI - declared in include/gpupoly.h, exported by libgpupoly, bound in `_ffi.SIGNATURES`; a C99 caller compiles against the
header, links, and gets an error code plus a message naming the function (never a crash) for null arguments, with its own
arrays left as they were; no rows is success whatever else is passed."""
import os
import subprocess

TARGETS = "gpupoly_matrix_lwe_targets"
COMBINE = "gpupoly_matrix_lwe_targets_combine"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    const char *at = msg ? strstr(msg, who) : NULL;
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    /* the entry's own name: "..._targets:" is not "..._targets_combine:" */
    return rc != 0 && at != NULL && at[strlen(who)] == ':';
}

int main(void) {
    GpuHashTags tags;
    GpuMatrix *outs[2] = {NULL, NULL};
    uint64_t y[2] = {7, 9}, x[2] = {0, 1};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_TABLE;
    ok = refused(gpupoly_matrix_lwe_targets(NULL, 2, NULL, NULL, 0, 12, y, 1, x, &tags), "gpupoly_matrix_lwe_targets") && ok;
    ok = refused(gpupoly_matrix_lwe_targets(outs, 2, NULL, NULL, 0, 12, y, 1, x, &tags), "gpupoly_matrix_lwe_targets") && ok;
    ok = refused(gpupoly_matrix_lwe_targets(outs, 2, NULL, NULL, 0, 12, NULL, 1, NULL, NULL), "gpupoly_matrix_lwe_targets") && ok;
    ok = refused(gpupoly_matrix_lwe_targets_combine(NULL, 2, NULL, NULL, NULL, 0, 12, y, 1, x), "gpupoly_matrix_lwe_targets_combine") && ok;
    ok = refused(gpupoly_matrix_lwe_targets_combine(outs, 2, NULL, NULL, NULL, 0, 12, y, 1, x), "gpupoly_matrix_lwe_targets_combine") && ok;
    /* no rows: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_lwe_targets(NULL, 0, NULL, NULL, 0, 0, NULL, 0, NULL, NULL) == 0;
    ok = ok && gpupoly_matrix_lwe_targets_combine(NULL, 0, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && y[0] == 7 && y[1] == 9 && x[0] == 0 && x[1] == 1;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (TARGETS, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    assert len(_ffi.SIGNATURES[TARGETS][1]) == 10 and len(_ffi.SIGNATURES[COMBINE][1]) == 10
    import mxx_amd
    from mxx_amd import lwe_lookup

    assert mxx_amd.lwe_lookup is lwe_lookup
    for name in ("LweShared", "derive_a_lt_matrix", "derive_k_low_chunk", "build_adjusted_target_chunk", "lwe_target_chunks",
                 "sample_lwe_preimages", "public_lookup"):
        assert callable(getattr(lwe_lookup, name))
    assert callable(mxx_amd.GpuDCRTPolyMatrix.lwe_targets)


def test_the_tags_are_the_reference_strings():
    from mxx_amd import lwe_lookup

    sh = lwe_lookup.LweShared(None, bytes(32), 7, 3, None, None, None)
    assert sh.tag(12) == b"LWE_R_G_7_3_12_slot0"
    assert lwe_lookup.LweShared(None, bytes(32), 7, 3, 5, None, None).tags([0, 41]) == [b"LWE_R_G_7_3_0_slot5", b"LWE_R_G_7_3_41_slot5"]


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + TARGETS + "(")
    comment = text[text.rindex("/* ----", 0, at):at]
    for needle in ("src/lookup/lwe/pubkey_gpu.rs:397-520", ":193-222", "G_d * G^-1(U) = U", "Overlap:", "Refused", "words_per_y == 0",
                   "base_bits of 0 or >= 63", "gpupoly_hash_seeds", "unsupported", "MXX_HIP_RNG_COMPAT=reference", "T = 0", "PACKED24",
                   "gpupoly_trapdoor_preimage_many"):
        assert needle in comment, needle
    at = text.index("int " + COMBINE + "(")
    assert "Test instrument" in text[text.rindex("/*", 0, at):at]


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "lwe_targets_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "lwe_targets_null"
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
    tags = _ffi.GpuHashTags()
    outs = (C.c_void_p * 2)()
    y, x = (C.c_uint64 * 2)(7, 9), (C.c_uint64 * 2)(0, 1)
    for args in ((None, 2, None, None, 0, 12, y, 1, x, C.byref(tags)), (outs, 2, None, None, 0, 12, y, 1, x, C.byref(tags)),
                 (outs, 2, None, None, 0, 12, None, 1, None, None)):
        assert lib.gpupoly_matrix_lwe_targets(*args) != 0
        assert TARGETS + ":" in _ffi.last_error_string()
    for args in ((None, 2, None, None, None, 0, 12, y, 1, x), (outs, 2, None, None, None, 0, 12, y, 1, x)):
        assert lib.gpupoly_matrix_lwe_targets_combine(*args) != 0
        assert COMBINE + ":" in _ffi.last_error_string()
    assert list(y) == [7, 9] and list(x) == [0, 1] and outs[0] is None and outs[1] is None
    assert lib.gpupoly_matrix_lwe_targets(None, 0, None, None, 0, 0, None, 0, None, None) == 0
    assert lib.gpupoly_matrix_lwe_targets_combine(None, 0, None, None, None, 0, 0, None, 0, None) == 0
