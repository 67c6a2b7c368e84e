"""CPU-only: `gpupoly_matrix_wee25_targets` (with its test instrument `gpupoly_matrix_wee25_targets_product`) is part of the
plain C ABI - declared in include/gpupoly.h, exported by libgpupoly, bound in `_ffi.SIGNATURES`; a C99 caller compiles against
the header, links, and gets an error code plus a message naming the function (never a crash) for null arguments, with its own
arrays left as they were; no blocks or no parts is success whatever else is passed."""
import os
import subprocess

TARGETS = "gpupoly_matrix_wee25_targets"
PRODUCT = "gpupoly_matrix_wee25_targets_product"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    const char *at = msg ? strstr(msg, who) : NULL;
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    /* the entry's own name: "..._targets:" is not "..._targets_product:" */
    return rc != 0 && at != NULL && at[strlen(who)] == ':';
}

int main(void) {
    GpuHashTags tags;
    GpuMatrix *outs[4] = {NULL, NULL, NULL, NULL};
    uint64_t idx[2] = {7, 9};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_TABLE;
    ok = refused(gpupoly_matrix_wee25_targets(NULL, 2, 2, NULL, 0, 1, 12, idx, &tags), "gpupoly_matrix_wee25_targets") && ok;
    ok = refused(gpupoly_matrix_wee25_targets(outs, 2, 2, NULL, 0, 1, 12, idx, &tags), "gpupoly_matrix_wee25_targets") && ok;
    ok = refused(gpupoly_matrix_wee25_targets(outs, 2, 2, NULL, 0, 1, 12, NULL, NULL), "gpupoly_matrix_wee25_targets") && ok;
    ok = refused(gpupoly_matrix_wee25_targets(outs, (size_t)-1, 2, NULL, 0, 1, 12, idx, &tags), "gpupoly_matrix_wee25_targets") && ok;
    ok = refused(gpupoly_matrix_wee25_targets_product(NULL, 2, 2, NULL, NULL, 0, 1, 12, idx), "gpupoly_matrix_wee25_targets_product") && ok;
    ok = refused(gpupoly_matrix_wee25_targets_product(outs, 2, 2, NULL, NULL, 0, 1, 12, idx), "gpupoly_matrix_wee25_targets_product") && ok;
    /* no blocks or no parts: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_wee25_targets(NULL, 0, 3, NULL, 0, 0, 0, NULL, NULL) == 0;
    ok = ok && gpupoly_matrix_wee25_targets(NULL, 3, 0, NULL, 0, 0, 0, NULL, NULL) == 0;
    ok = ok && gpupoly_matrix_wee25_targets_product(NULL, 0, 3, NULL, NULL, 0, 0, 0, NULL) == 0;
    ok = ok && gpupoly_matrix_wee25_targets_product(NULL, 3, 0, NULL, NULL, 0, 0, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && outs[2] == NULL && outs[3] == NULL && idx[0] == 7 && idx[1] == 9;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (TARGETS, PRODUCT):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    assert len(_ffi.SIGNATURES[TARGETS][1]) == 9 and len(_ffi.SIGNATURES[PRODUCT][1]) == 9
    import mxx_amd
    from mxx_amd import commit

    assert mxx_amd.commit is commit
    for name in ("build_j_2m_block", "t_top_target_block", "t_top_target_blocks", "sample_t_top_preimages", "sample_public_params", "commit_base",
                 "commit", "commit_recursive", "verifier_base", "verifier_recursive", "verifier", "open_base", "open_recursive", "open", "verify",
                 "j_2m_hit", "tag", "tags"):
        assert callable(getattr(commit.Wee25Commit, name)), name
    assert callable(mxx_amd.GpuDCRTPolyMatrix.wee25_targets)


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + TARGETS + "(")
    comment = text[text.rindex("/* ----", 0, at):at]
    for needle in ("src/commit/wee25.rs:494-758", ":696-728", ":536-584", "G_s * G^-1(X) = X", "Overlap:", "Refused", "secret_size == 0",
                   "base_bits of 0 or >= 63", "gpupoly_hash_seeds", "unsupported", "MXX_HIP_RNG_COMPAT=reference", "T = 0 or P = 0", "PACKED24",
                   "gpupoly_trapdoor_preimage_many"):
        assert needle in comment, needle
    at = text.index("int " + PRODUCT + "(")
    assert "Test instrument" in text[text.rindex("/*", 0, at):at]


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "wee25_targets_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "wee25_targets_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 6 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    tags = _ffi.GpuHashTags()
    outs = (C.c_void_p * 4)()
    idx = (C.c_uint64 * 2)(7, 9)
    for args in ((None, 2, 2, None, 0, 1, 12, idx, C.byref(tags)), (outs, 2, 2, None, 0, 1, 12, idx, C.byref(tags)),
                 (outs, 2, 2, None, 0, 1, 12, None, None), (outs, 2 ** 64 - 1, 2, None, 0, 1, 12, idx, C.byref(tags))):
        assert lib.gpupoly_matrix_wee25_targets(*args) != 0
        assert TARGETS + ":" in _ffi.last_error_string()
    for args in ((None, 2, 2, None, None, 0, 1, 12, idx), (outs, 2, 2, None, None, 0, 1, 12, idx)):
        assert lib.gpupoly_matrix_wee25_targets_product(*args) != 0
        assert PRODUCT + ":" in _ffi.last_error_string()
    assert list(idx) == [7, 9] and all(outs[i] is None for i in range(4))
    assert lib.gpupoly_matrix_wee25_targets(None, 0, 3, None, 0, 0, 0, None, None) == 0
    assert lib.gpupoly_matrix_wee25_targets(None, 3, 0, None, 0, 0, 0, None, None) == 0
    assert lib.gpupoly_matrix_wee25_targets_product(None, 0, 3, None, None, 0, 0, 0, None) == 0
