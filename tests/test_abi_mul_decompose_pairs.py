"""CPU-only: gpupoly_matrix_mul_decompose_pairs is part of the plain C ABI - declared in include/gpupoly.h with the reference
lines it replaces, exported by the library, bound in _ffi.SIGNATURES; a C99 caller compiles against the header, links
libgpupoly, and gets an error code plus a message that names the function (never a crash) for null arrays with n > 0, its own
arrays left as they were; n = 0 does nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpupoly_matrix_mul_decompose_pairs"

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(const char *what, int rc) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", what, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, "gpupoly_matrix_mul_decompose_pairs") != NULL;
}

int main(void) {
    GpuMatrix *outs[2] = {NULL, NULL};
    const GpuMatrix *lhss[2] = {NULL, NULL};
    const GpuMatrix *rhss[2] = {NULL, NULL};
    int rc, ok = 1;
    ok = refused("null arrays", gpupoly_matrix_mul_decompose_pairs(NULL, NULL, NULL, NULL, NULL, 2, 0, 12, 0)) && ok;
    ok = refused("null outs", gpupoly_matrix_mul_decompose_pairs(NULL, NULL, lhss, rhss, NULL, 2, 0, 12, 0)) && ok;
    ok = refused("null lhss", gpupoly_matrix_mul_decompose_pairs(outs, NULL, NULL, rhss, NULL, 2, 0, 12, 1)) && ok;
    ok = refused("null rhss", gpupoly_matrix_mul_decompose_pairs(outs, NULL, lhss, NULL, NULL, 2, 0, 12, 0)) && ok;
    ok = refused("null entries", gpupoly_matrix_mul_decompose_pairs(outs, NULL, lhss, rhss, NULL, 2, 0, 12, 0)) && ok;
    /* the caller's arrays are read, never written */
    ok = ok && outs[0] == NULL && outs[1] == NULL && lhss[0] == NULL && lhss[1] == NULL && rhss[0] == NULL && rhss[1] == NULL;
    rc = gpupoly_matrix_mul_decompose_pairs(NULL, NULL, NULL, NULL, NULL, 0, 0, 12, 0);
    printf("n=0 rc=%d\n", rc);
    ok = ok && rc == 0;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "mul_decompose_pairs_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "mul_decompose_pairs_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])


def test_binding_reports_null_arguments_as_errors_and_takes_n_zero():
    import ctypes as C

    from mxx_amd import _ffi

    assert NAME in _ffi.SIGNATURES
    lib = _ffi.lib()
    two = lambda: (C.c_void_p * 2)(None, None)
    for args in [(None, None, None, None, None), (None, None, two(), two(), None), (two(), None, None, two(), None),
                 (two(), None, two(), None, None), (two(), two(), two(), two(), two())]:
        assert lib.gpupoly_matrix_mul_decompose_pairs(*args, 2, 0, 12, 0) != 0
        assert NAME in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_pairs(None, None, None, None, None, 0, 0, 12, 1) == 0


def test_header_states_the_refusals_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + NAME)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("bgg_pubkey_gpu.rs:371-407,409-471", ":842", "Refused", "aliases", "base_bits of 0 or >= 63",
                   "multiplies the PRODUCT", "gpupoly_matrix_mul_decompose_many", "MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET"):
        assert needle in comment, needle
