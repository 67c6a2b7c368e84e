"""CPU-only: gpupoly_matrix_mul_decompose_many is part of the plain C ABI - a C99 caller compiles against include/gpupoly.h,
links libgpupoly, and gets an error code plus a message that names the function (never a crash) for null arrays and a null
right operand; n = 0 does nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpupoly_matrix_mul_decompose_many"

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(const char *what, int rc) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", what, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, "gpupoly_matrix_mul_decompose_many") != NULL;
}

int main(void) {
    GpuMatrix *const outs[1] = {NULL};
    const GpuMatrix *const lhss[1] = {NULL};
    int rc, ok = 1;
    ok = refused("null arrays", gpupoly_matrix_mul_decompose_many(NULL, NULL, NULL, NULL, 1, NULL, 12)) && ok;
    ok = refused("null outs", gpupoly_matrix_mul_decompose_many(NULL, lhss, NULL, NULL, 1, NULL, 12)) && ok;
    ok = refused("null lhss", gpupoly_matrix_mul_decompose_many(outs, NULL, NULL, NULL, 1, NULL, 12)) && ok;
    ok = refused("null rhs", gpupoly_matrix_mul_decompose_many(outs, lhss, NULL, NULL, 1, NULL, 12)) && ok;
    rc = gpupoly_matrix_mul_decompose_many(NULL, NULL, NULL, NULL, 0, NULL, 12);
    printf("n=0 rc=%d\n", rc);
    ok = ok && rc == 0;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "mul_decompose_many_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "mul_decompose_many_null"
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

    lib = _ffi.lib()
    one = (C.c_void_p * 1)(None)
    assert lib.gpupoly_matrix_mul_decompose_many(None, None, None, None, 1, None, 12) != 0
    assert NAME in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_many(one, None, None, None, 1, None, 12) != 0
    assert NAME in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_many(one, one, None, None, 1, None, 12) != 0  # null rhs
    assert NAME in _ffi.last_error_string() and "rhs" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_many(None, None, None, None, 0, None, 12) == 0


def test_header_states_the_refusals_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + NAME)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("src/bgg/encoding.rs:125-145", "src/bgg/poly_encoding.rs:327-357", "Refused", "aliases", "base_bits of 0 or >= 63"):
        assert needle in comment, needle
