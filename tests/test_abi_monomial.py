"""CPU-only: gpupoly_matrix_fill_monomial, gpupoly_matrix_mul_monomial and gpupoly_matrix_monomial_sum are part of the plain
C ABI - a C99 caller compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming
the function (never a crash) for null arguments."""
import os
import subprocess

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
    uint64_t shifts[2] = {1u, 2u};
    const GpuMatrix *mats[2] = {NULL, NULL};
    int ok = 1;
    ok = ok && refused(gpupoly_matrix_fill_monomial(NULL, 3u, GPU_POLY_FORMAT_EVAL), "gpupoly_matrix_fill_monomial");
    ok = ok && refused(gpupoly_matrix_fill_monomial(NULL, 3u, 7), "gpupoly_matrix_fill_monomial");
    ok = ok && refused(gpupoly_matrix_mul_monomial(NULL, NULL, 1u), "gpupoly_matrix_mul_monomial");
    ok = ok && refused(gpupoly_matrix_monomial_sum(NULL, NULL, NULL, NULL, 0, 0), "gpupoly_matrix_monomial_sum");
    ok = ok && refused(gpupoly_matrix_monomial_sum(NULL, NULL, mats, shifts, 2, 1), "gpupoly_matrix_monomial_sum");
    ok = ok && shifts[0] == 1u && shifts[1] == 2u;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "monomial_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "monomial_null"
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
    assert lib.gpupoly_matrix_fill_monomial(None, 5, _ffi.GPU_POLY_FORMAT_COEFF) != 0
    assert "gpupoly_matrix_fill_monomial" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_monomial(None, None, 5) != 0
    assert "gpupoly_matrix_mul_monomial" in _ffi.last_error_string()
    shifts = (C.c_uint64 * 2)(11, 12)
    mats = (C.c_void_p * 2)(None, None)
    assert lib.gpupoly_matrix_monomial_sum(None, None, mats, shifts, 2, 0) != 0
    assert "gpupoly_matrix_monomial_sum" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_monomial_sum(None, None, None, None, 0, 1) != 0
    assert "gpupoly_matrix_monomial_sum" in _ffi.last_error_string()
    assert list(shifts) == [11, 12]
