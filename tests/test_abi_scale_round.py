"""CPU-only: `gpupoly_matrix_scale_round` and `gpupoly_matrix_store_coeff_words` are part of the plain C ABI - a C99
caller compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message (never a crash) for
null arguments."""
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
    uint64_t words[4] = {0, 0, 0, 0};
    int ok = 1;
    ok = ok && refused(gpupoly_matrix_scale_round(NULL, NULL, 17u, 0), "gpupoly_matrix_scale_round");
    ok = ok && refused(gpupoly_matrix_scale_round(NULL, NULL, 0u, 1), "gpupoly_matrix_scale_round");
    ok = ok && refused(gpupoly_matrix_store_coeff_words(NULL, words, 4), "gpupoly_matrix_store_coeff_words");
    ok = ok && refused(gpupoly_matrix_store_coeff_words(NULL, NULL, 0), "gpupoly_matrix_store_coeff_words");
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "scale_round_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "scale_round_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 4 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    assert lib.gpupoly_matrix_scale_round(None, None, 3, 0) != 0
    assert "gpupoly_matrix_scale_round" in _ffi.last_error_string()
    buf = (C.c_uint64 * 2)()
    assert lib.gpupoly_matrix_store_coeff_words(None, buf, 2) != 0
    assert "gpupoly_matrix_store_coeff_words" in _ffi.last_error_string()
