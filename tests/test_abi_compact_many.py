"""CPU-only: the batched compact-bytes entries are part of the plain C ABI - a C99 caller compiles against include/gpupoly.h,
links libgpupoly, and gets an error code plus a message (never a crash) for bad arguments; n = 0 does nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

int main(void) {
    size_t total = 77;
    const char *msg;
    int rc, ok = 1;
    rc = gpupoly_matrix_store_compact_bytes_many(NULL, 1, NULL, 0, NULL, NULL, NULL, NULL, &total);
    msg = gpu_last_error();
    printf("store rc=%d msg=%s\n", rc, msg ? msg : "(null)");
    ok = ok && rc != 0 && msg != NULL && strstr(msg, "gpupoly_matrix_store_compact_bytes_many") != NULL && total == 77;
    rc = gpupoly_matrix_load_compact_bytes_many(NULL, 1, NULL, NULL, NULL);
    msg = gpu_last_error();
    printf("load rc=%d msg=%s\n", rc, msg ? msg : "(null)");
    ok = ok && rc != 0 && msg != NULL && strstr(msg, "gpupoly_matrix_load_compact_bytes_many") != NULL;
    rc = gpupoly_matrix_store_compact_bytes_many(NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, &total);
    printf("store n=0 rc=%d total=%lu\n", rc, (unsigned long)total);
    ok = ok && rc == 0 && total == 0;
    rc = gpupoly_matrix_load_compact_bytes_many(NULL, 0, NULL, NULL, NULL);
    printf("load n=0 rc=%d\n", rc);
    ok = ok && rc == 0;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arrays(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "compact_many_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "compact_many_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])


def test_binding_reports_null_arrays_as_errors_and_takes_n_zero():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    total = C.c_size_t(5)
    assert lib.gpupoly_matrix_store_compact_bytes_many(None, 1, None, 0, None, None, None, None, C.byref(total)) != 0
    assert "gpupoly_matrix_store_compact_bytes_many" in _ffi.last_error_string()
    assert total.value == 5
    assert lib.gpupoly_matrix_load_compact_bytes_many(None, 1, None, None, None) != 0
    assert "gpupoly_matrix_load_compact_bytes_many" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_store_compact_bytes_many(None, 0, None, 0, None, None, None, None, C.byref(total)) == 0
    assert total.value == 0
    assert lib.gpupoly_matrix_load_compact_bytes_many(None, 0, None, None, None) == 0
