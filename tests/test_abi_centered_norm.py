"""CPU-only: `gpupoly_matrix_centered_max_abs` is part of the plain C ABI - a C99 caller compiles against
include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming the function (never a crash) for null
arguments, with its output buffer left untouched."""
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
    uint64_t words[4] = {7u, 7u, 7u, 7u};
    int ok = 1, w;
    ok = ok && refused(gpupoly_matrix_centered_max_abs(NULL, words, 4), "gpupoly_matrix_centered_max_abs");
    ok = ok && refused(gpupoly_matrix_centered_max_abs(NULL, NULL, 0), "gpupoly_matrix_centered_max_abs");
    ok = ok && refused(gpupoly_matrix_centered_max_abs(NULL, words, 0), "gpupoly_matrix_centered_max_abs");
    for (w = 0; w < 4; ++w) ok = ok && words[w] == 7u;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "centered_norm_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "centered_norm_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 3 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    buf = (C.c_uint64 * 2)(11, 12)
    assert lib.gpupoly_matrix_centered_max_abs(None, buf, 2) != 0
    assert "gpupoly_matrix_centered_max_abs" in _ffi.last_error_string()
    assert list(buf) == [11, 12]


def test_axis_forms_of_the_host_reduction():
    from mxx_amd.matrix import _max_along

    e = [[3, 9, 1], [7, 2, 8]]
    assert _max_along(e, None, 2, 3) == 9
    assert _max_along(e, 1, 2, 3) == [9, 8]
    assert _max_along(e, 0, 2, 3) == [7, 9, 8]
    assert _max_along(e, "entries", 2, 3) is e
    assert _max_along([[], []], None, 2, 0) == 0 and _max_along([[], []], 1, 2, 0) == [0, 0]
    assert _max_along([], 0, 0, 3) == [0, 0, 0] and _max_along([], 1, 0, 3) == []
    for bad in ("rows", 2, -1):
        try:
            _max_along(e, bad, 2, 3)
        except ValueError:
            continue
        raise AssertionError(f"axis={bad!r} accepted")
