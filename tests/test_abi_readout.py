"""CPU-only: `gpupoly_matrix_extract_bits` and `gpupoly_matrix_store_coeff_ints` are part of the plain C ABI - a C99
caller compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming the function
(never a crash) for null arguments, with its buffers left untouched."""
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
    uint64_t lo[2] = {1u, 0u}, hi[2] = {9u, 0u}, count = 77u, first = 78u;
    uint8_t bits[4] = {7u, 7u, 7u, 7u};
    uint32_t ints[4] = {7u, 7u, 7u, 7u};
    int ok = 1, w;
    ok = ok && refused(gpupoly_matrix_extract_bits(NULL, lo, hi, 2, bits, 4), "gpupoly_matrix_extract_bits");
    ok = ok && refused(gpupoly_matrix_extract_bits(NULL, NULL, NULL, 0, NULL, 0), "gpupoly_matrix_extract_bits");
    ok = ok && refused(gpupoly_matrix_extract_bits(NULL, lo, hi, 0, bits, 0), "gpupoly_matrix_extract_bits");
    ok = ok && refused(gpupoly_matrix_store_coeff_ints(NULL, ints, 4, 0, 4, &count, &first), "gpupoly_matrix_store_coeff_ints");
    ok = ok && refused(gpupoly_matrix_store_coeff_ints(NULL, ints, 3, 1, 4, &count, &first), "gpupoly_matrix_store_coeff_ints");
    ok = ok && refused(gpupoly_matrix_store_coeff_ints(NULL, NULL, 8, 1, 0, NULL, NULL), "gpupoly_matrix_store_coeff_ints");
    for (w = 0; w < 4; ++w) ok = ok && bits[w] == 7u && ints[w] == 7u;
    ok = ok && count == 77u && first == 78u && lo[0] == 1u && hi[0] == 9u;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "readout_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "readout_null"
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
    lo, hi = (C.c_uint64 * 1)(3), (C.c_uint64 * 1)(5)
    bits = (C.c_uint8 * 2)(11, 12)
    assert lib.gpupoly_matrix_extract_bits(None, lo, hi, 1, bits, 2) != 0
    assert "gpupoly_matrix_extract_bits" in _ffi.last_error_string()
    assert list(bits) == [11, 12] and lo[0] == 3 and hi[0] == 5
    ints = (C.c_uint64 * 2)(11, 12)
    count, first = C.c_uint64(21), C.c_uint64(22)
    for args in ((None, C.cast(ints, C.c_void_p), 8, 0, 2, C.byref(count), C.byref(first)),
                 (None, None, 8, 0, 2, C.byref(count), C.byref(first)),
                 (None, C.cast(ints, C.c_void_p), 8, 1, 2, None, None)):
        assert lib.gpupoly_matrix_store_coeff_ints(*args) != 0
        assert "gpupoly_matrix_store_coeff_ints" in _ffi.last_error_string()
    assert list(ints) == [11, 12] and count.value == 21 and first.value == 22


def test_both_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in ("gpupoly_matrix_extract_bits", "gpupoly_matrix_store_coeff_ints"):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
