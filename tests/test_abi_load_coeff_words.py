"""CPU-only: `gpupoly_matrix_load_coeff_words` is part of the plain C ABI - a C99 caller compiles against
include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming the entry (never a crash) for null
arguments.  And the lazy-accumulator bound that csrc/coeff_load.hip derives for its 32-bit Horner step, checked in integers."""
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
    const uint64_t words[4] = {1, 2, 3, 4};
    int ok = 1;
    ok = ok && refused(gpupoly_matrix_load_coeff_words(NULL, words, 2, 2, GPU_POLY_FORMAT_COEFF), "gpupoly_matrix_load_coeff_words");
    ok = ok && refused(gpupoly_matrix_load_coeff_words(NULL, NULL, 0, 0, GPU_POLY_FORMAT_EVAL), "gpupoly_matrix_load_coeff_words");
    ok = ok && refused(gpupoly_matrix_load_coeff_words(NULL, NULL, 1, 1, 7), "gpupoly_matrix_load_coeff_words");
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "load_coeff_words_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "load_coeff_words_null"
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

    assert "gpupoly_matrix_load_coeff_words" in _ffi.SIGNATURES
    lib = _ffi.lib()
    buf = (C.c_uint64 * 2)()
    assert lib.gpupoly_matrix_load_coeff_words(None, buf, 2, 1, 0) != 0
    assert "gpupoly_matrix_load_coeff_words" in _ffi.last_error_string()
    assert lib.gpupoly_matrix_load_coeff_words(None, None, 1, 0, 1) != 0
    assert "gpupoly_matrix_load_coeff_words" in _ffi.last_error_string()


def test_lazy_accumulator_bound_of_the_32_bit_horner_step():
    """acc = r P_T + sum_{0<j<T} h_j P_j + h_0 with r, P_j <= q - 1 and h_j <= 2^32 - 1 fits 64 bits for the words per
    step S = T / 2 the kernel picks from the widest modulus (<= 29 bits: 4, 30: 2, 31: 1), and the next S would not."""
    def worst(bits, S):
        q, h, T = (1 << bits) - 1, (1 << 32) - 1, 2 * S
        return (q - 1) ** 2 + (T - 1) * h * (q - 1) + h

    for bits, S in ((29, 4), (30, 2), (31, 1)):
        assert worst(bits, S) < 1 << 64
    assert worst(31, 2) >= 1 << 64 and worst(30, 4) >= 1 << 64
    assert worst(28, 4) < 1 << 63
