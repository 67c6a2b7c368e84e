"""CPU-only: `gpupoly_matrix_crt_recompose_rounded` is part of the plain C ABI - a C99 caller compiles against
include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming the function (never a crash) for null
arguments - and the params classes carry the CRT reconstruction coefficients the recomposition is defined by
(`reconst_coeffs` / `to_crt_coeffs`, src/poly/mod.rs:45-76)."""
import math
import os
import random
import subprocess

NAME = "gpupoly_matrix_crt_recompose_rounded"
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
    const GpuMatrix *terms[2] = {NULL, NULL};
    int signs[2] = {1, -1};
    int ok = 1;
    ok = ok && refused(gpupoly_matrix_crt_recompose_rounded(NULL, NULL, NULL, 0, 0), "gpupoly_matrix_crt_recompose_rounded");
    ok = ok && refused(gpupoly_matrix_crt_recompose_rounded(NULL, terms, signs, 2, 1), "gpupoly_matrix_crt_recompose_rounded");
    ok = ok && refused(gpupoly_matrix_crt_recompose_rounded(NULL, terms, NULL, 1, 2), "gpupoly_matrix_crt_recompose_rounded");
    ok = ok && refused(gpupoly_matrix_crt_recompose_rounded(NULL, NULL, signs, 1, 2), "gpupoly_matrix_crt_recompose_rounded");
    ok = ok && signs[0] == 1 && signs[1] == -1 && terms[0] == NULL && terms[1] == NULL;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "crt_recompose_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "crt_recompose_null"
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
    terms = (C.c_void_p * 2)(None, None)
    signs = (C.c_int * 2)(1, -1)
    for args in ((None, None, None, 0, 0), (None, terms, signs, 2, 1), (None, terms, None, 1, 2), (None, None, signs, 1, 2)):
        assert lib.gpupoly_matrix_crt_recompose_rounded(*args) != 0
        assert NAME in _ffi.last_error_string()
    assert list(signs) == [1, -1] and list(terms) == [None, None]


def test_entry_is_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    assert f"int {NAME}(" in header
    assert NAME in _ffi.SIGNATURES and hasattr(_ffi.lib(), NAME)


def test_reconstruction_coefficients_of_the_cpu_params():
    from mxx_amd.params import DCRTPolyParams

    rnd = random.Random(20261019)
    for n, depth, bits in ((2, 2, 10), (16, 1, 24), (64, 5, 28), (32, 4, 51), (16, 9, 60)):
        p = DCRTPolyParams(n, depth, bits, 1)
        moduli, _, d = p.to_crt()
        Q = p.modulus()
        assert d == depth and Q == math.prod(moduli)
        es = p.reconst_coeffs()
        assert len(es) == depth
        for i, (qi, e) in enumerate(zip(moduli, es)):
            assert 0 <= e < Q
            assert [e % q for q in moduli] == [1 if j == i else 0 for j in range(depth)]  # e_i = delta_ij mod q_j
            q_over_qi, coeff = p.to_crt_coeffs(i)
            assert q_over_qi == Q // qi and q_over_qi * qi == Q and coeff == e
        for _ in range(8):  # sum_i v_i e_i mod Q has the residues v_j
            vs = [rnd.randrange(q) for q in moduli]
            x = sum(v * e for v, e in zip(vs, es)) % Q
            assert [x % q for q in moduli] == vs
