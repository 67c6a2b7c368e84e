"""CPU-only: gpupoly_matrix_mul_decompose_gadget_scalar_many and gpupoly_matrix_mul_decompose_gadget_const_many are part of
the plain C ABI - a C99 caller compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message
that names the entry (never a crash) for null arguments; the header states their rule and the reference lines they replace."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SM, CM = "gpupoly_matrix_mul_decompose_gadget_scalar_many", "gpupoly_matrix_mul_decompose_gadget_const_many"

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(const char *what, const char *entry, int rc) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", what, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, entry) != NULL;
}

int main(void) {
    int ok = 1;
    GpuMatrix *outs[1] = {NULL};
    const GpuMatrix *lhss[1] = {NULL};
    uint64_t words[1] = {5};
    const char *sm = "gpupoly_matrix_mul_decompose_gadget_scalar_many", *cm = "gpupoly_matrix_mul_decompose_gadget_const_many";
    ok = refused("scalar: all null", sm, gpupoly_matrix_mul_decompose_gadget_scalar_many(NULL, NULL, NULL, 1, NULL, 0, 6)) && ok;
    ok = refused("scalar: null scalar", sm, gpupoly_matrix_mul_decompose_gadget_scalar_many(outs, lhss, NULL, 1, NULL, 1, 6)) && ok;
    ok = refused("const: all null", cm, gpupoly_matrix_mul_decompose_gadget_const_many(NULL, NULL, NULL, 1, NULL, 0, 0, 6)) && ok;
    ok = refused("const: null arrays", cm, gpupoly_matrix_mul_decompose_gadget_const_many(NULL, NULL, NULL, 2, words, 1, 0, 6)) && ok;
    ok = refused("const: no words", cm, gpupoly_matrix_mul_decompose_gadget_const_many(outs, lhss, NULL, 1, words, 0, 1, 6)) && ok;
    ok = refused("const: null matrices", cm, gpupoly_matrix_mul_decompose_gadget_const_many(outs, lhss, NULL, 1, words, 1, 0, 6)) && ok;
    ok = refused("const: base 0", cm, gpupoly_matrix_mul_decompose_gadget_const_many(outs, lhss, NULL, 1, words, 1, 0, 0)) && ok;
    /* n = 0 does nothing */
    ok = (gpupoly_matrix_mul_decompose_gadget_const_many(NULL, NULL, NULL, 0, NULL, 0, 0, 6) == 0) && ok;
    ok = (gpupoly_matrix_mul_decompose_gadget_scalar_many(NULL, NULL, NULL, 0, NULL, 0, 6) == 0) && ok;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "gadget_scalar_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "gadget_scalar_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])


def test_binding_reports_null_arguments_as_errors():
    from mxx_amd import _ffi

    lib = _ffi.lib()
    one = (C.c_void_p * 1)(None)
    words = (C.c_uint64 * 1)(5)
    assert lib.gpupoly_matrix_mul_decompose_gadget_scalar_many(None, None, None, 1, None, 0, 6) != 0
    assert SM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_scalar_many(one, one, None, 1, None, 0, 6) != 0
    assert SM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_const_many(None, None, None, 1, words, 1, 0, 6) != 0
    assert CM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_const_many(one, one, None, 1, None, 1, 0, 6) != 0
    assert CM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_const_many(one, one, None, 1, words, 0, 0, 6) != 0
    assert CM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_const_many(one, one, None, 1, words, 1, 0, 6) != 0
    assert CM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_decompose_gadget_const_many(None, None, None, 0, None, 0, 0, 6) == 0


def test_header_states_the_rule_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for entry in (SM, CM):
        at = text.index("int " + entry)
        comment = text[text.rindex("/*", 0, at):at]
        for needle in ("Refused", "overlap", "src/bgg/encoding.rs:191", "src/bgg/public_key.rs:134", "src/bgg/poly_encoding.rs:431"):
            assert needle in comment, (entry, needle)
    rule = text[:text.index("#ifndef GPUPOLY_H")]
    assert SM in rule and CM in rule, "the conventions' overlap rule names the new entries"


def test_the_mirror_has_the_methods():
    from mxx_amd.matrix import GpuDCRTPolyMatrix as M

    for name in ("large_scalar_mul", "large_scalar_mul_many", "_large_scalar_mul_host"):
        assert callable(getattr(M, name))
