"""CPU-only: gpupoly_matrix_mul_sum and gpupoly_matrix_mul_acc are part of the plain C ABI - a C99 caller compiles against
include/gpupoly.h, links libgpupoly, and gets an error code plus a message that names the entry (never a crash) for null
matrices and, with n > 0, null arrays."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM, ACC = "gpupoly_matrix_mul_sum", "gpupoly_matrix_mul_acc"

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
    const GpuMatrix *const none[1] = {NULL};
    int ok = 1;
    ok = refused("sum: null out", "gpupoly_matrix_mul_sum", gpupoly_matrix_mul_sum(NULL, 0, 0, NULL, NULL, NULL, 0, 0)) && ok;
    ok = refused("sum: null out, null arrays", "gpupoly_matrix_mul_sum", gpupoly_matrix_mul_sum(NULL, 0, 3, NULL, NULL, NULL, 2, 1)) && ok;
    ok = refused("sum: null out, null terms", "gpupoly_matrix_mul_sum", gpupoly_matrix_mul_sum(NULL, 0, 3, NULL, none, none, 1, 0)) && ok;
    ok = refused("acc: all null", "gpupoly_matrix_mul_acc", gpupoly_matrix_mul_acc(NULL, NULL, NULL, 0)) && ok;
    ok = refused("acc: all null, negate", "gpupoly_matrix_mul_acc", gpupoly_matrix_mul_acc(NULL, NULL, NULL, 1)) && ok;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "mul_sum_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "mul_sum_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])


def test_binding_reports_null_arguments_as_errors():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    one = (C.c_void_p * 1)(None)
    assert lib.gpupoly_matrix_mul_sum(None, 0, 0, None, None, None, 0, 0) != 0
    assert SUM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_sum(None, 0, 1, None, None, None, 1, 0) != 0
    assert SUM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_sum(None, 0, 1, None, one, one, 1, 1) != 0
    assert SUM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_acc(None, None, None, 0) != 0
    assert ACC in _ffi.last_error_string()


def test_header_states_the_rule_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + SUM)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("src/lookup/ggh15/encoding.rs:205-298", "src/lookup/ggh15/pubkey_gpu.rs:408", "src/lookup/lwe/encoding_gpu.rs:142-223",
                   "src/sampler/trapdoor/gpu.rs:212", "Refused", "overlap", "dst_col + cols > out->cols"):
        assert needle in comment, needle
    rule = text[:text.index("#ifndef GPUPOLY_H")]
    assert SUM in rule and ACC in rule, "the conventions' overlap rule names the new entries"
