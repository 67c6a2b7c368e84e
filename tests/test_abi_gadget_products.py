"""CPU-only: gpupoly_matrix_mul_gadget and gpupoly_matrix_gadget_mul are part of the plain C ABI - a C99 caller compiles
against include/gpupoly.h, links libgpupoly, and gets an error code plus a message that names the entry (never a crash) for
null matrices; the header states their rule and the reference lines they replace."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG, GM = "gpupoly_matrix_mul_gadget", "gpupoly_matrix_gadget_mul"

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
    ok = refused("mul_gadget: all null", "gpupoly_matrix_mul_gadget", gpupoly_matrix_mul_gadget(NULL, 0, NULL, NULL, 0, 0, NULL, 0, 6, 0)) && ok;
    ok = refused("mul_gadget: null out, a window", "gpupoly_matrix_mul_gadget", gpupoly_matrix_mul_gadget(NULL, 2, NULL, NULL, 1, 3, NULL, 1, 6, 1)) && ok;
    ok = refused("mul_gadget: null out, base 0", "gpupoly_matrix_mul_gadget", gpupoly_matrix_mul_gadget(NULL, 0, NULL, NULL, 0, 0, NULL, 0, 0, 0)) && ok;
    ok = refused("gadget_mul: all null", "gpupoly_matrix_gadget_mul", gpupoly_matrix_gadget_mul(NULL, NULL, NULL, 0, 6, 0)) && ok;
    ok = refused("gadget_mul: all null, negate, small", "gpupoly_matrix_gadget_mul", gpupoly_matrix_gadget_mul(NULL, NULL, NULL, 1, 6, 1)) && ok;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "gadget_products_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "gadget_products_null"
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
    assert lib.gpupoly_matrix_mul_gadget(None, 0, None, None, 0, 0, None, 0, 6, 0) != 0
    assert MG in _ffi.last_error_string()
    assert lib.gpupoly_matrix_mul_gadget(None, 2, None, None, 1, 3, None, 1, 6, 1) != 0
    assert MG in _ffi.last_error_string()
    assert lib.gpupoly_matrix_gadget_mul(None, None, None, 0, 6, 0) != 0
    assert GM in _ffi.last_error_string()
    assert lib.gpupoly_matrix_gadget_mul(None, None, None, 1, 6, 1) != 0
    assert GM in _ffi.last_error_string()


def test_header_states_the_rule_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for entry in (MG, GM):
        at = text.index("int " + entry)
        comment = text[text.rindex("/*", 0, at):at]
        for needle in ("Refused", "overlap", "src/lookup/lwe/pubkey_gpu.rs:205", "src/bgg/sampler_gpu.rs:149", "src/lookup/ggh15/pubkey_gpu.rs:505"):
            assert needle in comment, (entry, needle)
    rule = text[:text.index("#ifndef GPUPOLY_H")]
    assert MG in rule and GM in rule, "the conventions' overlap rule names the new entries"
