"""CPU-only: gpupoly_matrix_decompose_rows and gpupoly_matrix_sample_decomposed_window are part of the plain C ABI - a C99
caller compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message that names the entry
(never a crash) for null arguments; the header states the window rule, the overlap rule, what is refused and the reference
lines the entries serve; the Python mirror has the methods."""
import inspect
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DR, SW = "gpupoly_matrix_decompose_rows", "gpupoly_matrix_sample_decomposed_window"

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
    GpuRngSeed seed;
    const char *dr = "gpupoly_matrix_decompose_rows", *sw = "gpupoly_matrix_sample_decomposed_window";
    memset(&seed, 0, sizeof seed);
    ok = refused("decompose_rows: all null", dr, gpupoly_matrix_decompose_rows(NULL, 6, 0, 0, NULL)) && ok;
    ok = refused("decompose_rows: all null, small", dr, gpupoly_matrix_decompose_rows(NULL, 6, 1, 3, NULL)) && ok;
    ok = refused("sample window: null out", sw, gpupoly_matrix_sample_decomposed_window(NULL, 0, 0.0, seed, 6, 0, 1, 1, 0, 0)) && ok;
    ok = refused("sample window: null out, gauss", sw, gpupoly_matrix_sample_decomposed_window(NULL, 1, 3.0, seed, 6, 1, 2, 4, 1, 2)) && ok;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_errors_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "decompose_window_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "decompose_window_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])


def test_binding_exports_both_and_reports_null_arguments_as_errors():
    from mxx_amd import _ffi

    lib = _ffi.lib()
    assert DR in _ffi.SIGNATURES and SW in _ffi.SIGNATURES
    seed = _ffi.GpuRngSeed()
    assert lib.gpupoly_matrix_decompose_rows(None, 6, 0, 0, None) != 0
    assert DR in _ffi.last_error_string()
    assert lib.gpupoly_matrix_sample_decomposed_window(None, 0, 0.0, seed, 6, 0, 1, 1, 0, 0) != 0
    assert SW in _ffi.last_error_string()


def test_header_states_the_window_rule_and_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    needles = {DR: ("The window rule", "row_start + R <= src->rows * k", "Overlap", "rule 3", "Refused", "poly_encoding_gpu.rs:515,566",
                    "base_bits of 0 or >= 63", "gpu_matrix_copy_block"),
               SW: ("The window rule", "col_offset + c <= full_ncol", "row_start + R <= src_rows * k", "Overlap", "Refused",
                    "pubkey_gpu.rs:398-407,495-504", "poly_encoding_gpu.rs:453-462,520-543", "MXX_HIP_RNG_COMPAT=reference", "48-bit")}
    for entry, wanted in needles.items():
        at = text.index("int " + entry)
        comment = text[text.rindex("/*", 0, at):at]
        for needle in wanted:
            assert needle in comment, (entry, needle)


def test_the_mirror_has_the_methods():
    from mxx_amd.matrix import GpuDCRTPolyMatrix as M
    from mxx_amd.sampler import GpuDCRTPolyHashSampler as H

    assert callable(M.decompose_rows) and callable(M.sample_distribution_decomposed_window)
    for name in ("sample_hash_decomposed_columns", "sample_hash_small_decomposed_columns"):
        params = inspect.signature(getattr(H, name)).parameters
        assert "row_start" in params and "row_end" in params, name
