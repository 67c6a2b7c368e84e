"""CPU-only: the mixed-key batched preimage entry `gpupoly_trapdoor_preimage_keyed` is part of the plain C ABI - a C99 caller
compiles against include/gpupoly.h, links libgpupoly, and gets an error code plus a message (never a crash) for bad
arguments."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

int main(void) {
    const GpuMatrix *keys[1] = {NULL};
    const GpuP1CovarianceCache *caches[1] = {NULL};
    const GpuMatrix *targets[1] = {NULL};
    GpuMatrix *outs[1] = {NULL};
    uint32_t key_of[1] = {0};
    GpuRngSeed seeds[3];
    const char *msg;
    int rc, rc2;
    memset(seeds, 0, sizeof seeds);
    rc = gpupoly_trapdoor_preimage_keyed(keys, caches, keys, 1, 17u, key_of, targets, 1, seeds, outs);
    msg = gpu_last_error();
    printf("rc=%d msg=%s\n", rc, msg ? msg : "(null)");
    if (rc == 0 || msg == NULL || strstr(msg, "gpupoly_trapdoor_preimage_keyed") == NULL) return 1;
    /* requests without keys */
    rc2 = gpupoly_trapdoor_preimage_keyed(NULL, NULL, NULL, 0, 17u, key_of, targets, 1, seeds, outs);
    msg = gpu_last_error();
    printf("rc2=%d msg=%s\n", rc2, msg ? msg : "(null)");
    if (rc2 == 0 || msg == NULL || strstr(msg, "gpupoly_trapdoor_preimage_keyed") == NULL) return 1;
    /* nothing asked: nothing done */
    return gpupoly_trapdoor_preimage_keyed(NULL, NULL, NULL, 0, 17u, NULL, NULL, 0, NULL, NULL) == 0 ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "preimage_keyed_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "preimage_keyed_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert "rc=" in run.stdout and "rc=0 " not in run.stdout


def test_symbol_is_exported_and_the_binding_reports_null_arguments():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    assert hasattr(C.CDLL(_ffi.LIB_PATH), "gpupoly_trapdoor_preimage_keyed")
    seeds = (_ffi.GpuRngSeed * 3)()
    ptrs = (C.c_void_p * 1)()
    key_of = (C.c_uint32 * 1)(0)
    assert lib.gpupoly_trapdoor_preimage_keyed(ptrs, ptrs, ptrs, 1, 17, key_of, ptrs, 1, seeds, ptrs) != 0
    assert "gpupoly_trapdoor_preimage_keyed" in _ffi.last_error_string()
    assert lib.gpupoly_trapdoor_preimage_keyed(None, None, None, 1, 17, key_of, ptrs, 1, seeds, ptrs) != 0
    assert "null" in _ffi.last_error_string()
