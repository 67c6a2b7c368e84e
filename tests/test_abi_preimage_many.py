"""CPU-only: the batched preimage entry `gpupoly_trapdoor_preimage_many` is part of the plain C ABI - a C99 caller compiles
against include/gpupoly.h, links libgpupoly, and gets an error code plus a message (never a crash) for bad arguments."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

int main(void) {
    const GpuMatrix *targets[1] = {NULL};
    GpuMatrix *outs[1] = {NULL};
    GpuRngSeed seeds[3];
    const char *msg;
    int rc;
    memset(seeds, 0, sizeof seeds);
    rc = gpupoly_trapdoor_preimage_many(NULL, NULL, NULL, 17u, targets, 1, seeds, outs);
    msg = gpu_last_error();
    printf("rc=%d msg=%s\n", rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, "gpupoly_trapdoor_preimage_many") != NULL ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "preimage_many_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "preimage_many_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert "rc=" in run.stdout and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    seeds = (_ffi.GpuRngSeed * 3)()
    ptrs = (C.c_void_p * 1)()
    assert lib.gpupoly_trapdoor_preimage_many(None, None, None, 17, ptrs, 1, seeds, ptrs) != 0
    assert "gpupoly_trapdoor_preimage_many" in _ffi.last_error_string()
