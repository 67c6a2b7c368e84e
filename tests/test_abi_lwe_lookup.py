"""CPU-only: `gpupoly_matrix_lwe_lookup` and its test instrument `gpupoly_matrix_lwe_lookup_combine` are part of the plain C
ABI - declared in include/gpupoly.h with the reference lines they replace, exported by libgpupoly, bound in
`_ffi.SIGNATURES` - and the mirror's functions exist; a C99 caller compiles against the header, links, and gets an error
code plus a message naming the function (never a crash) for null arguments, with its own arrays left as they were, and 0 for
no slots."""
import os
import re
import subprocess

LOOKUP = "gpupoly_matrix_lwe_lookup"
COMBINE = "gpupoly_matrix_lwe_lookup_combine"
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
    GpuHashTags tags;
    GpuMatrix *outs[2] = {NULL, NULL};
    const GpuMatrix *cbs[2] = {NULL, NULL}, *khs[2] = {NULL, NULL}, *czs[2] = {NULL, NULL};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_TABLE;
    ok = ok && refused(gpupoly_matrix_lwe_lookup(NULL, 2, 0, cbs, khs, czs, 0, 12, &tags), "gpupoly_matrix_lwe_lookup");
    ok = ok && refused(gpupoly_matrix_lwe_lookup(outs, 2, 0, cbs, khs, czs, 0, 12, &tags), "gpupoly_matrix_lwe_lookup");
    ok = ok && refused(gpupoly_matrix_lwe_lookup(outs, 2, 0, NULL, NULL, NULL, 0, 12, NULL), "gpupoly_matrix_lwe_lookup");
    ok = ok && refused(gpupoly_matrix_lwe_lookup(outs, 2, 0, cbs, khs, czs, 0, 12, NULL), "gpupoly_matrix_lwe_lookup");
    ok = ok && refused(gpupoly_matrix_lwe_lookup_combine(outs, 2, 0, cbs, khs, czs, 0, 12, NULL), "gpupoly_matrix_lwe_lookup_combine");
    ok = ok && refused(gpupoly_matrix_lwe_lookup_combine(NULL, 2, 0, NULL, NULL, NULL, 0, 12, NULL), "gpupoly_matrix_lwe_lookup_combine");
    /* no slots: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_lwe_lookup(NULL, 0, 0, NULL, NULL, NULL, 0, 0, NULL) == 0;
    ok = ok && gpupoly_matrix_lwe_lookup_combine(NULL, 0, 0, NULL, NULL, NULL, 0, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && cbs[0] == NULL && cbs[1] == NULL && khs[0] == NULL && khs[1] == NULL;
    ok = ok && czs[0] == NULL && czs[1] == NULL && tags.form == GPUPOLY_TAGS_TABLE;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_with_their_citations_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (LOOKUP, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    # the comment in front of the declaration cites what the entry replaces
    comment = header[:header.index(f"int {LOOKUP}(")].rsplit("/* ----", 1)[1]
    assert "src/lookup/lwe/poly_encoding_gpu.rs:419-453" in comment and "src/lookup/lwe/encoding_gpu.rs:225-370" in comment
    assert "MXX_HIP_LWE_LOOKUP_BUDGET" in comment and "overlap" in comment and "unsupported" in comment and "dst_col" in comment
    # the two declarations take the same arguments but for the last one
    decl = {name: re.sub(r"\s+", " ", header[header.index(f"int {name}("):].split(";", 1)[0]) for name in (LOOKUP, COMBINE)}
    args = {name: d[d.index("(") + 1:d.rindex(")")].split(", ") for name, d in decl.items()}
    assert args[LOOKUP][:-1] == args[COMBINE][:-1]
    assert args[LOOKUP][-1] == "const GpuHashTags *tags" and args[COMBINE][-1] == "const GpuMatrix *digits"
    assert len(_ffi.SIGNATURES[LOOKUP][1]) == len(args[LOOKUP]) == len(_ffi.SIGNATURES[COMBINE][1]) == 9


def test_the_mirror_has_the_lookup():
    import mxx_amd
    from mxx_amd import lwe_lookup

    assert mxx_amd.lwe_lookup is lwe_lookup
    for name in ("public_lookup", "public_lookup_slots", "public_lookup_poly"):
        assert callable(getattr(lwe_lookup, name))
    for name in ("lwe_lookup", "lwe_lookup_combine"):
        assert callable(getattr(mxx_amd.GpuDCRTPolyMatrix, name))
    # the entry index stands in the middle of a slot's tag: a table of literal tags
    sh = lwe_lookup.LweShared(None, b"", 23, 5, 4, None, None)
    assert sh.tag(12) == b"LWE_R_G_23_5_12_slot4" and sh.tags([1, 2]) == [b"LWE_R_G_23_5_1_slot4", b"LWE_R_G_23_5_2_slot4"]
    assert lwe_lookup.public_lookup_slots([], [], [], [], []) == []


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "lwe_lookup_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "lwe_lookup_null"
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
    tags = _ffi.GpuHashTags()
    outs, cbs, khs, czs = ((C.c_void_p * 2)() for _ in range(4))
    for args in ((None, 2, 0, cbs, khs, czs, 0, 12, C.byref(tags)), (outs, 2, 0, cbs, khs, czs, 0, 12, C.byref(tags)),
                 (outs, 2, 0, None, None, None, 0, 12, None), (outs, 2, 0, cbs, khs, czs, 0, 12, None)):
        assert lib.gpupoly_matrix_lwe_lookup(*args) != 0
        assert LOOKUP in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    for args in ((outs, 2, 0, cbs, khs, czs, 0, 12, None), (None, 2, 0, None, None, None, 0, 12, None)):
        assert lib.gpupoly_matrix_lwe_lookup_combine(*args) != 0
        assert COMBINE in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    assert all(a[i] is None for a in (outs, cbs, khs, czs) for i in range(2))
    assert lib.gpupoly_matrix_lwe_lookup(None, 0, 0, None, None, None, 0, 0, None) == 0
    assert lib.gpupoly_matrix_lwe_lookup_combine(None, 0, 0, None, None, None, 0, 0, None) == 0
