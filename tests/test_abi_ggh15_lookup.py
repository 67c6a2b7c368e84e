"""CPU-only: `gpupoly_matrix_ggh15_lookup` and its test instrument `gpupoly_matrix_ggh15_lookup_combine` are part of the plain
C ABI - declared in include/gpupoly.h with the reference lines they replace, exported by libgpupoly, bound in
`_ffi.SIGNATURES` - and the mirror's functions exist; a C99 caller compiles against the header, links, and gets an error
code plus a message naming the function (never a crash) for null arguments, with its own arrays left as they were, and 0 for
no slots."""
import os
import re
import subprocess

LOOKUP = "gpupoly_matrix_ggh15_lookup"
COMBINE = "gpupoly_matrix_ggh15_lookup_combine"
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
    const GpuMatrix *luts[2] = {NULL, NULL}, *xs[2] = {NULL, NULL};
    uint64_t y[2] = {7, 9};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_INDEXED_DECIMAL;
    ok = ok && refused(gpupoly_matrix_ggh15_lookup(NULL, 2, NULL, NULL, NULL, NULL, NULL, NULL, luts, xs, 0, 12, y, 1, &tags), "gpupoly_matrix_ggh15_lookup");
    ok = ok && refused(gpupoly_matrix_ggh15_lookup(outs, 2, NULL, NULL, NULL, NULL, NULL, NULL, luts, xs, 0, 12, y, 1, &tags), "gpupoly_matrix_ggh15_lookup");
    ok = ok && refused(gpupoly_matrix_ggh15_lookup(outs, 2, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 12, NULL, 1, NULL), "gpupoly_matrix_ggh15_lookup");
    ok = ok && refused(gpupoly_matrix_ggh15_lookup_combine(outs, 2, NULL, NULL, NULL, NULL, NULL, NULL, luts, xs, 0, 12, y, 1, NULL),
                       "gpupoly_matrix_ggh15_lookup_combine");
    ok = ok && refused(gpupoly_matrix_ggh15_lookup_combine(NULL, 2, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 12, NULL, 1, NULL),
                       "gpupoly_matrix_ggh15_lookup_combine");
    /* no slots: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_ggh15_lookup(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == 0;
    ok = ok && gpupoly_matrix_ggh15_lookup_combine(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && luts[0] == NULL && luts[1] == NULL && xs[0] == NULL && xs[1] == NULL;
    ok = ok && y[0] == 7 && y[1] == 9 && tags.form == GPUPOLY_TAGS_INDEXED_DECIMAL;
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
    assert "src/lookup/ggh15/encoding.rs:172-300" in comment and "src/lookup/ggh15/poly_encoding_gpu.rs:338-567,686-1420" in comment
    assert "MXX_HIP_GGH15_LOOKUP_BUDGET" in comment and "overlap" in comment and "unsupported" in comment
    # the two declarations take the same arguments but for the last one
    decl = {name: re.sub(r"\s+", " ", header[header.index(f"int {name}("):].split(";", 1)[0]) for name in (LOOKUP, COMBINE)}
    args = {name: d[d.index("(") + 1:d.rindex(")")].split(", ") for name, d in decl.items()}
    assert args[LOOKUP][:-1] == args[COMBINE][:-1]
    assert args[LOOKUP][-1] == "const GpuHashTags *tags" and args[COMBINE][-1] == "const GpuMatrix *digits"
    assert len(_ffi.SIGNATURES[LOOKUP][1]) == len(args[LOOKUP]) == len(_ffi.SIGNATURES[COMBINE][1]) == 15


def test_the_mirror_has_the_lookup():
    import mxx_amd
    from mxx_amd import ggh15_eval

    assert mxx_amd.ggh15_eval is ggh15_eval
    for name in ("PublicLookupShared", "build_public_lookup_output_chunk", "public_lookup_stage1", "public_lookup_stage2", "public_lookup_slots"):
        assert callable(getattr(ggh15_eval, name))
    for name in ("ggh15_lookup", "ggh15_lookup_combine"):
        assert callable(getattr(mxx_amd.GpuDCRTPolyMatrix, name))
    sh = ggh15_eval.PublicLookupShared.__new__(ggh15_eval.PublicLookupShared)
    sh.lut_id, sh.gate_id = 3, 11
    assert sh.v_tag(7) == b"ggh15_lut_v_idx_3_7" and sh.u_g_tag() == b"ggh15_lut_u_g_matrix_11"
    consecutive = sh.v_tags([98, 99, 100])
    assert isinstance(consecutive, mxx_amd.IndexedTags) and list(consecutive) == [sh.v_tag(k) for k in (98, 99, 100)]
    assert sh.v_tags([5, 5, 2]) == [sh.v_tag(5), sh.v_tag(5), sh.v_tag(2)]


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "ggh15_lookup_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "ggh15_lookup_null"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgpupoly", "-L/opt/rocm/lib", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib"))
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert run.stdout.count("rc=") == 5 and "rc=0 " not in run.stdout


def test_binding_reports_null_arguments_as_an_error():
    import ctypes as C

    from mxx_amd import _ffi

    lib = _ffi.lib()
    tags = _ffi.GpuHashTags()
    outs, luts, xs = (C.c_void_p * 2)(), (C.c_void_p * 2)(), (C.c_void_p * 2)()
    y = (C.c_uint64 * 2)(7, 9)
    mids = (None,) * 6
    for args in ((None, 2, *mids, luts, xs, 0, 12, y, 1, C.byref(tags)), (outs, 2, *mids, luts, xs, 0, 12, y, 1, C.byref(tags)),
                 (outs, 2, *mids, None, None, 0, 12, None, 1, None)):
        assert lib.gpupoly_matrix_ggh15_lookup(*args) != 0
        assert LOOKUP in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    for args in ((outs, 2, *mids, luts, xs, 0, 12, y, 1, None), (None, 2, *mids, None, None, 0, 12, None, 1, None)):
        assert lib.gpupoly_matrix_ggh15_lookup_combine(*args) != 0
        assert COMBINE in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    assert list(y) == [7, 9] and all(a[i] is None for a in (outs, luts, xs) for i in range(2))
    assert lib.gpupoly_matrix_ggh15_lookup(None, 0, *mids, None, None, 0, 0, None, 0, None) == 0
    assert lib.gpupoly_matrix_ggh15_lookup_combine(None, 0, *mids, None, None, 0, 0, None, 0, None) == 0
