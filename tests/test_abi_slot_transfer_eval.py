"""CPU-only: `gpupoly_matrix_slot_transfer_eval` and its test instrument `gpupoly_matrix_slot_transfer_eval_combine` are part
of the plain C ABI - declared in include/gpupoly.h with the reference lines they replace, exported by libgpupoly, bound in
`_ffi.SIGNATURES` - and the mirror's functions exist; a C99 caller compiles against the header, links, and gets an error
code plus a message naming the function (never a crash) for null arguments, with its own arrays left as they were, and 0 for
no outputs."""
import os
import re
import subprocess

EVAL = "gpupoly_matrix_slot_transfer_eval"
COMBINE = "gpupoly_matrix_slot_transfer_eval_combine"
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
    const GpuMatrix *pgs[2] = {NULL, NULL}, *p1s[2] = {NULL, NULL};
    GpuSlotTerm terms[2];
    size_t offsets[3] = {0, 1, 2};
    uint64_t mus[2] = {5, 7};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    memset(terms, 0, sizeof terms);
    terms[0].scalar = terms[1].scalar = 1;
    tags.form = GPUPOLY_TAGS_TABLE;
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval(NULL, 2, 0, NULL, pgs, p1s, terms, offsets, mus, 1, 0, 12, &tags), "gpupoly_matrix_slot_transfer_eval");
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval(outs, 2, 0, NULL, pgs, p1s, terms, offsets, mus, 1, 0, 12, &tags), "gpupoly_matrix_slot_transfer_eval");
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval(outs, 2, 0, NULL, NULL, NULL, NULL, NULL, NULL, 1, 0, 12, NULL), "gpupoly_matrix_slot_transfer_eval");
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval(outs, 2, 0, NULL, pgs, p1s, terms, offsets, mus, 1, 0, 12, NULL), "gpupoly_matrix_slot_transfer_eval");
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval_combine(outs, 2, 0, NULL, pgs, p1s, terms, offsets, mus, 1, 0, 12, NULL),
                       "gpupoly_matrix_slot_transfer_eval_combine");
    ok = ok && refused(gpupoly_matrix_slot_transfer_eval_combine(NULL, 2, 0, NULL, NULL, NULL, NULL, NULL, NULL, 1, 0, 12, NULL),
                       "gpupoly_matrix_slot_transfer_eval_combine");
    /* no outputs: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_slot_transfer_eval(NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, NULL) == 0;
    ok = ok && gpupoly_matrix_slot_transfer_eval_combine(NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && pgs[0] == NULL && pgs[1] == NULL && p1s[0] == NULL && p1s[1] == NULL;
    ok = ok && terms[0].c_in == NULL && terms[1].mid == NULL && terms[0].scalar == 1 && terms[1].shift == 0;
    ok = ok && offsets[0] == 0 && offsets[1] == 1 && offsets[2] == 2 && mus[0] == 5 && mus[1] == 7 && tags.form == GPUPOLY_TAGS_TABLE;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_with_their_citations_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (EVAL, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    # the comment in front of the declaration cites what the entry replaces
    comment = header[:header.index(f"int {EVAL}(")].rsplit("/* ----", 1)[1]
    for cite in ("src/slot_transfer/bgg_poly_encoding.rs:119-248", ":250-386", "src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786", ":748-786"):
        assert cite in comment, cite
    assert "MXX_HIP_SLOT_EVAL_BUDGET" in comment and "overlap" in comment and "unsupported" in comment and "dst_col" in comment
    between = header[header.index(f"int {EVAL}("):header.index(f"int {COMBINE}(")]
    assert "src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786" in between  # the instrument's own citation
    # the term structure as the issue states it
    struct = re.sub(r"/\*.*?\*/", "", comment[comment.index("typedef struct"):], flags=re.S)
    assert re.sub(r"\s+", " ", struct).strip() == \
        "typedef struct { const GpuMatrix *c_in; const GpuMatrix *mid; uint64_t shift; uint64_t scalar; } GpuSlotTerm;"
    # the two declarations take the same arguments but for the last one
    decl = {name: re.sub(r"\s+", " ", header[header.index(f"int {name}("):].split(";", 1)[0]) for name in (EVAL, COMBINE)}
    args = {name: d[d.index("(") + 1:d.rindex(")")].split(", ") for name, d in decl.items()}
    assert args[EVAL][:-1] == args[COMBINE][:-1]
    assert args[EVAL][-1] == "const GpuHashTags *tags" and args[COMBINE][-1] == "const GpuMatrix *digits"
    assert len(_ffi.SIGNATURES[EVAL][1]) == len(args[EVAL]) == len(_ffi.SIGNATURES[COMBINE][1]) == 13
    import ctypes as C

    assert C.sizeof(_ffi.GpuSlotTerm) == 32 and [f[0] for f in _ffi.GpuSlotTerm._fields_] == ["c_in", "mid", "shift", "scalar"]


def test_the_mirror_has_the_evaluation():
    import mxx_amd
    from mxx_amd import slot_transfer
    from mxx_amd.matrix import IndexedTags

    for name in ("SlotEvalShared", "output_slot", "slot_reduce_output_slot", "transfer_mids", "slot_transfer_slots", "slot_reduce_slots",
                 "slot_transfer", "slot_reduce"):
        assert callable(getattr(slot_transfer, name)), name
    for name in ("slot_transfer_eval", "slot_transfer_eval_combine"):
        assert callable(getattr(mxx_amd.GpuDCRTPolyMatrix, name))
    # the preprocessing half is still there
    for name in ("gate_target_chunks", "slot_reduce_gate_target_chunks", "sample_gate_preimages"):
        assert callable(getattr(slot_transfer, name))
    sh = slot_transfer.SlotEvalShared(None, b"", 2, None, None, None, None)
    assert sh.slot_a_tag(12) == b"slot_transfer_slot_a_12"
    # consecutive destinations: the indexed-decimal form; anything else: a table of literal tags
    tags = sh.slot_a_tags([3, 4, 5])
    assert isinstance(tags, IndexedTags) and tags.decimal and list(tags) == [sh.slot_a_tag(s) for s in (3, 4, 5)]
    assert sh.slot_a_tags([3, 5]) == [b"slot_transfer_slot_a_3", b"slot_transfer_slot_a_5"]


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "slot_transfer_eval_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "slot_transfer_eval_null"
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
    outs, pgs, p1s = ((C.c_void_p * 2)() for _ in range(3))
    terms = (_ffi.GpuSlotTerm * 2)()
    offsets = (C.c_size_t * 3)(0, 1, 2)
    mus = (C.c_uint64 * 2)(5, 7)
    for args in ((None, 2, 0, None, pgs, p1s, terms, offsets, mus, 1, 0, 12, C.byref(tags)),
                 (outs, 2, 0, None, pgs, p1s, terms, offsets, mus, 1, 0, 12, C.byref(tags)),
                 (outs, 2, 0, None, None, None, None, None, None, 1, 0, 12, None),
                 (outs, 2, 0, None, pgs, p1s, terms, offsets, mus, 1, 0, 12, None)):
        assert lib.gpupoly_matrix_slot_transfer_eval(*args) != 0
        assert EVAL in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    for args in ((outs, 2, 0, None, pgs, p1s, terms, offsets, mus, 1, 0, 12, None), (None, 2, 0, None, None, None, None, None, None, 1, 0, 12, None)):
        assert lib.gpupoly_matrix_slot_transfer_eval_combine(*args) != 0
        assert COMBINE in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    assert all(a[i] is None for a in (outs, pgs, p1s) for i in range(2)) and list(offsets) == [0, 1, 2] and list(mus) == [5, 7]
    assert lib.gpupoly_matrix_slot_transfer_eval(None, 0, 0, None, None, None, None, None, None, 0, 0, 0, None) == 0
    assert lib.gpupoly_matrix_slot_transfer_eval_combine(None, 0, 0, None, None, None, None, None, None, 0, 0, 0, None) == 0
