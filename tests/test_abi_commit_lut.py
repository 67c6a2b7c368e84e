"""CPU-only: `gpupoly_matrix_commit_lut_messages` (with its test instrument `gpupoly_matrix_commit_lut_messages_combine`) is
part of the plain C ABI - declared in include/gpupoly.h, exported by libgpupoly, bound in `_ffi.SIGNATURES`; a C99 caller
compiles against the header, links, and gets an error code plus a message naming the function (never a crash) for null
arguments, with its own arrays left as they were; no rows is success whatever else is passed.  The host mirror's tag strings
and stream layout are the reference's (src/lookup/commit_eval.rs:524-625)."""
import os
import subprocess

import commit_lut_levels

MESSAGES = "gpupoly_matrix_commit_lut_messages"
COMBINE = "gpupoly_matrix_commit_lut_messages_combine"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    const char *at = msg ? strstr(msg, who) : NULL;
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    /* the entry's own name: "..._messages:" is not "..._messages_combine:" */
    return rc != 0 && at != NULL && at[strlen(who)] == ':';
}

int main(void) {
    GpuHashTags tags;
    GpuMatrix *outs[2] = {NULL, NULL};
    const GpuMatrix *sums[1] = {NULL}, *a_outs[1] = {NULL};
    uint64_t y[2] = {7, 9}, idx[2] = {0, 1}, vslot[2] = {1, 0};
    uint32_t gate[2] = {0, 0};
    int ok = 1;
    memset(&tags, 0, sizeof tags);
    tags.form = GPUPOLY_TAGS_TABLE;
    ok = refused(gpupoly_matrix_commit_lut_messages(NULL, 2, NULL, NULL, vslot, sums, a_outs, 1, gate, 12, y, 1, idx, &tags),
                 "gpupoly_matrix_commit_lut_messages") && ok;
    ok = refused(gpupoly_matrix_commit_lut_messages(outs, 2, NULL, NULL, vslot, sums, a_outs, 1, gate, 12, y, 1, idx, &tags),
                 "gpupoly_matrix_commit_lut_messages") && ok;
    ok = refused(gpupoly_matrix_commit_lut_messages(outs, 2, NULL, NULL, NULL, NULL, NULL, 0, NULL, 12, NULL, 1, NULL, NULL),
                 "gpupoly_matrix_commit_lut_messages") && ok;
    ok = refused(gpupoly_matrix_commit_lut_messages_combine(NULL, 2, NULL, NULL, sums, a_outs, 1, gate, 12, y, 1),
                 "gpupoly_matrix_commit_lut_messages_combine") && ok;
    ok = refused(gpupoly_matrix_commit_lut_messages_combine(outs, 2, NULL, NULL, sums, a_outs, 1, gate, 12, y, 1),
                 "gpupoly_matrix_commit_lut_messages_combine") && ok;
    /* no rows: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_commit_lut_messages(NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, 0, NULL, NULL) == 0;
    ok = ok && gpupoly_matrix_commit_lut_messages_combine(NULL, 0, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, 0) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && y[0] == 7 && y[1] == 9 && idx[0] == 0 && idx[1] == 1 && vslot[0] == 1 && vslot[1] == 0 &&
         gate[0] == 0 && gate[1] == 0 && sums[0] == NULL && a_outs[0] == NULL;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (MESSAGES, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    assert len(_ffi.SIGNATURES[MESSAGES][1]) == 14 and len(_ffi.SIGNATURES[COMBINE][1]) == 11
    import mxx_amd
    from mxx_amd import commit_lookup

    assert mxx_amd.commit_lookup is commit_lookup
    for name in ("lut_layout", "compute_padded_len", "lut_gate_index", "derive_a_out_matrix", "derive_r_g_i_matrix", "derive_canceler_matrix",
                 "message_block_literal", "CommitMsgStream", "CommitBGGPubKeyPltEvaluator", "CommitBGGEncodingPltEvaluator"):
        assert callable(getattr(commit_lookup, name)), name
    assert callable(commit_lookup.CommitMsgStream.message_blocks)
    for name in ("setup", "public_lookup", "commit_all_lut_matrices"):
        assert callable(getattr(commit_lookup.CommitBGGPubKeyPltEvaluator, name))
    for name in ("setup", "public_lookup"):
        assert callable(getattr(commit_lookup.CommitBGGEncodingPltEvaluator, name))
    assert callable(mxx_amd.GpuDCRTPolyMatrix.commit_lut_messages) and callable(mxx_amd.GpuDCRTPolyMatrix.commit_lut_messages_combine)


def test_the_tags_are_the_reference_strings():
    from mxx_amd import commit_lookup

    assert commit_lookup.a_out_tag(7) == b"A_OUT_7"
    assert commit_lookup.r_g_i_tag(7, 12) == b"R_7_12"
    assert commit_lookup.B1_TAG == b"COMMIT_LUT_B1"
    # the indexed decimal form of a consecutive run generates the same strings
    from mxx_amd import IndexedTags

    assert list(IndexedTags(commit_lookup.r_g_i_prefix(7), 11, 2, decimal=True)) == [b"R_7_11", b"R_7_12"]


def test_lut_layout_matches_hand_computed_values():
    """gates given as ids 5 then 2 with 3 and 2 rows, tree_base 2: sorted by id, gate 2 owns [0, 2) and gate 5 [2, 5); five
    rows pad to 2^3 = 8 (:524-574)"""
    from mxx_amd import commit_lookup as cl

    luts = {10: {0: (0, 1), 1: (1, 0), 2: (2, 1)}, 11: {0: (1, 4), 1: (0, 5)}}
    layout = cl.lut_layout(luts, [(5, 10, "one5", "in5"), (2, 11, "one2", "in2")], 2)
    assert layout.lut_gate_start_ids == {2: 0, 5: 2}
    assert layout.lut_vector_len == 5 and layout.padded_len == 8
    assert layout.gate_ranges == [(0, 2, 2, 11, "one2", "in2"), (2, 5, 5, 10, "one5", "in5")]
    assert cl.lut_gate_index(layout.lut_gate_start_ids, 5, 2) == 4 and cl.lut_gate_index(layout.lut_gate_start_ids, 2, 1) == 1
    assert [cl.compute_padded_len(2, v) for v in (0, 1, 2, 3, 4, 5, 8, 9)] == [2, 2, 2, 4, 4, 8, 8, 16]
    assert [cl.compute_padded_len(3, v) for v in (1, 3, 4, 9, 10)] == [3, 3, 9, 9, 27]
    for bad in (lambda: cl.lut_gate_index({}, 3, 0), lambda: cl.lut_layout({}, [(1, 9, None, None)], 2)):
        try:
            bad()
        except KeyError:
            continue
        raise AssertionError("a missing gate or LUT is an error")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    at = text.index("int " + MESSAGES + "(")
    comment = text[text.rindex("/* ----", 0, at):at]
    for needle in ("src/lookup/commit_eval.rs:417-522", ":461-517", "Overlap:", "Refused", "words_per_y == 0", "base_bits of 0 or >= 63",
                   "gpupoly_hash_seeds", "unsupported", "MXX_HIP_RNG_COMPAT=reference", "T = 0", "PACKED24", "MXX_HIP_COMMIT_LUT_BUDGET",
                   "ngates == 0", "no inverse", "gate_of_row[t] >= ngates", "vslot[t] >= nV"):
        assert needle in comment, needle
    at = text.index("int " + COMBINE + "(")
    assert "Test instrument" in text[text.rindex("/*", 0, at):at]


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "commit_lut_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "commit_lut_null"
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
    outs, sums, a_outs = (C.c_void_p * 2)(), (C.c_void_p * 1)(), (C.c_void_p * 1)()
    y, idx, vslot = (C.c_uint64 * 2)(7, 9), (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(1, 0)
    gate = (C.c_uint32 * 2)(0, 0)
    for args in ((None, 2, None, None, vslot, sums, a_outs, 1, gate, 12, y, 1, idx, C.byref(tags)),
                 (outs, 2, None, None, vslot, sums, a_outs, 1, gate, 12, y, 1, idx, C.byref(tags)),
                 (outs, 2, None, None, None, None, None, 0, None, 12, None, 1, None, None)):
        assert lib.gpupoly_matrix_commit_lut_messages(*args) != 0
        assert MESSAGES + ":" in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    for args in ((None, 2, None, None, sums, a_outs, 1, gate, 12, y, 1), (outs, 2, None, None, sums, a_outs, 1, gate, 12, y, 1)):
        assert lib.gpupoly_matrix_commit_lut_messages_combine(*args) != 0
        assert COMBINE + ":" in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    assert list(y) == [7, 9] and list(idx) == [0, 1] and list(vslot) == [1, 0] and list(gate) == [0, 0]
    assert outs[0] is None and outs[1] is None and sums[0] is None and a_outs[0] is None
    assert lib.gpupoly_matrix_commit_lut_messages(None, 0, None, None, None, None, None, 0, None, 0, None, 0, None, None) == 0
    assert lib.gpupoly_matrix_commit_lut_messages_combine(None, 0, None, None, None, None, 0, None, 0, None, 0) == 0


def test_the_entries_have_their_rows_in_the_lower_level_table():
    import levels

    for name in (MESSAGES, COMBINE):
        assert levels.TABLE[name] == commit_lut_levels.ROWS[name] == ("test_gpu_commit_lut::test_operands_below_the_top_level_equal_the_literal",)
