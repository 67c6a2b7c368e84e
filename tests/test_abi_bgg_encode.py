"""CPU-only: `gpupoly_matrix_bgg_encode_slots` and its test instrument `gpupoly_matrix_bgg_encode_slots_combine` are part of
the plain C ABI - declared in include/gpupoly.h with the reference lines they replace, exported by libgpupoly, bound in
`_ffi.SIGNATURES` - and the mirror's classes and functions exist; a C99 caller compiles against the header, links, and gets an
error code plus a message naming the function (never a crash) for null arguments, with its own arrays left as they were,
and 0 for a call without inputs (the slot count is a matrix's row count: no matrix exists without a device)."""
import os
import re
import subprocess

import bgg_levels

ENCODE = "gpupoly_matrix_bgg_encode_slots"
COMBINE = "gpupoly_matrix_bgg_encode_slots_combine"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, who) != NULL && strstr(msg, "null") != NULL;
}

int main(void) {
    GpuRngSeed seeds[2];
    GpuMatrix *outs[2] = {NULL, NULL};
    const GpuMatrix *keys[2] = {NULL, NULL};
    int ok = 1;
    memset(seeds, 0, sizeof seeds);
    ok = ok && refused(gpupoly_matrix_bgg_encode_slots(NULL, 2, NULL, keys, NULL, 12, 3.5, seeds), "gpupoly_matrix_bgg_encode_slots");
    ok = ok && refused(gpupoly_matrix_bgg_encode_slots(outs, 2, NULL, NULL, NULL, 12, 3.5, seeds), "gpupoly_matrix_bgg_encode_slots");
    ok = ok && refused(gpupoly_matrix_bgg_encode_slots(outs, 2, NULL, keys, NULL, 12, 0.0, NULL), "gpupoly_matrix_bgg_encode_slots");
    ok = ok && refused(gpupoly_matrix_bgg_encode_slots_combine(NULL, 2, NULL, keys, NULL, 12, NULL), "gpupoly_matrix_bgg_encode_slots_combine");
    ok = ok && refused(gpupoly_matrix_bgg_encode_slots_combine(outs, 2, NULL, keys, NULL, 12, NULL), "gpupoly_matrix_bgg_encode_slots_combine");
    /* no inputs: nothing to do, whatever else is passed */
    ok = ok && gpupoly_matrix_bgg_encode_slots(NULL, 0, NULL, NULL, NULL, 0, 0.0, NULL) == 0;
    ok = ok && gpupoly_matrix_bgg_encode_slots_combine(NULL, 0, NULL, NULL, NULL, 0, NULL) == 0;
    ok = ok && outs[0] == NULL && outs[1] == NULL && keys[0] == NULL && keys[1] == NULL && seeds[0].words[0] == 0;
    return ok ? 0 : 1;
}
"""


def test_entries_are_declared_with_their_citations_exported_and_bound():
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    for name in (ENCODE, COMBINE):
        assert f"int {name}(" in header
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)
    # the comment in front of the declaration cites what the entry replaces
    comment = header[:header.index(f"int {ENCODE}(")].rsplit("/* ----", 1)[1]
    assert "src/bgg/sampler_gpu.rs:110-160" in comment and "src/bgg/sampler.rs:133-182" in comment
    assert "MXX_HIP_BGG_ENCODE_BUDGET" in comment and "overlap" in comment and "unsupported" in comment
    # the two declarations take the same arguments up to the base; then sigma and seeds, or the errors
    decl = {name: re.sub(r"\s+", " ", header[header.index(f"int {name}("):].split(";", 1)[0]) for name in (ENCODE, COMBINE)}
    args = {name: d[d.index("(") + 1:d.rindex(")")].split(", ") for name, d in decl.items()}
    assert args[ENCODE][:6] == args[COMBINE][:6] and args[ENCODE][5] == "uint32_t base_bits"
    assert args[ENCODE][6:] == ["double sigma", "const GpuRngSeed *seeds"] and args[COMBINE][6:] == ["const GpuMatrix *errors"]
    assert len(_ffi.SIGNATURES[ENCODE][1]) == len(args[ENCODE]) == 8 and len(_ffi.SIGNATURES[COMBINE][1]) == len(args[COMBINE]) == 7


def test_the_mirror_has_the_samplers():
    import mxx_amd
    from mxx_amd import bgg

    assert mxx_amd.bgg is bgg
    for name in ("BggPublicKey", "BggEncoding", "BggPolyEncoding", "BGGPublicKeySampler", "BGGEncodingSampler", "BGGPolyEncodingSampler"):
        assert isinstance(getattr(bgg, name), type), name
    for name in ("effective_gauss_sigma", "sample_poly_encoding_vectors_literal", "encode_slots"):
        assert callable(getattr(bgg, name)), name
    for name in ("sample", "sample_with_fresh_slot_secret_mats", "sample_slot_secret_mats", "slot_secrets"):
        assert callable(getattr(bgg.BGGPolyEncodingSampler, name)), name
    for name in ("sample", "sample_literal"):
        assert callable(getattr(bgg.BGGEncodingSampler, name)), name
    for name in ("bgg_encode_slots", "bgg_encode_slots_combine"):
        assert callable(getattr(mxx_amd.GpuDCRTPolyMatrix, name)), name


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "bgg_encode_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "bgg_encode_null"
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
    seeds = (_ffi.GpuRngSeed * 2)()
    outs, keys = ((C.c_void_p * 2)() for _ in range(2))
    for args in ((None, 2, None, keys, None, 12, 3.5, seeds), (outs, 2, None, None, None, 12, 3.5, seeds), (outs, 2, None, keys, None, 12, 0.0, None)):
        assert lib.gpupoly_matrix_bgg_encode_slots(*args) != 0
        assert ENCODE in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    for args in ((None, 2, None, keys, None, 12, None), (outs, 2, None, keys, None, 12, None)):
        assert lib.gpupoly_matrix_bgg_encode_slots_combine(*args) != 0
        assert COMBINE in _ffi.last_error_string() and "null" in _ffi.last_error_string()
    assert all(a[i] is None for a in (outs, keys) for i in range(2))
    assert lib.gpupoly_matrix_bgg_encode_slots(None, 0, None, None, None, 0, 0.0, None) == 0
    assert lib.gpupoly_matrix_bgg_encode_slots_combine(None, 0, None, None, None, 0, None) == 0


def test_the_entries_have_their_rows_in_the_lower_level_table():
    import levels

    for name in (ENCODE, COMBINE):
        assert levels.TABLE[name] == bgg_levels.ROWS[name] == ("test_gpu_bgg_encode::test_operands_below_the_top_level_equal_the_plain_reference",)
