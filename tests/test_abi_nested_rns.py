"""CPU-only: the nested-RNS entries (`gpupoly_matrix_nested_rns_decompose`, `gpupoly_matrix_fill_nested_rns_gadget`,
`gpupoly_matrix_nested_rns_residues`) are part of the plain C ABI - a C99 caller compiles against
include/gpupoly.h, links libgpupoly, and gets an error code plus a message naming the function (never a crash) for null
arguments - and `NestedRnsContext` carries the deterministic p-modulus selection of `sample_crt_primes`
(src/gadgets/arith/nested_rns/encoding.rs:14-71)."""
import math
import os
import subprocess

import pytest

NAMES = ("gpupoly_matrix_nested_rns_decompose", "gpupoly_matrix_fill_nested_rns_gadget", "gpupoly_matrix_nested_rns_residues")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gpupoly.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static int refused(int rc, const char *who) {
    const char *msg = gpu_last_error();
    printf("%s rc=%d msg=%s\n", who, rc, msg ? msg : "(null)");
    return rc != 0 && msg != NULL && strstr(msg, who) != NULL;
}

int main(void) {
    uint64_t p[3] = {3, 4, 5};
    int ok = 1;
    ok = ok && refused(gpupoly_matrix_nested_rns_decompose(NULL, NULL, NULL, 0, 0, 0, 0, 0), "gpupoly_matrix_nested_rns_decompose");
    ok = ok && refused(gpupoly_matrix_nested_rns_decompose(NULL, NULL, p, 3, 256, 0, 1, GPU_POLY_FORMAT_EVAL), "gpupoly_matrix_nested_rns_decompose");
    ok = ok && refused(gpupoly_matrix_fill_nested_rns_gadget(NULL, NULL, 0, 0, 0, 0, 0), "gpupoly_matrix_fill_nested_rns_gadget");
    ok = ok && refused(gpupoly_matrix_fill_nested_rns_gadget(NULL, p, 3, 256, 0, 1, GPU_POLY_FORMAT_COEFF), "gpupoly_matrix_fill_nested_rns_gadget");
    ok = ok && refused(gpupoly_matrix_nested_rns_residues(NULL, NULL, NULL, 0, 0, 0), "gpupoly_matrix_nested_rns_residues");
    ok = ok && refused(gpupoly_matrix_nested_rns_residues(NULL, NULL, p, 3, 0, 1), "gpupoly_matrix_nested_rns_residues");
    ok = ok && p[0] == 3 && p[1] == 4 && p[2] == 5;
    return ok ? 0 : 1;
}
"""


def test_c99_caller_compiles_links_and_gets_an_error_for_null_arguments(tmp_path):
    from mxx_amd import _ffi

    src = tmp_path / "nested_rns_null.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "nested_rns_null"
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
    p = (C.c_uint64 * 3)(3, 4, 5)
    calls = (
        (lib.gpupoly_matrix_nested_rns_decompose, NAMES[0], ((None, None, None, 0, 0, 0, 0, 0), (None, None, p, 3, 256, 0, 1, 1))),
        (lib.gpupoly_matrix_fill_nested_rns_gadget, NAMES[1], ((None, None, 0, 0, 0, 0, 0), (None, p, 3, 256, 0, 1, 0))),
        (lib.gpupoly_matrix_nested_rns_residues, NAMES[2], ((None, None, None, 0, 0, 0), (None, None, p, 3, 0, 1))),
    )
    for fn, name, argsets in calls:
        for args in argsets:
            assert fn(*args) != 0
            assert name in _ffi.last_error_string()
    assert list(p) == [3, 4, 5]


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_exported_and_bound(name):
    from mxx_amd import _ffi

    header = open(os.path.join(ROOT, "include", "gpupoly.h")).read()
    assert f"int {name}(" in header
    assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name)


def test_context_selects_the_reference_p_moduli():
    """(p bits 6, 18-bit q, 2 unreduced multiplications): 3, 4, 5, 7, 11, 13, ... - the first pairwise coprime integers
    from 3 up, stopped as soon as prod > ((sum p + D) q_max / 2)^muls (encoding.rs:14-22,39-71)."""
    import mxx_amd
    from mxx_amd.nested_rns import NestedRnsContext, mul_budget_bound, sample_crt_primes
    from mxx_amd.params import DCRTPolyParams

    assert mxx_amd.NestedRnsContext is NestedRnsContext
    params = DCRTPolyParams(4, 6, 18, 6)
    q_moduli, _, depth = params.to_crt()
    q_max = max(q_moduli)
    assert depth == 6 and q_max.bit_length() == 18
    ctx = NestedRnsContext(params, 6, 2, 1 << 8)
    ps = ctx.p_moduli
    assert ps[:6] == [3, 4, 5, 7, 11, 13] and ps == sample_crt_primes(6, q_max, 2)
    assert all(3 <= p < 1 << 6 for p in ps) and ps == sorted(ps)
    assert all(math.gcd(a, b) == 1 for i, a in enumerate(ps) for b in ps[:i])
    # greedy: every integer from 3 up to the last one is either chosen or shares a factor with an earlier choice
    for c in range(3, ps[-1]):
        assert c in ps or any(math.gcd(c, p) != 1 for p in ps if p < c)
    # the bound holds for the whole list and for no proper prefix (the selection stops at the first that reaches it)
    D = len(ps)
    assert math.prod(ps) > ((sum(ps) + D) * q_max // 2) ** 2 == mul_budget_bound(sum(ps), D, q_max) ** 2
    for k in range(1, D):
        assert math.prod(ps[:k]) <= ((sum(ps[:k]) + k) * q_max // 2) ** 2
    assert ctx.scale == 256 and ctx.chunk_width() == D + 1 and ctx.q_moduli == list(q_moduli)
    assert ctx.active_window() == (0, 6) and ctx.active_window(2, 1) == (1, 2) and ctx.active_window(None, 4) == (4, 2)
    assert NestedRnsContext(params, 6, 2, 1 << 8, q_level=3).active_window() == (0, 3)
    with pytest.raises(ValueError):
        sample_crt_primes(3, q_max, 2)  # 3, 4, 5, 7 cannot reach the bound
