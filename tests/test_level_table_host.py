"""Host-only: every C-ABI entry of include/gpupoly.h that takes a GpuMatrix has, in tests/levels.py, either the tests that
run it on matrices below the top level, the test that asserts that it refuses them, or the reason why its work does not
depend on the level.

Every launcher takes two limb counts that agree only at the top level - the matrix's L = level + 1 and the context's
limb_count - so an entry that is only ever run at the top level is never asked which one it uses.  The prototypes are
parsed from the header; a new entry point fails here until its row exists and its named tests do.
"""
import importlib
import os
import re

import pytest

import levels

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpupoly.h")
MARKS = ("refuses", "no limbs")


def _prototypes():
    with open(HEADER) as f:
        return levels.prototypes(f.read())


def _tests_of(row):
    """the "module::test" ids a row names"""
    if row[0] == "no limbs":
        return ()
    return tuple(row[1:]) if row[0] == "refuses" else tuple(row)


def _missing(protos, table):
    return sorted(set(protos) - set(table))


def test_the_parser_finds_the_prototypes():
    protos = _prototypes()
    assert len(protos) >= 100
    for name in ("gpu_matrix_create", "gpu_matrix_ntt_all", "gpupoly_trapdoor_preimage_keyed", "gpupoly_matrix_all_gather_columns",
                 "gpupoly_matrix_mul_decompose_gadget_const_many", "gpupoly_matrix_store_coeff_ints"):
        assert name in protos, name
    assert "gpu_context_create" not in protos and "gpupoly_hash_seeds" not in protos  # no matrix among their arguments
    assert levels.writes_a_matrix(protos["gpu_matrix_add"]) and not levels.writes_a_matrix(protos["gpu_matrix_equal"])
    assert levels.writes_a_matrix(protos["gpupoly_matrix_split_columns"])  # GpuMatrix *const *blocks
    assert not levels.writes_a_matrix(protos["gpupoly_matrix_centered_max_abs"])


def test_every_matrix_taking_entry_has_a_row_and_every_row_an_entry():
    protos = _prototypes()
    assert not _missing(protos, levels.TABLE), f"entries without a lower-level case, a refusal or a reason: {_missing(protos, levels.TABLE)}"
    stale = sorted(set(levels.TABLE) - set(protos))
    assert not stale, f"rows for entries the header no longer declares: {stale}"


def test_removing_a_row_is_noticed():
    protos = _prototypes()
    for gone in ("gpu_matrix_intt_all", "gpupoly_matrix_lwe_lookup_combine"):
        table = {k: v for k, v in levels.TABLE.items() if k != gone}
        assert _missing(protos, table) == [gone]


@pytest.mark.parametrize("entry", sorted(levels.TABLE))
def test_rows_are_well_formed_and_name_tests_that_exist(entry):
    row = levels.TABLE[entry]
    assert isinstance(row, tuple) and row and all(isinstance(x, str) and x for x in row), entry
    if row[0] == "no limbs":
        assert len(row) == 2 and len(row[1].split()) >= 4, f"{entry}: one line of reason"
        return
    if row[0] == "refuses":
        assert len(row) == 2, f"{entry}: the test that asserts the refusal"
    else:
        assert not set(row) & set(MARKS), entry
    for test_id in _tests_of(row):
        assert re.fullmatch(r"test_gpu_\w+::test_\w+", test_id), (entry, test_id)
        module, test = test_id.split("::")
        mod = importlib.import_module(module)
        assert callable(getattr(mod, test, None)), f"{entry}: {test_id} does not exist"
        mark = getattr(mod, "pytestmark", None)
        marks = mark if isinstance(mark, (list, tuple)) else [mark]
        assert any(getattr(m, "name", None) == "gpu" for m in marks), f"{entry}: {module} is not a GPU module"


def test_an_entry_whose_work_ignores_the_level_writes_no_matrix_or_says_why():
    protos = _prototypes()
    for entry, row in levels.TABLE.items():
        if row[0] == "no limbs" and levels.writes_a_matrix(protos[entry]):
            assert len(row[1].split()) >= 8, f"{entry} takes a matrix it may write: state why its work does not depend on the level"


def test_the_table_points_at_the_new_module_for_every_core_entry():
    """the entries of the reference ABI (gpu_matrix_*) that compute on residues are run by tests/test_gpu_levels.py itself"""
    core = [e for e in levels.TABLE if e.startswith("gpu_matrix_") and levels.TABLE[e][0] not in MARKS]
    assert len(core) >= 25
    for entry in core:
        assert any(t.startswith("test_gpu_levels::") for t in levels.TABLE[entry]), entry
