"""Host-only: every forced-path test has, for every (switch, value) it forces and every word class it runs, a case that
asserts the forced kernel ran.

The GPU tests skip the name assertion only where the forced kernel's own acceptance condition (a Python predicate next
to the test, read from the launcher) is false.  That rule alone would let a test whose every case is declined pass as a
second run of the default kernel, so the predicates are evaluated here over the tests' own parameter lists - the
`pytest.mark.parametrize` marks on the functions - without a GPU.
"""
import importlib
import inspect
import itertools

import pytest

import ran

MODULES = ["test_gpu_core", "test_gpu_modulus_classes", "test_gpu_surface", "test_gpu_serde", "test_gpu_compact_many",
           "test_gpu_mul_sum", "test_gpu_fused_width_classes"]


def _cases(fn):
    """the cartesian product of the function's parametrize marks, as dicts"""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        rows = []
        for v in mark.args[1]:
            if hasattr(v, "values") and hasattr(v, "marks"):  # pytest.param
                v = v.values if len(names) > 1 else v.values[0]
            rows.append(dict(zip(names, v)) if len(names) > 1 else {names[0]: v})
        axes.append(rows)
    out = []
    for combo in itertools.product(*axes):
        d = {}
        for part in combo:
            d.update(part)
        out.append(d)
    return out or [{}]


def _by_bits(c):
    return ran.Launched.word_class([1 << (c["bits"] - 1)])


def _registry():
    """(module, test, entry, cases) of every forced-path test"""
    for name in MODULES:
        mod = importlib.import_module(name)
        for test, entry in mod.FORCED.items():
            fn = getattr(mod, test)
            fixed = entry.get("fixed", {})
            yield name, test, entry, [dict(fixed, **c) for c in entry.get("cases") or _cases(fn)], fn


def _verdicts():
    """(module::test, pair, word class) -> the predicate's values over the cases that use the pair"""
    seen = {}
    for name, test, entry, cases, _ in _registry():
        cls = entry.get("cls", _by_bits)
        for pair, accepts in entry["pairs"].items():
            for c in cases:
                v = accepts(c)
                if v is None:
                    continue
                assert isinstance(v, bool), (name, test, pair, c, v)
                seen.setdefault((f"{name}::{test}", pair, cls(c)), []).append(v)
    return seen


def test_the_registries_name_tests_parameters_and_pairs_that_exist():
    count = 0
    for name, test, entry, cases, fn in _registry():
        assert callable(fn) and test.startswith("test_"), (name, test)
        args = set(inspect.signature(fn).parameters)
        for c in cases:
            assert "cases" in entry or set(c) - set(entry.get("fixed", {})) <= args, (name, test, c)
        for pair in entry["pairs"]:
            assert pair in ran.TABLE, (name, test, pair)
        count += len(cases)
    assert count > 100  # the parameter lists were found


def test_a_case_uses_a_pair_only_in_a_word_class_the_table_lists():
    for (test, pair, cls), _ in _verdicts().items():
        assert cls in ran.TABLE[pair], f"{test}: {pair} is forced in word class {cls}, which the table does not list"


def test_every_forced_test_asserts_each_pair_in_each_word_class_it_runs():
    missing = [(test, pair, cls) for (test, pair, cls), vs in _verdicts().items() if not any(vs)]
    assert not missing, f"no case reaches the forced kernel, so none asserts that it ran: {missing}"


def test_every_table_entry_is_asserted_by_some_test():
    asserted = {(pair, cls) for (_, pair, cls), vs in _verdicts().items() if any(vs)}
    missing = [(pair, cls) for pair, by_cls in ran.TABLE.items() for cls in by_cls if (pair, cls) not in asserted]
    assert not missing, f"table entries that no test asserts: {missing}"


@pytest.mark.parametrize("pair", sorted(ran.TABLE, key=str))
def test_table_entries_are_well_formed(pair):
    for cls, e in ran.TABLE[pair].items():
        assert cls in ("u32", "u64f", "u64")
        assert e.last or e.ran or e.forward or e.inverse, (pair, cls)
        for item in e.ran + e.forward + e.inverse:
            assert isinstance(item, str) or (isinstance(item, tuple) and all(isinstance(s, str) for s in item))
        # what must run is never what must not
        musts = [s for item in e.ran + e.forward + e.inverse for s in ((item,) if isinstance(item, str) else item)]
        assert not [s for s in musts if s.startswith(tuple(e.absent))] if e.absent else True, (pair, cls)
