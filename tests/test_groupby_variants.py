"""CPU: the library's variant registry (which compiled kernel instantiations exist) against the case table of
tests/groupby_variants.py. Together with tests/test_groupby_variants_gpu.py - every case proves on the GPU that it launches exactly
its labels, and checks the result - this means every compiled instantiation of the aggregate, partition and ring-scatter
families is run and checked, whatever the order or selection of the tests."""
import ctypes as C

import pytest

import groupby_variants as V
from cudf_amd import _lib


@pytest.fixture(scope="module")
def registry():
    _lib.profile_reset()  # (an earlier test of the same session may have launched kernels with profiling on)
    return _lib.profile_variants()


def test_registry_lists_every_instantiation_without_a_gpu(registry):
    """The registry is static data filled when the library is loaded: no device needed, and no launches since the reset."""
    assert {f for f, _ in registry} >= set(V.FAMILIES)
    assert all(n == 0 for n in registry.values())
    labels = [l for _, l in registry]
    assert len(labels) == len(set(labels)), "two instantiations registered one label"
    for family in V.FAMILIES:
        print(family, sum(1 for f, _ in registry if f == family), "instantiations")


def test_a_small_buffer_is_an_error_not_a_truncation():
    buf = C.create_string_buffer(64)
    with pytest.raises(ValueError, match="too small"):
        _lib.check(_lib.load().cudf_amd_profile_variants(buf, len(buf)))


def test_case_table_covers_every_registered_instantiation(registry):
    registered = {l for f, l in registry if f in V.FAMILIES}
    predicted = V.predicted_labels()
    unreachable = set(V.UNREACHABLE)
    assert not predicted & unreachable, sorted(predicted & unreachable)
    missing = registered - predicted - unreachable  # compiled, and no case launches it
    unknown = (predicted | unreachable) - registered  # the restatement names an instantiation the library does not have
    assert not missing and not unknown, f"registered but not covered: {sorted(missing)}\nnot registered: {sorted(unknown)}"


def test_case_names_are_unique_and_every_case_adds_to_the_table():
    names = [c.name for c in V.ALL_CASES]
    assert len(names) == len(set(names))
    for c in V.ALL_CASES:
        assert c.labels, c.name
        assert c.n <= 200_003 and c.n % 64 != 0 and c.n % 1024 != 0, c.name


def test_other_families_are_listed_not_required(registry):
    """The write-combining scatter (at least 2^22 rows: paths_hash.cpp) and the dense aggregate kernels are the follow-up."""
    others = sorted((f, l) for f, l in registry if f not in V.FAMILIES)
    assert others
    print(f"{len(others)} registered instantiations outside the case table:")
    for f, l in others:
        print(" ", f, l)


@pytest.mark.parametrize("keys,values,requests,error", V.OVER_LIMIT, ids=[e[3].replace(" ", "_") for e in V.OVER_LIMIT])
def test_restated_plan_refuses_what_the_planner_refuses(keys, values, requests, error):
    with pytest.raises(V.PlanError, match=error):
        V.Plan(keys, values, requests)


def test_restated_plan_of_known_shapes():
    p = V.Plan(["int64"], [("float64", False)], [(0, ["sum", "count_valid"])])  # the benchmark's plan
    assert (p.KU, p.NPAY, p.NACC, p.simple, p.flags_unit, p.sig()) == (1, 1, 2, True, -1, V.SUMF_CNT)
    p = V.Plan(["int64", "int32"], [("float64", True)], [(0, ["mean", "min", "max"])])  # C4: the flags ride in the key's spare half
    assert (p.KU, p.NPAY, p.NACC, p.simple, p.flags_unit, p.sig()) == (2, 1, 4, False, 1, V.MEAN_MIN_MAX_F_NULLS)
    p = V.Plan(["int64"], [("int64", True)], [(0, ["argmin"])])  # row id and flags share a unit
    assert (p.KU, p.NPAY, p.NACC, p.narg, p.flags_unit, p.sig()) == (1, 2, 3, 1, 2, "rt")
