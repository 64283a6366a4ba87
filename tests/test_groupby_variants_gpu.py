"""GPU: one call per case of tests/groupby_variants.py. Each case must launch exactly the kernel instantiations the restated
dispatch predicts (the library's variant registry counts launches per instantiation) and agree with the CPU oracle: keys,
integers, counts, MIN / MAX and ARGMIN / ARGMAX exactly, float sums within kat.sum_atol of the largest group (the generated float
columns hold multiples of 0.5, so these are exact too)."""
import pytest

import groupby_variants as V
import kat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


@pytest.fixture
def counting():
    """Launch counting on for the test, zeroed, and off again afterwards."""
    from cudf_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        yield _lib
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()


def _run(G, oracle, monkeypatch, counting, case, keys, requests):
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)

    def launched_exactly_the_predicted_labels():
        launched = {l: n for (f, l), n in counting.profile_variants().items() if f in V.FAMILIES and n > 0}
        print(case.name, G.last_path.name, launched)
        not_launched = case.labels - set(launched)
        assert not not_launched, f"predicted but not launched: {sorted(not_launched)}; launched: {sorted(launched)}"
        others = set(launched) - case.labels
        assert not others, f"launched but not predicted: {sorted(others)}"
    counting.profile_reset()
    kat.check_groupby_against_oracle(G, oracle, keys, requests, after_call=launched_exactly_the_predicted_labels)


@pytest.mark.parametrize("case", V.CASES, ids=repr)
def test_hash_groupby_instantiation(G, oracle, monkeypatch, counting, case):
    _run(G, oracle, monkeypatch, counting, case, *V.build_inputs(case))


@pytest.mark.parametrize("case", V.RING_CASES, ids=repr)
def test_ring_scatter_instantiation(G, oracle, monkeypatch, counting, case):
    _run(G, oracle, monkeypatch, counting, case, *V.build_ring_inputs(case))
    assert G.last_path.name == "DENSE_DIRECT"


@pytest.mark.parametrize("keys,values,requests,error", V.OVER_LIMIT, ids=[e[3].replace(" ", "_") for e in V.OVER_LIMIT])
def test_one_wider_than_a_plan_limit_is_refused(G, keys, values, requests, error):
    from cudf_amd._lib import CudfAmdError
    k, r = V.small_inputs(keys, values, requests)
    with pytest.raises(CudfAmdError, match=error):
        G.groupby(k, r)
