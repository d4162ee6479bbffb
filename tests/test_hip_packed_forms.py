"""Every packed weight form of eavsr_amd.ops does what the recording says (tests/packed_forms.py, tests/golden/packed_forms.json):
the same library calls in the same order with the same scalar arguments, a buffer of the same dtype and size, the same cache and
tag, the same bytes -- and a second call is a hit."""
import pytest

from tests import packed_forms as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


def test_the_recording_names_every_case_and_most_of_them_by_their_bytes():
    gold = P.golden()
    assert sorted(gold) == sorted(P.BY_ID)
    nulls = [k for k, v in gold.items() if v["bytes"] is None]
    assert len(nulls) <= P.MAX_NULL_FRACTION * len(gold), nulls


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.id)
def test_a_packed_form_is_the_recorded_one(ops, cuda, case):
    want = P.golden()[case.id]
    ws = P.weights_of(case, cuda)
    seen, value = P.observe(ops, case, ws)      # (a lab-only form raises LabBuildRequired on the default library: a skip, tests/conftest.py)
    print(f"{case.id}: {seen}")
    for key in ("log", "packed", "grew"):
        assert seen[key] == want[key], f"{case.id}: {key}: {seen[key]} != {want[key]}"
    if want["bytes"] is not None:
        assert seen["bytes"] == want["bytes"], f"{case.id}: the packed bytes differ from the recording"
    again, hit = P.observe(ops, case, ws)
    assert again["log"] == [] and again["grew"] == [], f"{case.id}: a second call is no hit: {again}"
    assert all(a is b for a, b in zip(P._tensors(hit), P._tensors(value))) and type(hit) is type(value)
    assert hit is value
