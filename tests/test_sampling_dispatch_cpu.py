"""CPU tier: which library calls every Python sampling entry point makes, in which order, and the scalars its loop entry point gets,
against the recorded traces of tests/golden/sampling_dispatch.json (tests/make_golden_dispatch.py: the matrix, the stubs and the
generator).  The stub technique of test_guidance_cpu.py::test_unguided_defaults_reach_no_guided_call, over every entry point crossed
with steps / eta / solver / guidance / keep_frames + record / restraints / injected noise / fix_noise / k_lo > 0."""
import json

import pytest

from tests import make_golden_dispatch as gd


@pytest.fixture(scope="module")
def golden():
    with open(gd.FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_the_whole_matrix(golden):
    assert golden["matrix"] == {"accepts": gd.ACCEPTS, "options": gd.OPTIONS}
    assert {e: len(v) for e, v in golden["rows"].items()} == {e: sum(1 for _, e2, _ in gd.matrix() if e2 == e) for e in gd.ACCEPTS}
    used = [row for v in golden["rows"].values() for row in v if not isinstance(row, str)]
    assert {c for c, _ in used} == set(range(len(golden["calls"]))) and {a for _, a in used} == set(range(len(golden["args"])))
    assert {c[-1] for c in golden["calls"]} == set(gd.LOOPS)          # every loop entry point is reached by some row


@pytest.mark.parametrize("entry", list(gd.ACCEPTS))
def test_entry_point_reaches_the_recorded_calls(golden, entry):
    case = gd.Case()
    rows = [(key, opt) for key, e, opt in gd.matrix() if e == entry]
    assert rows
    for i, (key, opt) in enumerate(rows):
        got = gd.trace(case, entry, opt)                 # (asserts itself that an argument error comes before any library call)
        assert got == gd.expected(golden, entry, i), key
