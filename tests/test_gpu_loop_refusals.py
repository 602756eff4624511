"""GPU tier (-m gpu): what the five sampling entry points and hd_nll_terms answer to calls they refuse - return code and
hd_last_error text, record for record against tests/golden/loop_refusals.json.  tests/make_golden_loop_refusals.py walks one handle
and one topology through every state and makes the calls (one thing wrong each, and a dozen with two things wrong where entry points
order their checks differently); none of them gets as far as a launch.  The same for what a caller attaches to the topology -
steering, diversity, framed restraints, a sink - and for the argument refusals of those terms' setters, attach calls and
single-transition entry points."""
import json

import pytest

from tests import make_golden_loop_refusals as gen

pytestmark = pytest.mark.gpu


def test_every_refusal_keeps_its_code_and_text():
    from hierdiff_amd import _lib
    _lib.require_gpu()
    with open(gen.FIXTURE) as fh:
        want = json.load(fh)
    got = gen.records(_lib.load())
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert sum(k.startswith("two wrong|") for k in want) >= 12
    for entry in gen.ENTRY:
        assert any(k.startswith(entry + "|") for k in want), entry
