"""GPU tier (-m gpu): what the path setters (hd_set_path, hd_set_path_up, hd_set_path_multistep, hd_set_path_multistep_sde), the row
setters (hd_set_restraint, hd_set_steer) and the row check of hd_restrain_eps answer to calls they refuse - return code and
hd_last_error text, record for record against tests/golden/setter_refusals.json.  tests/make_golden_setter_refusals.py walks one
handle (T = 8, B = 2, N = 4) through its states and makes the calls (one thing wrong each, and some with two things wrong to pin
the order of the checks); none of them gets as far as a launch or an upload."""
import json

import pytest

from tests import make_golden_setter_refusals as gen

pytestmark = pytest.mark.gpu


def test_every_setter_refusal_keeps_its_code_and_text():
    from hierdiff_amd import _lib
    _lib.require_gpu()
    with open(gen.FIXTURE) as fh:
        want = json.load(fh)
    got = gen.records(_lib.load())
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert sum(k.startswith("two wrong|") for k in want) >= 20
    for entry in gen.ENTRY:
        assert any(k.startswith(entry + "|") or k.startswith("two wrong|" + entry + "|") for k in want), entry
        assert any(k.startswith("two wrong|" + entry + "|") for k in want), entry
