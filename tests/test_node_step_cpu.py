"""CPU tier of the node-step harness: the float32 evaluation of the restatement (tests/node_step_reference.py) stays inside the
bars committed for the GPU tier (tests/test_gpu_node_step.py) on every batch and variant, every named mutant of the restatement
is rejected by them, and hd_node_step is exported and fails cleanly without a handle."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import node_step_reference as nsr

H = 64
CASES = [(b, v) for b in ("small", "wide") for v in nsr.VARIANTS] + [(b, "plain") for b in nsr.BATCHES if b not in ("small", "wide")]
CASES += [("long", "mean")]


def test_batches_are_the_rows_the_thresholds_need():
    for batch, rows in nsr.ROWS.items():
        assert nsr.table(batch)["M"] == rows == sum(nsr.BATCHES[batch][0])
    small, at = nsr.table("small"), nsr.table("f32_at")
    assert small["M"] % 32 == 20 and small["M"] % 16 == 4 and at["M"] == 169 * 32 + 14 and nsr.table("f16_at")["M"] % 32 == 0
    assert np.array_equal(at["pstart"][:53], small["pstart"])
    wide = nsr.table("wide")
    assert wide["M"] == sum(nsr.BATCHES["wide"][0]) + 1                  # the padded node an unmasked edge makes active
    dead = nsr.masked_active_rows(wide)
    assert len(dead) == 1 and np.diff(wide["pstart"])[dead[0]] == 1      # ... with a part row of its own
    assert np.diff(wide["pstart"]).max() == 4 and np.diff(wide["pstart"])[nsr.zero_row(wide)] == 0
    parts = np.diff(nsr.table("long")["pstart"])
    assert parts.min() == 7 and parts.max() == 8                         # the longest part chains of the harness


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("layer", nsr.LAYERS)
@pytest.mark.parametrize("batch,variant", CASES)
def test_float32_evaluation_stays_inside_its_own_bars(batch, variant, layer, scaled):
    """Ratio 1 by construction - and the properties the bars lean on: no reference row of h' or AB is entirely zero except where an
    exact zero is demanded, everything is finite."""
    tab, inp = nsr.table(batch), nsr.inputs(batch, H, variant, scaled)
    w = nsr.layer_weights(nsr.state_dict(H, variant), layer, scaled)
    r64, e32 = nsr.reference(batch, H, variant, layer, scaled)
    r32 = nsr.node_step(inp, tab, w, nsr.norm_of(batch, variant), float32=True)
    for f16 in (False, True):
        assert nsr.check(r32, r64, e32, tab, w, f16, True) == []
    demanded = np.zeros(tab["M"], dtype=bool)
    if layer >= 0:
        demanded[nsr.masked_active_rows(tab)] = True
    elif variant == "zero":
        demanded[nsr.zero_row(tab)] = True                               # AB only, on a zero row of h: [b1 | 0]
    assert np.array_equal(~r64["h"].any(1), demanded)
    for ab in r64["AB"]:
        assert ab[:, :H].any(1).all()                                    # (a masked row's A half is b1)
        assert np.array_equal(~ab[:, H:].any(1), demanded)
    assert all(np.isfinite(a).all() for a in [r64["h"]] + r64["AB"])
    assert 0 < e32["h"] < 1e-5 or layer < 0
    if variant == "zero" and layer >= 0:                                 # X = 0: T = SiLU(b3), h' = T W4^T + b4
        r, n = nsr.zero_row(tab), w["node"]
        T = n["b3"] / (1.0 + np.exp(-n["b3"]))
        assert not inp["h"][r].any() and not inp["part"][tab["pstart"][r]:tab["pstart"][r + 1]].any()
        assert np.allclose(r64["T"][r], T, rtol=1e-14, atol=0) and np.allclose(r64["h"][r], T @ n["W4"].T + n["b4"], rtol=1e-13, atol=1e-16)
    if variant == "negbias" and layer >= 0:
        assert np.abs(r64["T"]).max() < 1e-10


MUTANT_CASES = {        # mutant -> (batch, variant, layer) it is rejected on
    "lastpart": ("long", "plain", 0), "nonorm": ("small", "plain", 0), "maskfirst": ("wide", "plain", 1), "b1both": ("small", "plain", -1),
    "swapab": ("small", "plain", 1), "round11": ("small", "plain", 0), "spikeround": ("small", "spike", 0), "ragged": ("small", "plain", 1),
    "maxpremask": ("wide", "plain", 1),
}


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("mutant", sorted(nsr.MUTANTS))
def test_every_mutant_is_rejected_at_the_committed_margins(mutant, f16):
    """The mutant, evaluated in float32 like the yardstick, misses a check of the GPU tier on its named case - under the exact-fp32
    margins and under the fp16x3 one."""
    assert set(MUTANT_CASES) == set(nsr.MUTANTS)
    batch, variant, layer = MUTANT_CASES[mutant]
    tab, inp = nsr.table(batch), nsr.inputs(batch, H, variant, f16)
    w = nsr.layer_weights(nsr.state_dict(H, variant), layer, f16)
    r64, e32 = nsr.reference(batch, H, variant, layer, f16)
    got = nsr.node_step(inp, tab, w, nsr.norm_of(batch, variant), float32=True, mutant=mutant)
    bad = nsr.check(got, r64, e32, tab, w, f16, True)
    assert bad, f"mutant {mutant} ({nsr.MUTANTS[mutant]}) passes every check on {batch} / {variant} / layer {layer}"
    if mutant == "maxpremask":
        assert all(b.startswith("abmax") for b in bad)
    if mutant == "spikeround":                  # ... and the rows it spares stay inside their bars
        rest = np.setdiff1d(np.arange(tab["M"]), nsr.spike_rows(tab["M"]))
        assert nsr.err(got["h"][rest], r64["h"][rest]) <= nsr.bar(nsr.family("h", f16), e32["h"])


def test_margins_follow_the_rule():
    assert set(nsr.MARGINS) == {"NH", "NA", "NX"}
    for m in nsr.MARGINS.values():
        assert 1.0 <= m <= 32.0 and np.log2(m) == int(np.log2(m))


def test_entry_is_exported_and_fails_cleanly_without_a_handle():
    from hierdiff_amd import _lib
    lib = _lib.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "hierdiff_hip.h").read_text()
    m = re.search(r"\bint hd_node_step\(([^;]*)\);", header)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES["hd_node_step"][1]) == 12
    path = C.c_int(-7)
    assert lib.hd_node_step(None, None, 0, None, None, None, None, None, None, None, C.byref(path), None) == -1
    assert "hd_node_step" in lib.hd_last_error().decode() and path.value == -7
