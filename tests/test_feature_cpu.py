"""CPU tier of the feature restraints: the float64 restatement of tests/feature_reference.py against the product's differentiable
torch formulas, the bounds, the host side of hierdiff_amd.restraints (Features, FeatureSum, JSON, refusals, the ratio, slicing), the
exported symbols, the mutants and the fp32 twin against the bars of tests/test_gpu_feature.py on that test's inputs, and the input
conditions of its kernel cases and chains.

Measured here (printed by the tests).  Over the kernel cases of N in {5, 33} x F in {1, 8}: the fp32 twin's worst error is 0.100 of the
element-wise bar (8 * 2^-23 of the sum of the absolute terms); the smallest miss of a mutant is 1.3e4 bars (`masked_in_n`, N = 33,
F = 1).  `clip_per_element` equals the per-node clip at F = 1 and misses at F = 8 only (1.7e6 bars and more)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, restraints, steering
from hierdiff_amd.restraints import Features, FeatureSum, Restraints, feature_energy_terms, feature_ratio
from tests import feature_reference as fr
from tests import sampling_reference as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 1), (5, 8), (33, 1), (33, 8)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ----------------------------------------------------------------------------- the formulas

@pytest.mark.autograd
def test_autograd_of_the_product_equals_the_analytic_gradient_of_the_restatement():
    """feature_energy_terms' autograd gradient against the restatement's hand-written one: 1e-12 relative (of the gradient's largest
    element per case); the energies and the m_r to 1e-12 too."""
    worst = 0.0
    for N, F in SHAPES:
        for c in fr.kernel_cases(N, F):
            v = fr.v_f32(c.z, c.eps, c.row[0], c.row[1], c.nv1, c.nb1).double()
            U, g, _, m, _ = fr.feature_energy_grad(c.ft, v.numpy(), c.nm)
            h = v.clone().requires_grad_(True)
            Ut, mt = feature_energy_terms(c.rs, h, c.nm.unsqueeze(-1))
            Ut.sum().backward()
            got = torch.nan_to_num(h.grad, nan=0.0).numpy() * c.nm.numpy()[:, :, None]
            scale = max(1.0, float(np.abs(g).max()))
            err = float(np.abs(got - g).max()) / scale
            worst = max(worst, err)
            assert err <= 1e-12, (N, F, c.name, err)
            assert np.abs(Ut.detach().numpy() - U).max() <= 1e-12 * max(1.0, np.abs(U).max()), c.name
            assert m.size == 0 or np.abs(mt.detach().numpy() - m).max() <= 1e-12 * max(1.0, np.abs(m).max()), c.name
    print(f"autograd vs analytic gradient: worst relative difference {worst:.2e}")


def test_energy_is_zero_on_a_bound_and_positive_on_either_side():
    nm = torch.ones(1, 2, 1)
    rs = Restraints(features=Features([[1.0, -2.0], [0.5, 0.5]], [[2.0, -2.0], [math.inf, 3.0]], k=2.0,
                                      sums=[FeatureSum([1.0, 1.0], lo=0.0, hi=4.0, k=3.0), FeatureSum([1.0, 0.0], lo=1.5, hi=1.5, reduce="mean")]))
    on = torch.tensor([[[2.0, -2.0], [0.5, 3.0]]], dtype=torch.float64)           # every element on a bound; sum 3.5 inside, mean 1.25 below
    U, m = rs.feature_energy(on, nm, return_sums=True)
    assert float(U[0, 0]) == 0.0 and m.tolist() == [[3.5, 1.25]] and float(U[0, 1]) == 0.5 * 0.25 ** 2
    eps = 1e-3
    for i, c, sign in ((0, 0, 1), (0, 1, 1), (0, 1, -1), (1, 0, -1), (1, 1, 1)):
        h = on.clone()
        h[0, i, c] += sign * eps
        Ub = float(rs.feature_energy(h, nm)[0, 0])
        assert abs(Ub - 0.5 * 2.0 * eps ** 2) <= 1e-12 * eps ** 2, (i, c, sign, Ub)
    h = on.clone()
    h[0, 0, 0] -= 0.5                                         # inside [1, 2]: still 0
    assert float(rs.feature_energy(h, nm)[0, 0]) == 0.0
    # the sum row exactly on its bounds, and outside
    rs2 = Restraints(features=Features(sums=[FeatureSum([1.0, 1.0], lo=0.0, hi=3.5, k=3.0)]))
    assert float(rs2.feature_energy(on, nm)[0, 1]) == 0.0
    h = on.clone()
    h[0, 0, 0] += 0.25
    assert abs(float(rs2.feature_energy(h, nm)[0, 1]) - 0.5 * 3.0 * 0.25 ** 2) < 1e-15
    h[0, 0, 0] -= 4.0
    assert abs(float(rs2.feature_energy(h, nm)[0, 1]) - 0.5 * 3.0 * 0.25 ** 2) < 1e-15
    # the restatement agrees
    U2, _, _, m2, _ = fr.feature_energy_grad(rs.features, on.numpy(), np.ones((1, 2)))
    assert U2.tolist() == U.tolist() and m2.tolist() == m.tolist()
    # a non-finite element has no band term, and a row that reads it contributes nothing; the other row stays
    h = on.clone()
    h[0, 0, 1] = float("nan")
    U, m = rs.feature_energy(h, nm, return_sums=True)
    assert float(U[0, 0]) == 0.0 and m.tolist() == [[0.0, 1.25]] and float(U[0, 1]) == 0.5 * 0.25 ** 2
    # no valid node: nothing
    U, m = rs.feature_energy(on, torch.zeros(1, 2, 1), return_sums=True)
    assert U.tolist() == [[0.0, 0.0]] and m.tolist() == [[0.0, 0.0]]


# ----------------------------------------------------------------------------- the host side

def test_containers_shapes_slicing_and_the_batch_check():
    ft = Features.target(np.zeros((2, 3, 4)), k=np.ones(4), tol=0.5, sums=[FeatureSum(np.ones(4), hi=[1.0, 2.0])])
    assert (ft.F, ft.W, ft.S, ft.band_rows(), ft.sum_rows()) == (4, 3, 1, 2, 2)
    assert torch.equal(ft.lo, torch.full((2, 3, 4), -0.5)) and torch.equal(ft.hi, torch.full((2, 3, 4), 0.5))
    rs = Restraints(features=ft)
    assert rs.feature_sizes == (3, 1) and rs.feature_rows() == (2, 2) and rs.sizes == (0, 0, 0)
    rs.check_batch(2)
    with pytest.raises(ValueError, match="feature"):
        rs.check_batch(3)
    one = rs.slice(1, 2)
    assert one.features.band_rows() == 1 and one.features.sums[0].hi.tolist() == [2.0] and one.feature_rows() == (1, 1)
    shared = Restraints(features=Features(hi=np.ones((3, 4)), sums=FeatureSum(np.ones(4), lo=0.0)))
    assert shared.slice(0, 1).features.lo is shared.features.lo and shared.features.lo.shape == (1, 3, 4)
    assert bool(torch.isinf(shared.features.lo).all()) and Restraints().feature_sizes == (0, 0)
    lo, hi, k, coef, f = ft.tables()
    assert lo.shape == hi.shape == k.shape == (2, 3, 4) and coef.shape == (2, 1, 4) and f.shape == (2, 1, 4)
    assert f[:, 0].tolist() == [[-math.inf, 1.0, 1.0, 0.0], [-math.inf, 2.0, 1.0, 0.0]]
    only = Features(sums=[FeatureSum([1.0, 0.0], reduce="mean")]).tables()
    assert only[0].shape == (1, 0, 2) and only[4][0, 0].tolist() == [-math.inf, math.inf, 1.0, 1.0]
    # steering: per-molecule rows must agree inside a group
    st = steering.Steer(2, 1.0, 0.5, None)
    nm = torch.ones(2, 3, 1)
    steering.check_groups(st, nm, None, shared, None)
    with pytest.raises(ValueError, match="features"):
        steering.check_groups(st, nm, None, rs, None)


def test_json_round_trip_reproduces_the_tables(tmp_path):
    c = next(iter(fr.kernel_cases(5, 8)))
    cases = [c.ft, fr.chain_features(), Features(sums=[FeatureSum([1.0, -1.0], hi=5.0, reduce="mean")]),
             list(fr.kernel_cases(5, 8))[3].ft]
    for n, ft in enumerate(cases):
        p = tmp_path / f"r{n}.json"
        p.write_text(json.dumps({"obstacles": [[0, 0, 0, 1.0, 1.0]], "features": ft.to_dict()}))
        back = Restraints.from_json(str(p))
        assert back.sizes == (1, 0, 0)
        for a, b in zip(ft.tables(), back.features.tables()):
            assert a.shape == b.shape and torch.equal(a, b)
    p = tmp_path / "t.json"
    p.write_text(json.dumps({"features": {"bands": {"target": [[1.0, 2.0]], "tol": 0.5, "k": 2.0},
                                          "sums": [{"coef": [1, 1], "hi": 5, "reduce": "mean"}]}}))
    ft = Restraints.from_json(str(p)).features
    assert ft.lo.tolist() == [[[0.5, 1.5]]] and ft.hi.tolist() == [[[1.5, 2.5]]] and ft.k.tolist() == [[[2.0, 2.0]]]
    assert ft.sums[0].reduce == "mean" and ft.sums[0].hi.tolist() == [5.0] and math.isinf(float(ft.sums[0].lo[0]))
    for bad in ({"features": []}, {"features": {"bands": {"lo": [[0.0]], "target": [[0.0]]}}}, {"features": {"else": 1}},
                {"features": {"sums": [{"lo": 0}]}}, {"features": {"sums": {"coef": [1]}}}, {"features": {"sums": [{"coef": [1], "reduce": "max"}]}},
                {"features": {"bands": {"lo": [[2.0]], "hi": [[1.0]]}}}, {"features": {}}):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            Restraints.from_json(str(p))


def test_every_refusal_is_a_value_error_on_the_host():
    nan, inf = math.nan, math.inf
    ok = np.zeros((3, 2))
    bad_features = [
        dict(), dict(lo=ok, hi=ok - 1.0), dict(lo=np.full((3, 2), nan)), dict(hi=np.full((3, 2), nan)), dict(lo=ok, k=nan), dict(lo=ok, k=inf),
        dict(lo=ok, k=-1.0), dict(lo=ok, k=np.ones(5)), dict(lo=np.zeros(3)), dict(lo=np.zeros((1, 2, 3, 4))), dict(lo=ok, hi=np.zeros((3, 3))),
        dict(lo=ok, k=True), dict(lo="x"), dict(lo=ok, sums=[FeatureSum([1.0, 1.0, 1.0])]), dict(lo=ok, sums="x"), dict(lo=ok, sums=[1]),
        dict(sums=[FeatureSum([1.0])] * 9), dict(sums=[FeatureSum([1.0], hi=[1.0, 2.0]), FeatureSum([1.0], hi=[1.0, 2.0, 3.0])]),
        dict(sums=[FeatureSum([1.0]), FeatureSum([1.0, 2.0])]),
    ]
    for kw in bad_features:
        with pytest.raises(ValueError):
            Features(**kw)
    bad_sums = [dict(coef=[nan]), dict(coef=[inf]), dict(coef=[[1.0]]), dict(coef=[]), dict(coef="x"), dict(coef=True), dict(coef=[1.0], lo=nan),
                dict(coef=[1.0], hi=nan), dict(coef=[1.0], lo=2.0, hi=1.0), dict(coef=[1.0], k=nan), dict(coef=[1.0], k=inf), dict(coef=[1.0], k=-1.0),
                dict(coef=[1.0], reduce="max"), dict(coef=[1.0], reduce=1), dict(coef=[1.0], lo=[[0.0]]), dict(coef=[1.0], lo=[0.0, 1.0], hi=[1.0, 2.0, 3.0])]
    for kw in bad_sums:
        with pytest.raises(ValueError):
            FeatureSum(**kw)
    for kw in (dict(values=[[nan]]), dict(values=None), dict(values=[[0.0]], tol=-1.0), dict(values=[[0.0]], tol=nan), dict(values=[[0.0]], tol=np.ones(3))):
        with pytest.raises(ValueError):
            Features.target(**kw)
    with pytest.raises(ValueError):
        Restraints(features=[1])
    rs = Restraints(features=Features(lo=ok))
    with pytest.raises(ValueError):
        rs.feature_energy(torch.zeros(1, 3, 3), torch.ones(1, 3, 1))              # F
    with pytest.raises(ValueError):
        rs.feature_energy(torch.zeros(1, 2, 2), torch.ones(1, 2, 1))              # W > N
    with pytest.raises(ValueError):
        Restraints().feature_energy(torch.zeros(1, 3, 2), torch.ones(1, 3, 1))    # no features
    # F against the model's feature width, before a device is looked at
    from tests import edit_reference as er
    sd_np, _ = er.weights(32, 2)
    model = er.cpu_diffusion(sd_np, 32, 2, 8)
    with pytest.raises(ValueError, match="channels"):
        restraints.resolve(model, rs, 1.0, "score", None, 1)
    assert restraints.resolve(model, Restraints(features=fr.chain_features()), 1.0, "score", None, 4) is not None


def test_the_ratio_follows_the_schedule():
    assert feature_ratio("score", 2.0, 5.0) == 2.5 and feature_ratio("sigma", 2.0, 5.0) == 1.0
    assert feature_ratio([0.1, 0.2], 2.0, 5.0) == 1.0 and feature_ratio(np.ones(3), 2.0, 5.0) == 1.0


def test_feature_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in ("hd_restraint_features", "hd_restrain_feat", "hd_restraint_feature_energy"):
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} not declared in the header"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+HD_MAX_FEATURE_SUMS\s+8\b", hdr) and restraints.MAX_FEATURE_SUMS == 8


# ----------------------------------------------------------------------------- the GPU tier's inputs and bars

def _ratio(a, ref, mag):
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.abs(a - ref) / np.maximum(sref.BOUND * sref.U * mag, 1e-300)))


def test_kernel_cases_meet_the_input_conditions():
    for N, F in SHAPES:
        for c in fr.kernel_cases(N, F):
            out_, in_, on, rows = fr.input_conditions(c)
            assert fr.conditions_hold(c), (N, F, c.name, out_, in_, on, rows)
            assert c.ft.lo is None or (out_ >= 0.25 and in_ >= 0.1 and on >= 1), (N, F, c.name)
            assert all(v > 0 and s > 0 for v, s in rows), (N, F, c.name, rows)
            nm = c.nm.numpy()
            assert nm.sum(1).tolist()[2:4] == [1, 0] and float(c.scale[1]) == 0.0 and torch.isnan(c.z[fr.NAN_AT[0], fr.NAN_AT[1], 3 + fr.NAN_AT[2]])
            assert nm[fr.NAN_AT[0], fr.NAN_AT[1]] and c.ratio != 1.0 and (c.nv1, c.nb1) == (1.7, 0.3)


def test_every_mutant_misses_the_bar_and_the_twin_alone_stays_within():
    smallest, twin_worst = {}, 0.0
    for N, F in SHAPES:
        miss = {m: 0.0 for m in fr.MUTANTS}
        for c in fr.kernel_cases(N, F):
            args = (c.ft, c.z, c.eps, c.nm, c.scale, c.row, c.nv1, c.nb1, c.ratio)
            ref, mag = fr.restrain_feat_ref(*args)
            twin = fr.restrain_feat_twin(*args)
            r = _ratio(twin.double().numpy(), ref, mag)
            twin_worst = max(twin_worst, r)
            assert r <= 1.0, (N, F, c.name, r)
            e = c.eps.numpy()
            assert (twin.numpy()[:, :, :3] == e[:, :, :3]).all() and (twin.numpy()[~c.nm.numpy()] == e[~c.nm.numpy()]).all()
            assert (twin.numpy()[1] == e[1]).all()            # s_b = 0
            for m in fr.MUTANTS:
                bad, _ = fr.restrain_feat_ref(*args, mutant=m)
                miss[m] = max(miss[m], _ratio(bad, ref, mag))
        print(f"N={N} F={F}: largest miss of each mutant, in bars: " + ", ".join(f"{m} {v:.3g}" for m, v in miss.items()))
        for m, v in miss.items():
            if m == "clip_per_element" and F == 1:            # one channel: the element is the node
                assert v == 0.0
                continue
            assert v > 1.0, (N, F, m, v)
            smallest[m] = min(smallest.get(m, math.inf), v)
    print(f"the fp32 twin's worst error: {twin_worst:.3f} of the bar; the smallest miss of a mutant: {min(smallest.values()):.3g} bars "
          f"({min(smallest, key=smallest.get)})")
    assert set(smallest) == set(fr.MUTANTS)


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_the_feature_term_changes_eps_in_every_network_call_of_every_chain(precision):
    """On the CPU with the oracle's forward.  The steered chain runs with restraint_scale = 0 - selection on U_feat alone - so there
    it is the weights that must move: it resamples, with margins far above the fp32 noise of the energies."""
    for kind in fr.CHAIN_KINDS:
        c = fr.chain_reference(kind, precision)
        R = c.get("R", 1)
        assert c["calls"] == fr.CHAIN_K * R, (kind, c["calls"])
        if kind == "steered":
            res = [bool(i["resampled"].any()) for i in c["infos"]]
            margin = min(min(i["margin"], i["margin_ess"]) for i in c["infos"])
            print(f"steered chain [{precision}]: resampled {res}; smallest margin {margin:.3g}")
            assert any(res) and margin > 1e-3 and c["active"] == 0
            continue
        assert c["active"] == c["calls"], (kind, c["active"], c["calls"])
        d = float(np.linalg.norm(c["states"][-1].numpy() - c["plain"].numpy()) / np.linalg.norm(c["plain"].numpy()))
        print(f"chain {kind} [{precision}]: the feature term moved eps^ in {c['active']} of {c['calls']} network calls; distance of the "
              f"featured z_0 from the unfeatured one {d:.2e}")
        assert d > 1e-3
