"""CPU tier of the template restraints: the float64 restatement of tests/template_reference.py against itself (central differences,
rigid invariance, chirality, the exact fit), its mutants against the bars of tests/test_gpu_template.py on that test's inputs, and
the host side of hierdiff_amd.restraints (Template, the CPU energy, JSON, refusals, slicing)."""
import json
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import restraints as R
from hierdiff_amd.restraints import Restraints, Template
from tests import restraint_reference as rr
from tests import sampling_reference as sref
from tests import template_reference as tr


def rotation(seed):
    q, _ = np.linalg.qr(np.random.Generator(np.random.PCG64(seed)).normal(size=(3, 3)))
    return q if np.linalg.det(q) > 0 else -q


def small_case(seed=0, B=2, N=7):
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.normal(0.0, 1.5, (B, N, 3))
    nm = np.ones((B, N), dtype=bool)
    nm[1, N - 2:] = False
    rs = Restraints(templates=[Template([0, 2, 3, 5, 6, 2], g.normal(0.0, 1.5, (6, 3)), weights=[1.0, 0.5, 2.0, 1.0, 0.0, 1.5], k=1.5),
                               Template([1, 4, 0], g.normal(0.0, 1.5, (3, 3)) + 3.0, k=0.7, fit="translation")])
    return rs, x, nm


def total(rs, x, nm):
    return tr.template_energy_grad(rs, x, nm)[0].sum()


def test_gradient_against_central_differences():
    rs, x, nm = small_case()
    assert tr.worst_cond(rs, x, nm) >= tr.COND_MIN
    g = tr.template_energy_grad(rs, x, nm)[2]
    h, worst = 1e-5, 0.0
    for b in range(x.shape[0]):
        for i in range(x.shape[1]):
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[b, i, c] += h
                xm[b, i, c] -= h
                fd = (total(rs, xp, nm) - total(rs, xm, nm)) / (2 * h)
                worst = max(worst, abs(fd - g[b, i, c]))
    print(f"template gradient against central differences: worst |fd - g| {worst:.2e}")
    assert worst < 1e-7 and np.abs(g).max() > 0.1
    assert (g[1, -2:] == 0).all()                                # masked nodes gather nothing
    # the gradient is exact: the centroid term vanishes, sum_m w r = 0, so the gradient sums to 0 per template
    assert np.abs(g.sum(1)).max() < 1e-12


def test_rigid_motion_leaves_the_energy_and_rotates_the_gradient():
    rs, x, nm = small_case(1)
    rs = Restraints(templates=rs.templates[:1])                   # (a translation-only fit is invariant under translations alone)
    Q, s = rotation(3), np.array([4.0, -2.0, 7.0])
    U, _, g, _, _ = tr.template_energy_grad(rs, x, nm)
    U2, _, g2, _, _ = tr.template_energy_grad(rs, x @ Q.T + s, nm)
    assert np.abs(U2 - U).max() < 1e-12 * max(1.0, U.max()) and np.abs(g2 - g @ Q.T).max() < 1e-11
    rt = Restraints(templates=small_case(1)[0].templates[1:])
    U, _, g, _, _ = tr.template_energy_grad(rt, x, nm)
    U2, _, g2, _, _ = tr.template_energy_grad(rt, x + s, nm)
    assert np.abs(U2 - U).max() < 1e-12 * max(1.0, U.max()) and np.abs(g2 - g).max() < 1e-11


def test_a_mirror_image_does_not_fit_though_every_distance_does():
    g = np.random.Generator(np.random.PCG64(2))
    y = g.normal(0.0, 1.5, (5, 3))
    x = (y * np.array([1.0, 1.0, -1.0]))[None]                   # the mirror image of the template
    nm = np.ones((1, 5), dtype=bool)
    rs = Restraints(templates=Template(range(5), y, k=2.0))
    U = tr.template_energy_grad(rs, x, nm)[0][0, 0]
    pairs = [[i, j, d, d, 1.0] for i in range(5) for j in range(i + 1, 5) for d in [float(np.float32(np.linalg.norm(y[i] - y[j])))]]
    Up = rr.energy_grad(Restraints(pairs=pairs), x, nm)[0][0, 1]
    print(f"mirror image: U_tpl {U:.3f}, pair-distance energy {Up:.2e}")
    assert U > 0.1 and Up < 1e-10
    Ue, fit = rs.template_energy(torch.from_numpy(x), torch.ones(1, 5, 1))
    assert abs(float(Ue[0, 0]) - U) < 1e-12 * U and abs(float(torch.linalg.det(fit[0, 0, :9].reshape(3, 3))) - 1.0) < 1e-12


def test_an_exact_fit_has_no_energy_and_returns_the_template_frame():
    g = np.random.Generator(np.random.PCG64(4))
    y = g.normal(0.0, 1.5, (6, 3)).astype(np.float32).astype(np.float64)
    Q, s = rotation(5), np.array([3.0, -1.0, 2.0])
    x = (y @ Q.T + s)[None]
    rs = Restraints(templates=Template(range(6), y))
    U, _, gr, _, fits = tr.template_energy_grad(rs, x, np.ones((1, 6), dtype=bool))
    assert U[0, 0] < 1e-24 and np.abs(gr).max() < 1e-12 and np.abs(fits[0][0]["R"] - Q).max() < 1e-12
    res = rs.template_results(torch.from_numpy(x), torch.ones(1, 6, 1))
    assert res["x_template_frame"].dtype == torch.float64 and np.abs(res["x_template_frame"][0].numpy() - y).max() < 1e-12
    assert float(res["template_rmsd"][0, 0]) < 1e-12 and res["restraint_template_energy"].shape == (1, 1)


def gpu_bar_missed(c, mutant):
    """Whether the mutant's update leaves the element-wise bar of the kernel test on case c."""
    ref, mag = tr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known)
    bad, _ = tr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known, mutant=mutant)
    return bool((np.abs(bad - ref) > sref.BOUND * sref.U * mag).any())


def test_kernel_cases_are_conditioned_and_every_mutant_misses_the_bar():
    for N, D in ((5, 4), (33, 11)):
        for framed in (False, True):
            cases = list(tr.kernel_cases(N, D, framed))
            assert sum(c.degenerate for c in cases) <= 2
            missed = {m: 0 for m in tr.MUTANTS}
            for c in cases:
                cond = tr.worst_cond(c.rs, tr.data_prediction(c), c.nm.numpy())
                assert c.degenerate or cond >= tr.COND_MIN, (c.name, cond)
                assert not c.degenerate or cond < 1e-6, (c.name, cond)
                if c.degenerate:
                    continue
                for m in tr.MUTANTS:
                    missed[m] += int(gpu_bar_missed(c, m))
            print(f"N={N} D={D} framed={framed}: cases in which each mutant misses the bar {missed} of {len(cases) - 2}")
            assert all(v > 0 for v in missed.values()), missed


@pytest.mark.autograd
def test_template_energy_on_the_cpu_equals_the_restatement_and_autograd_the_gradient():
    for c in list(tr.kernel_cases(5, 4, False)) + list(tr.kernel_cases(33, 4, False))[:4]:
        x = torch.from_numpy(tr.data_prediction(c))
        U, _, g, _, fits = tr.template_energy_grad(c.rs, x.numpy(), c.nm.numpy())
        got, fit = c.rs.template_energy(x, c.nm.unsqueeze(-1))
        assert got.dtype == torch.float64 and np.abs(got.numpy() - U).max() <= 1e-12 * max(1.0, U.max()), c.name
        xr = x.clone().requires_grad_(True)
        R.template_energy_terms(c.rs, xr, c.nm.unsqueeze(-1)).sum().backward()
        if not c.degenerate:
            assert np.abs(xr.grad.numpy() - g).max() <= 1e-10 * max(1.0, np.abs(g).max()), c.name
            want = np.stack([np.stack([tr.fit16(f) for f in row]) for row in fits])
            assert np.abs(fit.numpy() - want).max() < 1e-10, c.name
        assert torch.isfinite(xr.grad).all() and torch.isfinite(fit).all()
    # a non-finite active coordinate: nothing from that template, the others unchanged
    rs, x, nm = small_case()
    x[0, 4, 1] = math.nan                                        # named by template 1 alone
    got, _ = rs.template_energy(torch.from_numpy(x), torch.from_numpy(nm).unsqueeze(-1))
    U = tr.template_energy_grad(rs, x, nm)[0]
    assert got[0, 1] == 0 and U[0, 1] == 0 and abs(float(got[0, 0]) - U[0, 0]) < 1e-12 * U[0, 0] and got[0, 0] > 0


def test_json_round_trip(tmp_path):
    d = {"obstacles": [[0.0, 0.0, 0.0, 1.0, 1.0]],
         "templates": [{"index": [0, 2, 3], "positions": [[0.0, 0.5, 1.0], [1.0, 0.0, 0.25], [2.0, 1.0, 0.0]], "weights": [1.0, 0.5, 2.0],
                        "k": 1.5, "fit": "translation"},
                       {"index": [1, 2], "positions": [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]}]}
    p = tmp_path / "r.json"
    p.write_text(json.dumps(d))
    rs = Restraints.from_json(str(p))
    assert rs.n_templates == 2 and rs.sizes == (1, 0, 0)
    t0, t1 = rs.templates
    assert t0.index.tolist() == [[0, 2, 3]] and t0.weights.tolist() == [[1.0, 0.5, 2.0]] and t0.k == 1.5 and t0.fit == "translation"
    assert t0.positions[0].tolist() == d["templates"][0]["positions"]
    assert t1.k == 1.0 and t1.fit == "rigid" and t1.weights.tolist() == [[1.0, 1.0]]
    idx, f, geom = rs.template_tables()
    assert idx.shape == (1, 2, 3) and idx[0, 1].tolist() == [1, 2, -1] and f[0, 1, 2].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert geom.tolist() == [[1.5, 1.0], [1.0, 0.0]]
    for bad in ({"templates": {}}, {"templates": [{"index": [0]}]}, {"templates": [{"index": [0], "positions": [[0, 0, 0]], "scale": 1}]},
                {"template": []}):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            Restraints.from_json(str(p))


def test_every_refusal():
    y = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    ok = Template([0, 1, 2], y)
    bad = [dict(index=[0, 1], positions=y), dict(index=[], positions=[]), dict(index=[0, 1.5, 2], positions=y),
           dict(index=[0, -2, 2], positions=y), dict(index=[0, 1, math.nan], positions=y), dict(index="abc", positions=y),
           dict(index=[0, 1, 2], positions=[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), dict(index=[0, 1, 2], positions=[y[0], y[1], [0.0, math.inf, 0.0]]),
           dict(index=[0, 1, 2], positions=[y[0], y[1], [0.0, math.nan, 0.0]]), dict(index=[0, 1, 2], positions=y, weights=[1.0, 1.0]),
           dict(index=[0, 1, 2], positions=y, weights=[1.0, -1.0, 1.0]), dict(index=[0, 1, 2], positions=y, weights=[1.0, math.inf, 1.0]),
           dict(index=[0, 1, 2], positions=y, weights=[1.0, math.nan, 1.0]), dict(index=[0, 1, 2], positions=y, k=-1.0),
           dict(index=[0, 1, 2], positions=y, k=math.inf), dict(index=[0, 1, 2], positions=y, k=math.nan), dict(index=[0, 1, 2], positions=y, k="1"),
           dict(index=[0, 1, 2], positions=y, fit="scaling"), dict(index=[0, 1, 2], positions=y, fit=None),
           dict(index=[[0, 1, 2]] * 2, positions=[y] * 3)]
    for kw in bad:
        with pytest.raises(ValueError):
            Template(**kw)
    with pytest.raises(ValueError):
        Restraints(templates=[ok] * 5)
    with pytest.raises(ValueError):
        Restraints(templates=[ok, "no"])
    with pytest.raises(ValueError):
        Restraints(templates=[Template([[0, 1, 2]] * 2, y), Template([[0, 1, 2]] * 3, y)])
    with pytest.raises(ValueError):
        Restraints(templates=Template([[0, 1, 2]] * 2, y)).check_batch(3)
    with pytest.raises(ValueError):
        Restraints().template_energy(torch.zeros(1, 3, 3), torch.ones(1, 3, 1))
    Restraints(templates=Template([[0, 1, 2]] * 2, y)).check_batch(2)
    assert Restraints(templates=ok).n_templates == 1 and Restraints(templates=[ok] * 4).n_templates == 4 and Restraints().n_templates == 0


def test_slicing():
    g = np.random.Generator(np.random.PCG64(6))
    per = Template(g.integers(0, 5, (4, 3)), g.normal(size=(4, 3, 3)), g.uniform(0.5, 1.0, (4, 3)), k=2.0)
    shared = Template([0, 1, 2], g.normal(size=(3, 3)), fit="translation")
    rs = Restraints(templates=[per, shared])
    assert rs.template_rows() == 4
    cut = rs.slice(1, 3)
    assert cut.template_rows() == 2 and cut.templates[1] is shared
    assert torch.equal(cut.templates[0].index, per.index[1:3]) and torch.equal(cut.templates[0].positions, per.positions[1:3])
    assert torch.equal(cut.templates[0].weights, per.weights[1:3]) and cut.templates[0].k == 2.0
    x, nm = torch.from_numpy(g.normal(size=(4, 5, 3))), torch.ones(4, 5, 1)
    whole = rs.template_energy(x, nm)[0]
    assert torch.equal(cut.template_energy(x[1:3], nm[1:3])[0], whole[1:3])
    cut.check_batch(2)
    with pytest.raises(ValueError):
        cut.check_batch(4)


# ----------------------------------------------------------------------------- the steered fixture of the GPU tier

@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_steered_reference_is_far_from_every_boundary(precision):
    """The steered chain with templates only (tests/template_reference.steered_reference): some transitions resample and some do not,
    and every resampling point and ESS threshold lies MARGIN_FACTOR times further from a boundary than the reference moves when its
    network runs in float64 instead of fp32 - the noise a device network within the chain bar can have."""
    from tests import steer_reference as st
    a = tr.steered_reference(precision)
    b = tr.steered_reference(precision, dtype=torch.float64)
    noise, same = st.cumulative_difference(a[1], b[1])
    margin = min(min(i["margin"], i["margin_ess"]) for i in a[1])
    res = [i["resampled"].tolist() for i in a[1]]
    print(f"steered template fixture [{precision}]: resampled {res}; smallest margin {margin:.3g}, fp32-vs-float64 noise {noise:.3g}")
    assert same and margin > st.MARGIN_FACTOR * noise
    assert any(any(r) for r in res) and not all(all(r) for r in res)
    assert all(np.isfinite(i["U"]).all() for i in a[1])
