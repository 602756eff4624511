"""CPU tier of diverse sampling: the C ABI (symbols, argument errors without a device), the float64 restatement of
tests/diversity_reference.py against autograd through `diversity.energy_terms` (the envelope claim: the gradient is exact without
dR/dx), its fp32 twin and its mutants against the element-wise bar of the GPU tier on the GPU tier's inputs, the conditioning margins of
those inputs, the mirror-image property, and every refusal of `Diversity`, the plan and the Python entry points."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, diversity, plan as hplan
from hierdiff_amd.diversity import Diversity
from hierdiff_amd.restraints import Restraints
from tests import diversity_reference as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hd_set_diversity", "hd_diversity_attach", "hd_diversity_detach", "hd_diverse_eps", "hd_diversity_energy"]
SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]


def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


@pytest.fixture(scope="module")
def cases():
    """The kernel cases of the GPU tier at N in {5, 33} (D does not enter the x columns; D = 4), and the P = 32 case."""
    return [c for N in (5, 33) for c in dr.kernel_cases(N, 4)] + [dr.big_case()]


# ----------------------------------------------------------------------------- the C ABI

def test_symbols_exported_declared_and_null_safe():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.hd_version() == 12
    r4 = (C.c_float * 4)(0.8, 0.6, 1.0, math.inf)
    one = (C.c_float * 1)(1.0)
    assert lib.hd_set_diversity(None, 1, r4) == -1 and b"hd_set_diversity" in lib.hd_last_error()
    assert lib.hd_diversity_attach(None, 4, 1.0, 1.0, one, 1, 1.0, None) == -1 and b"null topology" in lib.hd_last_error()
    assert lib.hd_diversity_detach(None) == 0
    assert lib.hd_diverse_eps(None, None, None, None, r4, None, None) == -1 and b"hd_diverse_eps" in lib.hd_last_error()
    assert lib.hd_diversity_energy(None, None, None, None, None, None) == -1 and b"hd_diversity_energy" in lib.hd_last_error()


# ----------------------------------------------------------------------------- the restatement

def test_the_generator_terminates_and_every_pair_clears_the_margin(cases):
    """No case is left out: the generator re-seeds until every contributing pair is conditioned, for every shape of the GPU tier."""
    worst, tried = math.inf, 0
    for c in cases:
        tried = max(tried, c.attempts)
        if c.degenerate:
            continue
        w = dr.worst_cond(c)
        assert w >= dr.MARGIN * dr.COND_MIN, (c.name, w)
        worst = min(worst, w)
    print(f"{len(cases)} cases, the smallest conditioning measure {worst:.3f} (bar {dr.COND_MIN}), at most {tried} seeds tried; excluded: 0")
    assert len(cases) == 2 * (3 * (len(dr.KINDS) + 1) + len(dr.DEGENERATE)) + 1


@pytest.mark.autograd
def test_gradient_equals_autograd_through_energy_terms(cases):
    """The envelope claim: dPhi/dx with R held at the maximiser IS the gradient.  1e-9 relative, on the conditioned cases."""
    worst = 0.0
    for c in cases:
        if c.degenerate or c.kind == "nan coordinate" or c.P > 8:
            continue
        x0 = dr.data_prediction(c)
        phi, rmsd, g, _, _ = dr.phi_grad(x0, c.nm.numpy(), c.P, c.kappa, c.length)
        x = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
        with torch.enable_grad():
            pt, rt = diversity.energy_terms(x, c.nm[:, :, None], c.P, c.length, c.kappa, return_rmsd=True)
            pt.sum().backward()
        assert np.allclose(pt.detach().numpy(), phi, rtol=1e-12, atol=0), c.name
        assert np.allclose(rt.numpy(), rmsd, rtol=1e-10, atol=1e-12, equal_nan=True), c.name
        ga = x.grad.numpy()
        err = float(np.abs(ga - g).max() / max(np.abs(g).max(), 1e-300))
        worst = max(worst, err)
        assert err < 1e-9, (c.name, err)
    print(f"restatement against autograd: worst relative error {worst:.2e}")
    # ... and against central differences of Phi on one small case, the rotation re-fitted at every point
    c = dr.conditioned_case(1, 3, 5, 4, seed=3)
    x0 = dr.data_prediction(c)
    g = dr.phi_grad(x0, c.nm.numpy(), 3, c.kappa, c.length)[2]
    h = 1e-6
    for (b, i, k) in [(0, 0, 0), (1, 3, 2), (2, 4, 1)]:
        xp, xm = x0.copy(), x0.copy()
        xp[b, i, k] += h
        xm[b, i, k] -= h
        fd = (dr.phi_grad(xp, c.nm.numpy(), 3, c.kappa, c.length)[0][0] - dr.phi_grad(xm, c.nm.numpy(), 3, c.kappa, c.length)[0][0]) / (2 * h)
        assert abs(fd - g[b, i, k]) < 1e-7 * max(1.0, abs(g[b, i, k])), (b, i, k, fd, g[b, i, k])


def _update(c, **kw):
    return dr.diverse_ref(c.z, c.eps, c.nm, c.P, c.kappa, c.length, c.scale, c.row, c.nv0, **kw)


def test_fp32_twin_inside_the_bar_and_every_mutant_far_outside(cases):
    """The bar of the GPU tier - 8 * 2^-23 of the sum of the absolute terms of the element - on the GPU tier's inputs."""
    worst = 0.0
    miss = {m: 0.0 for m in dr.MUTANTS}
    for c in cases:
        if c.degenerate:
            continue
        ref, mag = _update(c)
        bound = dr.BOUND * dr.U * mag
        twin, _ = _update(c, twin=True)
        r = float((np.abs(twin - ref) / np.maximum(bound, 1e-300)).max())
        worst = max(worst, r)
        assert r <= 1.0, (c.name, r)
        if c.P > 8:
            continue
        for m in dr.MUTANTS:
            got, _ = _update(c, mutant=m, twin=True)
            miss[m] = max(miss[m], float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
    print(f"fp32 twin: worst err / bound {worst:.3f}; mutants miss by (x the bound): " + ", ".join(f"{m} {v:.3g}" for m, v in miss.items()))
    for m, v in miss.items():
        assert v > 100.0, (m, v)


def test_exact_zeros_of_the_restatement(cases):
    for c in cases:
        ref, _ = _update(c)
        e = c.eps.double().numpy()
        valid = c.nm.numpy()
        assert (ref[:, :, 3:] == e[:, :, 3:]).all() and (ref[~valid] == e[~valid]).all(), c.name
        s = np.broadcast_to(c.scale.numpy(), (c.G,)) if c.scale.numel() == 1 else c.scale.numpy()
        for g in range(c.G):
            if s[g] == 0:
                assert (ref[g * c.P:(g + 1) * c.P] == e[g * c.P:(g + 1) * c.P]).all(), c.name
    c = dr.conditioned_case(1, 2, 5, 4, kind="identical rows", seed=1)
    ref, _ = _update(c)
    # r = 0: no step at all (the SVD's R is I up to rounding, so here the step is a rounding residue; the kernel's is exactly 0)
    assert np.abs(ref - c.eps.double().numpy()).max() < 1e-14


def test_mirror_images_stay_apart():
    """Every intra-row distance agrees, yet the aligned RMSD is > 0: R is a proper rotation."""
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.normal(0.0, 1.5, (7, 3))
    x = np.stack([a, a * np.array([1.0, 1.0, -1.0])])
    dist = lambda v: np.linalg.norm(v[:, None] - v[None], axis=-1)
    assert np.allclose(dist(x[0]), dist(x[1]), rtol=0, atol=1e-14)
    nm = np.ones((2, 7), dtype=bool)
    _, rmsd, g, _, _ = dr.phi_grad(x, nm, 2, 1.0, 1.0)
    assert rmsd[0, 0, 1] > 0.3 and np.abs(g).max() > 1e-3
    _, refl, _, _, _ = dr.phi_grad(x, nm, 2, 1.0, 1.0, mutant="no_det")
    assert refl[0, 0, 1] < 1e-12                                # with the reflection allowed they would coincide
    t = diversity.pairwise_rmsd(torch.from_numpy(x), torch.from_numpy(nm)[:, :, None], 2)
    assert abs(float(t[0, 0, 1]) - rmsd[0, 0, 1]) < 1e-12 and float(t[0, 0, 0]) == 0.0
    # a rotated copy, on the other hand, is at distance 0
    y = np.stack([a, a @ dr._rotation(rng).T + 2.0])
    assert dr.phi_grad(y, nm, 2, 1.0, 1.0)[1][0, 0, 1] < 1e-12


def test_cpu_helpers():
    c = dr.conditioned_case(2, 4, 5, 4, kind="unequal masks", seed=2)
    x = torch.from_numpy(dr.data_prediction(c))
    phi, rmsd, _, _, _ = dr.phi_grad(x.numpy(), c.nm.numpy(), 4, 2.0, 0.9)
    dv = Diversity(4, 0.9, strength=2.0)
    p, r = dv.energy(x.float(), c.nm[:, :, None])
    assert p.dtype == torch.float64 and tuple(r.shape) == (2, 4, 4)
    assert np.allclose(p.numpy(), phi, rtol=1e-12) and np.allclose(r.numpy(), rmsd, rtol=1e-10, atol=1e-12, equal_nan=True)
    assert torch.equal(torch.nan_to_num(r, nan=-1.0), torch.nan_to_num(r.transpose(1, 2), nan=-1.0)) and bool((r.diagonal(dim1=1, dim2=2) == 0).all())
    assert bool(torch.isnan(r[1, 3, :3]).all())                 # the masked row: every pair with it contributes nothing
    res = diversity.result(p, r)
    assert tuple(res.mean_rmsd.shape) == (2,) and bool(torch.isfinite(res.mean_rmsd).all()) and res.group.tolist() == [0] * 4 + [1] * 4
    out = [dict() for _ in range(8)]
    diversity.into(out, res, group0=3)
    assert int(out[5]['diversity_group']) == 4 and torch.equal(out[5]['diversity_rmsd'][:3], r[1, 1, :3]) and float(out[5]['diversity_rmsd'][1]) == 0.0
    with pytest.raises(ValueError, match="multiple"):
        diversity.pairwise_rmsd(x, c.nm[:, :, None], 3)
    with pytest.raises(ValueError, match=r"x must be"):
        diversity.pairwise_rmsd(x[:, :4], c.nm[:, :, None], 4)


# ----------------------------------------------------------------------------- the keyword, the plan, the entry points

def test_diversity_keyword_refusals():
    for bad in (0, -1, 2.5, "4", True, None):
        with pytest.raises(ValueError, match="particles must be"):
            Diversity(bad, 1.0)
    with pytest.raises(ValueError, match="<= 32"):
        Diversity(33, 1.0)
    for bad in (0, 0.0, -1.0, math.inf, math.nan, "x", None, True):
        with pytest.raises(ValueError, match="length must be"):
            Diversity(4, bad)
    for bad in (-1.0, math.inf, math.nan, "x", True):
        with pytest.raises(ValueError, match="strength must be"):
            Diversity(4, 1.0, strength=bad)
    for bad in ([1.0, math.nan], [[1.0]], "x", True, []):
        with pytest.raises(ValueError, match="scale must be"):
            Diversity(4, 1.0, scale=bad)
    for bad in ("linear", [1.0, math.inf], [], "x"):
        with pytest.raises(ValueError, match="schedule"):
            Diversity(4, 1.0, schedule=bad)
    for bad in (0, -1.0, "x", True):
        with pytest.raises(ValueError, match="clip must be"):
            Diversity(4, 1.0, clip=bad)
    d = Diversity(4, 1.5)
    assert (d.P, d.length, d.strength, d.schedule, d.clip) == (4, 1.5, 1.0, "score", math.inf) and d.active
    assert not Diversity(1, 1.0).active and not Diversity(4, 1.0, strength=0).active and not Diversity(4, 1.0, scale=[0.0, 0.0]).active
    assert Diversity(4, 1.0, scale=[0.0, 1.0]).active and Diversity(4, 1.0, scale=[1.0, 2.0, 3.0]).slice(1, 3).scale.tolist() == [2.0, 3.0]


def test_plan_off_is_the_plan_without_the_keyword():
    m = small_model()
    assert "diversity" in hplan.KEYWORDS
    base = hplan.plan(m, "t", B=4)
    assert base.diversity is None and base.path is None
    for dv in (None, Diversity(1, 1.0), Diversity(2, 1.0, strength=0.0), Diversity(2, 1.0, scale=0.0), Diversity(2, 1.0, scale=[0.0, 0.0])):
        assert hplan.plan(m, "t", B=4, diversity=dv) == base
    few = hplan.plan(m, "t", B=4, steps=5, eta=0.0)
    assert hplan.plan(m, "t", B=4, steps=5, eta=0.0, diversity=Diversity(1, 1.0)) == few
    dv = Diversity(2, 1.2, strength=0.7)
    p = hplan.plan(m, "t", B=4, diversity=dv)
    assert p.diversity is dv and p.path == list(range(20, -1, -1)) and p.eta == 1.0 and p.K == 20      # always on a path: the identity one
    for kw in (dict(steps=5, eta=0.0), dict(steps=5, solver="dpm2m"), dict(steps=5, solver="sde2m"), dict(steps=5, eta=0.5)):
        p = hplan.plan(m, "t", B=4, diversity=dv, **kw)
        assert p.diversity is dv and p.K == 5 and p[:9] == hplan.plan(m, "t", B=4, **kw)[:9]
    m.diversity = dv
    assert hplan.plan(m, "t", B=4).diversity is dv and hplan.plan(m, "t", B=4, diversity=Diversity(1, 1.0)).diversity is None
    rows = diversity.rows(torch.linspace(-5, 5, 21), p.path, Diversity(2, 1.0, schedule=[1, 0, 1, 2, 0.5], clip=0.25), 1.7)
    assert rows.shape == (5, 4) and rows.dtype == np.float32 and rows[:, 2].tolist() == [1, 0, 1, 2, 0.5] and (rows[:, 3] == 0.25).all()
    rows = diversity.rows(torch.linspace(-5, 5, 21), p.path, dv, 1.7)
    assert np.allclose(rows[:, 2], 1.7 * rows[:, 1] / rows[:, 0], rtol=1e-6) and np.isinf(rows[:, 3]).all()


def test_refusals_come_from_the_plan_before_the_gpu():
    m = small_model()
    nm = torch.ones(4, 3, 1, dtype=torch.bool)
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    z3, z8, z11 = torch.zeros(4, 3, 3), torch.zeros(4, 3, 8), torch.zeros(4, 3, 11)
    mol = {"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}
    dv = Diversity(2, 1.0)
    run = lambda **k: m.sample_from_masks(nm, None, None, **k)
    with pytest.raises(ValueError, match="must be a hierdiff_amd.diversity.Diversity"):
        run(diversity=dict(particles=2))
    with pytest.raises(NotImplementedError, match=r"diversity= and steering \(particles=\)"):
        run(diversity=dv, restraints=rs, particles=2, steer_scale=1.0)
    with pytest.raises(ValueError, match="multiple of the diversity's particles"):
        run(diversity=Diversity(3, 1.0))
    with pytest.raises(ValueError, match=r"one value per group \(\[2\]\)"):
        run(diversity=Diversity(2, 1.0, scale=[1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match=r"one finite weight per transition \(5\)"):
        run(steps=5, diversity=Diversity(2, 1.0, schedule=[1.0, 2.0]))
    with pytest.raises(ValueError, match="fix_noise"):
        run(diversity=dv, fix_noise=True)
    with pytest.raises(ValueError, match="fix_noise"):
        run(diversity=dv, fix_noise=True, steps=4, solver="sde2m")
    nm2 = nm.clone()
    nm2[1, 2] = False
    with pytest.raises(ValueError, match="node masks differ inside a group"):
        m.sample_from_masks(nm2, None, None, diversity=dv)
    with pytest.raises(ValueError, match="context rows differ"):
        diversity.check_groups(dv, nm, torch.arange(12.0).reshape(4, 3, 1))
    diversity.check_groups(dv, nm, torch.arange(6.0).reshape(2, 1, 3, 1).expand(2, 2, 3, 1).reshape(4, 3, 1))
    # what passes the plan reaches the device check: fix_noise on a path that draws nothing, raw_noises, every solver
    for kw in (dict(fix_noise=True, steps=4, eta=0.0), dict(fix_noise=True, steps=4, solver="dpm2m"), dict(steps=4, solver="sde2m"),
               dict(raw_noises=[(z3, z8)] * 22), dict(restraints=rs, restraint_scale=1.0), dict(keep_frames=3, record="x0")):
        with pytest.raises(_lib.HierDiffHipError, match="runs only on an MI355X"):
            run(diversity=dv, **kw)
    with pytest.raises(_lib.HierDiffHipError, match="runs only on an MI355X"):
        m.path_steps(z11, nm, diversity=dv, steps=4)
    # the entry points that take none: the model's attribute is refused, not ignored
    m.diversity = dv
    fm = torch.zeros(4, 3, 1, dtype=torch.bool)
    for call in (lambda: m.sample_inpaint(nm, fm, z3, z8), lambda: m.inpaint_steps(z11, 20, 0, nm, fm, z3, z8),
                 lambda: m.sample_grow([mol], [4], "cpu"), lambda: m.sample_batches(2, 1, "cpu"),
                 lambda: m.encode(z3, z8, nm), lambda: m.interpolate(mol, mol, 3, "cpu")):
        with pytest.raises(NotImplementedError, match="diverse sampling is not supported here"):
            call()
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="noise_mode 'torch'"):
        run()
    m.noise_mode = "philox"
    m.diversity = None
    with pytest.raises(ValueError, match="multiples of the diversity's particles"):
        m.vary([mol], "cpu", 10, n_variants=3, diversity=dv)


def test_no_earlier_error_moves():
    """Every error the plan raised before still comes first, with its message, when diversity= is given as well."""
    m = small_model()
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    bad_dv = dict(particles=2)                                  # itself an error - raised last
    earlier = [(dict(steps=4, timesteps=[20, 10, 0]), "either steps or timesteps"), (dict(eta=2.0), "eta"), (dict(spacing="x"), "spacing"),
               (dict(solver="nope"), "solver"), (dict(guidance_scale="x"), "guidance_scale"),
               (dict(restraints=rs, restraint_scale="x"), "restraint_scale"), (dict(record="z"), "records nothing without keep_frames"),
               (dict(keep_frames=2.5), "keep_frames must be an integer"),
               (dict(restraints=rs, particles=3, steer_scale=1.0), "multiple of particles"),
               (dict(restraints=rs, particles=2, steer_scale=1.0, eta=0.0, steps=4), "eta = 0")]
    for kw, msg in earlier:
        for dv in (None, bad_dv, Diversity(2, 1.0)):
            with pytest.raises((ValueError, NotImplementedError)) as a:
                hplan.plan(m, "t", B=4, diversity=dv, **kw)
            with pytest.raises((ValueError, NotImplementedError)) as b:
                hplan.plan(m, "t", B=4, **kw)
            assert str(a.value) == str(b.value) and msg in str(a.value), (kw, str(a.value))


def test_cli_refusals(tmp_path, capsys):
    """The argument parser refuses what the entry points would, before a model is built."""
    from hierdiff_amd import sampler
    base = ["--hidden-nf", "32", "--n-layers", "1", "--timesteps", "8", "--batch-size", "4", "--out", str(tmp_path / "o.pkl")]
    dv = ["--diverse", "2", "--diverse-length", "1.0"]
    bad = [(["--diverse", "2"], "go together"), (["--diverse-length", "1.0"], "go together"), (["--diverse-strength", "2"], "need --diverse"),
           (["--diverse-clip", "0.1"], "need --diverse"), (["--diverse-schedule", "sigma"], "need --diverse"),
           (["--diverse", "33", "--diverse-length", "1"], "1 .. 32"), (["--diverse", "0", "--diverse-length", "1"], "1 .. 32"),
           (["--diverse", "2", "--diverse-length", "0"], "--diverse-length must be"), (["--diverse", "2", "--diverse-length", "nan"], "--diverse-length must be"),
           (dv + ["--diverse-strength", "-1"], "--diverse-strength must be"), (dv + ["--diverse-clip", "0"], "--diverse-clip must be"),
           (dv + ["--diverse-schedule", "linear"], "invalid choice"), (["--diverse", "3", "--diverse-length", "1"], "multiple of --diverse"),
           (dv + ["--restraints", "r.json", "--particles", "2", "--steer-scale", "1"], "does not combine with --particles"),
           (dv + ["--known", "k.pkl", "--grow", "2"], "does not combine with --known"),
           (dv + ["--vary", "v.pkl", "--t-start", "4", "--variants", "3"], "multiple of --diverse")]
    for extra, msg in bad:
        with pytest.raises(SystemExit) as e:
            sampler.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, (extra, msg)
