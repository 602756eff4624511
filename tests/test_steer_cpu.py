"""CPU tier of steered sampling: the C ABI (symbols, argument errors without a device), the uniform host twin, the reference resampler
of tests/steer_reference.py against the properties of systematic resampling, every refusal of the Python entry points and the CLI
(raised from the plan, before a device is looked at), and the margins of every fixture the GPU tier compares ancestors on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, plan as hplan, steering
from hierdiff_amd.restraints import Restraints
from tests import steer_reference as st

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hd_set_steer", "hd_steer_attach", "hd_steer_detach", "hd_steer_step", "hd_steer_read", "hd_philox_uniform_host"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


# ----------------------------------------------------------------------------- the C ABI

def test_symbols_exported_declared_and_null_safe(lib):
    header = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.hd_version() == 12
    r3 = (C.c_float * 3)(0.8, 0.6, 1.0)
    assert lib.hd_set_steer(None, 1, r3) == -1 and b"hd_set_steer" in lib.hd_last_error()
    assert lib.hd_steer_attach(None, 4, 0.5, 1, None) == -1 and b"null topology" in lib.hd_last_error()
    assert lib.hd_steer_detach(None) == 0
    assert lib.hd_steer_step(None, None, None, None, r3, 0, 0, 0, None) == -1 and b"hd_steer_step" in lib.hd_last_error()
    assert lib.hd_steer_read(None, None, None, None, None, None, None) == -1 and b"hd_steer_read" in lib.hd_last_error()


def test_uniform_host_twin(lib):
    u = lambda seed, s, d, i=st.UNIFORM_INDEX: lib.hd_philox_uniform_host(seed, s, d, i)
    n = 20000
    v = np.array([u(7, i, 3) for i in range(n)])
    assert ((v > 0.0) & (v < 1.0)).all()
    assert u(7, 5, 3) == u(7, 5, 3) and u(7, 5, 3) == v[5]
    assert len({u(7, 5, 3), u(8, 5, 3), u(7, 6, 3), u(7, 5, 4), u(7, 5, 3, 0)}) == 5        # every part of the key counts
    assert abs(v.mean() - 0.5) < 3 * math.sqrt(1 / 12 / n)
    var_se = math.sqrt((1 / 80 - 1 / 144) / n)                   # Var[(U - 1/2)^2] = E[.^4] - Var^2 = 1/80 - 1/144
    assert abs(((v - 0.5) ** 2).mean() - 1 / 12) < 3 * var_se
    # distinct from the normal stream of the same counter block (the normals take words 0 and 1)
    nrm = np.array([lib.hd_philox_normal_host(7, i, 3, st.UNIFORM_INDEX) for i in range(2000)])
    assert abs(np.corrcoef(v[:2000], nrm)[0, 1]) < 3 / math.sqrt(2000)
    # 52 bits: a value is an odd multiple of 2^-53
    assert all(float(x * 2.0 ** 53).is_integer() and int(x * 2.0 ** 53) % 2 == 1 for x in v[:100])


# ----------------------------------------------------------------------------- the reference resampler

def test_reference_resampler_properties():
    rng = np.random.Generator(np.random.PCG64(5))
    for P in (2, 3, 8, 64):
        w = rng.uniform(0.05, 1.0, P)
        w[rng.integers(0, P)] = 0.0 if P > 2 else w[0]
        grid = (np.arange(4096) + 0.5) / 4096
        counts = np.zeros(P)
        for u in grid:
            anc, _ = st.systematic(w, float(u))
            assert (np.diff(anc) >= 0).all()                     # ascending
            counts += np.bincount(anc, minlength=P)
        assert np.abs(counts / grid.size - P * w / w.sum()).max() <= 1.0 / grid.size * P + 1e-12
    one = np.zeros(8)
    one[5] = 1.0
    assert (st.systematic(one, 0.3)[0] == 5).all()               # all mass on one particle
    assert (st.systematic(np.array([1.0, 0.0, 0.0]), 0.999999)[0] == 0).all()
    anc, ess, m1, m2, _ = st.resample_group(np.zeros(8), 0.3, 0.5)
    assert anc is None and ess == 8.0                            # equal weights: no resampling
    anc, ess, _, _, _ = st.resample_group(np.zeros(8), 0.3, 1.0)
    assert anc is None                                           # ESS = P is not below rho P even at rho = 1
    anc, ess, _, _, _ = st.resample_group(np.array([-math.inf] * 4), 0.3, 0.5)
    assert anc is None and ess is None                           # an all-zero group is left alone
    anc, ess, _, _, _ = st.resample_group(np.array([0.0, -math.inf, -30.0, -math.inf]), 0.3, 0.5)
    assert (anc == 0).all() and abs(ess - 1.0) < 1e-12


def test_reference_stage_moves_state_with_the_rows():
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 5.0, 1.0]])
    nm = torch.ones(4, 2, dtype=torch.bool)
    z = torch.zeros(4, 2, 4)
    z[:, :, 0] = torch.tensor([0.5, 4.0, 1.0, 2.0]).reshape(4, 1)        # row 1 lies nearest the rim: the lowest energy
    eps = torch.arange(32, dtype=torch.float32).reshape(4, 2, 4)
    eps[:, :, :3] = 0
    state = st.State(4, 4)
    zz, ee, info = st.stage(rs, z, eps, nm, (1.0, 0.0, 50.0), 1.0, state, 0.5, 1, 0, 1, uniforms=[0.5])
    assert info["resampled"].all() and (info["anc"] == 1).all() and (state.root == 1).all() and (state.logw == 0).all()
    assert torch.equal(zz, z[[1, 1, 1, 1]]) and torch.equal(ee, eps[[1, 1, 1, 1]]) and (state.uprev == info["U"][1]).all()
    assert state.stats[0, 0] == 1 and state.stats[0, 1] < 1.01


# ----------------------------------------------------------------------------- the plan

def test_plan_off_is_the_unsteered_plan():
    m = small_model()
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    assert set(("particles", "steer_scale", "steer_ess", "steer_schedule")) <= set(hplan.KEYWORDS)
    base = hplan.plan(m, "t", B=4, restraints=rs, restraint_scale=1.0)
    for kw in (dict(particles=None, steer_scale=1.0), dict(particles=1, steer_scale=1.0), dict(particles=4, steer_scale=None),
               dict(particles=4, steer_scale=0), dict(particles=4, steer_scale=0.0)):
        p = hplan.plan(m, "t", B=4, restraints=rs, restraint_scale=1.0, **kw)
        assert p.steer is None and p.path == base.path and p.restraints.key() == base.restraints.key()
    assert hplan.plan(m, "t", B=4, particles=4, steer_scale=0).restraints is None and hplan.plan(m, "t", B=4).path is None
    p = hplan.plan(m, "t", B=8, restraints=rs, particles=4, steer_scale=2.0)
    assert p.steer == steering.Steer(4, 2.0, 0.5, None) and p.path is not None and p.eta == 1.0
    assert p.restraints is not None and float(p.restraints.scale.abs().sum()) == 0.0        # steering without the gradient update
    m.particles, m.steer_scale, m.steer_ess = 2, 1.5, 0.25
    p = hplan.plan(m, "t", B=8, restraints=rs, steps=5, eta=0.5, steer_schedule=[1, 0, 1, 2, 0.5])
    assert p.steer == steering.Steer(2, 1.5, 0.25, (1.0, 0.0, 1.0, 2.0, 0.5))
    rows = steering.beta_rows(torch.linspace(-5, 5, 21), p.path, p.steer)
    assert rows.shape == (5, 3) and rows.dtype == np.float32 and np.allclose(rows[:, 2], [1.5, 0, 1.5, 3.0, 0.75])
    assert np.allclose(rows[:, 0] ** 2 + rows[:, 1] ** 2, 1.0, atol=1e-6)


def test_refusals_come_from_the_plan_before_the_gpu():
    from hierdiff_amd import DiffusionQM9
    m = small_model()
    nm = torch.ones(4, 3, 1, dtype=torch.bool)
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    z3, z8, z11 = torch.zeros(4, 3, 3), torch.zeros(4, 3, 8), torch.zeros(4, 3, 11)
    mol = {"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}
    kw = dict(restraints=rs, particles=2, steer_scale=1.0)
    run = lambda **k: m.sample_from_masks(nm, None, None, **k)
    with pytest.raises(ValueError, match="eta = 0"):
        run(steps=4, eta=0.0, **kw)
    with pytest.raises(ValueError, match="dpm2m"):
        run(steps=4, solver="dpm2m", **kw)
    with pytest.raises(ValueError, match="restraints= is required"):
        run(particles=2, steer_scale=1.0)
    with pytest.raises(ValueError, match="multiple of particles"):
        run(restraints=rs, particles=3, steer_scale=1.0)
    with pytest.raises(ValueError, match="<= 256"):
        run(restraints=rs, particles=257, steer_scale=1.0)
    for bad in (0, -2, 2.5, "4", True):
        with pytest.raises(ValueError, match="particles must be"):
            run(restraints=rs, particles=bad, steer_scale=1.0)
    for bad in (0.0, -0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="steer_ess"):
            run(steer_ess=bad, **kw)
    for bad in (-1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="steer_scale"):
            run(restraints=rs, particles=2, steer_scale=bad)
    for bad in ([1.0, 2.0], [1.0] * 19 + [float("nan")], [1.0] * 19 + [-1.0], "x"):
        with pytest.raises(ValueError, match="steer_schedule"):
            run(steer_schedule=bad, **kw)
    with pytest.raises(NotImplementedError, match="raw_noises"):
        run(raw_noises=[(z3, z8)] * 22, **kw)
    # unequal rows inside a group: masks, context, per-molecule tables, scales - on the host
    nm2 = nm.clone()
    nm2[1, 2] = False
    with pytest.raises(ValueError, match="node masks differ inside a group"):
        m.sample_from_masks(nm2, None, None, **kw)
    obs = torch.tensor([[[0, 0, 0, 1.0, 1]], [[0, 0, 0, 1.0, 1]], [[1, 0, 0, 1.0, 1]], [[2, 0, 0, 1.0, 1]]])
    with pytest.raises(ValueError, match=r"restraint rows \(obs\) differ inside a group"):
        run(restraints=Restraints(obstacles=obs), particles=2, steer_scale=1.0)
    with pytest.raises(ValueError, match="restraint scales differ inside a group"):
        run(restraint_scale=torch.tensor([1.0, 1.0, 1.0, 2.0]), **kw)
    steering.check_groups(steering.Steer(2, 1.0, 0.5, None), nm, None, Restraints(obstacles=obs[[0, 0, 2, 2]]), torch.tensor([1.0, 1, 2, 2]))
    with pytest.raises(ValueError, match="context rows differ"):
        steering.check_groups(steering.Steer(2, 1.0, 0.5, None), nm, torch.arange(12.0).reshape(4, 3, 1), rs, None)
    with pytest.raises(ValueError, match="multiple of particles"):
        DiffusionQM9.sample(m, 5, "cpu", **kw)
    with pytest.raises(ValueError, match="n_variants"):
        m.vary([mol], "cpu", 5, n_variants=3, **kw)
    with pytest.raises(ValueError, match="batch_size"):
        m.vary([mol], "cpu", 5, n_variants=2, batch_size=3, **kw)
    with pytest.raises(ValueError, match="every row's own noise"):
        m.path_steps(z11, nm, steps=4, fix_noise=True, **kw)
    # the entry points that do not steer
    m.particles, m.steer_scale = 2, 1.0
    try:
        for call in (lambda: m.sample_inpaint(nm, nm, z3, z8), lambda: m.sample_grow([mol], 4, "cpu"),
                     lambda: m.sample_batches(2, 1, "cpu"), lambda: m.encode(z3, z8, nm), lambda: m.interpolate(mol, mol, 3, "cpu"),
                     lambda: m.inpaint_steps(z11, 3, 1, nm, nm, z3, z8)):
            with pytest.raises(NotImplementedError, match="steered sampling is not supported here"):
                call()
        m.steer_scale = 0                                        # the old code path: the refusals are gone
        with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
            m.encode(z3, z8, nm)
    finally:
        m.particles, m.steer_scale = None, None
    # configurations it does not run in
    with pytest.raises(NotImplementedError, match="pocket"):
        run(pocket=(None,) * 4, **kw)
    m.pocket = True
    try:
        with pytest.raises(NotImplementedError, match="pocket"):
            m.path_steps(z11, nm, steps=4, **kw)
    finally:
        m.pocket = False
    m.noise_mode = "torch"
    try:
        with pytest.raises(NotImplementedError, match="noise_mode"):
            run(**kw)
    finally:
        m.noise_mode = "philox"
    m.dynamics.mode = "gnn_dynamics"
    try:
        with pytest.raises(NotImplementedError, match="gnn_dynamics"):
            run(**kw)
    finally:
        m.dynamics.mode = "egnn_dynamics"
    # a steered call reaches the device check, as do the spellings of "off"
    for k2 in (kw, dict(kw, restraint_scale=0.5, steer_ess=1.0), dict(kw, particles=1), dict(kw, steer_scale=0)):
        with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
            run(**k2)


def test_sampler_cli_arguments():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--restraints", "r.json", "--particles", "4", "--steer-scale", "2.5", "--batch-size", "8"])
    assert (a.particles, a.steer_scale, a.steer_ess, a.restraint_scale) == (4, 2.5, None, None)
    a = sampler.parse_args(["--restraints", "r.json", "--particles", "2", "--steer-scale", "1", "--steer-ess", "0.25", "--restraint-scale",
                            "0.1", "--vary", "m.pkl", "--t-start", "10", "--variants", "4"])
    assert (a.particles, a.steer_ess, a.restraint_scale, a.variants) == (2, 0.25, 0.1, 4)
    a = sampler.parse_args(["--restraints", "r.json"])
    assert (a.particles, a.steer_scale, a.restraint_scale) == (None, None, 1.0)
    for bad in (["--particles", "4", "--steer-scale", "1", "--batch-size", "8"], ["--restraints", "r.json", "--particles", "4"],
                ["--restraints", "r.json", "--steer-scale", "1"], ["--restraints", "r.json", "--steer-ess", "0.5"],
                ["--restraints", "r.json", "--particles", "4", "--steer-scale", "1", "--batch-size", "6"],
                ["--restraints", "r.json", "--particles", "300", "--steer-scale", "1", "--batch-size", "300"],
                ["--restraints", "r.json", "--particles", "2", "--steer-scale", "-1"],
                ["--restraints", "r.json", "--particles", "2", "--steer-scale", "1", "--steer-ess", "0"],
                ["--restraints", "r.json", "--particles", "2", "--steer-scale", "1", "--vary", "m.pkl", "--t-start", "5", "--variants", "3"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)


# ----------------------------------------------------------------------------- the margins of the GPU tier's fixtures

def test_margins_of_the_kernel_fixtures():
    """Every case of tests/test_gpu_steer.py::test_steer_step_against_the_reference is used - none has to be left out: both margins of
    every stage are at least MARGIN_BAR, and the cases do what their names say."""
    worst, worst_ess = math.inf, math.inf
    for c in st.step_cases():
        case = st.step_case(*c)
        ref = st.step_reference(case)
        for _, _, info, _ in ref:
            worst, worst_ess = min(worst, info["margin"]), min(worst_ess, info["margin_ess"])
            assert info["margin"] >= st.MARGIN_BAR and info["margin_ess"] >= st.MARGIN_BAR, c
        last, state = ref[-1][2], ref[-1][3]
        kind = c[3]
        assert not ref[0][2]["resampled"].any()
        if kind == "none":
            assert not last["resampled"].any() and (last["anc"] == np.arange(last["anc"].size)).all()
        elif kind == "allzero":
            assert last["resampled"].tolist() == [True, False] and state.stats[1, 2] == 1 and np.isinf(state.logw[c[0]:]).all()
        else:
            assert last["resampled"].all() and (last["anc"] != np.arange(last["anc"].size)).any()
        if kind == "nonfinite":
            assert not (last["anc"] == 1).any() and np.isinf(last["U"][1])
    print(f"kernel fixtures: smallest resampling margin {worst:.3g} of S, smallest |ESS / P - rho| {worst_ess:.3g} (bar {st.MARGIN_BAR:g})")


@pytest.mark.parametrize("precision,eta,restrained", st.CHAIN_CASES)
def test_margins_of_the_chain_fixtures(precision, eta, restrained):
    """The fixture of tests/test_gpu_steer.py::test_steered_chain_against_the_reference: its smallest margin (resampling points and
    ESS / P against rho, all transitions) is at least MARGIN_FACTOR times the largest difference of the normalised prefix sums between
    the reference with the oracle in float64 and in float32 - the reference's own fp32 noise - the two agree on every ancestor, and
    the chain has a transition that resamples and one that does not."""
    _, i32, _, _, _ = st.chain_reference(precision, eta, restrained)
    _, i64, _, _, _ = st.chain_reference(precision, eta, restrained, dtype=torch.float64)
    margin = min(min(i["margin"], i["margin_ess"]) for i in i32)
    diff, same = st.cumulative_difference(i32, i64)
    events = [bool(i["resampled"].any()) for i in i32]
    print(f"chain fixture {precision} eta={eta} restrained={restrained}: smallest margin {margin:.3g}, float64 / float32 reference "
          f"difference {diff:.3g} (ratio {margin / max(diff, 1e-300):.3g}), resampling transitions {sum(events)} of {len(events)}")
    assert same
    assert margin >= st.MARGIN_FACTOR * diff
    assert any(events) and not all(bool(i["resampled"].all()) for i in i32)
