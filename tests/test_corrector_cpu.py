"""CPU tier of predictor-corrector sampling: the restatement of tests/corrector_reference.py against itself (its float32 twin inside
the element-wise bar of the GPU tier, six mutants outside it on the same inputs), against the analytic variance recursion of a
Gaussian under its exact score, and the host side - the `Corrector` keyword, the plan, the refusals (raised before a device is looked
at), the rows, the CLI, the C ABI's null-argument refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, corrector, plan as hplan
from hierdiff_amd.corrector import Corrector
from hierdiff_amd.restraints import Restraints
from tests import corrector_reference as cr

NEW_SYMBOLS = ["hd_set_corrector", "hd_corrector_attach", "hd_corrector_detach", "hd_corrector_read", "hd_langevin_step"]
SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]
SEED, BASE, T = 99, 10, 8


def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


# ----------------------------------------------------------------------------- the restatement: its fp32 twin and the mutants

@pytest.mark.parametrize("N,D", SHAPES)
def test_the_float32_twin_stays_inside_the_bar(N, D):
    c = cr.kernel_case(N, D)
    worst = 0.0
    for name, row, adaptive in cr.kernel_rows():
        for rows in (c["B"], 1):                              # every molecule's own normals, one shared row
            rx, rh = c["raw_x"][:rows], c["raw_h"][:rows]
            ref, A, g, kept = cr.langevin_ref(c["z"], c["eps"], c["nm"], row, adaptive, rx, rh)
            got, g32 = cr.langevin_f32(c["z"], c["eps"], c["nm"], row, adaptive, rx, rh)
            r = cr.ratio(got, ref, A, c["nm"])
            worst = max(worst, r)
            assert r <= cr.BOUND, (name, rows, r)
            assert np.allclose(g32, g, rtol=1e-6)              # (the twin's norms are sums of fp32-centred values)
            quiet = row[1] == 0.0
            assert (kept == (c["keeps"] | quiet)).all(), name
            assert (ref[kept] == c["z"][kept].astype(np.float64)).all() and (g[kept] == 0).all()
            assert (ref[c["nm"] == 0] == c["z"][c["nm"] == 0]).all()          # masked rows are never written
            if row[0] == 0.0 and not quiet:                   # sigma_t = 0: both coefficients vanish, only the re-centring acts
                assert not kept[0] and np.abs(ref[0][:, 3:] - c["z"][0][:, 3:]).max() == 0.0
            if name == "snr capped":
                assert g[0] == float(np.float32(row[2])) and g[1] == float(np.float32(row[2]))
            if name == "snr":
                assert 0 < g[0] < 1.0 and g[0] != g[1]
    print(f"langevin twin N={N} D={D}: worst err / (2^-23 A) {worst:.3f} (bar {cr.BOUND:g})")


@pytest.mark.parametrize("mutant", cr.MUTANTS[:5])
def test_every_mutant_of_the_step_misses_the_bar(mutant):
    c = cr.kernel_case(33, 11)
    name, row, adaptive = cr.kernel_rows()[1 if mutant == "cap_ignored" else 0]
    ref, A, _, kept = cr.langevin_ref(c["z"], c["eps"], c["nm"], row, adaptive, c["raw_x"], c["raw_h"])
    good = cr.ratio(cr.langevin_f32(c["z"], c["eps"], c["nm"], row, adaptive, c["raw_x"], c["raw_h"])[0], ref, A, c["nm"])
    bad = cr.ratio(cr.langevin_f32(c["z"], c["eps"], c["nm"], row, adaptive, c["raw_x"], c["raw_h"], mutant=mutant)[0], ref, A, c["nm"])
    print(f"mutant {mutant} on '{name}': err / (2^-23 A) {bad:.3g} against the twin's {good:.3g} (bar {cr.BOUND:g})")
    assert good <= cr.BOUND < bad


def test_the_stream_mutant_of_the_chain_misses_the_bar():
    """Corrector step c on stream c instead of 1 + c: step 0 would reuse the predictor's normals."""
    c = cr.kernel_case(5, 11)
    z, nm = torch.from_numpy(c["z"]), torch.from_numpy(c["nm"])
    eps_fn = lambda zz, t: torch.from_numpy(c["eps"])
    _, row, adaptive = cr.kernel_rows()[0]
    good = cr.Draws(SEED, BASE, T, c["B"], 5, 8)
    bad = cr.Draws(SEED, BASE, T, c["B"], 5, 8, mutant="stream_c")
    rx, rh = good.corrector(0, 6)
    assert torch.equal(bad.corrector(0, 6)[0], good.at(0, 6)[0]) and not torch.equal(rx, good.at(0, 6)[0])
    ref, A, _, _ = cr.langevin_ref(c["z"], c["eps"], c["nm"], row, adaptive, rx.numpy(), rh.numpy())
    for draws, inside in ((good, True), (bad, False)):
        got, _ = cr.corrector_block(z, eps_fn, 8, 6, nm, row, adaptive, 1, draws, step=cr.langevin_f32)
        assert (cr.ratio(got.numpy(), ref, A, c["nm"]) <= cr.BOUND) == inside


def test_the_draw_layout():
    d = cr.Draws(SEED, BASE, T, 2, 3, 8)
    lib = _lib.load()
    rx, rh = d.corrector(1, 2)                                # stream 2, arrival s = 2: draw (T + 2) * 2 + (T - 2)
    assert rx[1, 2, 1].item() == lib.hd_philox_normal_host(SEED, BASE + 1, 26, 2 * 11 + 1)
    assert rh[0, 1, 7].item() == lib.hd_philox_normal_host(SEED, BASE, 26, 1 * 11 + 10)
    assert d.at(0, 2)[0][0, 0, 0].item() == lib.hd_philox_normal_host(SEED, BASE, 6, 0)      # the predictor's draw does not move
    one = cr.Draws(SEED, BASE, T, 2, 3, 8, rows=1).corrector(0, 2)
    assert one[0].shape == (1, 3, 3) and torch.equal(one[0][0], d.corrector(0, 2)[0][0])


# ----------------------------------------------------------------------------- the analytic check

def gaussian_chain(var0, g, sigma, alpha, v, steps, seed, B=256, N=8, F=8):
    """`steps` fixed-gain steps of the restatement on B * N * F independent N(0, var0) values in the feature columns (which are not
    centred) under the exact score of data N(0, v); returns the sample variance after every step."""
    rng = np.random.Generator(np.random.PCG64(seed))
    D = 3 + F
    z = np.zeros((B, N, D))
    z[:, :, 3:] = rng.standard_normal((B, N, F)) * math.sqrt(var0)
    nm = np.ones((B, N), dtype=np.uint8)
    out = []
    for _ in range(steps):
        eps = cr.gaussian_eps(z, alpha, sigma, v)
        z, _, gains, kept = cr.langevin_ref(z, eps, nm, (sigma, g, math.inf), 0, rng.standard_normal((B, N, 3)), rng.standard_normal((B, N, F)))
        assert not kept.any() and (gains == float(np.float32(g))).all()
        out.append(float((z[:, :, 3:] ** 2).mean()))
    return out


def test_fixed_gain_steps_follow_the_variance_recursion_of_a_gaussian():
    alpha, sigma, v = 0.8, 0.6, 2.5                            # both are float32-exact enough: the row is rounded to fp32
    sigma = float(np.float32(sigma))
    s2 = alpha * alpha * v + sigma * sigma
    g = float(np.float32(0.3 * s2 / (sigma * sigma)))          # g sigma^2 / s2 = 0.3: the distance to the fixed point shrinks by 0.49 a step
    n = 256 * 8 * 8
    tol = 4.0 * math.sqrt(2.0 / n)                             # four standard errors of a sample variance of n normal values
    fixed = cr.variance_fixed_point(g, sigma, s2)
    assert abs(cr.variance_step(fixed, g, sigma, s2) - fixed) < 1e-12 * fixed
    assert abs(fixed - s2 / (1.0 - 0.15)) < 1e-6 * fixed       # the known bias of the unadjusted chain: s2 / (1 - g sigma^2 / (2 s2))
    # the stationary variance
    got = gaussian_chain(fixed, g, sigma, alpha, v, 30, seed=1)
    assert abs(got[-1] - fixed) <= tol * fixed, (got[-1], fixed)
    # C steps from a wrong variance contract towards it at the recursion's rate
    for var0 in (4.0 * s2, 0.1 * s2):
        got = gaussian_chain(var0, g, sigma, alpha, v, 4, seed=2)
        want, rate = var0, (1.0 - g * sigma * sigma / s2) ** 2
        for c in range(4):
            want = cr.variance_step(want, g, sigma, s2)
            assert abs((want - fixed) - rate ** (c + 1) * (var0 - fixed)) < 1e-9 * fixed
            assert abs(got[c] - want) <= tol * want, (var0, c, got[c], want)
        assert abs(got[3] - fixed) < 0.1 * abs(var0 - fixed)
        print(f"gaussian var0 = {var0:.3g}: after 1..4 steps {[round(x, 4) for x in got]}, recursion ends at {want:.4f}, fixed point {fixed:.4f}")


# ----------------------------------------------------------------------------- the keyword, the rows, the plan

def test_keyword_validation_and_rows():
    for bad in (-1, 9, 1.5, True, "2"):
        with pytest.raises(ValueError, match="steps must be"):
            Corrector(bad)
    for bad in (-0.1, math.inf, math.nan, "x", True, [], [0.1, -1.0]):
        with pytest.raises(ValueError, match="snr"):
            Corrector(1, snr=bad)
    with pytest.raises(ValueError, match="mode must be"):
        Corrector(1, mode="langevin")
    with pytest.raises(ValueError, match="needs gain"):
        Corrector(1, mode="fixed")
    with pytest.raises(ValueError, match="gain goes with mode 'fixed'"):
        Corrector(1, gain=0.1)
    for bad in (0, -1.0, math.nan, "x"):
        with pytest.raises(ValueError, match="max_gain must be"):
            Corrector(1, max_gain=bad)
    c = Corrector()
    assert (c.steps, c.snr, c.mode, c.gain, c.max_gain, c.adaptive) == (1, 0.16, "snr", None, math.inf, 1) and c.active
    assert not Corrector(0).active and not Corrector(2, snr=0).active and not Corrector(2, snr=[0, 0]).active
    assert not Corrector(2, mode="fixed", gain=0.0).active and Corrector(2, mode="fixed", gain=[0, 0.1]).active
    assert Corrector(2, mode="fixed", gain=0.1).adaptive == 0
    g = torch.linspace(-5, 5, 21, dtype=torch.float64)
    path = [20, 15, 10, 5, 0]
    rows = corrector.rows(g, path, Corrector(2, snr=0.16, max_gain=0.5))
    want = cr.rows_from_grid(g, path, "snr", 0.16, 0.5)
    assert rows.shape == (4, 3) and rows.dtype == np.float32 and (rows == want).all()
    a2 = [torch.sigmoid(-g[t]) / torch.sigmoid(-g[s]) for t, s in zip(path[:-1], path[1:])]
    assert np.allclose(rows[:, 1], [2 * 0.16 ** 2 * float(a) for a in a2], rtol=1e-6) and (rows[:, 2] == 0.5).all()
    assert np.allclose(rows[:, 0], [math.sqrt(float(torch.sigmoid(g[t]))) for t in path[:-1]], rtol=1e-7)
    rows = corrector.rows(g, path, Corrector(1, mode="fixed", gain=[0.1, 0.0, 0.2, 0.3]))
    assert np.allclose(rows[:, 1], [0.1, 0.0, 0.2, 0.3]) and np.isinf(rows[:, 2]).all()
    assert (corrector.rows(g, path, Corrector(1, snr=[0.1, 0.2, 0.0, 0.3])) == cr.rows_from_grid(g, path, "snr", [0.1, 0.2, 0.0, 0.3])).all()
    with pytest.raises(ValueError, match="one value per transition"):
        corrector.rows(g, path, Corrector(1, snr=[0.1, 0.2]))


def test_plan_off_is_the_plan_without_the_keyword():
    m = small_model()
    assert "corrector" in hplan.KEYWORDS and hplan.Plan._fields[-1] == "corrector"
    base = hplan.plan(m, "t", B=4)
    assert base.corrector is None and base.path is None
    for off in (None, Corrector(0), Corrector(2, snr=0.0), Corrector(1, snr=[0.0] * 20), Corrector(3, mode="fixed", gain=0)):
        assert hplan.plan(m, "t", B=4, corrector=off) == base
    few = hplan.plan(m, "t", B=4, steps=5, eta=0.0)
    assert hplan.plan(m, "t", B=4, steps=5, eta=0.0, corrector=Corrector(0)) == few
    c = Corrector(2)
    p = hplan.plan(m, "t", B=4, corrector=c)
    assert p.corrector is c and p.path == list(range(20, -1, -1)) and p.eta == 1.0 and p.K == 20      # always on a path: the identity one
    for kw in (dict(steps=5, eta=0.0), dict(steps=5, solver="dpm2m"), dict(steps=5, solver="sde2m"), dict(steps=5, eta=0.5)):
        p = hplan.plan(m, "t", B=4, corrector=c, **kw)
        assert p.corrector is c and p.K == 5 and p[:10] == hplan.plan(m, "t", B=4, **kw)[:10]
    p = hplan.plan(m, "t", B=4, corrector=c, steps=5, keep_frames=3, record="x0")       # frames are the predictor's: the recording plan's own
    q = hplan.plan(m, "t", B=4, steps=5, keep_frames=3, record="x0")
    assert p.corrector is c and p.frames == q.frames and p.record == q.record == 1 and torch.equal(p.chain_t, q.chain_t)
    p = hplan.plan(m, "t", B=4, corrector=c, steps=5, restraints=Restraints(obstacles=[[0, 0, 0, 1, 1]]), restraint_scale=1.0)
    assert p.corrector is c and p.restraints is not None
    assert hplan.plan(m, "t", "latent", t_start=10, steps=2, corrector=c).corrector is c
    m.corrector = c
    assert hplan.plan(m, "t", B=4).corrector is c and hplan.plan(m, "t", B=4, corrector=Corrector(0)).corrector is None


def test_refusals_come_from_the_plan_before_the_gpu():
    m = small_model()
    nm = torch.ones(4, 3, 1, dtype=torch.bool)
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    z3, z8, z11 = torch.zeros(4, 3, 3), torch.zeros(4, 3, 8), torch.zeros(4, 3, 11)
    mol = {"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}
    c = Corrector(2)
    run = lambda **k: m.sample_from_masks(nm, None, None, **k)
    with pytest.raises(ValueError, match="must be a hierdiff_amd.corrector.Corrector"):
        run(corrector=dict(steps=2))
    with pytest.raises(NotImplementedError, match=r"corrector= and steering \(particles=\)"):
        run(corrector=c, restraints=rs, particles=2, steer_scale=1.0)
    with pytest.raises(NotImplementedError, match="no injected noise"):
        run(corrector=c, raw_noises=[(z3, z8)] * 22)
    with pytest.raises(NotImplementedError, match="no injected noise"):
        m.sample_from_latent(z11, nm, steps=2, t_start=10, corrector=c, raw_noises=[(z3, z8)] * 3)
    with pytest.raises(ValueError, match=r"one value per transition \(5\)"):
        run(steps=5, corrector=Corrector(1, snr=[0.1, 0.2]))
    with pytest.raises(NotImplementedError, match="pocket models"):
        run(corrector=c, pocket=(z3, z8, nm, torch.ones(4, 3, 3)))
    with pytest.raises(ValueError, match="fix_noise"):
        from hierdiff_amd.diversity import Diversity
        run(corrector=c, diversity=Diversity(2, 1.0), fix_noise=True, steps=4, eta=0.0)
    # what passes the plan reaches the device check
    for kw in (dict(), dict(fix_noise=True), dict(steps=4, eta=0.0), dict(steps=4, solver="dpm2m"), dict(steps=4, solver="sde2m"),
               dict(restraints=rs, restraint_scale=1.0), dict(keep_frames=3, record="x0")):
        with pytest.raises(_lib.HierDiffHipError, match="runs only on an MI355X"):
            run(corrector=c, **kw)
    with pytest.raises(_lib.HierDiffHipError, match="runs only on an MI355X"):
        m.path_steps(z11, nm, corrector=c, steps=4)
    with pytest.raises(_lib.HierDiffHipError, match="runs only on an MI355X"):
        m.sample(4, 3, nm, None, None, corrector=c)            # the EDM signature takes the keyword
    with pytest.raises(NotImplementedError, match="predictor-corrector sampling is not supported here"):
        m.score([mol], "cpu", corrector=c)
    # the entry points that take none: the model's attribute is refused, not ignored
    m.corrector = c
    fm = torch.zeros(4, 3, 1, dtype=torch.bool)
    for call in (lambda: m.sample_inpaint(nm, fm, z3, z8), lambda: m.inpaint_steps(z11, 20, 0, nm, fm, z3, z8),
                 lambda: m.sample_grow([mol], [4], "cpu"), lambda: m.sample_batches(2, 1, "cpu"),
                 lambda: m.encode(z3, z8, nm), lambda: m.interpolate(mol, mol, 3, "cpu"), lambda: m.score([mol], "cpu")):
        with pytest.raises(NotImplementedError, match="predictor-corrector sampling is not supported here"):
            call()
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="noise_mode 'torch'"):
        run()
    m.noise_mode = "philox"
    m.dynamics.mode = "gnn_dynamics"
    with pytest.raises(NotImplementedError, match="gnn_dynamics"):
        run()


def test_no_earlier_error_moves():
    """Every error the plan raised before still comes first, with its message, when corrector= is given as well."""
    from hierdiff_amd.diversity import Diversity
    m = small_model()
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    earlier = [(dict(steps=4, timesteps=[20, 10, 0]), "either steps or timesteps"), (dict(eta=2.0), "eta"), (dict(solver="nope"), "solver"),
               (dict(guidance_scale="x"), "guidance_scale"), (dict(restraints=rs, restraint_scale="x"), "restraint_scale"),
               (dict(record="z"), "records nothing without keep_frames"), (dict(restraints=rs, particles=3, steer_scale=1.0), "multiple of particles"),
               (dict(diversity=Diversity(3, 1.0)), "multiple of the diversity's particles")]
    for kw, msg in earlier:
        for c in (None, dict(steps=2), Corrector(2)):
            with pytest.raises((ValueError, NotImplementedError)) as a:
                hplan.plan(m, "t", B=4, corrector=c, **kw)
            with pytest.raises((ValueError, NotImplementedError)) as b:
                hplan.plan(m, "t", B=4, **kw)
            assert str(a.value) == str(b.value) and msg in str(a.value), (kw, str(a.value))


def test_cli_parse_and_refusals(tmp_path, capsys):
    from hierdiff_amd import sampler
    base = ["--hidden-nf", "32", "--n-layers", "1", "--timesteps", "8", "--batch-size", "4", "--out", str(tmp_path / "o.pkl")]
    a = sampler.parse_args(base + ["--steps", "4", "--correctors", "2", "--corrector-snr", "0.1"])
    assert (a.correctors, a.corrector_snr, a.corrector_mode, a.corrector_gain) == (2, 0.1, None, None)
    a = sampler.parse_args(base + ["--correctors", "1", "--corrector-mode", "fixed", "--corrector-gain", "0.02", "--solver", "dpm2m", "--steps", "4"])
    assert (a.correctors, a.corrector_mode, a.corrector_gain) == (1, "fixed", 0.02)
    cc = ["--correctors", "2"]
    bad = [(["--corrector-snr", "0.1"], "need --correctors"), (["--corrector-mode", "snr"], "need --correctors"),
           (["--corrector-gain", "0.1"], "need --correctors"), (["--correctors", "0"], "1 .. 8"), (["--correctors", "9"], "1 .. 8"),
           (cc + ["--corrector-gain", "0.1"], "go together"), (cc + ["--corrector-mode", "fixed"], "go together"),
           (cc + ["--corrector-mode", "fixed", "--corrector-gain", "0.1", "--corrector-snr", "0.1"], "--corrector-snr goes with"),
           (cc + ["--corrector-snr", "-1"], "--corrector-snr must be"), (cc + ["--corrector-snr", "nan"], "--corrector-snr must be"),
           (cc + ["--corrector-mode", "mala"], "invalid choice"),
           (cc + ["--restraints", "r.json", "--particles", "2", "--steer-scale", "1"], "does not combine with --particles"),
           (cc + ["--known", "k.pkl", "--grow", "2"], "does not combine with --known")]
    for extra, msg in bad:
        with pytest.raises(SystemExit) as e:
            sampler.parse_args(base + extra)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, (extra, msg)


# ----------------------------------------------------------------------------- the C ABI without a device

def test_new_symbols_and_null_refusals():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    r3 = (C.c_float * 3)(0.5, 0.1, math.inf)
    assert lib.hd_set_corrector(None, 1, r3) == -1 and b"hd_set_corrector" in lib.hd_last_error()
    assert lib.hd_corrector_attach(None, 1, 1, None) == -1 and b"hd_corrector_attach: null topology" in lib.hd_last_error()
    assert lib.hd_corrector_detach(None) == 0
    assert lib.hd_corrector_read(None, None, None) == -1
    assert lib.hd_langevin_step(None, None, None, None, r3, 1, None, None, 1, 0, 0, 0, None, None, None) == -1
    assert b"hd_langevin_step: null handle/topology" in lib.hd_last_error()
    with open(__import__("os").path.join(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))), "include",
                                         "hierdiff_hip.h")) as f:
        header = f.read()
    for s in NEW_SYMBOLS:
        assert f" {s}(" in header
