"""CPU tier of stochastic second-order multistep sampling (solver="sde2m": hierdiff_amd/paths.py, hd_set_path_multistep_sde /
hd_multistep_sde_step): the coefficient rows against the published form (tests/sde_solver_reference.py), the folded update against
the published update, the convergence order of the SHIPPED rows through the exact variance recursion of the analytic model, the
keywords, the CLI, the new C-ABI symbols and the steering plan - all without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from hierdiff_amd import _lib, paths, plan as hplan, steering
from hierdiff_amd.restraints import Restraints
from tests import sde_solver_reference as sd
from tests.test_inpaint_cpu import cpu_model
from tests.test_solver_cpu import grids

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


def cases(T):
    return [("uniform", paths.uniform_path(T, min(T, 20))), ("quadratic", paths.quadratic_path(T, min(T, 33))),
            ("explicit", [T, T - 1, T // 2, T // 2 - 1, 3, 1, 0]), ("one", [T, 0]), ("two", [T, T // 2, 0])]


# ----------------------------------------------------------------------------- rows

@pytest.mark.parametrize("T", [50, 1000])
def test_rows_match_the_published_form_and_keep_the_eta_1_bits(T):
    worst = 0.0
    for name, g in grids(T):
        for pname, path in cases(T):
            for lof in (True, False):
                K = len(path) - 1
                rows = paths.multistep_sde_coefficients(g, path, lof)
                assert rows.dtype == torch.float64 and tuple(rows.shape) == (K, 6)
                pt = paths.path_tables(g, path, solver="sde2m", lower_order_final=lof)
                assert pt["form"] == 3 and pt["coef_inpaint"] is None and pt["K"] == K and pt["eta"] == 1.0
                assert pt["solver"] == "sde2m" and pt["lower_order_final"] == lof
                assert pt["coef"].dtype == torch.float32 and tuple(pt["coef"].shape) == (K, 6)
                assert torch.equal(pt["coef"], rows.to(torch.float32))                       # rounded once
                ref = sd.sde_rows(g, path, lof)
                for k, r in enumerate(ref):
                    for j in range(6):                                                       # relative 1e-6 after the fp32 rounding
                        got = float(pt["coef"][k, j])
                        assert abs(got - r[j]) <= 1e-6 * abs(r[j]), (name, pname, lof, k, j, got, r[j])
                        if r[j] != 0.0:
                            worst = max(worst, abs(got - r[j]) / abs(r[j]))
                assert float(rows[0, 3]) == 0.0
                if K > 1:
                    assert (float(rows[-1, 3]) == 0.0) == lof, (name, pname, lof)
                    assert all(float(v) > 0.0 for v in rows[1:-1, 3])
                # a, b, c are the very fp32 values of the eta = 1 linear rows (what hd_set_path takes as form 1)
                idx = torch.as_tensor(path, dtype=torch.int64)
                lin = paths.linear_coefficients(g[idx[1:]], g[idx[:-1]], 1.0)
                assert torch.equal(pt["coef"][:, :3], lin[:, :3].to(torch.float32)), (name, pname)
                p2 = paths.path_tables(g, path, solver="dpm2m", lower_order_final=lof)
                assert torch.equal(pt["t_idx"], p2["t_idx"]) and torch.equal(pt["s_idx"], p2["s_idx"])
                assert torch.equal(pt["coef"][:, 4:], p2["coef"][:, 3:])                     # p, q
                assert paths.path_tables(g, path, paths.Multistep(lof, True))["coef"].equal(pt["coef"])
    print(f"T={T}: worst relative difference of an fp32 row entry from the published form {worst:.2e} (bar 1e-6)")


def test_multistep_keeps_its_first_field_and_the_other_solvers_their_tables():
    assert paths.Multistep(True) == paths.Multistep(True, False) and paths.Multistep().stochastic is False
    assert paths.Multistep(False).lower_order_final is False and "sde2m" in paths.SOLVERS
    assert paths.check_solver("dpm2m") == paths.Multistep(True) and paths.check_solver("sde2m", None, False) == paths.Multistep(False, True)
    assert paths.check_solver("sde2m", 1.0) == paths.Multistep(True, True) and paths.check_solver(None) is None
    for bad in (0.0, 0.5):
        with pytest.raises(ValueError, match="sde2m"):
            paths.check_solver("sde2m", bad)
    for _, g in grids(50):
        path = paths.uniform_path(50, 9)
        assert paths.path_tables(g, path, solver="dpm2m")["form"] == 2 and paths.path_tables(g, path, 0.5)["form"] == 1
        assert paths.path_tables(g, path)["form"] == 0
    g = torch.tensor([-3.0, -1.0, -1.0, 2.0, 1.5, 4.0])
    paths.multistep_sde_coefficients(g, [5, 3, 1, 0])
    for path in ([5, 2, 1, 0], [5, 4, 3, 0]):
        with pytest.raises(ValueError, match="increases strictly"):
            paths.path_tables(g, path, solver="sde2m")


# ----------------------------------------------------------------------------- the folded update is the published one

def test_folded_update_equals_the_published_form():
    T = 1000
    gen = torch.Generator().manual_seed(0)
    for name, g in grids(T):
        for pname, path in cases(T):
            rows = sd.sde_rows(g, path, lower_order_final=False)
            prows = paths.multistep_sde_coefficients(g, path, False)
            for k in range(len(path) - 1):
                z, eps, xp, xi = (torch.randn(64, generator=gen, dtype=torch.float64) for _ in range(4))
                for row in (rows[k], tuple(float(v) for v in prows[k])):
                    xk, folded = sd.folded_step(row, z, eps, xp if k > 0 else None, xi)
                    a_t, s_t = sd.alpha_sigma(float(g[path[k]]))
                    assert float((xk - (z - s_t * eps) / a_t).abs().max()) <= 1e-12 * float(xk.abs().max())
                    book = sd.published_step(g, path[k], path[k + 1], path[k - 1] if k > 0 else None, z, xk, xp if k > 0 else None, xi)
                    assert float((folded - book).abs().max()) <= 1e-12 * max(1.0, float(book.abs().max())), (name, pname, k)


# ----------------------------------------------------------------------------- convergence of the shipped rows

def shipped_errors(rows_fn):
    g = sd.analytic_grid(1000)
    gt = torch.tensor(g, dtype=torch.float64)
    return {K: sd.variance_error(rows_fn(gt, sd.uniform_path(1000, K)), g, sd.uniform_path(1000, K), 1.0) for K in (20, 40, 80, 160)}


def ancestral_shipped(gt, path):
    idx = torch.as_tensor(path, dtype=torch.int64)
    lin = paths.linear_coefficients(gt[idx[1:]], gt[idx[:-1]], 1.0)
    two = paths.multistep_coefficients(gt, path)
    return [(float(lin[k, 0]), float(lin[k, 1]), float(lin[k, 2]), 0.0, float(two[k, 3]), float(two[k, 4])) for k in range(len(path) - 1)]


def test_convergence_order_of_the_shipped_rows():
    """Var(z_0) of the analytic Gaussian-data model (variance 1) by the exact recursion: second order for sde2m, first for eta = 1."""
    e2 = shipped_errors(lambda gt, path: paths.multistep_sde_coefficients(gt, path).tolist())
    e1 = shipped_errors(ancestral_shipped)
    for K in (20, 40, 80, 160):
        print(f"K={K}: relative error of Var(z_0): eta=1 {e1[K]:.3e}  sde2m {e2[K]:.3e}")
    r2, r1 = (e2[40] / e2[80], e2[80] / e2[160]), (e1[40] / e1[80], e1[80] / e1[160])
    print(f"ratios 40->80, 80->160: sde2m {r2[0]:.2f} {r2[1]:.2f}; eta=1 {r1[0]:.2f} {r1[1]:.2f}")
    assert r2[0] >= 3.0 and r2[1] >= 3.0, r2
    assert r1[0] <= 2.2 and r1[1] <= 2.2, r1
    assert e2[20] <= e1[20] / 5.0, (e2[20], e1[20])
    # the reference's own rows give the same figures, and the two likely mistakes miss the bars
    g = sd.analytic_grid(1000)
    for K in (20, 160):
        p = sd.uniform_path(1000, K)
        assert abs(sd.variance_error(sd.sde_rows(g, p), g, p) - e2[K]) <= 1e-9 * e2[K]

    def mutant(kind):
        def rows(gt, path):
            out = paths.multistep_sde_coefficients(gt, path).tolist()
            two = paths.multistep_coefficients(gt, path)
            for k, r in enumerate(out):
                r[3] = float(two[k, 2]) if kind == "h" else 2.0 * r[3]
            return out
        return shipped_errors(rows)
    for kind in ("h", "no_half"):
        m = mutant(kind)
        assert not (m[40] / m[80] >= 3.0 and m[80] / m[160] >= 3.0), (kind, m)


# ----------------------------------------------------------------------------- keywords

def test_keywords_before_the_gpu_is_touched(monkeypatch):
    m, _ = cpu_model(T=6, L=1)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    fm = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool).view(B, N, 1)
    xk, hk, z = torch.zeros(B, N, 3), torch.zeros(B, N, 8), torch.zeros(B, N, 11)
    known = [{"x": torch.zeros(1, 3), "h": torch.zeros(1, 8)}]
    samples = [{"x": torch.zeros(2, 3), "h": torch.zeros(2, 8)}]
    sampling = [lambda **kw: m.sample_from_masks(nm, None, **kw), lambda **kw: m.sample(2, "cpu", **kw),
                lambda **kw: m.sample_batches(2, 2, "cpu", **kw), lambda **kw: m.path_steps(z, nm, **kw),
                lambda **kw: m.sample_from_latent(z, nm, t_start=4, **kw), lambda **kw: m.latent_steps(z, nm, t_start=4, **kw),
                lambda **kw: m.vary(samples, "cpu", 4, **kw)]
    for call in sampling:
        for bad in (0.5, 0.0):
            with pytest.raises(ValueError, match="eta"):
                call(solver="sde2m", steps=3, eta=bad)
        with pytest.raises(ValueError, match="steps"):
            call(solver="sde2m", steps=7)
        with pytest.raises(ValueError, match="spacing"):
            call(solver="sde2m", steps=3, spacing="log")
    refused = [lambda **kw: m.sample_inpaint(nm, fm, xk, hk, **kw), lambda **kw: m.sample_grow(known, [3], "cpu", **kw)]
    for call in refused:
        with pytest.raises(ValueError, match="sde2m"):
            call(solver="sde2m", steps=3)
    with pytest.raises(ValueError, match="sde2m"):
        m.encode(xk, hk, nm, solver="sde2m")
    m.sample_solver = "sde2m"
    for call in refused:
        with pytest.raises(ValueError, match="sde2m"):
            call(steps=3)
    with pytest.raises(ValueError, match="sde2m"):
        m.inpaint_steps(z, 6, 0, nm, fm, xk, hk)                         # takes the model's attribute
    with pytest.raises(ValueError, match="eta"):
        m.sample_from_masks(nm, None, steps=3, eta=0.5)
    m.sample_eta = 0.0                                                   # ignored by sde2m: eta defaults to 1
    sde = paths.Multistep(True, True)
    assert m._resolve_path(steps=3) == ([6, 4, 2, 0], sde)
    assert m._resolve_path(steps=3, lower_order_final=False) == ([6, 4, 2, 0], paths.Multistep(False, True))
    assert m._resolve_path() == ([6, 5, 4, 3, 2, 1, 0], sde)                                 # never the plain loop
    assert m._resolve_path(steps=3, solver="dpm2m") == ([6, 4, 2, 0], paths.Multistep(True))
    m.sample_solver, m.sample_eta = None, 1.0
    assert m._resolve_path(steps=3, solver="sde2m") == ([6, 4, 2, 0], sde)
    assert m._resolve_path(steps=3, solver="sde2m", eta=1.0) == ([6, 4, 2, 0], sde)
    assert m._latent_path(4, 2, None, None, None, "sde2m", False) == (4, [4, 2, 0], paths.Multistep(False, True))
    assert m._resolve_path() is None


# ----------------------------------------------------------------------------- the steering plan

def test_steering_takes_the_stochastic_solver_and_still_refuses_the_deterministic_one():
    from hierdiff_amd import EnVariationalDiffusion, default_config
    m = EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=20))
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    kw = dict(B=8, restraints=rs, particles=4, steer_scale=2.0, steps=5)
    p = hplan.plan(m, "t", solver="sde2m", **kw)
    assert p.steer == steering.Steer(4, 2.0, 0.5, None) and p.eta == paths.Multistep(True, True) and p.K == 5
    assert p.restraints is not None and p.path == paths.uniform_path(20, 5)
    p = hplan.plan(m, "t", solver="sde2m", lower_order_final=False, steer_ess=0.75, **kw)
    assert p.steer.ess == 0.75 and p.eta == paths.Multistep(False, True)
    with pytest.raises(ValueError, match="dpm2m"):
        hplan.plan(m, "t", solver="dpm2m", **kw)
    with pytest.raises(ValueError, match="eta = 0"):
        hplan.plan(m, "t", eta=0.0, **kw)
    with pytest.raises(NotImplementedError, match="raw_noises"):
        hplan.plan(m, "t", solver="sde2m", injected=True, **kw)
    nm = torch.ones(8, 3, 1, dtype=torch.bool)
    with pytest.raises(ValueError, match="fix_noise"):
        m.sample_from_masks(nm, None, None, fix_noise=True, solver="sde2m", **{k: v for k, v in kw.items() if k != "B"})


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_set_path_multistep_sde", "hd_multistep_sde_step"]


def test_sde_symbols_exported_declared_and_null_safe(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        mm = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert mm, name
        assert len([a for a in mm.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays
    assert "#define HD_ABI_VERSION 12" in hdr
    ti, si, rows = (C.c_int * 2)(4, 2), (C.c_int * 2)(2, 0), (C.c_float * 12)()
    assert lib.hd_set_path_multistep_sde(None, 2, ti, si, rows) == -1 and b"hd_set_path_multistep_sde" in lib.hd_last_error()
    assert lib.hd_set_path_multistep_sde(None, 0, ti, si, rows) == -1
    assert lib.hd_multistep_sde_step(None, None, None, None, rows, None, None, None, None, 1, 0, 0, 0, 0, -1, None, None) == -1
    assert b"hd_multistep_sde_step: null" in lib.hd_last_error()


# ----------------------------------------------------------------------------- CLI

def test_cli_flags():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--spacing", "quadratic"])
    assert (a.solver, a.steps, a.eta, a.spacing, a.lower_order_final) == ("sde2m", 20, 1.0, "quadratic", True)
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--eta", "1", "--no-lower-order-final"])
    assert (a.solver, a.eta, a.lower_order_final) == ("sde2m", 1.0, False)
    a = sampler.parse_args(["--solver", "sde2m", "--vary", "m.pkl", "--t-start", "300", "--steps", "10"])
    assert a.solver == "sde2m" and a.vary == "m.pkl"
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--guidance", "2.0", "--context", "0.5"])
    assert a.solver == "sde2m" and a.guidance == 2.0
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--chain", "4"])
    assert a.solver == "sde2m"
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--restraints", "r.json", "--particles", "4", "--steer-scale", "1e-4",
                            "--batch-size", "8"])
    assert (a.solver, a.particles, a.steer_scale) == ("sde2m", 4, 1e-4)
    a = sampler.parse_args(["--solver", "sde2m", "--steps", "20", "--restraints", "r.json", "--restraint-scale", "0.1"])
    assert a.solver == "sde2m" and a.restraint_scale == 0.1
    for bad in (["--solver", "sde2m", "--eta", "0.5"], ["--solver", "sde2m", "--eta", "0"],
                ["--solver", "sde2m", "--known", "k.pkl", "--grow", "2"], ["--solver", "sde2m", "--score", "m.pkl"],
                ["--solver", "sde2m", "--interpolate", "m.pkl", "--frames", "4"], ["--no-lower-order-final"],
                ["--solver", "sde3m"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
    # dpm2m as before
    a = sampler.parse_args(["--solver", "dpm2m", "--steps", "20"])
    assert (a.solver, a.eta) == ("dpm2m", 0.0)
