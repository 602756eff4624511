"""CPU tier of second-order multistep sampling (solver="dpm2m": hierdiff_amd/paths.py, hd_set_path_multistep / hd_multistep_step):
the coefficient rows against tests/solver_reference.py, the folded update against the textbook D-form, the convergence order on
the analytic Gaussian-data model in float64, the new C-ABI symbols, and the Python / CLI argument errors - all without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.noise_model import PredefinedNoiseSchedule, schedule_tables
from tests import solver_reference as sr
from tests.test_inpaint_cpu import cpu_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


def grids(T):
    m, _ = cpu_model(T=T, L=1)
    out = [("learned", schedule_tables(m.gamma, T)["gamma"]),
           ("cosine", schedule_tables(PredefinedNoiseSchedule("cosine", T, 1e-4), T)["gamma"]),
           ("polynomial_2", schedule_tables(PredefinedNoiseSchedule("polynomial_2", T, 1e-5), T)["gamma"])]
    return [(n, torch.as_tensor(g, dtype=torch.float32).reshape(-1)) for n, g in out]


def cases(T):
    return [("uniform", paths.uniform_path(T, min(T, 20))), ("quadratic", paths.quadratic_path(T, min(T, 33))),
            ("explicit", [T, T - 1, T // 2, T // 2 - 1, 3, 1, 0]), ("partial", paths.partial_path(T, T // 3, 7)),
            ("one", [T, 0]), ("two", [T, T // 2, 0])]


# ----------------------------------------------------------------------------- A1. rows

@pytest.mark.parametrize("T", [50, 1000])
def test_rows_match_the_reference_and_keep_the_eta_0_bits(T):
    for name, g in grids(T):
        for pname, path in cases(T):
            for lof in (True, False):
                rows = paths.multistep_coefficients(g, path, lof)
                ref = sr.multistep_rows(g, path, lof)
                assert rows.dtype == torch.float64 and tuple(rows.shape) == (len(path) - 1, 5)
                for k, r in enumerate(ref):
                    for j in range(5):
                        assert abs(float(rows[k, j]) - r[j]) <= 1e-12 * max(1.0, abs(r[j])), (name, pname, lof, k, j)
                assert float(rows[0, 2]) == 0.0
                if len(path) > 2:
                    assert (float(rows[-1, 2]) == 0.0) == lof, (name, pname, lof)
                    assert all(float(v) != 0.0 for v in rows[1:-1, 2])
                pt = paths.path_tables(g, path, solver="dpm2m", lower_order_final=lof)
                p0 = paths.path_tables(g, path, 0.0)
                assert pt["form"] == 2 and pt["coef_inpaint"] is None and pt["K"] == len(path) - 1
                assert pt["coef"].dtype == torch.float32 and tuple(pt["coef"].shape) == (len(path) - 1, 5)
                assert torch.equal(pt["coef"], rows.to(torch.float32))                       # rounded once
                assert torch.equal(pt["coef"][:, :2], p0["coef"][:, :2]), (name, pname)      # the very fp32 a, b of eta = 0
                assert torch.equal(pt["t_idx"], p0["t_idx"]) and torch.equal(pt["s_idx"], p0["s_idx"])
                assert paths.path_tables(g, path, paths.Multistep(lof))["coef"].equal(pt["coef"])


def test_first_order_tables_are_untouched():
    T = 50
    for _, g in grids(T):
        path = paths.uniform_path(T, 9)
        for eta in (0.0, 0.5, 1.0):
            a, b = paths.path_tables(g, path, eta), paths.path_tables(g, path, eta, solver="ddim")
            assert a["form"] == b["form"] == (0 if eta == 1.0 else 1) and torch.equal(a["coef"], b["coef"])
        assert torch.equal(paths.path_tables(g, path)["coef"], paths.path_tables(g, path, 1.0)["coef"])


# ----------------------------------------------------------------------------- A2. the folded form is the textbook D-form

def test_folded_update_equals_the_textbook_form():
    T = 1000
    gen = torch.Generator().manual_seed(0)
    for name, g in grids(T):
        for pname, path in cases(T):
            rows = sr.multistep_rows(g, path, lower_order_final=False)
            prows = paths.multistep_coefficients(g, path, False)
            for k in range(len(path) - 1):
                z = torch.randn(64, generator=gen, dtype=torch.float64)
                eps = torch.randn(64, generator=gen, dtype=torch.float64)
                xp = torch.randn(64, generator=gen, dtype=torch.float64)
                for a, b, c2, p, q in (rows[k], tuple(float(v) for v in prows[k])):
                    xk = p * z - q * eps
                    folded = (a * z - b * eps) + (c2 * (xk - xp) if k > 0 else 0.0)
                    book = sr.textbook_step(g, path[k], path[k + 1], path[k - 1] if k > 0 else None, z, xk, xp if k > 0 else None)
                    assert float((folded - book).abs().max()) <= 1e-12 * max(1.0, float(book.abs().max())), (name, pname, k)


# ----------------------------------------------------------------------------- A3. convergence order on the analytic model

def analytic_errors(run):
    """K -> relative error of z_0 for K in {20, 40, 80, 160}; run(path, second) -> z_0."""
    T, c2data = 1000, 4.0
    g = sr.analytic_grid(T)
    zT = torch.randn(110, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    exact = sr.analytic_exact(g, T, zT, c2data)
    return {second: {K: sr.rel_err(run(g, sr.uniform_path(T, K), zT, c2data, second), exact) for K in (20, 40, 80, 160)}
            for second in (True, False)}


def check_order(err):
    e2, e1 = err[True], err[False]
    for K in (20, 40, 80, 160):
        print(f"K={K}: eta=0 {e1[K]:.2e}  2M {e2[K]:.2e}")
    for K in (40, 80):
        assert 3.0 <= e2[K] / e2[2 * K] <= 5.0, (K, e2[K] / e2[2 * K])
        assert 1.7 <= e1[K] / e1[2 * K] <= 2.3, (K, e1[K] / e1[2 * K])
    assert e2[80] < e1[80] / 10.0, (e2[80], e1[80])


def test_convergence_order_on_the_analytic_model():
    check_order(analytic_errors(sr.analytic_run))                       # the reference's rows

    def with_product_rows(g, path, zT, c2data, second):                 # the product's rows, same chain
        rows = paths.multistep_coefficients(torch.tensor(g, dtype=torch.float64), path, True)
        z, xp = zT, None
        for k, t in enumerate(path[:-1]):
            a, b, c2, p, q = (float(v) for v in rows[k])
            ev = sr.analytic_eps(g, t, z, c2data)
            xk = p * z - q * ev
            z, xp = (a * z - b * ev) + (c2 * (xk - xp) if second and c2 != 0.0 else 0.0), xk
        return z
    check_order(analytic_errors(with_product_rows))


# ----------------------------------------------------------------------------- A4. argument errors, no GPU and no library

def test_value_errors_before_the_gpu_is_touched(monkeypatch):
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
        for bad in (0.5, 1.0):
            with pytest.raises(ValueError, match="eta"):
                call(solver="dpm2m", steps=3, eta=bad)
        with pytest.raises(ValueError, match="solver"):
            call(solver="dpm3m", steps=3)
        with pytest.raises(ValueError, match="steps"):
            call(solver="dpm2m", steps=7)
        with pytest.raises(ValueError, match="spacing"):
            call(solver="dpm2m", steps=3, spacing="log")
    refused = [lambda **kw: m.sample_inpaint(nm, fm, xk, hk, **kw), lambda **kw: m.sample_grow(known, [3], "cpu", **kw)]
    for call in refused:
        with pytest.raises(ValueError, match="dpm2m"):
            call(solver="dpm2m", steps=3)
        with pytest.raises(ValueError, match="solver"):
            call(solver="heun")
    with pytest.raises(ValueError, match="dpm2m"):
        m.encode(xk, hk, nm, solver="dpm2m")
    # the attribute is the keyword's default; "ddim" spells the first-order path out
    m.sample_solver = "dpm2m"
    for call in refused:
        with pytest.raises(ValueError, match="dpm2m"):
            call(steps=3)
    with pytest.raises(ValueError, match="eta"):
        m.sample_from_masks(nm, None, steps=3, eta=1.0)
    m.sample_eta = 1.0                                                   # ignored by dpm2m
    assert m._resolve_path(steps=3) == ([6, 4, 2, 0], paths.Multistep(True))
    assert m._resolve_path(steps=3, lower_order_final=False) == ([6, 4, 2, 0], paths.Multistep(False))
    assert m._resolve_path() == ([6, 5, 4, 3, 2, 1, 0], paths.Multistep(True))               # never the plain loop
    assert m._resolve_path(steps=3, solver="ddim") == ([6, 4, 2, 0], 1.0)
    assert m._resolve_path(solver="ddim") is None
    m.sample_solver = None
    assert m._resolve_path() is None and m._resolve_path(steps=3, eta=0.0) == ([6, 4, 2, 0], 0.0)
    assert m._resolve_path(steps=3, solver="dpm2m", eta=0.0) == ([6, 4, 2, 0], paths.Multistep(True))
    assert m._latent_path(4, 2, None, None, None, "dpm2m", False) == (4, [4, 2, 0], paths.Multistep(False))


def test_a_grid_that_does_not_increase_raises():
    g = torch.tensor([-3.0, -1.0, -1.0, 2.0, 1.5, 4.0])
    paths.multistep_coefficients(g, [5, 3, 1, 0])
    for path in ([5, 2, 1, 0], [5, 4, 3, 0], [4, 3, 0]):                 # a flat step, two decreasing ones
        with pytest.raises(ValueError, match="increases strictly"):
            paths.multistep_coefficients(g, path)
        with pytest.raises(ValueError, match="increases strictly"):
            paths.path_tables(g, path, solver="dpm2m")


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_set_path_multistep", "hd_multistep_step"]


def test_solver_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays


def test_solver_entry_points_reject_bad_arguments_without_a_gpu(lib):
    ti, si, rows = (C.c_int * 2)(4, 2), (C.c_int * 2)(2, 0), (C.c_float * 10)()
    assert lib.hd_set_path_multistep(None, 2, ti, si, rows) == -1 and b"hd_set_path_multistep" in lib.hd_last_error()
    assert lib.hd_set_path_multistep(None, 0, ti, si, rows) == -1
    assert lib.hd_multistep_step(None, None, None, None, rows, None, None, None, None) == -1
    assert b"hd_multistep_step: null" in lib.hd_last_error()


# ----------------------------------------------------------------------------- CLI

def test_cli_flags():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--solver", "dpm2m", "--steps", "20", "--spacing", "quadratic"])
    assert (a.solver, a.steps, a.eta, a.spacing, a.lower_order_final) == ("dpm2m", 20, 0.0, "quadratic", True)
    a = sampler.parse_args(["--solver", "dpm2m", "--steps", "20", "--eta", "0", "--no-lower-order-final"])
    assert (a.solver, a.eta, a.lower_order_final) == ("dpm2m", 0.0, False)
    a = sampler.parse_args(["--solver", "dpm2m", "--vary", "m.pkl", "--t-start", "300", "--steps", "10"])
    assert a.solver == "dpm2m" and a.vary == "m.pkl"
    a = sampler.parse_args(["--solver", "dpm2m", "--steps", "20", "--guidance", "2.0", "--context", "0.5"])
    assert a.solver == "dpm2m" and a.guidance == 2.0
    a = sampler.parse_args(["--solver", "ddim", "--eta", "0.5"])
    assert (a.solver, a.eta) == ("ddim", 0.5)
    a = sampler.parse_args([])
    assert (a.solver, a.eta, a.lower_order_final) == (None, 1.0, True) and type(a.eta) is float
    for bad in (["--solver", "dpm2m", "--eta", "0.5"], ["--solver", "dpm2m", "--eta", "1"], ["--solver", "heun"],
                ["--solver", "dpm2m", "--known", "k.pkl", "--grow", "2"], ["--no-lower-order-final"],
                ["--solver", "ddim", "--no-lower-order-final"], ["--solver", "dpm2m", "--score", "m.pkl"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
