"""CPU tier of few-step sampling (hierdiff_amd/paths.py, hd_set_path / hd_sample_path / hd_sample_path_inpaint): the path
builders, the coefficient rows against the plain tables and an independent fp64 evaluation, the DDIM consistency of the host
formula, the new C-ABI symbols and their argument checks, and the Python / CLI argument errors - all without a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.noise_model import PredefinedNoiseSchedule, schedule_tables
from tests.test_inpaint_cpu import cpu_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


def schedules(T):
    """(name, gamma module) of the learned and the two predefined schedules."""
    m, _ = cpu_model(T=T, L=1)
    return [("learned", m.gamma), ("cosine", PredefinedNoiseSchedule("cosine", T, 1e-4)),
            ("polynomial_2", PredefinedNoiseSchedule("polynomial_2", T, 1e-5))]


# ----------------------------------------------------------------------------- 1. path builders

@pytest.mark.parametrize("T", [1, 7, 50, 1000])
def test_builders_give_strictly_decreasing_paths_from_T_to_0(T):
    for K in range(1, T + 1):
        for build in (paths.uniform_path, paths.quadratic_path):
            p = build(T, K)
            assert len(p) == K + 1 and p[0] == T and p[-1] == 0, (build.__name__, T, K)
            assert all(isinstance(v, int) for v in p)
            assert all(a > b for a, b in zip(p[:-1], p[1:])), (build.__name__, T, K)
    assert paths.uniform_path(T, T) == list(range(T, -1, -1))
    assert paths.quadratic_path(T, T) == list(range(T, -1, -1))
    assert paths.build_path(T) == list(range(T, -1, -1))


def test_uniform_is_the_documented_formula_and_quadratic_is_denser_near_zero():
    T, K = 1000, 7
    assert paths.uniform_path(T, K) == [T - (2 * k * T + K) // (2 * K) for k in range(K + 1)] == [1000, 857, 714, 571, 429, 286, 143, 0]
    q = paths.quadratic_path(1000, 10)
    gaps = [a - b for a, b in zip(q[:-1], q[1:])]
    assert gaps == sorted(gaps, reverse=True) and gaps[0] > gaps[-1]


def test_explicit_lists_are_validated():
    assert paths.build_path(10, timesteps=[10, 7, 3, 0]) == [10, 7, 3, 0]
    assert paths.build_path(10, timesteps=np.array([10, 4, 0])) == [10, 4, 0]
    for bad in ([9, 3, 0], [10, 3, 1], [10, 3, 3, 0], [10, 3, 5, 0], [10], [10, 2.5, 0], [10, True, 0], 5):
        with pytest.raises(ValueError):
            paths.build_path(10, timesteps=bad)
    with pytest.raises(ValueError, match="not both"):
        paths.build_path(10, steps=3, timesteps=[10, 0])
    for bad in (0, -1, 11, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            paths.build_path(10, steps=bad)
    with pytest.raises(ValueError, match="spacing"):
        paths.build_path(10, steps=3, spacing="cosine")


# ----------------------------------------------------------------------------- 2. identity path = the plain tables

@pytest.mark.parametrize("T", [7, 1000])
def test_identity_path_rows_are_the_plain_tables_bit_for_bit(T):
    for name, gamma in schedules(T):
        tabs = schedule_tables(gamma, T)
        pt = paths.path_tables(tabs["gamma"], paths.uniform_path(T, T), 1.0)
        assert pt["form"] == 0 and pt["K"] == T
        # transition k of the identity path is the plain loop's step s = T - 1 - k
        assert torch.equal(pt["coef"].flip(0), tabs["coef"]), name
        assert pt["t_idx"].tolist() == list(range(T, 0, -1)) and pt["s_idx"].tolist() == list(range(T - 1, -1, -1))
        # the inpainting rows as DiffusionQM9._inpaint_schedule builds them
        g = tabs["gamma"].to(torch.float32).reshape(-1)[:-1]
        c = tabs["coef"]
        rows = torch.stack([torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g)), c[:, 0], torch.sqrt(c[:, 1])], dim=1)
        assert torch.equal(pt["coef_inpaint"].flip(0), rows), name


# ----------------------------------------------------------------------------- 3. linear rows

def fp64_rows(g, path, eta):
    """Independent evaluation with Python floats (math module): a, b, c and sigma_s^2 - sigma~^2 per transition."""
    out = []
    for t, s in zip(path[:-1], path[1:]):
        gs, gt = float(g[s]), float(g[t])
        sig = lambda v: 1.0 / (1.0 + math.exp(-v))
        softplus = lambda v: max(v, 0.0) + math.log1p(math.exp(-abs(v)))
        a_s, a_t = math.sqrt(sig(-gs)), math.sqrt(sig(-gt))
        s_s, s_t = math.sqrt(sig(gs)), math.sqrt(sig(gt))
        s2_ts = -math.expm1(softplus(gs) - softplus(gt))
        st = eta * math.sqrt(s2_ts) * s_s / s_t
        rest = s_s * s_s - st * st
        out.append((a_s / a_t, a_s * s_t / a_t - math.sqrt(max(rest, 0.0)), st, rest, a_t, s2_ts, s_t, s_s))
    return out


@pytest.mark.parametrize("T", [50, 1000])
def test_linear_rows_match_an_independent_fp64_evaluation(T):
    for name, gamma in schedules(T):
        g = schedule_tables(gamma, T)["gamma"]
        for path in (paths.uniform_path(T, min(T, 20)), paths.quadratic_path(T, min(T, 33)), paths.uniform_path(T, T), [T, 0]):
            for eta in (0.0, 0.5, 1.0):
                lin = paths.linear_coefficients(g[path[1:]], g[path[:-1]], eta)
                ref = fp64_rows(g, path, eta)
                for k, r in enumerate(ref):
                    for j in range(3):
                        assert abs(float(lin[k, j]) - r[j]) <= 1e-12 * max(1.0, abs(r[j])), (name, eta, k, j)
                    assert r[3] >= -1e-15, (name, eta, k, r[3])                    # sigma_s^2 - sigma~^2 >= 0
                    assert float(lin[k, 3]) >= -1e-15
                if eta < 1.0:
                    pt = paths.path_tables(g, path, eta)
                    assert pt["form"] == 1 and pt["coef_inpaint"] is None
                    assert torch.equal(pt["coef"][:, :3], lin[:, :3].to(torch.float32)) and bool((pt["coef"][:, 3] == 0).all())
                    if eta == 0.0:
                        assert bool((pt["coef"][:, 2] == 0).all())                 # the kernel's "no normals" switch


def test_linear_row_at_eta_1_is_the_ancestral_update():
    """a = 1 / alpha_t|s, b = sigma2_t|s / alpha_t|s / sigma_t, c = sigma_t|s sigma_s / sigma_t - to fp64 round-off."""
    T = 1000
    for name, gamma in schedules(T):
        g = schedule_tables(gamma, T)["gamma"]
        for path in (paths.uniform_path(T, 50), paths.uniform_path(T, T)):
            for a, b, c, _, a_t, s2_ts, s_t, s_s in fp64_rows(g, path, 1.0):
                a_ts = 1.0 / a                      # alpha_t / alpha_s
                assert abs(b - s2_ts / a_ts / s_t) <= 1e-9 * max(1.0, abs(b)), name
                assert abs(c - math.sqrt(s2_ts) * s_s / s_t) <= 1e-12, name


# ----------------------------------------------------------------------------- 4. DDIM consistency

def test_eta_0_with_a_fixed_eps_composes_over_intermediate_points():
    """With eps held fixed, t -> s in one noise-free transition equals t -> m -> s."""
    T = 1000
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(64, generator=gen, dtype=torch.float64)
    eps = torch.randn(64, generator=gen, dtype=torch.float64)
    for name, gamma in schedules(T):
        g = schedule_tables(gamma, T)["gamma"]
        for t, m, s in ((1000, 500, 0), (900, 899, 10), (400, 37, 36), (1000, 1, 0)):
            step = lambda a, b_, zz: (lambda r: r[0, 0] * zz - r[0, 1] * eps)(paths.linear_coefficients(g[b_:b_ + 1], g[a:a + 1], 0.0))
            one = step(t, s, z)
            two = step(m, s, step(t, m, z))
            assert float((one - two).abs().max()) <= 1e-11 * max(1.0, float(one.abs().max())), (name, t, m, s)


# ----------------------------------------------------------------------------- 5. C ABI

NEW_SYMBOLS = ["hd_set_path", "hd_sample_path", "hd_sample_path_inpaint", "hd_path_graph_builds"]


def test_path_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays
    assert "FINE-GRID index of the arrival step" in hdr        # the path draw layout, next to the existing one at hd_noise


def test_path_entry_points_reject_bad_arguments_without_a_gpu(lib):
    ti, si, coef = (C.c_int * 2)(4, 2), (C.c_int * 2)(2, 0), (C.c_float * 8)()
    assert lib.hd_set_path(None, 2, ti, si, coef, 0, None) == -1 and b"hd_set_path" in lib.hd_last_error()
    assert lib.hd_set_path(None, 2, ti, si, coef, 1, coef) == -1 and b"ancestral rows only" in lib.hd_last_error()
    assert lib.hd_set_path(None, 2, ti, si, coef, 2, None) == -1 and b"form" in lib.hd_last_error()
    assert lib.hd_sample_path(None, None, None, None, -1, 0, 1, None, None, 1, 0, 0, 0, None) == -1
    assert b"hd_sample_path: null" in lib.hd_last_error()
    assert lib.hd_sample_path(None, None, None, None, -1, 2, 1, None, None, 1, 0, 0, 0, None) == -1
    assert b"k_lo <= k_hi" in lib.hd_last_error()
    assert lib.hd_sample_path_inpaint(None, None, None, None, -1, 0, 1, None, None, 1, 0, 0, 0, None, None, 1, None) == -1
    assert b"hd_sample_path_inpaint: null" in lib.hd_last_error()
    assert lib.hd_sample_path_inpaint(None, None, None, None, -1, 3, 1, None, None, 1, 0, 0, 0, None, None, 1, None) == -1
    assert b"k_lo <= k_hi" in lib.hd_last_error()
    assert lib.hd_path_graph_builds(None) == -1
    # (HD_E_STATE for an unset schedule / path needs a handle, i.e. a device: tests/test_gpu_fewstep.py)


# ----------------------------------------------------------------------------- 6. Python and CLI argument errors

def test_python_entry_points_raise_on_bad_arguments_before_touching_the_gpu(monkeypatch):
    m, _ = cpu_model(T=6, L=1)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    fm = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool).view(B, N, 1)
    xk, hk = torch.zeros(B, N, 3), torch.zeros(B, N, 8)
    known = [{"x": torch.zeros(1, 3), "h": torch.zeros(1, 8)}]
    calls = [lambda **kw: m.sample_from_masks(nm, None, **kw), lambda **kw: m.sample(2, "cpu", **kw),
             lambda **kw: m.sample_batches(2, 2, "cpu", **kw), lambda **kw: m.sample_inpaint(nm, fm, xk, hk, **kw),
             lambda **kw: m.sample_grow(known, [3], "cpu", **kw), lambda **kw: m.path_steps(torch.zeros(B, N, 11), nm, **kw)]
    for call in calls:
        for bad in (0, 7, -3, 2.5):
            with pytest.raises(ValueError, match="steps"):
                call(steps=bad)
        for bad in (-0.1, 1.5, float("nan"), "x"):
            with pytest.raises(ValueError, match="eta"):
                call(steps=3, eta=bad)
        with pytest.raises(ValueError, match="not both"):
            call(steps=3, timesteps=[6, 3, 0])
        with pytest.raises(ValueError, match="timesteps"):
            call(timesteps=[6, 3, 4, 0])
        with pytest.raises(ValueError, match="spacing"):
            call(steps=3, spacing="log")
    for call in calls[3:5]:
        with pytest.raises(ValueError, match="ancestral"):
            call(steps=3, eta=0.0)
    # the attributes are the keywords' defaults
    m.sample_steps = 9
    with pytest.raises(ValueError, match="steps"):
        m.sample_from_masks(nm, None)
    m.sample_steps, m.sample_eta = None, 2.0
    with pytest.raises(ValueError, match="eta"):
        m.sample_from_masks(nm, None)
    m.sample_eta = 1.0
    # the step-by-step modes say so instead of walking the full chain
    m.dynamics.mode = "gnn_dynamics"
    with pytest.raises(NotImplementedError, match="gnn_dynamics"):
        m.sample_from_masks(nm, None, steps=3)
    m.dynamics.mode = "egnn_dynamics"
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="torch"):
        m.sample_from_masks(nm, None, steps=3)


def test_defaults_resolve_to_the_plain_loop():
    m, _ = cpu_model(T=6, L=1)
    assert m._resolve_path() is None and m._resolve_path(steps=6, eta=1.0) is None            # the plain loop, untouched
    assert m._resolve_path(timesteps=[6, 5, 4, 3, 2, 1, 0]) is None
    assert m._resolve_path(steps=3) == ([6, 4, 2, 0], 1.0)
    assert m._resolve_path(eta=0.0) == ([6, 5, 4, 3, 2, 1, 0], 0.0)
    assert m._resolve_path(steps=2, eta=0.5, spacing="quadratic") == (paths.quadratic_path(6, 2), 0.5)
    m._force_path_loop = True
    assert m._resolve_path() == ([6, 5, 4, 3, 2, 1, 0], 1.0)
    m._force_path_loop = False
    m.sample_steps, m.sample_eta = 2, 0.25
    assert m._resolve_path() == ([6, 3, 0], 0.25)
    assert m._resolve_path(steps=3, eta=1.0) == ([6, 4, 2, 0], 1.0)


def test_cli_flags():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--steps", "100", "--eta", "0", "--spacing", "quadratic"])
    assert (a.steps, a.eta, a.spacing) == (100, 0.0, "quadratic")
    a = sampler.parse_args([])
    assert (a.steps, a.eta, a.spacing) == (None, 1.0, "uniform")
    a = sampler.parse_args(["--steps", "50", "--known", "k.pkl", "--grow", "2"])
    assert a.steps == 50 and a.known == "k.pkl"
    for bad in (["--steps", "0"], ["--eta", "1.5"], ["--eta", "-1"], ["--spacing", "log"],
                ["--steps", "5", "--eta", "0.5", "--known", "k.pkl", "--grow", "2"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
