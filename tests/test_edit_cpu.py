"""CPU tier of editing given molecules (hierdiff_amd/paths.py: partial / ascending paths and inversion rows; hd_diffuse /
hd_set_path_up / hd_slerp; DiffusionQM9.diffuse / encode / sample_from_latent / slerp / vary / interpolate): the host arithmetic, the
restatement tests/edit_reference.py that tests/test_gpu_edit.py holds the HIP path against, the new C-ABI symbols and their argument
checks, and the Python / CLI argument errors - all without a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.noise_model import schedule_tables
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests.helpers import fixture_model, load, rel_l2
from tests.test_inpaint_cpu import cpu_model, gamma_grid_fp64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


# ----------------------------------------------------------------------------- 1. partial and ascending paths

@pytest.mark.parametrize("T", [1, 7, 50, 1000])
def test_partial_paths_decrease_strictly_from_start_to_0(T):
    starts = sorted({1, 2, T // 3, T // 2, T - 1, T} & set(range(1, T + 1)))
    for start in starts:
        ks = range(1, start + 1) if start <= 50 else (1, 2, 7, start // 2, start - 1, start)
        for K in ks:
            for spacing in paths.SPACINGS:
                p = paths.partial_path(T, start, K, spacing)
                assert len(p) == K + 1 and p[0] == start and p[-1] == 0, (T, start, K, spacing)
                assert all(isinstance(v, int) for v in p) and all(a > b for a, b in zip(p[:-1], p[1:])), (T, start, K, spacing)
                assert paths.ascending_path(T, start, K, spacing) == p[::-1]
        assert paths.partial_path(T, start) == list(range(start, -1, -1))
    for K in (1, max(1, T // 3), T):
        for spacing in paths.SPACINGS:
            assert paths.partial_path(T, T, K, spacing) == paths.build_path(T, K, spacing)
    assert paths.partial_path(T, T) == paths.build_path(T)


def test_partial_path_arguments_are_validated():
    assert paths.partial_path(20, 12, timesteps=[12, 7, 3, 0]) == [12, 7, 3, 0]
    assert paths.ascending_path(20, 12, timesteps=[12, 7, 3, 0]) == [0, 3, 7, 12]
    for bad in (0, 21, -1, 2.0, True, "5"):
        with pytest.raises(ValueError, match="start"):
            paths.partial_path(20, bad)
        with pytest.raises(ValueError, match="end"):
            paths.ascending_path(20, bad)
    for bad in (0, 13, -1, 2.5):
        with pytest.raises(ValueError, match="steps"):
            paths.partial_path(20, 12, bad)
    with pytest.raises(ValueError, match="timesteps"):
        paths.partial_path(20, 12, timesteps=[20, 5, 0])                 # must start at `start`
    with pytest.raises(ValueError, match="timesteps"):
        paths.partial_path(20, 12, timesteps=[12, 5, 5, 0])
    with pytest.raises(ValueError, match="not both"):
        paths.partial_path(20, 12, 3, timesteps=[12, 0])
    with pytest.raises(ValueError, match="spacing"):
        paths.partial_path(20, 12, 3, "log")
    g = torch.linspace(-5, 5, 21)
    for bad in ([0], [0, 3, 3], [3, 0], [0, 21], [-1, 4]):
        with pytest.raises(ValueError):
            paths.up_tables(g, bad)


# ----------------------------------------------------------------------------- 2. inversion rows

def grids(T):
    from hierdiff_amd.noise_model import PredefinedNoiseSchedule
    m, _ = cpu_model(T=T, L=1)
    return [("learned", m.gamma), ("cosine", PredefinedNoiseSchedule("cosine", T, 1e-4)),
            ("polynomial_2", PredefinedNoiseSchedule("polynomial_2", T, 1e-5))]


@pytest.mark.parametrize("T", [50, 1000])
def test_inversion_rows_match_an_independent_fp64_evaluation_and_undo_the_down_rows(T):
    """Rows to 1e-12 relative against Python floats; up row then eta = 0 down row under the same eps is the identity on z to 1e-12.
    The composition computes a' (a z - b e) - b' e with a' = alpha_u / alpha_v, so its float64 rounding error is about
    2^-52 a' |z_v|: 1e-12 is reachable while a' stays below a few thousand, which holds on every multi-step path here (largest:
    1.6e3, the last of 20 uniform steps of the cosine grid at T = 1000, measured 5.2e-13).  The single jump 0 -> T is therefore not
    among the paths: on that grid a' = 2.0e4 and the same arithmetic measures 8.6e-12."""
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(64, generator=gen, dtype=torch.float64)
    eps = torch.randn(64, generator=gen, dtype=torch.float64)
    for name, gamma in grids(T):
        g = schedule_tables(gamma, T)["gamma"]
        for up in (paths.ascending_path(T, T, min(T, 20)), paths.ascending_path(T, T // 2, 7, "quadratic"), paths.ascending_path(T, T),
                   [0, T // 4, T // 2]):
            u, v = torch.tensor(up[:-1]), torch.tensor(up[1:])
            ab = paths.inversion_coefficients(g[u], g[v])
            assert ab.dtype == torch.float64 and tuple(ab.shape) == (len(up) - 1, 2)
            down = paths.linear_coefficients(g[u], g[v], 0.0)              # the eta = 0 rows v -> u
            for k in range(len(up) - 1):
                a, b = er.up_row(float(g[up[k]]), float(g[up[k + 1]]))
                assert abs(float(ab[k, 0]) - a) <= 1e-12 * max(1.0, abs(a)), (name, k)
                assert abs(float(ab[k, 1]) - b) <= 1e-12 * max(1.0, abs(b)), (name, k)
                zv = ab[k, 0] * z - ab[k, 1] * eps
                back = down[k, 0] * zv - down[k, 1] * eps
                assert float((back - z).abs().max()) <= 1e-12 * max(1.0, float(zv.abs().max()), float(z.abs().max())), (name, k)
            ut = paths.up_tables(g, up)
            assert ut["K"] == len(up) - 1 and ut["from_idx"].tolist() == up[:-1] and ut["to_idx"].tolist() == up[1:]
            assert torch.equal(ut["coef"][:, :2], ab.to(torch.float32)) and bool((ut["coef"][:, 2:] == 0).all())


# ----------------------------------------------------------------------------- 3. round trip under a fixed eps

@pytest.mark.parametrize("T,K", [(20, 20), (20, 7), (1000, 50)])
def test_encode_then_eta_0_decode_returns_the_start_under_a_fixed_eps(T, K):
    """With the network replaced by a fixed eps, `encode_ref` then the eta = 0 `partial_chain_ref` on the same points is the identity
    up to the fp32 rounding of the state (the rows are float64).

    Bound.  With e fixed, z_j / alpha_j = z_0 / alpha_0 + (sigma_j / alpha_j - sigma_0 / alpha_0) e at every visited level j, so
    |z_j| alpha_0 / alpha_j <= |z_0| + (sigma_j / alpha_j) |e|.  A perturbation d of the state at level j travels up and back down
    to level j unchanged (the down row undoes the up row) and reaches level 0 multiplied by alpha_0 / alpha_j.  Each of the 2 K
    transitions perturbs the state twice by at most 2^-24 max|z_j|: the rounding of the new state to fp32, and the removal of the x
    mean, which for a mean-free state is the mean of earlier rounding errors.  Hence, in the max norm,
        |z_0' - z_0| <= 4 K 2^-24 (max|z_0| + max_j exp(gamma_j / 2) max|e|),   sigma_j / alpha_j = exp(gamma_j / 2)."""
    m, _ = cpu_model(T=T, L=1)
    gg = gamma_grid_fp64(m, T)
    x, h, nm, _, _ = er.molecules(er.MAIN["n_list"])
    xh = er.normalised_data(x, h, nm)
    B, N = nm.shape[:2]
    r = er.raw_draws(1, B, N, seed=8)[0]
    eps = orc.combined_noise(r[0], r[1], nm.float())
    net = er.FixedEps(eps, nm)
    down = paths.build_path(T, K)
    z_top = er.encode_ref(net, gg, down[::-1], xh, nm)
    z_back = er.partial_chain_ref(net, gg, down, 0.0, z_top, nm, [None] * K, decode=False)
    z0 = torch.sqrt(torch.sigmoid(-gg[0])) * xh
    bound = 4 * K * 2.0 ** -24 * (float(z0.abs().max()) + math.exp(float(gg.max()) / 2) * float(eps.abs().max()))
    err = float((z_back - z0).abs().max())
    print(f"round trip T={T} K={K}: max |z_0' - z_0| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert torch.all(z_top[~nm.expand_as(z_top)] == 0) and torch.isfinite(z_top).all()
    assert not torch.equal(z_top, z0)


# ----------------------------------------------------------------------------- 4. the partial chain against the oracle

def test_partial_chain_ref_from_T_on_the_identity_path_is_the_oracle_chain():
    fx = load("f5_chain_h32_l2")
    sd_np, sd, cfg = fixture_model(fx)
    T, n_list = 10, [6, 3, 5, 1]
    m, _ = cpu_model(H=32, L=int(fx["n_layers"]), T=T, seed=int(fx["weight_seed"]))
    gg = gamma_grid_fp64(m, T)
    nm, em = orc.canonical_masks(n_list)
    B, N = nm.shape[:2]
    raws = er.raw_draws(T + 2, B, N, seed=3)
    xo, ho = orc.sample_chain(sd, cfg, T, nm, em, None, raws, gamma_grid=gg)
    zT = orc.combined_noise(raws[0][0], raws[0][1], nm)
    net = er.RefNet(sd_np, cfg, T, nm, em)
    x, h, _ = er.partial_chain_ref(net, gg, paths.partial_path(T, T), 1.0, zT, nm, raws[1:])
    assert torch.equal(x, xo) and torch.equal(h, ho)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()


# ----------------------------------------------------------------------------- 5. slerp

def test_slerp_ref_endpoints_norm_and_degenerate_cases():
    x, h, nm, _, _ = er.molecules(er.WRAP["n_list"], seed=2)
    g = torch.Generator().manual_seed(4)
    B, N = nm.shape[:2]
    a = (torch.randn(B, N, 11, generator=g) * nm).numpy()
    b = (torch.randn(B, N, 11, generator=g) * nm).numpy()
    lam = [0.0, 0.25, 0.5, 0.9, 1.0]
    out = er.slerp_ref(a, b, lam, nm)
    assert out.shape == (5, B, N, 11)
    assert np.array_equal(out[0], a.astype(np.float64)) and np.array_equal(out[-1], b.astype(np.float64))
    assert np.all(out[:, ~nm.numpy().reshape(B, N)] == 0)
    # |a| = |b|: the norm is preserved
    nrm = lambda v: np.sqrt((v.astype(np.float64) ** 2).sum(axis=(-2, -1)))
    b_same = b * (nrm(a) / nrm(b))[:, None, None]
    o2 = er.slerp_ref(a, b_same, lam, nm)
    assert np.allclose(nrm(o2), nrm(a)[None, :], rtol=1e-12, atol=0)
    # a == b: every frame is a (theta = 0: the linear form)
    o3 = er.slerp_ref(a, a, lam, nm)
    assert all(np.allclose(o3[l], a, rtol=1e-15, atol=0) for l in range(5))
    # nearly parallel: the fallback is continuous with the spherical form
    b_near = a * (1 + 1e-9)
    o4 = er.slerp_ref(a, b_near, [0.5], nm)
    assert np.allclose(o4[0], 0.5 * (a.astype(np.float64) + b_near), rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- 6. C ABI

NEW_SYMBOLS = ["hd_diffuse", "hd_set_path_up", "hd_slerp"]


def test_edit_symbols_exported_and_declared(lib):
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
    assert "draw 0 re-purposed and draws 1 .. T - t_start unused" in hdr      # the editing draw layout, next to the others at hd_noise


def test_edit_entry_points_reject_bad_arguments_without_a_gpu(lib):
    assert lib.hd_diffuse(None, None, None, 1.0, 0.5, None, None, 1, 0, 0, 0, 0, None, None) == -1
    assert b"hd_diffuse: null" in lib.hd_last_error()
    assert lib.hd_slerp(None, None, None, None, None, 1, None, None) == -1 and b"hd_slerp: null" in lib.hd_last_error()
    u, v, coef = (C.c_int * 2)(0, 2), (C.c_int * 2)(2, 4), (C.c_float * 8)(1.0, 0.1, 0.0, 0.0, 1.0, 0.1, 0.0, 0.0)
    assert lib.hd_set_path_up(None, 2, u, v, coef) == -1 and b"hd_set_path_up: null handle" in lib.hd_last_error()
    assert lib.hd_set_path_up(None, 0, u, v, coef) == -1 and b"hd_set_path_up: bad argument" in lib.hd_last_error()
    assert lib.hd_set_path_up(None, 2, None, v, coef) == -1
    noisy = (C.c_float * 8)(1.0, 0.1, 0.0, 0.0, 1.0, 0.1, 0.3, 0.0)
    assert lib.hd_set_path_up(None, 2, u, v, noisy) == -1 and b"draws nothing" in lib.hd_last_error()
    assert lib.hd_set_path_up(None, 2, v, u, coef) == -1 and b"from_idx[k] < to_idx[k]" in lib.hd_last_error()      # descending
    gap = (C.c_int * 2)(0, 3)
    assert lib.hd_set_path_up(None, 2, gap, v, coef) == -1 and b"start where" in lib.hd_last_error()
    # hd_set_path keeps refusing what it refused (the ascending pair is reported once a handle exists: tests/test_gpu_edit.py)
    assert lib.hd_set_path(None, 2, u, v, coef, 1, None) == -1
    # (HD_E_INVALID of hd_diffuse / hd_slerp for noise_rows, unpaired raw tensors, L < 1 and aliasing needs a topology, i.e. a
    # device: tests/test_gpu_edit.py)


# ----------------------------------------------------------------------------- 7. Python and CLI argument errors

def test_python_entry_points_raise_on_bad_arguments_before_touching_the_gpu(monkeypatch):
    m, _ = cpu_model(T=6, L=1)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    x, h, z = torch.zeros(B, N, 3), torch.zeros(B, N, 8), torch.zeros(B, N, 11)
    mol3 = {"x": torch.randn(3, 3), "h": torch.randn(3, 8)}
    mol2 = {"x": torch.randn(2, 3), "h": torch.randn(2, 8)}
    for bad in (-1, 7, 2.5, True):
        with pytest.raises(ValueError, match="t must be"):
            m.diffuse(x, h, nm, bad)
    for bad in (0, 7, -2, 1.5):
        with pytest.raises(ValueError, match="t_start"):
            m.sample_from_latent(z, nm, t_start=bad)
        with pytest.raises(ValueError, match="t_start"):
            m.vary([mol3], "cpu", bad)
        with pytest.raises(ValueError, match="t_end"):
            m.encode(x, h, nm, t_end=bad)
        with pytest.raises(ValueError, match="t_end"):
            m.interpolate(mol3, mol3, 3, "cpu", t_end=bad)
    with pytest.raises(ValueError, match="steps"):
        m.sample_from_latent(z, nm, t_start=4, steps=5)                  # more transitions than steps below the start
    with pytest.raises(ValueError, match="steps"):
        m.encode(x, h, nm, t_end=3, steps=4)
    with pytest.raises(ValueError, match="eta"):
        m.sample_from_latent(z, nm, t_start=4, eta=1.5)
    with pytest.raises(ValueError, match="spacing"):
        m.sample_from_latent(z, nm, t_start=4, steps=2, spacing="log")
    with pytest.raises(ValueError, match="timesteps"):
        m.sample_from_latent(z, nm, t_start=4, timesteps=[6, 2, 0])
    with pytest.raises(ValueError, match="k_lo"):
        m.latent_steps(z, nm, t_start=4, k_lo=3, k_hi=2)
    with pytest.raises(ValueError, match="x must be"):
        m.diffuse(x[:, :3], h, nm, 3)
    with pytest.raises(ValueError, match="z must be"):
        m.sample_from_latent(z[:, :, :10], nm)
    with pytest.raises(ValueError, match="raw_noise"):
        m.diffuse(x, h, nm, 3, raw_noise=(torch.zeros(1, N, 3), torch.zeros(1, N, 8)))
    with pytest.raises(ValueError, match="raw_noises"):
        m.sample_from_latent(z, nm, t_start=4, steps=2, raw_noises=[(torch.zeros(B, N, 3), torch.zeros(B, N, 8))] * 2)
    with pytest.raises(ValueError, match="sample_id_base"):
        m.diffuse(x, h, nm, 3, sample_id_base=-1)
    with pytest.raises(ValueError, match="equal node counts"):
        m.interpolate(mol3, mol2, 3, "cpu")
    for bad in (1, 0, 2.0, True):
        with pytest.raises(ValueError, match="frames"):
            m.interpolate(mol3, mol3, bad, "cpu")
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n_variants"):
            m.vary([mol3], "cpu", 3, n_variants=bad)
    with pytest.raises(ValueError, match="no samples"):
        m.vary([], "cpu", 3)
    with pytest.raises(ValueError, match="unsupported keyword"):
        m.vary([mol3], "cpu", 3, resamplings=2)
    with pytest.raises(ValueError, match="lambdas"):
        m.slerp(z, z, [], nm)
    with pytest.raises(ValueError, match="z_b must be"):
        m.slerp(z, z[:1], [0.5], nm)
    calls = [lambda: m.diffuse(x, h, nm, 3), lambda: m.encode(x, h, nm), lambda: m.sample_from_latent(z, nm),
             lambda: m.vary([mol3], "cpu", 3), lambda: m.interpolate(mol3, mol3, 3, "cpu")]
    m.pocket = True
    for call in calls + [lambda: m.slerp(z, z, [0.5], nm)]:
        with pytest.raises(ValueError, match="pocket"):
            call()
    m.pocket = False
    m.dynamics.mode = "gnn_dynamics"
    for call in calls:
        with pytest.raises(NotImplementedError, match="gnn_dynamics"):
            call()
    m.dynamics.mode = "egnn_dynamics"
    m.noise_mode = "torch"
    for call in (calls[0], calls[2], calls[3], calls[4]):
        with pytest.raises(NotImplementedError, match="torch"):
            call()
    m.noise_mode = "philox"
    for call in calls + [lambda: m.slerp(z, z, [0.5], nm)]:             # valid input on the CPU: the library's loud error, no fallback
        with pytest.raises(_lib.HierDiffHipError, match="no CPU fallback"):
            call()


def test_cli_flags():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--vary", "s.pkl", "--t-start", "500", "--variants", "3", "--steps", "100", "--eta", "0.5"])
    assert (a.vary, a.t_start, a.variants, a.steps, a.eta) == ("s.pkl", 500, 3, 100, 0.5)
    a = sampler.parse_args(["--interpolate", "s.pkl", "--frames", "5", "--steps", "50", "--spacing", "quadratic"])
    assert (a.interpolate, a.frames, a.steps, a.spacing) == ("s.pkl", 5, 50, "quadratic")
    a = sampler.parse_args([])
    assert (a.vary, a.t_start, a.variants, a.interpolate, a.frames) == (None, None, 1, None, None)
    for bad in (["--vary", "s.pkl"], ["--t-start", "5"], ["--vary", "s.pkl", "--t-start", "0"], ["--variants", "2"],
                ["--vary", "s.pkl", "--t-start", "5", "--variants", "0"], ["--interpolate", "s.pkl"], ["--frames", "3"],
                ["--interpolate", "s.pkl", "--frames", "1"], ["--interpolate", "s.pkl", "--frames", "3", "--eta", "0.5"],
                ["--vary", "s.pkl", "--t-start", "5", "--interpolate", "s.pkl", "--frames", "3"],
                ["--vary", "s.pkl", "--t-start", "5", "--score", "s.pkl"], ["--vary", "s.pkl", "--t-start", "5", "--known", "k.pkl", "--grow", "1"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)


# ----------------------------------------------------------------------------- 8. the parity bar is passable in fp32

def _restatements(case, C_, dtype):
    """Every quantity tests/test_gpu_edit.py compares at the 1e-4 bar, from the restatement in `dtype`."""
    T, H, L, n_list = case["T"], case["H"], case["L"], case["n_list"]
    sd_np, cfg = er.weights(H, L, C_)
    gg = gamma_grid_fp64(er.cpu_diffusion(sd_np, H, L, T, C_), T)
    x, h, nm, em, ctx = er.molecules(n_list, C_=C_)
    B, N = nm.shape[:2]
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx, dtype=dtype)
    xh = er.normalised_data(x, h, nm, dtype)
    out = {}
    t_mid = min(12, T)
    out["diffuse"] = er.diffuse_ref(x, h, nm, gg[t_mid], er.raw_draws(1, B, N, seed=11)[0], dtype)
    for eta in (1.0, 0.0):
        path = paths.partial_path(T, t_mid, 5)
        xs, hs, _ = er.partial_chain_ref(net, gg, path, eta, out["diffuse"], nm, er.raw_draws(6, B, N, seed=12))
        out[f"latent eta={eta} x"], out[f"latent eta={eta} h"] = xs * nm, hs
    for K in case.get("encode_K", (T, 7)):
        up = paths.ascending_path(T, T, K)
        out[f"encode K={K}"] = er.encode_ref(net, gg, up, xh, nm)
        if K == 7:          # the round trip is compared at (T = 20, K = 7) only, see the test's docstring
            xs, hs, _ = er.partial_chain_ref(net, gg, up[::-1], 0.0, out[f"encode K={K}"], nm, er.raw_draws(K + 1, B, N, seed=13))
            out[f"round trip K={K} x"], out[f"round trip K={K} h"] = xs * nm, hs
    return out


@pytest.mark.parametrize("name,case,C_", [("main", er.MAIN, 0), ("main+context", er.MAIN, 1), ("wrap", er.WRAP, 0),
                                          ("T1000", dict(T=1000, H=32, L=2, n_list=er.MAIN["n_list"], encode_K=(50,)), 0)])
def test_fp32_restatement_stays_a_tenth_of_the_bar_from_the_fp64_one(name, case, C_):
    """The cases of tests/test_gpu_edit.py: the float32 restatement against the float64 one below 1e-5 rel-L2, a tenth of the 1e-4
    parity bar, so that bar is passable by correct fp32 arithmetic.

    The round trip (encode, then the eta = 0 chain back) is held to the bar at (T = 20, K = 7) only.  At (T = 1000, K = 50) the two
    restatements themselves differ by 9.1e-3 on x: the way down from z_T multiplies a perturbation of the latent by alpha_0 / alpha_T
    and the network is evaluated on the perturbed states, so fp32 rounding alone moves the result by more than the bar (the known
    ill-conditioning of DDIM inversion over many steps).  That case was shortened as the bar is not to be widened; `encode` itself is
    compared at (T = 1000, K = 50), where the restatements agree to 7.9e-8."""
    f32 = _restatements(case, C_, torch.float32)
    f64 = _restatements(case, C_, torch.float64)
    for key in f32:
        r = rel_l2(f32[key].double().numpy(), f64[key].double().numpy())
        print(f"{name}: {key}: fp32 vs fp64 restatement rel_l2 {r:.2e}")
        assert f64[key].dtype == torch.float64 and r < 1e-5, (name, key, r)
