"""CPU tier of restraint-guided sampling: the float64 restatement of tests/restraint_reference.py against float64 autograd of the same
energy (the independent derivation), the descent property of the projected step, `lambda_rows` against an independent evaluation
from the gamma grid, the restrained chain through `RestrainedNet` over the oracle, the C ABI (symbols, argument errors without a
device) and every refusal of the Python entry points and the CLI (raised before a device is looked at)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths, restraints
from hierdiff_amd.restraints import Restraints
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import restraint_reference as rr
from tests import solver_reference as sr
from tests.helpers import rel_l2
from tests.test_inpaint_cpu import gamma_grid_fp64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ----------------------------------------------------------------------------- the energy and its gradient

def autograd_grad(rs, x, nm):
    with torch.enable_grad():
        xv = x.clone().double().requires_grad_(True)
        U = restraints.energy_terms(rs, xv, nm.reshape(nm.shape[0], -1, 1))
        U.sum().backward()
    return U.detach().numpy(), xv.grad.numpy()


def test_hand_derived_gradient_equals_float64_autograd():
    rs, x, nm = rr.seven_node_case()
    U, _, g, ga = rr.energy_grad(rs, x.numpy(), nm.numpy())
    Ua, gauto = autograd_grad(rs, x, nm)
    assert (U > 0).all(), U                                  # all three kinds of term are active in the case
    err_u, err_g = np.abs(U - Ua).max(), np.abs(g - gauto).max()
    print(f"7-node case: U {U[0]}, |U - autograd| {err_u:.2e}, |g - autograd| {err_g:.2e}")
    assert err_u <= 1e-13 * np.abs(U).max()
    assert (np.abs(g - gauto) <= 1e-13 * np.maximum(ga, 1.0)).all()
    assert (ga >= np.abs(g) - 1e-15).all()


@pytest.mark.parametrize("per_molecule", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("P,Q,A", [(0, 0, 0), (1, 0, 2), (7, 3, 0), (70, 3, 2)])
def test_gradient_on_random_tables_with_masks_and_padding(P, Q, A, per_molecule):
    B, N = 3, 9
    rs, centre = rr.random_tables(B, N, P, Q, A, seed=P + 10 * Q + 100 * A, per_molecule=per_molecule)
    g_ = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, 3, generator=g_, dtype=torch.float64) * 1.5
    nm = torch.ones(B, N, dtype=torch.bool)
    nm[1, 5:] = False
    nm[2, 1:] = False
    if centre is not None:
        x[0, 2] = torch.from_numpy(centre)                   # a node exactly on an obstacle's centre: energy, no gradient
    U, _, g, ga = rr.energy_grad(rs, x.numpy(), nm.numpy())
    Ua, gauto = autograd_grad(rs, x, nm)
    assert np.allclose(U, Ua, rtol=1e-13, atol=1e-13)
    assert (np.abs(g - gauto) <= 1e-13 * np.maximum(ga, 1.0)).all()
    assert (g[~nm.numpy()] == 0).all()
    assert np.isfinite(g).all()


def test_projected_step_is_a_descent_direction():
    """x - h * project(g): U falls for data-space steps from 1e-3 to 0.2 on the fixed case, and the centre of mass stays."""
    rs, x, nm = rr.seven_node_case()
    U0, _, g, ga = rr.energy_grad(rs, x.numpy(), nm.numpy())
    d, _ = rr.project_step(g, ga, nm.numpy(), np.ones(1), math.inf)
    assert np.abs(d.sum(1)).max() < 1e-12
    unit = d / np.sqrt((d * d).sum())
    for h in (1e-3, 1e-2, 0.05, 0.1, 0.2):
        U1 = rr.energy_grad(rs, x.numpy() - h * unit, nm.numpy())[0]
        print(f"step {h}: U {U0.sum():.6f} -> {U1.sum():.6f}")
        assert U1.sum() < U0.sum()
    # the clip bounds every node's step and keeps the direction
    dc, _ = rr.project_step(g, ga, nm.numpy(), np.ones(1), 0.25)
    raw = g.copy()
    ln = np.sqrt((raw * raw).sum(-1, keepdims=True))
    clipped = np.where(ln > 0.25, raw * 0.25 / np.maximum(ln, 1e-300), raw)
    assert np.allclose(dc, clipped - clipped.mean(1, keepdims=True), atol=1e-15)
    assert (ln > 0.25).any() and (ln < 0.25).any()


def test_update_leaves_features_masked_rows_and_single_nodes():
    B, N, D = 3, 5, 11
    rs, _ = rr.random_tables(B, N, 7, 3, 2, seed=4, per_molecule=True)
    g_ = torch.Generator().manual_seed(8)
    nm = torch.ones(B, N, dtype=torch.bool)
    nm[1, 3:] = False
    nm[2, 1:] = False
    z = torch.randn(B, N, D, generator=g_) * nm[:, :, None]
    eps = torch.randn(B, N, D, generator=g_) * nm[:, :, None]
    row = (0.8, 0.6, 0.75, math.inf)
    out, mag = rr.restrain_ref(rs, z, eps, nm, torch.tensor([1.0, 0.5, 2.0]), row, 1.0)
    e = eps.double().numpy()
    assert (out[:, :, 3:] == e[:, :, 3:]).all() and (out[~nm.numpy()] == e[~nm.numpy()]).all()
    assert (out[2] == e[2]).all()                            # one valid node: the projection removes its whole step
    assert not (out[0, :, :3] == e[0, :, :3]).all()
    assert np.abs((out - e)[:, :, :3].sum(1)).max() < 1e-12  # mean-free
    zero, _ = rr.restrain_ref(rs, z, eps, nm, torch.tensor([0.0, 0.0, 0.0]), row, 1.0)
    assert (zero == e).all()
    lam0, _ = rr.restrain_ref(rs, z, eps, nm, torch.ones(1), (0.8, 0.6, 0.0, math.inf), 1.0)
    assert (lam0 == e).all()
    assert (mag >= np.abs(out) - 1e-12).all()


def test_x0_is_the_x0_frame_arithmetic():
    """`x0_f32` is (1 / alpha) * (z - sigma * eps) * nv0 in fp32, operation by operation (numpy float32 scalars as the witness)."""
    g_ = torch.Generator().manual_seed(1)
    z, eps = torch.randn(2, 4, 5, generator=g_), torch.randn(2, 4, 5, generator=g_)
    al, sg, nv0 = np.float32(0.83), np.float32(0.55), np.float32(1.7)
    got = rr.x0_f32(z, eps, al, sg, nv0).numpy()
    ra = np.float32(1.0) / al
    want = (ra * (z[:, :, :3].numpy() - sg * eps[:, :, :3].numpy())) * nv0
    assert want.dtype == np.float32 and (got == want).all()


# ----------------------------------------------------------------------------- the rows

@pytest.mark.parametrize("schedule", ["score", "sigma", [0.5, 0.25, 0.0, 2.0]])
def test_lambda_rows_against_an_independent_evaluation(schedule):
    T = 20
    gg = torch.linspace(-6.0, 7.0, T + 1, dtype=torch.float64) + 0.1 * torch.sin(torch.arange(T + 1, dtype=torch.float64))
    path = [20, 13, 7, 2, 0]
    rows = restraints.lambda_rows(gg, path, schedule, clip=0.3, nv0=2.5)
    assert rows.shape == (4, 4) and rows.dtype == np.float32
    ref = rr.rows_from_grid(gg, path, schedule, 0.3, 2.5)
    for k, t in enumerate(path[:-1]):
        assert tuple(float(v) for v in rows[k]) == tuple(float(np.float32(v)) for v in ref[t]), (k, rows[k], ref[t])
    assert np.isinf(restraints.lambda_rows(gg, path, schedule)[:, 3]).all()
    for bad in ("linear", [1.0, 2.0], [1.0, 2.0, float("nan"), 1.0]):
        with pytest.raises(ValueError, match="restraint_schedule"):
            restraints.lambda_rows(gg, path, bad)
    for bad in (0.0, -1.0, True, "1"):
        with pytest.raises(ValueError, match="restraint_clip"):
            restraints.lambda_rows(gg, path, "score", clip=bad)


# ----------------------------------------------------------------------------- the restrained chain over the oracle

T = 8


def chain_setup(n_list, dtype=torch.float32):
    sd_np, cfg = er.weights(32, 2)
    x, h, nm, em, _ = er.molecules(n_list)
    model = er.cpu_diffusion(sd_np, 32, 2, T)
    gg = gamma_grid_fp64(model, T)
    return model, gg, nm, em, er.RefNet(sd_np, cfg, T, nm, em, None, dtype=dtype)


def chain_tables(N):
    return Restraints(obstacles=[[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]],
                      pairs=[[0, 1, 2.0, 2.5, 1.0], [2, 3, 0.0, 0.5, 1.0], [1, N + 3, 0.0, 1.0, 1.0]],
                      anchors=[[0, 1.0, 1.0, 1.0, 0.25, 1.5]])


@pytest.mark.parametrize("eta,steps", [(1.0, None), (0.0, 4), (1.0, 4)])
def test_restrained_chain_moves_the_sample_and_scale_zero_does_not(eta, steps):
    model, gg, nm, em, net = chain_setup([7, 4, 1])
    B, N = nm.shape[:2]
    path = paths.build_path(T, steps)
    raws = er.raw_draws(len(path), B, N, seed=6)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    rs = chain_tables(N)
    rows = rr.rows_from_grid(gg, path, "score", 0.3)          # clipped: lambda = sigma / alpha is large at the noisy end
    plain = gr.guided_chain_ref(gr.GuidedNet(net, net, 1.0, 0.0), gg, path, eta, z, nm, raws)
    off = gr.guided_chain_ref(rr.RestrainedNet(net, rs, torch.zeros(B), rows), gg, path, eta, z, nm, raws)
    on = gr.guided_chain_ref(rr.RestrainedNet(net, rs, torch.tensor([0.05, 0.02, 0.05]), rows), gg, path, eta, z, nm, raws)
    for a, b in zip(plain, off):
        assert torch.equal(a, b)
    assert not torch.equal(on[2][0], plain[2][0]) and not torch.equal(on[2][1], plain[2][1])
    assert torch.isfinite(on[0]).all() and torch.isfinite(on[2]).all()
    nmf = nm.float()
    print(f"eta {eta} steps {steps}: max |z_0| plain {float(plain[2].abs().max()):.3g} restrained {float(on[2].abs().max()):.3g}, "
          f"distance {rel_l2(on[2].numpy(), plain[2].numpy()):.3g}")
    # the state stays free of centre of mass (a few fp32 ulps of |z|, as the unrestrained chain)
    assert float((on[2][:, :, :3] * nmf).sum(1).abs().max()) < 1e-5 * max(1.0, float(on[2].abs().max()))
    # the one-node molecule: the projection removes its step, the chain is the plain one
    assert torch.equal(on[2][2], plain[2][2])


def test_restrained_multistep_chain_runs_through_the_solver_restatement():
    model, gg, nm, em, net = chain_setup([7, 4])
    B, N = nm.shape[:2]
    path = paths.build_path(T, 4)
    raw = er.raw_draws(1, B, N, seed=2)[0]
    z = orc.combined_noise(raw[0], raw[1], nm.float())
    rnet = rr.RestrainedNet(net, chain_tables(N), torch.tensor([0.1]), rr.rows_from_grid(gg, path, "sigma", 0.3))
    plain = sr.chain_ref(net.net, gg, path, z, nm.float())
    on = sr.chain_ref(rnet.net, gg, path, z, nm.float())
    assert torch.isfinite(on).all() and not torch.equal(on, plain)


# ----------------------------------------------------------------------------- the container

def test_restraints_accept_lists_and_tensors_shared_and_per_molecule():
    a = Restraints(obstacles=[[0, 0, 0, 1, 2]], pairs=torch.tensor([[0, 1, 1.0, 2.0, 1.0]]), anchors=[[2, 1, 1, 1, 0.5, 3.0]])
    assert a.sizes == (1, 1, 1) and a.rows() == (1, 1, 1)
    assert a.pair_idx.dtype == torch.int32 and a.anc_idx.dtype == torch.int32 and a.obs.dtype == torch.float32
    b = Restraints(obstacles=torch.zeros(4, 3, 5), anchors=np.zeros((4, 2, 6)))
    assert b.sizes == (3, 0, 2) and b.rows() == (4, 1, 4)
    b.check_batch(4)
    with pytest.raises(ValueError, match="molecules"):
        b.check_batch(3)
    assert b.slice(1, 3).rows() == (2, 1, 2)
    assert Restraints().sizes == (0, 0, 0)
    x = torch.zeros(1, 3, 3, dtype=torch.float64)
    x[0, 1, 0] = 3.0
    U = a.energy(x, torch.ones(1, 3, 1))
    assert U.shape == (1, 3) and U.dtype == torch.float64
    assert math.isclose(float(U[0, 0]), 0.5 * 2 * 1.0 * 2) and math.isclose(float(U[0, 1]), 0.5 * 1.0)   # two nodes at the centre


@pytest.mark.parametrize("kw,match", [
    (dict(pairs=[[0, 1, 2.0, 1.0, 1.0]]), "lo > hi"),
    (dict(pairs=[[2, 2, 0.0, 1.0, 1.0]]), "i == j"),
    (dict(pairs=[[0, -2, 0.0, 1.0, 1.0]]), "indices"),
    (dict(pairs=[[0, -1, 0.0, 1.0, 1.0]]), "padding"),
    (dict(pairs=[[0, 1, 0.0, 1.0, -1.0]]), ">= 0"),
    (dict(pairs=[[0.5, 1, 0.0, 1.0, 1.0]]), "integers"),
    (dict(obstacles=[[0, 0, 0, -1.0, 1.0]]), ">= 0"),
    (dict(obstacles=[[0, 0, 0, 1.0, -1.0]]), ">= 0"),
    (dict(obstacles=[[0, 0, float("nan"), 1.0, 1.0]]), "finite"),
    (dict(obstacles=[[0, 0, 0, 1.0]]), "obstacles must be"),
    (dict(anchors=[[0, 0, 0, 0, -0.5, 1.0]]), ">= 0"),
    (dict(anchors=[[-3, 0, 0, 0, 0.5, 1.0]]), "indices"),
    (dict(anchors=[[0, 0, 0, float("inf"), 0.5, 1.0]]), "finite"),
])
def test_restraints_reject_bad_tables(kw, match):
    with pytest.raises(ValueError, match=match):
        Restraints(**kw)


def test_json_file(tmp_path):
    p = tmp_path / "r.json"
    p.write_text(json.dumps({"obstacles": [[0, 0, 0, 1, 2]], "anchors": [[0, 1, 1, 1, 0.5, 1.0]]}))
    assert Restraints.from_json(str(p)).sizes == (1, 0, 1)
    p.write_text(json.dumps({"spheres": []}))
    with pytest.raises(ValueError, match="obstacles / pairs / anchors"):
        Restraints.from_json(str(p))


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_set_restraint", "hd_restraint_attach", "hd_restraint_detach", "hd_restrain_eps", "hd_restraint_energy"]


def test_restraint_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} not declared in the header"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays


def test_restraint_entry_points_reject_bad_arguments_without_a_gpu(lib):
    rows = (C.c_float * 8)(1, 0, 1, 1, 1, 0, 1, 1)
    assert lib.hd_set_restraint(None, 2, rows) == -1 and b"hd_set_restraint" in lib.hd_last_error()
    assert lib.hd_set_restraint(None, 0, rows) == -1
    assert lib.hd_restraint_attach(None, None, 1, 0, None, None, 1, 0, None, None, 1, 0, None, 1, 1.0, None) == -1
    assert b"hd_restraint_attach: null topology" in lib.hd_last_error()
    assert lib.hd_restraint_detach(None) == 0
    assert lib.hd_restrain_eps(None, None, None, None, rows, None, None) == -1 and b"hd_restrain_eps: null" in lib.hd_last_error()
    assert lib.hd_restraint_energy(None, None, None, None, None) == -1 and b"hd_restraint_energy: null" in lib.hd_last_error()


# ----------------------------------------------------------------------------- refusals of the Python entry points and the CLI

def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


def test_python_refusals_come_before_the_gpu():
    from hierdiff_amd import DiffusionQM9
    m = small_model()
    nm = torch.ones(2, 3, 1, dtype=torch.bool)
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    z3, z8, z11 = torch.zeros(2, 3, 3), torch.zeros(2, 3, 8), torch.zeros(2, 3, 11)
    mol = {"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}
    # the entry points that take none
    with pytest.raises(NotImplementedError, match="sample_inpaint: restraints"):
        m.sample_inpaint(nm, nm, z3, z8, restraints=rs)
    with pytest.raises(NotImplementedError, match="sample_grow: restraints"):
        m.sample_grow([mol], 4, "cpu", restraints=rs)
    with pytest.raises(NotImplementedError, match="sample_batches: restraints"):
        m.sample_batches(2, 1, "cpu", restraints=rs)
    with pytest.raises(NotImplementedError, match="encode: restraints"):
        m.encode(z3, z8, nm, restraints=rs)
    with pytest.raises(NotImplementedError, match="interpolate: restraints"):
        m.interpolate(mol, mol, 3, "cpu", restraints=rs)
    m.restraints, m.restraint_scale = rs, 1.0                # ... nor through the model's attributes
    try:
        for call in (lambda: m.sample_inpaint(nm, nm, z3, z8), lambda: m.sample_grow([mol], 4, "cpu"),
                     lambda: m.sample_batches(2, 1, "cpu"), lambda: m.encode(z3, z8, nm), lambda: m.interpolate(mol, mol, 3, "cpu")):
            with pytest.raises(NotImplementedError, match="restraints are not supported here"):
                call()
        m.restraint_scale = 0.0                              # a zero scale is the old code path: the refusals are gone
        with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
            m.encode(z3, z8, nm)
    finally:
        m.restraints, m.restraint_scale = None, None
    # argument errors of the restrained entry points
    kw = dict(restraints=rs, restraint_scale=1.0)
    with pytest.raises(ValueError, match="Restraints"):
        m.sample_from_masks(nm, None, None, restraints=[[0, 0, 0, 1, 1]], restraint_scale=1.0)
    with pytest.raises(ValueError, match="restraint_scale"):
        m.sample_from_masks(nm, None, None, restraints=rs, restraint_scale=torch.ones(3))
    with pytest.raises(ValueError, match="restraint_scale"):
        m.sample_from_masks(nm, None, None, restraints=rs, restraint_scale=float("nan"))
    with pytest.raises(ValueError, match="restraint_schedule"):
        m.sample_from_masks(nm, None, None, restraint_schedule="linear", **kw)
    with pytest.raises(ValueError, match="restraint_clip"):
        m.path_steps(z11, nm, steps=4, restraint_clip=-1.0, **kw)
    with pytest.raises(ValueError, match="molecules"):
        m.sample_from_latent(z11, nm, restraints=Restraints(obstacles=torch.ones(3, 1, 5)), restraint_scale=1.0)
    with pytest.raises(ValueError, match="restraint_scale"):
        DiffusionQM9.sample(m, 2, "cpu", restraints=rs, restraint_scale=torch.ones(5))
    with pytest.raises(ValueError, match="restraint_scale"):
        m.vary([mol], "cpu", 5, n_variants=2, restraints=rs, restraint_scale=torch.ones(3))
    # configurations restraints do not run in
    with pytest.raises(NotImplementedError, match="pocket"):
        m.sample_from_masks(nm, None, None, pocket=(None,) * 4, **kw)
    m.pocket = True
    try:
        with pytest.raises(NotImplementedError, match="pocket"):
            m.path_steps(z11, nm, steps=4, **kw)
    finally:
        m.pocket = False
    m.noise_mode = "torch"
    try:
        with pytest.raises(NotImplementedError, match="noise_mode"):
            m.sample_from_masks(nm, None, None, **kw)
        with pytest.raises(NotImplementedError, match="noise_mode"):
            DiffusionQM9.sample(m, 2, "cpu", **kw)
    finally:
        m.noise_mode = "philox"
    m.dynamics.mode = "gnn_dynamics"
    try:
        with pytest.raises(NotImplementedError, match="gnn_dynamics"):
            m.sample_from_masks(nm, None, None, **kw)
    finally:
        m.dynamics.mode = "egnn_dynamics"
    # a restrained call reaches the device check; a zero scale and no restraints are the old path and reach it too
    for k2 in (kw, dict(restraints=rs, restraint_scale=0.0), dict(restraints=rs), {}):
        with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
            m.sample_from_masks(nm, None, None, **k2)


def test_sampler_cli_arguments():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--restraints", "r.json"])
    assert (a.restraints, a.restraint_scale, a.restraint_schedule, a.restraint_clip) == ("r.json", 1.0, None, None)
    a = sampler.parse_args(["--restraints", "r.json", "--restraint-scale", "0.5", "--restraint-schedule", "sigma", "--restraint-clip",
                            "0.2", "--steps", "10", "--solver", "dpm2m", "--chain", "3", "--record", "x0"])
    assert (a.restraint_scale, a.restraint_schedule, a.restraint_clip, a.solver) == (0.5, "sigma", 0.2, "dpm2m")
    a = sampler.parse_args(["--restraints", "r.json", "--vary", "m.pkl", "--t-start", "10", "--guidance", "2", "--context", "0.5"])
    assert a.vary == "m.pkl" and a.guidance == 2.0
    assert sampler.parse_args([]).restraints is None
    for bad in (["--restraint-scale", "2"], ["--restraint-clip", "0.1"], ["--restraint-schedule", "sigma"],
                ["--restraints", "r.json", "--known", "k.pkl", "--grow", "2"], ["--restraints", "r.json", "--score", "m.pkl"],
                ["--restraints", "r.json", "--interpolate", "m.pkl", "--frames", "3"],
                ["--restraints", "r.json", "--restraint-clip", "0"], ["--restraints", "r.json", "--restraint-schedule", "linear"],
                ["--restraints", "r.json", "--restraint-scale", "nan"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
