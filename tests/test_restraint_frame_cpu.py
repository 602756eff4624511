"""CPU tier of restraints in the known fragments' frame: the float64 restatement of tests/restraint_frame_reference.py against
float64 autograd of the product's energy on x - tau (tau detached, free nodes only), its reduction to the plain update without
fixed nodes, the invariants of the update (mean-free, one common vector on the fixed block, untouched features / masked rows / all-
fixed molecules), the property the construction exists for (behind the posterior step and the replacement a free node has moved
relative to the block by its own step times the step's coefficient), the sensitivity of the restatement to the one-ulp freedom of the
fp32 data prediction on the inputs of the GPU test, the C ABI (symbols, prototypes, argument errors without a device), and the
Python / CLI refusals - raised before any library call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, restraints
from hierdiff_amd.restraints import Restraints
from tests import restraint_frame_reference as fr
from tests import restraint_reference as rr
from tests import sampling_reference as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ----------------------------------------------------------------------------- the definition

def small_case(seed=3, B=4, N=9):
    """Positions around the origin (the model's frame), known positions and tables around CENTRE (the user's frame)."""
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, generator=g_, dtype=torch.float64) * 1.5
    nm = torch.ones(B, N, dtype=torch.bool)
    nm[1, 5:] = False
    fm = torch.zeros(B, N, dtype=torch.bool)
    fm[0, :3] = True
    fm[1, 1:4] = True
    fm[1, 7] = True                                          # a fixed byte on a masked row: ignored
    fm[3] = True                                             # every valid node fixed (molecule 2 has none)
    centre = torch.tensor(fr.CENTRE, dtype=torch.float64)
    xk = centre + torch.randn(B, N, 3, generator=g_, dtype=torch.float64) * 1.5
    return x, xk, nm, fm


@pytest.mark.parametrize("per_molecule", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("P,Q,A", [(1, 0, 2), (7, 3, 0), (70, 3, 2)])
def test_reference_equals_autograd_of_the_energy_in_the_known_frame(P, Q, A, per_molecule):
    x, xk, nm, fm = small_case()
    B, N = nm.shape
    rs = fr.framed_tables(B, N, P, Q, A, seed=P + 10 * Q + 100 * A, per_molecule=per_molecule)
    U, Um, g, ga, tau = fr.framed_energy_grad(rs, x.numpy(), xk.numpy(), nm.numpy(), fm.numpy())
    t_prod = restraints.frame_shift(x, nm, fm, xk)
    assert np.allclose(tau, t_prod.numpy(), rtol=0, atol=1e-13)
    assert (tau[2] == 0).all() and np.abs(tau[0]).max() > 5  # no fixed node: no shift; the others are far from the origin
    with torch.enable_grad():
        xv = x.clone().requires_grad_(True)
        Ua = restraints.energy_terms(rs, xv - t_prod.detach()[:, None, :], nm.reshape(B, N, 1))
        Ua.sum().backward()
    free = (nm & ~fm).numpy()
    gauto = np.where(free[:, :, None], xv.grad.numpy(), 0.0)
    assert np.allclose(U, Ua.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert (np.abs(g - gauto) <= 1e-12 * np.maximum(ga, 1.0)).all()
    assert (g[~free] == 0).all() and np.abs(g).max() > 0
    assert (ga >= np.abs(g) - 1e-12).all()
    # the CPU form of `Restraints.energy` is the same number
    Ue, te = rs.energy(x, nm.reshape(B, N, 1), fixed_mask=fm.reshape(B, N, 1), x_known=xk, return_shift=True)
    assert np.allclose(Ue.numpy(), U, rtol=1e-12, atol=1e-12) and torch.equal(te, t_prod)
    with pytest.raises(ValueError, match="go together"):
        rs.energy(x, nm.reshape(B, N, 1), fixed_mask=fm.reshape(B, N, 1))


def update_case(N=9, D=11, seed=8):
    x, xk, nm, fm = small_case(seed, 4, N)
    B = 4
    g_ = torch.Generator().manual_seed(seed)
    z = torch.randn(B, N, D, generator=g_)
    eps = torch.randn(B, N, D, generator=g_)
    nv0 = 1.7
    known = torch.zeros(B, N, D)
    known[:, :, :3] = (xk / nv0).float()
    return z, eps, nm, fm, known, nv0


def test_without_fixed_nodes_it_is_the_plain_update():
    z, eps, nm, fm, known, nv0 = update_case()
    B, N, _ = z.shape
    rs, _ = rr.random_tables(B, N, 7, 3, 2, seed=4, per_molecule=True)
    scale = torch.tensor([1.0, 0.5, 2.0, 1.5])
    for clip in (math.inf, 0.2):
        row = (0.8, 0.6, 0.75, clip)
        none = torch.zeros_like(fm)
        got, mag, _ = fr.restrain_framed_ref(rs, z, eps, nm, none, known, scale, row, nv0)
        want, wmag = rr.restrain_ref(rs, z, eps, nm, scale, row, nv0)
        assert (got == want).all() and (mag == wmag).all()
        # ... and molecule by molecule: the one without fixed nodes among molecules that have some
        mixed, _, _ = fr.restrain_framed_ref(rs, z, eps, nm, fm, known, scale, row, nv0)
        assert (mixed[2] == want[2]).all() and not (mixed[0] == want[0]).all()


def test_invariants_of_the_framed_update():
    z, eps, nm, fm, known, nv0 = update_case()
    B, N, _ = z.shape
    rs = fr.framed_tables(B, N, 70, 3, 2, seed=5, per_molecule=False)     # many obstacles: the two free nodes of molecule 1 meet some
    scale = torch.tensor([1.0, 0.5, 2.0, 1.5])
    e = eps.double().numpy()
    valid, fixed = nm.numpy(), (fm & nm).numpy()
    for clip in (math.inf, 0.2):
        out, mag, act = fr.restrain_framed_ref(rs, z, eps, nm, fm, known, scale, (0.8, 0.6, 0.75, clip), nv0)
        d = out - e
        assert (out[:, :, 3:] == e[:, :, 3:]).all() and (out[~valid] == e[~valid]).all()
        assert np.abs((d[:, :, :3] * valid[:, :, None]).sum(1)).max() < 1e-12            # mean-free
        assert (out[3] == e[3]).all() and not act[3]                                      # every valid node fixed: untouched
        assert act[0] and act[1]
        for b in (0, 1):                                                                  # the block moves as one: -m
            blk = d[b][fixed[b]][:, :3]
            assert np.abs(blk - blk[0]).max() < 1e-12 and np.abs(blk[0]).max() > 0
        assert (mag >= np.abs(out) - 1e-12).all()
    zero, _, _ = fr.restrain_framed_ref(rs, z, eps, nm, fm, known, torch.zeros(1), (0.8, 0.6, 0.75, 0.2), nv0)
    assert (zero == e).all()
    # the fixed byte on a masked row is ignored: clearing it changes nothing
    fm2 = fm.clone()
    fm2[1, 7] = False
    a, _, _ = fr.restrain_framed_ref(rs, z, eps, nm, fm, known, scale, (0.8, 0.6, 0.75, 0.2), nv0)
    b_, _, _ = fr.restrain_framed_ref(rs, z, eps, nm, fm2, known, scale, (0.8, 0.6, 0.75, 0.2), nv0)
    assert (a == b_).all()


class _Masks:
    """What `guidance_reference.ancestral_on_eps` takes from a network: the node mask, in fp32."""
    dtype = torch.float32

    def __init__(self, nm):
        self.nm = nm

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_a_free_node_moves_relative_to_the_block_by_its_own_step():
    """The point of the construction: posterior step, then the replacement - the position of a free node relative to the centre of
    the fixed block differs between the restrained and the unrestrained transition by -(sigma2_t|s / alpha_t|s / sigma_t) d_i."""
    from oracle import egnn_oracle as orc
    from tests import guidance_reference as gr
    z, eps, nm, fm, known, nv0 = update_case(D=11)
    B, N, D = z.shape
    nm3 = nm.reshape(B, N, 1).float()
    z = torch.cat([orc.remove_mean_with_mask(z[:, :, :3] * nm3, nm3), z[:, :, 3:] * nm3], dim=2)
    eps = torch.cat([orc.remove_mean_with_mask(eps[:, :, :3] * nm3, nm3), eps[:, :, 3:] * nm3], dim=2)
    rs = fr.framed_tables(B, N, 7, 3, 2, seed=5, per_molecule=False)
    gg = torch.linspace(-4.0, 4.0, 9, dtype=torch.float64)
    s, t = 3, 5
    al, sg = float(torch.sqrt(torch.sigmoid(-gg[t].float()))), float(torch.sqrt(torch.sigmoid(gg[t].float())))
    out, _, _ = fr.restrain_framed_ref(rs, z, eps, nm, fm, known, torch.ones(1), (al, sg, 0.5, 0.2), nv0)
    d = out[:, :, :3] - eps.double().numpy()[:, :, :3]
    g_ = torch.Generator().manual_seed(2)
    raw0 = (torch.randn(B, N, 3, generator=g_), torch.randn(B, N, D - 3, generator=g_))
    raw1 = (torch.randn(B, N, 3, generator=g_), torch.randn(B, N, D - 3, generator=g_))
    net = _Masks(nm3)
    fm3 = (fm & nm).reshape(B, N, 1).float()
    a_s, s_s = torch.sqrt(torch.sigmoid(-gg[s])).float().view(1, 1, 1), torch.sqrt(torch.sigmoid(gg[s])).float().view(1, 1, 1)
    rel = []
    for e_ in (eps, torch.from_numpy(out).float()):
        zs = gr.ancestral_on_eps(net, z, e_, s, t, raw0, gg.float()).float()
        zs = fr.replace_ref(zs, known * fm3, nm3, fm3, a_s, s_s, raw1).double().numpy()[:, :, :3]
        rel.append([zs[b] - zs[b][(fm & nm)[b].numpy()].mean(0) for b in (0, 1)])
    sigma2_ts, _, alpha_ts = orc.sigma_and_alpha_t_given_s(gg[t].view(1, 1), gg[s].view(1, 1))
    coef = float(sigma2_ts / alpha_ts) / math.sqrt(float(torch.sigmoid(gg[t])))
    for i, b in enumerate((0, 1)):
        free = (nm & ~fm)[b].numpy()
        moved = (rel[1][i] - rel[0][i])[free]
        own = d[b][free] - d[b][(fm & nm)[b].numpy()][0]      # eps^ changed by d_i - m, the block by -m: the node's own step d_i
        assert np.abs(own).max() > 1e-3
        assert np.abs(moved + coef * own).max() < 2e-5, np.abs(moved + coef * own).max()   # fp32 states of O(10)


@pytest.mark.parametrize("N,D", [(5, 4), (33, 11)])
def test_the_gpu_cases_tolerate_the_one_ulp_freedom_of_x0(N, D):
    """The device may contract z - sigma eps into one fused multiply-add (tests/restraint_reference.py): the restatement evaluated on
    that x^0 must stay inside the GPU test's bar of the restatement on torch's x^0 - otherwise the inputs, not the kernel, would
    decide the GPU test."""
    c = fr.kernel_case(N, D)
    worst = 0.0
    for (P, Q, A) in fr.PQA:
        for per in (False, True):
            rs = fr.framed_tables(c.B, N, P, Q, A, seed=P + 10 * Q + 100 * A + int(per), per_molecule=per)
            for clip in (math.inf, 0.2):
                row = (0.8, 0.6, 0.75, clip)
                ref, mag, _ = fr.restrain_framed_ref(rs, c.z, c.eps, c.nm, c.fm, c.known, c.scale, row, c.nv0)
                f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
                inner = (c.z[:, :, :3].double() - f32(0.6).double() * c.eps[:, :, :3].double()).float()      # one rounding
                x0 = ((f32(1.0) / f32(0.8)) * inner) * f32(c.nv0)
                alt, _, _ = fr.restrain_framed_ref(rs, c.z, c.eps, c.nm, c.fm, c.known, c.scale, row, c.nv0, x0=x0.numpy())
                ratio = float((np.abs(alt - ref) / (sref.BOUND * sref.U * np.maximum(mag, 1e-300))).max())
                worst = max(worst, ratio)
                # half the bar: the rounding of the kernel's own output (2^-24 of |eps^ + Delta|, 1/16 of the bar) fits on top
                assert ratio <= 0.5, (P, Q, A, per, clip, ratio)
    print(f"N={N} D={D}: worst |ref(x0 fused) - ref(x0)| / bound over all cases {worst:.3f}")


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_restraint_frame", "hd_restrain_eps_framed", "hd_restraint_energy_framed"]


def test_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12         # additive: the ABI version stays
    assert "#define HD_ABI_VERSION 12" in hdr
    assert "tau     = mean_F(x^0) - mean_F(xk)" in hdr


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    rows = (C.c_float * 4)(1, 0, 1, 1)
    assert lib.hd_restraint_frame(None, 1) == -1 and b"hd_restraint_frame: null topology" in lib.hd_last_error()
    assert lib.hd_restrain_eps_framed(None, None, None, None, rows, None, None, None, None) == -1
    assert b"hd_restrain_eps_framed: null" in lib.hd_last_error()
    assert lib.hd_restraint_energy_framed(None, None, None, None, None, None, None, None) == -1
    assert b"hd_restraint_energy_framed: null" in lib.hd_last_error()
    # hd_restraint_frame reads the topology's host-side flags and nothing else: a zeroed block stands in for a topology that never
    # had restraints attached (hd_topology_create value-initialises the structure), so HD_E_STATE shows without a device
    blank = C.create_string_buffer(1 << 16)
    assert lib.hd_restraint_frame(C.cast(blank, C.c_void_p), 7) == -1 and b"frame is 0" in lib.hd_last_error()
    for frame in (0, 1):
        assert lib.hd_restraint_frame(C.cast(blank, C.c_void_p), frame) == -4
        assert b"no restraints attached" in lib.hd_last_error()
    assert blank.raw == bytes(1 << 16)


# ----------------------------------------------------------------------------- Python and CLI

def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


def test_python_errors_and_refusals_come_before_any_library_call(monkeypatch):
    m = small_model()
    nm = torch.ones(2, 3, 1, dtype=torch.bool)
    fm = torch.zeros(2, 3, 1, dtype=torch.bool)
    fm[:, 0] = True
    rs = Restraints(obstacles=[[0, 0, 0, 1, 1]])
    z3, z8, z11 = torch.zeros(2, 3, 3), torch.zeros(2, 3, 8), torch.zeros(2, 3, 11)
    mol = {"x": torch.zeros(2, 3), "h": torch.zeros(2, 8)}
    kw = dict(restraints=rs, restraint_scale=1.0)

    def no_library():
        raise AssertionError("a library call was made before the refusal")

    monkeypatch.setattr(_lib, "load", no_library)
    assert m.restraint_frame is None
    # the keyword's own errors
    for bad in ("pocket", 1, True):
        with pytest.raises(ValueError, match="restraint_frame"):
            m.sample_inpaint(nm, fm, z3, z8, restraint_frame=bad, **kw)
        with pytest.raises(ValueError, match="restraint_frame"):
            m.sample_grow([mol], 4, "cpu", restraint_frame=bad, **kw)
        with pytest.raises(ValueError, match="restraint_frame"):
            m.inpaint_steps(z11, 2, 0, nm, fm, z3, z8, restraint_frame=bad, **kw)
    # the default path and the explicit model frame refuse as before
    for frame in (None, "model"):
        with pytest.raises(NotImplementedError, match="sample_inpaint: restraints are not supported here: inpainting re-centres"):
            m.sample_inpaint(nm, fm, z3, z8, restraint_frame=frame, **kw)
        with pytest.raises(NotImplementedError, match="sample_grow: restraints are not supported here: inpainting re-centres"):
            m.sample_grow([mol], 4, "cpu", restraint_frame=frame, **kw)
    # argument errors of the framed calls: those of the restrained entry points
    fk = dict(restraint_frame="known")
    with pytest.raises(ValueError, match="Restraints"):
        m.sample_inpaint(nm, fm, z3, z8, restraints=[[0, 0, 0, 1, 1]], restraint_scale=1.0, **fk)
    with pytest.raises(ValueError, match="restraint_scale"):
        m.sample_inpaint(nm, fm, z3, z8, restraints=rs, restraint_scale=torch.ones(3), **fk)
    with pytest.raises(ValueError, match="restraint_scale"):
        m.sample_grow([mol, mol], 4, "cpu", restraints=rs, restraint_scale=torch.ones(3), **fk)
    with pytest.raises(ValueError, match="restraint_schedule"):
        m.sample_inpaint(nm, fm, z3, z8, restraint_schedule="linear", **kw, **fk)
    with pytest.raises(ValueError, match="restraint_clip"):
        m.inpaint_steps(z11, 2, 0, nm, fm, z3, z8, restraint_clip=-1.0, **kw, **fk)
    with pytest.raises(ValueError, match="molecules"):
        m.sample_inpaint(nm, fm, z3, z8, restraints=Restraints(obstacles=torch.ones(3, 1, 5)), restraint_scale=1.0, **fk)
    with pytest.raises(ValueError, match="ancestral"):
        m.sample_inpaint(nm, fm, z3, z8, eta=0.5, **kw, **fk)
    with pytest.raises(ValueError, match="ancestral"):
        m.sample_inpaint(nm, fm, z3, z8, solver="dpm2m", **kw, **fk)
    # "known" anywhere else
    m.restraint_frame = "known"
    try:
        with pytest.raises(ValueError, match="restraint_frame='known'"):
            m.sample_from_masks(nm, None, None, **kw)
        with pytest.raises(ValueError, match="restraint_frame='known'"):
            m.path_steps(z11, nm, steps=4, **kw)
        with pytest.raises(ValueError, match="restraint_frame='known'"):
            m.sample_from_latent(z11, nm, **kw)
        with pytest.raises(ValueError, match="restraint_frame='known'"):
            m.vary([mol], "cpu", 5, **kw)
        with pytest.raises(ValueError, match="restraint_frame='known'"):
            m.vary([mol], "cpu", 5, restraint_frame="known", **kw)
        # steering stays refused with inpainting; pocket models, gnn_dynamics and torch noise too
        m.particles, m.steer_scale = 2, 1.0
        try:
            with pytest.raises(NotImplementedError, match="steered"):
                m.sample_inpaint(nm, fm, z3, z8, **kw)
            with pytest.raises(NotImplementedError, match="steered"):
                m.sample_grow([mol], 4, "cpu", **kw)
        finally:
            m.particles, m.steer_scale = None, None
        m.pocket = True
        try:
            with pytest.raises(NotImplementedError, match="pocket"):
                m.sample_inpaint(nm, fm, z3, z8, **kw)
        finally:
            m.pocket = False
        m.noise_mode = "torch"
        try:
            with pytest.raises(NotImplementedError, match="noise_mode"):
                m.sample_inpaint(nm, fm, z3, z8, **kw)
        finally:
            m.noise_mode = "philox"
        m.dynamics.mode = "gnn_dynamics"
        try:
            with pytest.raises(NotImplementedError, match="gnn_dynamics"):
                m.sample_inpaint(nm, fm, z3, z8, **kw)
        finally:
            m.dynamics.mode = "egnn_dynamics"
        # set once on the model, a framed call reaches the device check - and so does an unrestrained one, whatever the frame
        for k2 in (kw, dict(restraints=rs, restraint_scale=0.0), {}):
            with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
                m.sample_inpaint(nm, fm, z3, z8, **k2)
        with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
            m.sample_from_masks(nm, None, None)               # the frame alone asks for nothing
    finally:
        m.restraint_frame = None
    with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
        m.sample_inpaint(nm, fm, z3, z8, **kw, **fk)


def test_sampler_cli_arguments():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--restraints", "r.json", "--restraint-frame", "known", "--known", "k.pkl", "--grow", "2"])
    assert (a.restraints, a.restraint_frame, a.known, a.grow, a.restraint_scale) == ("r.json", "known", "k.pkl", 2, 1.0)
    a = sampler.parse_args(["--restraints", "r.json", "--restraint-frame", "known", "--known", "k.pkl", "--grow", "2", "--steps", "10",
                            "--resamplings", "2", "--restraint-clip", "0.2", "--chain", "3", "--record", "x0"])
    assert (a.steps, a.resamplings, a.restraint_clip, a.record) == (10, 2, 0.2, "x0")
    assert sampler.parse_args(["--restraints", "r.json", "--restraint-frame", "model"]).restraint_frame == "model"
    assert sampler.parse_args(["--restraints", "r.json"]).restraint_frame is None
    for bad in (["--restraints", "r.json", "--known", "k.pkl", "--grow", "2"],                               # the old refusal stands
                ["--restraints", "r.json", "--restraint-frame", "model", "--known", "k.pkl", "--grow", "2"],
                ["--restraints", "r.json", "--restraint-frame", "known"],                                    # needs fragments
                ["--restraint-frame", "known", "--known", "k.pkl", "--grow", "2"],                            # needs --restraints
                ["--restraints", "r.json", "--restraint-frame", "pocket", "--known", "k.pkl", "--grow", "2"],
                ["--restraints", "r.json", "--restraint-frame", "known", "--vary", "m.pkl", "--t-start", "5"],
                ["--restraints", "r.json", "--restraint-frame", "known", "--known", "k.pkl", "--grow", "2", "--particles", "2",
                 "--steer-scale", "1", "--batch-size", "4"],
                ["--restraints", "r.json", "--restraint-frame", "known", "--known", "k.pkl", "--grow", "2", "--eta", "0.5"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
