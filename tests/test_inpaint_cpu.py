"""CPU tier of fragment-constrained sampling (inpainting): the new C-ABI symbols and their argument checks, the Python entry
points' input errors, and the CPU restatement of the algorithm (include/hierdiff_hip.h, "Fragment-constrained sampling") that
tests/test_gpu_inpaint.py holds the HIP loop against.

The restatement is built from the oracle's own pieces (posterior_step, final_decode, combined_noise, remove_mean_with_mask) with
normals from the library's host generator in the documented draw layout
    draw = (T + 2) * (3 j + k) + (T - s),   k = 0 posterior step, 1 known-part noise, 2 jump noise, round j;
    draw 0 = z_T, draw T + 1 = final decode.
It is pinned here before a GPU sees it: without fixed nodes and with one round it IS the oracle's plain chain, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from oracle import egnn_oracle as orc
from tests.helpers import fixture_model, load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2022


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


# ----------------------------------------------------------------------------- the restatement

def philox_raw(lib, seed, ids, draw, N, F=8):
    """(raw_x [B,N,3], raw_h [B,N,F]): normal(seed, id, draw, n * D + c) from the host twin of the device generator."""
    D = 3 + F
    out = np.empty((len(ids), N, D), dtype=np.float32)
    for b, sid in enumerate(ids):
        for e in range(N * D):
            out[b, e // D, e % D] = lib.hd_philox_normal_host(int(seed), int(sid), int(draw), e)
    t = torch.from_numpy(out)
    return t[:, :, :3].contiguous(), t[:, :, 3:].contiguous()


def gamma_grid_fp64(model, T):
    """The schedule values the product's default path tabulates (fp64 on the host, rounded once)."""
    import copy
    from hierdiff_amd.noise_model import evaluate_gamma
    return evaluate_gamma(copy.deepcopy(model.gamma).cpu(), (torch.arange(T + 1, dtype=torch.int64).view(-1, 1) / T)).view(-1)


def replace_ref(z_gen, xh_known, nm, fm, alpha_s, sigma_s, raw):
    """Steps 2 - 3: re-noised known rows, shifted to the generated rows' centre of gravity, blended in; molecules without
    fixed nodes keep z_gen bit for bit."""
    e_kn = torch.cat(raw, dim=2) * fm
    z_kn = (alpha_s * xh_known + sigma_s * e_kn) * fm
    nfix = fm.sum(1, keepdim=True)
    has = nfix > 0
    den = torch.where(has, nfix, torch.ones_like(nfix))
    c = (z_gen[:, :, :3] * fm).sum(1, keepdim=True) / den - (z_kn[:, :, :3] * fm).sum(1, keepdim=True) / den
    shift = torch.cat([c.expand(-1, z_gen.shape[1], -1), torch.zeros_like(z_gen[:, :, 3:])], dim=2)
    z = torch.where(fm.bool(), z_kn + shift, z_gen)
    z = torch.cat([orc.remove_mean_with_mask(z[:, :, :3], nm), z[:, :, 3:]], dim=2)
    return torch.where(has, z, z_gen)


def inpaint_steps_ref(lib, sd, cfg, T, gg, z, s_hi, s_lo, nm, em, context, fm, xh_known, r, seed, ids):
    """z_{s_hi} -> z_{s_lo}: rounds j = 0 .. r-1 of (posterior step, replace, jump back unless last) per step."""
    B, N = nm.shape[:2]
    for s in reversed(range(s_lo, s_hi)):
        s_arr = torch.full((B, 1), s, dtype=torch.int64)
        t_arr = s_arr + 1
        gs, gt = gg[s].expand(B, 1), gg[s + 1].expand(B, 1)
        _, sigma_ts, alpha_ts = orc.sigma_and_alpha_t_given_s(gt, gs)
        alpha_s = torch.sqrt(torch.sigmoid(-gs)).view(-1, 1, 1)
        sigma_s = torch.sqrt(torch.sigmoid(gs)).view(-1, 1, 1)
        for j in range(r):
            draw = lambda k: (T + 2) * (3 * j + k) + (T - s)
            z = orc.posterior_step(sd, cfg, s_arr / T, t_arr / T, z, nm, em, context, philox_raw(lib, seed, ids, draw(0), N),
                                   mol_shape=N, gammas=(gs, gt))
            z = replace_ref(z, xh_known, nm, fm, alpha_s, sigma_s, philox_raw(lib, seed, ids, draw(1), N))
            if j < r - 1:
                e = orc.combined_noise(*philox_raw(lib, seed, ids, draw(2), N), nm)
                z = alpha_ts.view(-1, 1, 1) * z + sigma_ts.view(-1, 1, 1) * e
    return z


def inpaint_chain_ref(lib, sd, cfg, T, gg, node_mask, edge_mask, context, fixed_mask, x_known, h_known, r, seed, ids,
                      norm_values=(1.0, 1.0, 1.0), norm_biases=(None, 0.0, 0.0)):
    """The whole algorithm: z_T (draw 0), T steps, the plain decode (draw T + 1), the fix-up of the fixed rows.  Returns
    (x, h, z_0)."""
    nm, fm = node_mask.float(), fixed_mask.float()
    B, N = nm.shape[:2]
    gg = torch.as_tensor(gg, dtype=torch.float32).view(-1)
    xk, hk = x_known.float(), h_known.float()
    xh_known = torch.cat([xk / norm_values[0], (hk - (norm_biases[1] or 0.0)) / norm_values[1]], dim=2) * fm
    z = orc.combined_noise(*philox_raw(lib, seed, ids, 0, N), nm)
    z = inpaint_steps_ref(lib, sd, cfg, T, gg, z, T, 0, nm, edge_mask, context, fm, xh_known, r, seed, ids)
    x, h = orc.final_decode(sd, cfg, z, nm, edge_mask, context, philox_raw(lib, seed, ids, T + 1, N), gamma_0=gg[0].expand(B, 1),
                            norm_values=norm_values, norm_biases=norm_biases)
    nfix = fm.sum(1, keepdim=True)
    den = torch.where(nfix > 0, nfix, torch.ones_like(nfix))
    c = (x * fm).sum(1, keepdim=True) / den - (xk * fm).sum(1, keepdim=True) / den
    x = torch.where(fm.bool(), xk + c, x)
    h = torch.where(fm.bool(), hk, h)
    return x, h, z


def cpu_model(H=32, L=2, T=10, C_=0, seed=10):
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict
    sd_np = synthetic_state_dict(9, C_, H, L, 2, True, seed, 1.0)
    m = DiffusionQM9(default_config(hidden_nf=H, n_layers=L, context_node_nf=C_, timesteps=T))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd_np.items()})
    return m, sd_np


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_set_inpaint_schedule", "hd_sample_loop_inpaint", "hd_inpaint_decode_fix"]


def test_inpaint_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
    # argument counts of the binding follow the header's declarations
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays
    assert "draw = (T + 2) * (3 j + k) + (T - s)" in hdr       # the draw layout is documented next to the noise entry point


def test_inpaint_entry_points_reject_bad_arguments_without_a_gpu(lib):
    coef = (C.c_float * 8)()
    assert lib.hd_set_inpaint_schedule(None, 2, coef) == -1 and b"hd_set_inpaint_schedule" in lib.hd_last_error()
    assert lib.hd_sample_loop_inpaint(None, None, None, None, -1, 1, 0, None, None, 1, 0, 0, 0, None, None, 1, None) == -1
    assert b"hd_sample_loop_inpaint" in lib.hd_last_error()
    assert lib.hd_inpaint_decode_fix(None, None, None, None, None, None, None, None) == -1
    assert b"hd_inpaint_decode_fix" in lib.hd_last_error()


def test_python_entry_points_raise_on_bad_input_before_touching_the_gpu():
    m, _ = cpu_model(T=4, L=1)
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    fm = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool).view(B, N, 1)
    xk, hk = torch.zeros(B, N, 3), torch.zeros(B, N, 8)
    with pytest.raises(ValueError, match="subset"):
        m.sample_inpaint(nm, torch.ones_like(nm), xk, hk)
    with pytest.raises(ValueError, match="fixed_mask"):
        m.sample_inpaint(nm, fm[:, :3], xk, hk)
    with pytest.raises(ValueError, match="x_known"):
        m.sample_inpaint(nm, fm, xk[:, :, :2], hk)
    with pytest.raises(ValueError, match="h_known"):
        m.sample_inpaint(nm, fm, xk, hk[:1])
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="resamplings"):
            m.sample_inpaint(nm, fm, xk, hk, resamplings=bad)
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="torch"):
        m.sample_inpaint(nm, fm, xk, hk)
    m.noise_mode = "philox"
    m.pocket = True
    with pytest.raises(NotImplementedError, match="pocket"):
        m.sample_inpaint(nm, fm, xk, hk)
    m.pocket = False
    m.dynamics.mode = "gnn_dynamics"
    with pytest.raises(NotImplementedError, match="gnn_dynamics"):
        m.sample_inpaint(nm, fm, xk, hk)
    m.dynamics.mode = "egnn_dynamics"
    # list level: sizes below the known part, malformed fragments
    with pytest.raises(ValueError, match="smaller"):
        m.sample_grow([{"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}], [2], "cpu")
    with pytest.raises(ValueError, match="known\\[0\\]"):
        m.sample_grow([{"x": torch.zeros(3, 3), "h": torch.zeros(2, 8)}], [5], "cpu")
    if not torch.cuda.is_available():           # valid input, no GPU: the library's loud error, not a fallback
        with pytest.raises(_lib.HierDiffHipError):
            m.sample_inpaint(nm, fm, xk, hk)


def test_cli_known_and_grow_go_together():
    from hierdiff_amd import sampler
    with pytest.raises(SystemExit):
        sampler.main(["--known", "x.pkl"])
    with pytest.raises(SystemExit):
        sampler.main(["--grow", "3"])


def test_read_known_accepts_both_layouts(tmp_path):
    import pickle
    from hierdiff_amd import sampler
    res = [{"x": torch.randn(3, 3), "h": torch.randn(3, 8)}, {"x": torch.randn(2, 3), "h": torch.randn(2, 8)}]
    a, b, c = tmp_path / "a.pkl", tmp_path / "b.pkl", tmp_path / "c.pt"
    sampler.write_results(str(a), res)
    pickle.dump(res, open(b, "wb"))
    torch.save(res, c)
    for p in (a, b, c):
        got = sampler.read_known(str(p))
        assert len(got) == 2 and all(torch.equal(g["x"], r["x"]) and torch.equal(g["h"], r["h"]) for g, r in zip(got, res))
    pickle.dump({"x": 1}, open(b, "wb"))
    with pytest.raises(ValueError):
        sampler.read_known(str(b))


# ----------------------------------------------------------------------------- the yardstick, pinned

def test_restatement_without_fixed_nodes_is_the_oracle_chain(lib):
    """All-false fixed_mask, r = 1: exactly oracle.sample_chain on the same draws (T = 10, H = 32)."""
    fx = load("f5_chain_h32_l2")
    sd_np, sd, cfg = fixture_model(fx)
    T, n_list = 10, [6, 3, 5, 1]
    m, _ = cpu_model(H=32, L=int(fx["n_layers"]), T=T, seed=int(fx["weight_seed"]))
    gg = gamma_grid_fp64(m, T)
    nm, em = orc.canonical_masks(n_list)
    B, N = nm.shape[:2]
    ids = [40 + b for b in range(B)]
    fm = torch.zeros_like(nm, dtype=torch.bool)
    x, h, _ = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, None, fm, torch.randn(B, N, 3), torch.randn(B, N, 8), 1, SEED, ids)
    raws = [philox_raw(lib, SEED, ids, d, N) for d in range(T + 2)]
    xo, ho = orc.sample_chain(sd, cfg, T, nm, em, None, raws, gamma_grid=gg)
    assert torch.equal(x, xo) and torch.equal(h, ho)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()


def test_restatement_keeps_the_known_part_and_the_centre_of_gravity(lib):
    """With fixed nodes: z stays centre-of-gravity free after every replace step, the returned known rows are a translation of the
    input, and the known values reach the free nodes (a different x_known gives a different molecule)."""
    fx = load("f5_chain_h32_l2")
    _, sd, cfg = fixture_model(fx)
    T, n_list = 6, [6, 4, 5]
    m, _ = cpu_model(H=32, L=int(fx["n_layers"]), T=T, seed=int(fx["weight_seed"]))
    gg = gamma_grid_fp64(m, T)
    nm, em = orc.canonical_masks(n_list)
    B, N = nm.shape[:2]
    fm = torch.zeros(B, N, 1, dtype=torch.bool)
    fm[0, :3] = True
    fm[1, :4] = True                       # all nodes of molecule 1; molecule 2: none
    g = torch.Generator().manual_seed(3)
    xk, hk = torch.randn(B, N, 3, generator=g) + 5.0, torch.randn(B, N, 8, generator=g)
    ids = [7, 8, 9]
    for r in (1, 2):
        x, h, z0 = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, None, fm, xk, hk, r, SEED, ids)
        assert float((z0[:, :, :3] * nm).sum(1).abs().max()) < 1e-5 * max(1.0, float(z0.abs().max()))      # a few fp32 ulps of |z|
        assert torch.equal(h[fm.expand_as(h)], hk[fm.expand_as(h)])
        d = (x - xk)[0, :3]
        assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(x[0, :3].abs().max())))
        assert torch.all(x[~nm.expand_as(x).bool()] == 0) and torch.all(h[~nm.expand_as(h).bool()] == 0)
    x1, _, _ = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, None, fm, xk, hk, 1, SEED, ids)
    xk2 = xk.clone()
    xk2[0, 1] += 1.0
    x2, _, _ = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, None, fm, xk2, hk, 1, SEED, ids)
    assert not torch.equal(x1[0, 3:6], x2[0, 3:6])
    assert torch.equal(x1[1:], x2[1:])
