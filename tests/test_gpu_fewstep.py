"""GPU tier (-m gpu) of few-step sampling: the path loops (hd_sample_path, hd_sample_path_inpaint) against the plain loops at
stride 1 (bit for bit), against the CPU oracle on strided paths, and their reproducibility across graph replay, batch split and
seeds.

The oracle for a strided chain is `path_chain_ref` below: `oracle.egnn_oracle.posterior_step(sd, cfg, s, t, ...)` looped over the
path (eta = 1), or the fp64 formula z_s = a z_t - b eps + c noise applied to `oracle.egnn_oracle.dynamics_forward` (eta < 1), and
`final_decode`.  Bar: rel-L2 < 1e-3 on the final x and h, the bar of the existing compounded chains
(tests/test_gpu_configs.py::test_full_length_chain_production_width gives the reason); a K-step chain compounds less, so the
same bar is a condition, not a measurement.  Measured values are printed.

Weights: `synthetic_state_dict(..., coord_gain 0.02)`, the gain the repository's trajectory tests use (tests/test_gpu_configs.py
`_syn`: the predicted velocity is O(1) like a trained model's)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.helpers import rel_l2
from tests.test_gpu_inpaint import N_FIXED, make_case
from tests.test_gpu_parity import PRECISIONS, build_diffusion
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
N_LIST = [8, 5, 7, 3, 6]


def dev(t):
    return None if t is None else t.to(DEV)


def make_model(H, L, T, C_=0, precision="fp32", seed=31):
    from hierdiff_amd.weights import synthetic_state_dict
    sd_np = synthetic_state_dict(9, C_, H, L, 2, True, seed, 0.02)
    model = build_diffusion(sd_np, H, L, C_=C_, T=T, precision=precision)
    model.seed = SEED
    cfg = orc.DynCfg(in_node_nf=9, context_node_nf=C_, hidden_nf=H, n_layers=L)
    return model, orc.as_torch_sd(sd_np), cfg


def raw_draws(n, B, N, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    b = B if rows is None else rows
    return [(torch.randn(b, N, 3, generator=g), torch.randn(b, N, 8, generator=g)) for _ in range(n)]


def context_for(nm, seed=3):
    g = torch.Generator().manual_seed(seed)
    B, N = nm.shape[:2]
    return torch.randn(B, 1, 1, generator=g).expand(B, N, 1).contiguous() * nm.float()


def linear_row(gs, gt, eta):
    """(a, b, c) of z_s = a z_t - b eps + c noise in Python floats (section 1 of the issue; independent of hierdiff_amd.paths)."""
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    softplus = lambda v: max(v, 0.0) + math.log1p(math.exp(-abs(v)))
    a_s, a_t, s_s, s_t = math.sqrt(sig(-gs)), math.sqrt(sig(-gt)), math.sqrt(sig(gs)), math.sqrt(sig(gt))
    st = eta * math.sqrt(-math.expm1(softplus(gs) - softplus(gt))) * s_s / s_t
    return a_s / a_t, a_s * s_t / a_t - math.sqrt(max(s_s * s_s - st * st, 0.0)), st


def path_chain_ref(sd, cfg, T, gg, path, eta, nm, em, ctx, raws):
    """(x, h, z_0) of the chain on `path` with injected normals raws = [z_T, one per transition, decode]."""
    nmf = nm.float()
    B, N = nmf.shape[:2]
    z = orc.combined_noise(raws[0][0], raws[0][1], nmf)
    if z.size(0) == 1 and B > 1:
        z = z.expand(B, -1, -1).clone()
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        s_arr, t_arr = torch.full((B, 1), s, dtype=torch.int64), torch.full((B, 1), t, dtype=torch.int64)
        if eta == 1.0:
            z = orc.posterior_step(sd, cfg, s_arr / T, t_arr / T, z, nm, em, ctx, raws[1 + k], mol_shape=N,
                                   gammas=(gg[s].expand(B, 1), gg[t].expand(B, 1)))
            continue
        a, b, c = linear_row(float(gg[s]), float(gg[t]), eta)
        eps = orc.dynamics_forward(sd, cfg, t_arr / T, z, nm, em, ctx, N, prefix="dynamics.egnn.").double()
        eps[:, :, :3] = orc.remove_mean_with_mask(eps[:, :, :3], nmf.double())
        noise = orc.combined_noise(raws[1 + k][0], raws[1 + k][1], nmf).double()
        zs = a * z.double() - b * eps + c * noise
        zs = torch.cat([orc.remove_mean_with_mask(zs[:, :, :3], nmf.double()), zs[:, :, 3:]], dim=2)
        z = zs.float()
    x, h = orc.final_decode(sd, cfg, z, nm, em, ctx, raws[len(path)], gamma_0=gg[0].expand(B, 1))
    return x, h, z


def check_chain(model, sd, cfg, T, nm, em, ctx, what, **few):
    from hierdiff_amd import paths
    path = paths.build_path(T, few.get("steps"), few.get("spacing") or "uniform", few.get("timesteps"))
    eta = float(few.get("eta", 1.0))
    B, N = nm.shape[:2]
    raws = raw_draws(len(path) + 1, B, N, seed=len(path))
    x, h = model.sample_from_masks(dev(nm), dev(em), dev(ctx), raw_noises=raws, **few)
    with torch.no_grad():
        xo, ho, _ = path_chain_ref(sd, cfg, T, gamma_grid_fp64(model, T), path, eta, nm, em, ctx, raws)
    nmf = nm.float().numpy()
    rx, rh = rel_l2(x.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(h.cpu().numpy(), ho.numpy())
    print(f"{what}: K={len(path) - 1} eta={eta}: x rel_l2 {rx:.2e} h rel_l2 {rh:.2e} (bar {BAR:.0e})")
    assert torch.isfinite(x).all() and torch.isfinite(h).all()
    assert rx < BAR and rh < BAR, (what, rx, rh)


# ----------------------------------------------------------------------------- 7. bit identity at stride 1

def both_loops(model, call):
    """`call()` through the plain loop and, forced, through the path loop on the identity path."""
    model._force_path_loop = False
    plain = call()
    model._force_path_loop = True
    try:
        forced = call()
    finally:
        model._force_path_loop = False
    return plain, forced


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
@pytest.mark.parametrize("graph", [True, False])
def test_identity_path_is_the_plain_loop_bit_for_bit(graph, C_, precision):
    T = 12
    model, _, _ = make_model(64, 2, T, C_=C_, precision=precision)
    model.use_graph = graph
    nm, em = orc.canonical_masks(N_LIST)
    nm = nm.bool()
    B, N = nm.shape[:2]
    ctx = context_for(nm) if C_ else None
    nmd, ctxd = dev(nm), dev(ctx)
    # counter-based noise, steps = T and eta = 1.0 spelled out
    (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_from_masks(nmd, None, ctxd, sample_id_base=17, steps=T, eta=1.0))
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    xd, hd = model.sample_from_masks(nmd, None, ctxd, sample_id_base=17)
    assert torch.equal(x0, xd) and torch.equal(h0, hd)                 # and the keywords' defaults are that same chain
    # fix_noise: one shared row of counter-based noise
    (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_from_masks(nmd, None, ctxd, fix_noise=True, sample_id_base=4))
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    # injected normals, per molecule and shared
    for rows in (None, 1):
        raws = raw_draws(T + 2, B, N, seed=5, rows=rows)
        (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_from_masks(nmd, dev(em), ctxd, fix_noise=rows == 1, raw_noises=raws))
        assert torch.equal(x0, x1) and torch.equal(h0, h1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [True, False])
def test_identity_path_with_pocket_rows_is_the_plain_loop_bit_for_bit(graph, precision):
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict
    H, L, T, P = 64, 2, 10, 6
    cfg = default_config(hidden_nf=H, n_layers=L, timesteps=T)
    cfg["pocket"] = True
    model = DiffusionQM9(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_state_dict(9, 0, H, L, 2, True, 7, 0.02, pocket=True).items()})
    model = model.to(DEV)
    model.dynamics.precision = precision
    model.use_graph = graph
    nm, em = orc.canonical_masks([6, 4, 5])
    B, N = nm.shape[:2]
    g = torch.Generator().manual_seed(2)
    p_nm = torch.ones(B, P, 1, dtype=torch.bool)
    p_nm[1, 4:] = False
    p_em = (p_nm & p_nm.transpose(1, 2)) & ~torch.eye(P, dtype=torch.bool)[None]
    feat = model.pocket_embed(torch.randint(0, 21, (B, P), generator=g).to(DEV)) * dev(p_nm).float()
    pocket = (dev(torch.randn(B, P, 3, generator=g) * p_nm.float()), feat.detach(), dev(p_nm), dev(p_em))
    (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_from_masks(dev(nm.bool()), dev(em), None, sample_id_base=3, pocket=pocket))
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    raws = raw_draws(T + 2, B, N, seed=6)
    (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_from_masks(dev(nm.bool()), dev(em), None, raw_noises=raws, pocket=pocket))
    assert torch.equal(x0, x1) and torch.equal(h0, h1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("r", [1, 3])
def test_identity_path_inpainting_is_the_plain_inpainting_loop_bit_for_bit(r, precision):
    T = 12
    for C_ in (0, 1):
        model, _, _ = make_model(64, 2, T, C_=C_, precision=precision)
        nm, em, fm, xk, hk, ctx = make_case(C_=C_)
        for graph in (True, False):
            model.use_graph = graph
            (x0, h0), (x1, h1) = both_loops(model, lambda: model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), context=dev(ctx),
                                                                                 resamplings=r, sample_id_base=21))
            assert torch.equal(x0, x1) and torch.equal(h0, h1)


# ----------------------------------------------------------------------------- 8. strided ancestral chains vs the oracle

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("few", [dict(steps=50), dict(steps=100), dict(steps=100, spacing="quadratic"),
                                 dict(timesteps=[1000, 999, 700, 650, 400, 399, 398, 120, 30, 7, 1, 0])],
                         ids=["K50", "K100", "K100quadratic", "explicit"])
def test_strided_ancestral_chain_vs_oracle_T1000(few, precision):
    T = 1000
    model, sd, cfg = make_model(64, 2, T, precision=precision)
    nm, em = orc.canonical_masks(N_LIST)
    check_chain(model, sd, cfg, T, nm.bool(), em, None, f"T=1000 H=64 [{precision}]", **few)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
def test_strided_ancestral_chain_vs_oracle_T20_K7(C_, precision):
    T = 20
    model, sd, cfg = make_model(64, 2, T, C_=C_, precision=precision)
    nm, em = orc.canonical_masks(N_LIST)
    ctx = context_for(nm) if C_ else None
    check_chain(model, sd, cfg, T, nm.bool(), em, ctx, f"T=20 H=64 ctx={C_} [{precision}]", steps=7)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eta", [1.0, 0.0])
def test_strided_chain_vs_oracle_production_width(eta, precision):
    T = 1000
    model, sd, cfg = make_model(256, 6, T, precision=precision, seed=21)
    nm, em = orc.canonical_masks([8, 5, 7, 3])
    check_chain(model, sd, cfg, T, nm.bool(), em, None, f"T=1000 H=256 L=6 [{precision}]", steps=50, eta=eta)


# ----------------------------------------------------------------------------- 9. eta < 1

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("few", [dict(steps=50), dict(steps=100, spacing="quadratic")], ids=["K50", "K100quadratic"])
def test_ddim_family_chain_vs_the_fp64_formula(few, eta, precision):
    T = 1000
    model, sd, cfg = make_model(64, 2, T, precision=precision)
    nm, em = orc.canonical_masks(N_LIST)
    check_chain(model, sd, cfg, T, nm.bool(), em, None, f"T=1000 H=64 [{precision}]", eta=eta, **few)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_eta_0_reads_no_normal_on_the_path(precision):
    """Two seeds, the same z_T: z_0 before the decode is the same tensor - and eta = 0.5 is not."""
    T = 40
    model, _, _ = make_model(64, 2, T, precision=precision)
    nm, _ = orc.canonical_masks(N_LIST)
    B, N = nm.shape[:2]
    r = raw_draws(1, B, N, seed=9)[0]
    zT = dev(orc.combined_noise(r[0], r[1], nm.float()))
    out = {}
    for eta in (0.0, 0.5):
        for seed in (1, 2):
            model.seed = seed
            out[eta, seed] = model.path_steps(zT, dev(nm.bool()), steps=10, eta=eta, sample_id_base=5)
    assert torch.equal(out[0.0, 1], out[0.0, 2])
    assert not torch.equal(out[0.5, 1], out[0.5, 2])
    assert torch.isfinite(out[0.0, 1]).all()


# ----------------------------------------------------------------------------- 10. graph replay, its cache

@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replay_equals_plain_launches_and_the_graph_is_cached(precision):
    from hierdiff_amd import _lib
    lib = _lib.load()
    T = 60
    model, _, _ = make_model(64, 2, T, precision=precision)
    nm, _ = orc.canonical_masks(N_LIST)
    nmd = dev(nm.bool())
    B, N = nm.shape[:2]
    builds = lambda: int(lib.hd_path_graph_builds(model.dynamics.topology(nmd, None, B, N).ptr))
    res = {}
    for eta in (1.0, 0.0, 0.5):
        for graph in (True, False):
            model.use_graph = graph
            res[eta, graph] = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, eta=eta)
        assert torch.equal(res[eta, True][0], res[eta, False][0]) and torch.equal(res[eta, True][1], res[eta, False][1]), eta
    model.use_graph = True
    a = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9)
    n0 = builds()
    assert n0 >= 1
    b = model.sample_from_masks(nmd, None, None, sample_id_base=77, steps=9)
    assert builds() == n0, "another sample_id_base must replay the cached graph"
    assert not torch.equal(a[0], b[0])
    a2 = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9)
    assert builds() == n0 and torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=10)
    assert builds() == n0 + 1, "a new path must rebuild the graph"
    # a chain cut into pieces gives the bits of the whole (draws are keyed by the arrival step)
    raw = raw_draws(1, B, N, seed=1)[0]
    zT = dev(orc.combined_noise(raw[0], raw[1], nm.float()))
    whole = model.path_steps(zT, nmd, steps=9, sample_id_base=6)
    cut = model.path_steps(model.path_steps(zT, nmd, steps=9, sample_id_base=6, k_hi=4), nmd, steps=9, sample_id_base=6, k_lo=4)
    assert torch.equal(whole, cut)


def test_path_loops_need_a_schedule_and_a_path():
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _ = make_model(32, 1, 8)
    nm, _ = orc.canonical_masks([4, 3])
    nmd = dev(nm.bool())
    h = model._lib_handle()                      # weights set, no schedule yet
    topo = model.dynamics.topology(nmd, None, 2, 4)
    z = torch.zeros(2, 4, 11, device=DEV)
    ti, si, coef = (C.c_int * 2)(8, 3), (C.c_int * 2)(3, 0), (C.c_float * 8)(*([1.0] * 8))
    assert lib.hd_set_path(h, 2, ti, si, coef, 0, None) == -4 and b"schedule not set" in lib.hd_last_error()
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), None, -1, 0, 1, None, None, 2, 0, 0, 0, None) == -4
    model._schedule()
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), None, -1, 0, 1, None, None, 2, 0, 0, 0, None) == -4
    assert b"path not set" in lib.hd_last_error()
    bad_t = (C.c_int * 2)(9, 3)
    assert lib.hd_set_path(h, 2, bad_t, si, coef, 0, None) == -1
    gap = (C.c_int * 2)(2, 0)
    assert lib.hd_set_path(h, 2, ti, gap, coef, 0, None) == -1                    # transition 1 does not start where 0 arrived
    assert lib.hd_set_path(h, 2, ti, si, coef, 1, None) == 0
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), None, -1, 0, 3, None, None, 2, 0, 0, 0, None) == -1      # k_hi > K
    fm = torch.zeros(8, dtype=torch.uint8, device=DEV)
    args = (h, topo.ptr, z.data_ptr(), None, -1, 0, 2, None, None, 2, 0, 0, 0, fm.data_ptr(), z.data_ptr(), 1, None)
    assert lib.hd_sample_path_inpaint(*args) == -1 and b"ancestral rows only" in lib.hd_last_error()
    assert lib.hd_set_path(h, 2, ti, si, coef, 0, None) == 0
    assert lib.hd_sample_path_inpaint(*args) == -4 and b"without inpainting rows" in lib.hd_last_error()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 11. shard independence

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eta", [1.0, 0.0])
def test_a_shard_with_its_global_ids_gives_its_rows_of_the_whole_batch(eta, precision):
    T, K, B, lo, n = 1000, 100, 256, 96, 32
    model, _, _ = make_model(64, 2, T, precision=precision)
    rng = np.random.default_rng(0)
    sizes = [int(v) for v in rng.integers(3, 13, size=B)]
    sizes[0] = 12                                 # the shard is padded to the batch's width below
    nm, _ = orc.canonical_masks(sizes)
    nm = nm.bool()
    x, h = model.sample_from_masks(dev(nm), None, None, sample_id_base=1000, steps=K, eta=eta)
    xs, hs = model.sample_from_masks(dev(nm[lo:lo + n].contiguous()), None, None, sample_id_base=1000 + lo, steps=K, eta=eta)
    assert torch.equal(x[lo:lo + n], xs) and torch.equal(h[lo:lo + n], hs)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()


# ----------------------------------------------------------------------------- 12. inpainting on a path

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("r", [1, 3])
def test_inpainting_on_a_path(r, precision):
    T, K = 1000, 100
    model, _, _ = make_model(64, 2, T, precision=precision)
    nm, em, fm, xk, hk, _ = make_case(seed=3)
    x, h = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=9, steps=K)
    model.use_graph = False
    xp, hp = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=9, steps=K)
    model.use_graph = True
    assert torch.equal(x, xp) and torch.equal(h, hp)
    xplain, hplain = model.sample_from_masks(dev(nm), None, None, sample_id_base=9, steps=K)
    x, h, xplain, hplain = x.cpu(), h.cpu(), xplain.cpu(), hplain.cpu()
    assert torch.isfinite(x).all() and torch.isfinite(h).all()
    assert torch.equal(h[fm.expand_as(h)], hk[fm.expand_as(h)])
    for b, k in enumerate(N_FIXED):
        if k == 0 and r == 1:                    # no fixed nodes, one round: the plain path sample
            assert torch.equal(x[b], xplain[b]) and torch.equal(h[b], hplain[b])
        if k < 2:
            continue
        got = x[b, :k, None, :] - x[b, None, :k, :]              # a pure translation of the input (the existing inpaint test's bar)
        want = xk[b, :k, None, :] - xk[b, None, :k, :]
        mag = max(float(x[b, :k].abs().max()), float(xk[b, :k].abs().max()))
        assert float((got - want).abs().max()) <= 2 * float(np.spacing(np.float32(mag))), b
    assert torch.all(x[~nm.expand_as(x)] == 0) and torch.all(h[~nm.expand_as(h)] == 0)
    # centre of gravity of z_0 (before the decode), the loop's invariant: the existing check's bar
    model.debug_checks = True
    xd, hd = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=9, steps=K)
    model.debug_checks = False
    assert torch.equal(xd.cpu(), x) and torch.equal(hd.cpu(), h)
    free_only = [b for b, k in enumerate(N_FIXED) if k == 0]
    cog = x[free_only].sum(1).abs().max()
    print(f"inpaint on a path r={r} [{precision}]: |centre of gravity| of the molecules without fixed nodes {float(cog):.2e}")
    assert float(cog) < 1e-3


# ----------------------------------------------------------------------------- 13. properties

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eta", [1.0, 0.5, 0.0])
def test_outputs_are_finite_masked_and_mean_free(eta, precision):
    T = 200
    model, _, _ = make_model(64, 2, T, precision=precision)
    nm, _ = orc.canonical_masks(N_LIST)
    nm = nm.bool()
    nmd = dev(nm)
    B, N = nm.shape[:2]
    for spacing in ("uniform", "quadratic"):
        raw = raw_draws(1, B, N, seed=4)[0]
        z0 = model.path_steps(dev(orc.combined_noise(raw[0], raw[1], nm.float())), nmd, steps=25, eta=eta, spacing=spacing).cpu()
        assert torch.isfinite(z0).all() and torch.all(z0[~nm.expand_as(z0)] == 0)
        scale = max(1.0, float(z0[:, :, :3].abs().max()))
        assert float(z0[:, :, :3].sum(1).abs().max()) < 1e-3 * scale
        x, h = model.sample_from_masks(nmd, None, None, steps=25, eta=eta, spacing=spacing)
        x, h = x.cpu(), h.cpu()
        assert torch.isfinite(x).all() and torch.isfinite(h).all()
        assert torch.all(x[~nm.expand_as(x)] == 0) and torch.all(h[~nm.expand_as(h)] == 0)
        assert float(x.sum(1).abs().max()) < 1e-3 * max(1.0, float(x.abs().max()))
    # fix_noise: equal masks -> every molecule of the batch is the same sample
    full = dev(torch.ones(4, 6, 1, dtype=torch.bool))
    for graph in (True, False):
        model.use_graph = graph
        x, h = model.sample_from_masks(full, None, None, fix_noise=True, steps=25, eta=eta)
        assert all(torch.equal(x[0], x[b]) and torch.equal(h[0], h[b]) for b in range(1, 4))
    model.use_graph = True


def test_list_level_entry_points_take_the_keywords():
    model, _, _ = make_model(32, 1, 30)
    torch.manual_seed(0)
    a = model.sample(3, DEV, sample_id_base=2, steps=5, eta=0.0)
    torch.manual_seed(0)
    model.sample_steps, model.sample_eta = 5, 0.0                  # the same through the attributes
    b = model.sample(3, DEV, sample_id_base=2)
    model.sample_steps, model.sample_eta = None, 1.0
    assert all(torch.equal(p["x"], q["x"]) and torch.equal(p["h"], q["h"]) for p, q in zip(a, b))
    torch.manual_seed(0)
    res, _ = model.sample_batches(2, 2, DEV, steps=5, spacing="quadratic")
    assert len(res) == 4 and all(torch.isfinite(r["x"]).all() for r in res)
    known = [{"x": a[0]["x"][:2], "h": a[0]["h"][:2]}]
    grown = model.sample_grow(known, [5], DEV, steps=6)
    assert grown[0]["x"].shape == (5, 3) and torch.equal(grown[0]["h"][:2], known[0]["h"])


# ----------------------------------------------------------------------------- 14. every captured loop on one topology

def test_the_loops_share_a_topology_without_evicting_each_other():
    """The every-step loop, a strided path, the same path guided, the every-step inpainting loop (r = 2) and the scoring terms, twice
    over on one handle and one topology: each keeps its own graph slot (one instantiation each) while all of them move the handle's
    one set of replay words, and every output is the bits of plain launches on a fresh topology."""
    from hierdiff_amd import _lib
    lib = _lib.load()
    T = 8
    nm, _, fm, xk, hk, ctx = make_case(n_list=[5, 3, 5], n_fixed=[2, 0, 3], C_=1)       # B = 3, N = 5, one molecule shorter than N
    B, N = nm.shape[:2]
    xh, _, _ = orc.random_inputs([5, 3, 5], 8, seed=3)
    nmd, ctxd = dev(nm), dev(ctx)
    x_in, h_in = dev(xh[:, :, :3].contiguous()), dev(xh[:, :, 3:].contiguous())
    path = dict(steps=3, eta=0.5, sample_id_base=7)

    def one_round(model, graph):
        model.use_graph = graph
        out = list(model.sample_from_masks(nmd, None, ctxd, sample_id_base=5))
        out += model.sample_from_masks(nmd, None, ctxd, **path)
        out += model.sample_from_masks(nmd, None, ctxd, guidance_scale=2.5, guidance_rescale=0.7, **path)
        out += model.sample_inpaint(nmd, dev(fm), dev(xk), dev(hk), context=ctxd, resamplings=2, sample_id_base=9)
        nll, (_, e) = model.nll_full(x_in, h_in, nmd, None, ctxd, sample_id_base=11, return_terms=True, use_graph=graph)
        return out + [nll, e]

    model, _, _ = make_model(32, 1, T, C_=1)
    first, second = one_round(model, True), one_round(model, True)
    assert len(first) == 10 and all(torch.isfinite(a).all() for a in first)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"output {i}: the second round differs from the first"
    topo = model.dynamics.topology(nmd, None, B, N).ptr
    builds = (int(lib.hd_path_graph_builds(topo)), int(lib.hd_guided_graph_builds(topo)), int(lib.hd_nll_graph_builds(topo)))
    assert builds == (1, 1, 1), builds
    other, _, _ = make_model(32, 1, T, C_=1)                  # a fresh handle and topology, plain launches
    for i, (a, b) in enumerate(zip(first, one_round(other, False))):
        assert torch.equal(a, b), f"output {i}: graph replay differs from plain launches"
    topo = other.dynamics.topology(nmd, None, B, N).ptr
    assert (lib.hd_path_graph_builds(topo), lib.hd_guided_graph_builds(topo), lib.hd_nll_graph_builds(topo)) == (0, 0, 0)
