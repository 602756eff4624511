"""GPU tier (-m gpu) of editing given molecules: hd_diffuse / hd_set_path_up / hd_slerp and DiffusionQM9.diffuse / encode /
sample_from_latent / slerp / vary / interpolate against the CPU restatement tests/edit_reference.py, and their bit-level
guarantees (sharding, split chains, graph replay and its cache, endpoints of the interpolation).

Bar: rel-L2 <= 1e-4, the project's parity bar; tests/test_edit_cpu.py shows that the float32 restatement stays a tenth of it from the
float64 one on the same cases.  Shapes: T = 20, H = 32, L = 2, B = 3, N = 7 with node counts (7, 4, 1) - the one-node molecule has
x noise that is exactly 0 after the mean removal - and one case at N = 30 with counts (30, 17), where N * D = 330 > 256 and the
strided loops of k_diffuse and k_slerp wrap.  Measured values are printed."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from hierdiff_amd import paths
from tests import edit_reference as er
from tests.helpers import rel_l2
from tests.test_gpu_parity import PRECISIONS, build_diffusion
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-4
_MODELS = {}


def dev(t):
    return None if t is None else t.to(DEV)


def setup(case, C_=0, precision="fp32", T=None):
    """(model, sd_np, oracle cfg, gamma grid) for a case; one model per configuration and module."""
    T = case["T"] if T is None else T
    key = (case["H"], case["L"], T, C_)
    if key not in _MODELS:
        sd_np, cfg = er.weights(case["H"], case["L"], C_)
        model = build_diffusion(sd_np, case["H"], case["L"], C_=C_, T=T)
        model.seed = SEED
        _MODELS[key] = (model, sd_np, cfg, gamma_grid_fp64(model, T))
    model, sd_np, cfg, gg = _MODELS[key]
    model.dynamics.precision = precision
    model.use_graph = True
    model.seed = SEED
    return model, sd_np, cfg, gg


def topo_of(model, nm):
    return model.dynamics.topology(dev(nm), None, nm.shape[0], nm.shape[1])


# ----------------------------------------------------------------------------- 1 - 4. diffuse

@pytest.mark.parametrize("case", [er.MAIN, er.WRAP], ids=["main", "wrap"])
def test_diffuse_with_injected_normals_matches_the_restatement(case):
    model, _, _, gg = setup(case)
    x, h, nm, _, _ = er.molecules(case["n_list"])
    B, N = nm.shape[:2]
    for rows in (None, 1):
        raw = er.raw_draws(1, B, N, seed=11, rows=rows)[0]
        for t in (12, 0, case["T"]):
            z = model.diffuse(dev(x), dev(h), dev(nm), t, raw_noise=raw, fix_noise=rows == 1).cpu()
            ref = er.diffuse_ref(x, h, nm, gg[t], raw)
            r = rel_l2(z.numpy(), ref.numpy())
            print(f"diffuse N={N} t={t} rows={rows}: rel_l2 {r:.2e} (bar {BAR:.0e})")
            assert r <= BAR, (t, rows, r)
            assert torch.all(z[~nm.expand_as(z)] == 0)


@pytest.mark.parametrize("case", [er.MAIN, er.WRAP], ids=["main", "wrap"])
def test_diffuse_from_the_generator_is_hd_noise_at_draw_0_and_shards_reproduce(case):
    """Each element within 2^-23 (|alpha xh| + |sigma eps|) of alpha xh + sigma eps formed in torch from hd_noise(draw 0): the kernel
    may contract the sum into one FMA, torch multiplies, rounds and adds.  x is made of quarter integers so that its re-centring is
    the same fp32 value on the host and on the device."""
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _, _ = setup(case)
    x, h, nm, _, _ = er.molecules(case["n_list"])
    x = torch.round(x * 4) / 4
    B, N = nm.shape[:2]
    t, base = 12, 100
    z = model.diffuse(dev(x), dev(h), dev(nm), t, sample_id_base=base)
    eps = torch.empty_like(z)
    handle, topo = model._lib_handle(), topo_of(model, nm)
    _lib.check(lib.hd_noise(handle, topo.ptr, None, None, B, model.seed, base, 0, 0, eps.data_ptr(), None), "hd_noise")
    alpha, sigma = model._alpha_sigma(model._schedule(rows=B), t)
    xh = dev(er.normalised_data(x, h, nm))
    a_xh, s_eps = torch.tensor(alpha, device=DEV) * xh, torch.tensor(sigma, device=DEV) * eps
    tol = 2.0 ** -23 * (a_xh.abs() + s_eps.abs())
    diff = (z - (a_xh + s_eps)).abs()
    print(f"diffuse N={N}: worst |z - (alpha xh + sigma eps)| / tolerance {float((diff / tol.clamp(min=1e-30)).max()):.2f}")
    assert bool((diff <= tol).all())
    # outputs: masked entries exactly 0, the x part mean-free (each of the <= N summands is rounded to 2^-24 of max |z|)
    zc = z.cpu()
    assert torch.isfinite(zc).all() and torch.all(zc[~nm.expand_as(zc)] == 0)
    assert float(zc[:, :, :3].sum(1).abs().max()) <= N * 2.0 ** -22 * float(zc.abs().max())
    if case is er.MAIN:                            # one valid node: the x noise is exactly 0 after the mean removal
        assert torch.equal(zc[2, 0, :3], (alpha * xh[2, 0, :3]).cpu())
    # a shard with its global ids gives its rows of the whole batch; other seeds and ids give other noise
    zs = model.diffuse(dev(x[1:]), dev(h[1:]), dev(nm[1:]), t, sample_id_base=base + 1)
    assert torch.equal(z[1:], zs)
    assert not torch.equal(z, model.diffuse(dev(x), dev(h), dev(nm), t, sample_id_base=base + 1))
    assert not torch.equal(z, model.diffuse(dev(x), dev(h), dev(nm), t, sample_id_base=base, seed=SEED + 1))
    zf = model.diffuse(dev(x), dev(h), dev(nm), case["T"], sample_id_base=base, fix_noise=True).cpu()
    assert torch.isfinite(zf).all() and torch.all(zf[~nm.expand_as(zf)] == 0)


# ----------------------------------------------------------------------------- 5 - 7. sample_from_latent

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
@pytest.mark.parametrize("graph", [True, False])
def test_sample_from_latent_at_T_on_the_identity_path_is_sample_from_masks(graph, C_, precision):
    model, _, _, _ = setup(er.MAIN, C_, precision)
    model.use_graph = graph
    x, h, nm, _, ctx = er.molecules(er.MAIN["n_list"], C_=C_)
    z = model.diffuse(dev(x), dev(h), dev(nm), er.MAIN["T"], sample_id_base=7)
    xa, ha = model.sample_from_latent(z, dev(nm), None, dev(ctx), sample_id_base=7)
    xb, hb = model.sample_from_masks(dev(nm), None, dev(ctx), sample_id_base=7, z_init=z)
    assert torch.equal(xa, xb) and torch.equal(ha, hb)
    assert torch.isfinite(xa).all() and torch.isfinite(ha).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
@pytest.mark.parametrize("eta", [1.0, 0.0])
def test_partial_chain_vs_the_restatement(eta, C_, precision):
    for case in ((er.MAIN, er.WRAP) if C_ == 0 else (er.MAIN,)):
        model, sd_np, cfg, gg = setup(case, C_, precision)
        T = case["T"]
        x, h, nm, em, ctx = er.molecules(case["n_list"], C_=C_)
        B, N = nm.shape[:2]
        z12 = er.diffuse_ref(x, h, nm, gg[12], er.raw_draws(1, B, N, seed=11)[0])
        raws = er.raw_draws(6, B, N, seed=12)
        path = paths.partial_path(T, 12, 5)
        for graph in (True, False):
            model.use_graph = graph
            xg, hg = model.sample_from_latent(dev(z12), dev(nm), dev(em), dev(ctx), t_start=12, steps=5, eta=eta, raw_noises=raws)
            if graph:
                first = (xg, hg)
        assert torch.equal(first[0], xg) and torch.equal(first[1], hg)
        xo, ho, _ = er.partial_chain_ref(er.RefNet(sd_np, cfg, T, nm, em, ctx), gg, path, eta, z12, nm, raws)
        nmf = nm.float().numpy()
        rx, rh = rel_l2(xg.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(hg.cpu().numpy(), ho.numpy())
        print(f"partial chain N={N} ctx={C_} eta={eta} [{precision}]: x rel_l2 {rx:.2e} h rel_l2 {rh:.2e} (bar {BAR:.0e})")
        assert rx <= BAR and rh <= BAR, (N, rx, rh)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_partial_chain_cut_into_pieces_gives_the_bits_of_the_whole(precision):
    model, _, _, _ = setup(er.MAIN, 0, precision)
    x, h, nm, _, _ = er.molecules(er.MAIN["n_list"])
    z = model.diffuse(dev(x), dev(h), dev(nm), 12, sample_id_base=3)
    for eta in (1.0, 0.5):
        kw = dict(t_start=12, steps=5, eta=eta, sample_id_base=3)
        whole = model.latent_steps(z, dev(nm), **kw)
        cut = model.latent_steps(model.latent_steps(z, dev(nm), k_hi=2, **kw), dev(nm), k_lo=2, **kw)
        assert torch.equal(whole, cut), eta
        assert not torch.equal(whole, model.latent_steps(z, dev(nm), **dict(kw, sample_id_base=4)))


# ----------------------------------------------------------------------------- 8 - 10. encode

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_,T,K", [(0, 20, 20), (1, 20, 20), (0, 20, 7), (1, 20, 7), (0, 1000, 50)])
def test_encode_vs_the_restatement(C_, T, K, precision):
    for case in ((er.MAIN, er.WRAP) if (C_, T, K) == (0, 20, 7) else (er.MAIN,)):
        model, sd_np, cfg, gg = setup(case, C_, precision, T=T)
        x, h, nm, em, ctx = er.molecules(case["n_list"], C_=C_)
        z = model.encode(dev(x), dev(h), dev(nm), dev(em), dev(ctx), steps=K).cpu()
        ref = er.encode_ref(er.RefNet(sd_np, cfg, T, nm, em, ctx), gg, paths.ascending_path(T, T, K), er.normalised_data(x, h, nm), nm)
        r = rel_l2(z.numpy(), ref.numpy())
        print(f"encode N={nm.shape[1]} ctx={C_} T={T} K={K} [{precision}]: rel_l2 {r:.2e} (bar {BAR:.0e})")
        assert r <= BAR, r
        assert torch.isfinite(z).all() and torch.all(z[~nm.expand_as(z)] == 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_encode_draws_nothing_replays_a_cached_graph_and_shares_the_tables_safely(precision):
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _, _ = setup(er.MAIN, 0, precision)
    x, h, nm, _, _ = er.molecules(er.MAIN["n_list"])
    xd, hd, nmd = dev(x), dev(h), dev(nm)
    builds = lambda: int(lib.hd_path_graph_builds(topo_of(model, nm).ptr))
    s0 = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=5)
    n0 = builds()
    z1 = model.encode(xd, hd, nmd, steps=7)
    assert builds() == n0 + 1, "an ascending path must rebuild the captured transition"
    model.seed = SEED + 5
    z2 = model.encode(xd, hd, nmd, steps=7)
    model.seed = SEED
    assert torch.equal(z1, z2), "encode draws nothing: the seed must not matter"
    assert builds() == n0 + 1, "a second call must replay the cached graph"
    model.use_graph = False
    z3 = model.encode(xd, hd, nmd, steps=7)
    model.use_graph = True
    assert torch.equal(z1, z3)
    # the two directions share the handle's tables: each must find its own rows again
    s1 = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=5)
    assert builds() == n0 + 2, "a descending path set afterwards rebuilds the graph once"
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
    assert torch.equal(z1, model.encode(xd, hd, nmd, steps=7)) and builds() == n0 + 3
    # a shard gives its rows of the whole batch
    assert torch.equal(z1[1:], model.encode(xd[1:], hd[1:], nmd[1:], steps=7))
    assert not torch.equal(z1, model.encode(xd, hd, nmd, steps=7, t_end=12))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
def test_round_trip_vs_the_restatement(C_, precision):
    """encode, then sample_from_latent(eta = 0) on the same points, against the restatement's round trip at (T = 20, K = 7) (the
    case at which tests/test_edit_cpu.py shows the bar to be passable).  The distance to the input is a property of the weights: it
    is printed, not asserted."""
    case, K = er.MAIN, 7
    model, sd_np, cfg, gg = setup(case, C_, precision)
    T = case["T"]
    x, h, nm, em, ctx = er.molecules(case["n_list"], C_=C_)
    B, N = nm.shape[:2]
    raws = er.raw_draws(K + 1, B, N, seed=13)
    z = model.encode(dev(x), dev(h), dev(nm), dev(em), dev(ctx), steps=K)
    xg, hg = model.sample_from_latent(z, dev(nm), dev(em), dev(ctx), steps=K, eta=0.0, raw_noises=raws)
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    up = paths.ascending_path(T, T, K)
    z_ref = er.encode_ref(net, gg, up, er.normalised_data(x, h, nm), nm)
    xo, ho, _ = er.partial_chain_ref(net, gg, up[::-1], 0.0, z_ref, nm, raws)
    nmf = nm.float().numpy()
    rx, rh = rel_l2(xg.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(hg.cpu().numpy(), ho.numpy())
    x_in = er.normalised_data(x, h, nm)
    dx = rel_l2(xg.cpu().numpy() * nmf, x_in[:, :, :3].numpy())
    dh = rel_l2(hg.cpu().numpy(), x_in[:, :, 3:].numpy())
    print(f"round trip ctx={C_} K={K} [{precision}]: x rel_l2 {rx:.2e} h rel_l2 {rh:.2e} (bar {BAR:.0e}); "
          f"distance to the input (weights' property, synthetic here): x {dx:.2e} h {dh:.2e}")
    assert rx <= BAR and rh <= BAR, (rx, rh)


# ----------------------------------------------------------------------------- 11. slerp

@pytest.mark.parametrize("case", [er.MAIN, er.WRAP], ids=["main", "wrap"])
def test_slerp_endpoints_interior_and_degenerate_cases(case):
    """Interior frames against the float64 `slerp_ref` at rel-L2 <= 1e-6.  The kernel forms the sums, the angle and the two weights
    in double and rounds the weights to fp32 (2^-24 each); an output element is fl(wa za + wb zb) with at most three more fp32
    roundings, so |error| <= 4 * 2^-24 (|wa za| + |wb zb|) per element and, per molecule, rel-L2 <= 2^-22 (wa |za| + wb |zb|) / |out|.
    For |za| ~ |zb| that ratio is (wa + wb) = cos((1/2 - lam) theta) / cos(theta / 2) <= 1 / cos(theta / 2), about 1.5 for the
    near-orthogonal random latents used here: 3.6e-7, below the bar."""
    model, _, _, _ = setup(case)
    _, _, nm, _, _ = er.molecules(case["n_list"])
    B, N = nm.shape[:2]
    g = torch.Generator().manual_seed(4)
    a = torch.randn(B, N, 11, generator=g) * nm
    b = torch.randn(B, N, 11, generator=g) * nm
    lam = [0.0, 0.25, 0.5, 0.9, 1.0]
    out = model.slerp(dev(a), dev(b), lam, dev(nm)).cpu()
    assert tuple(out.shape) == (5, B, N, 11)
    assert torch.equal(out[0], a) and torch.equal(out[4], b)
    assert torch.all(out[:, ~nm.reshape(B, N)] == 0) and torch.isfinite(out).all()
    ref = er.slerp_ref(a.numpy(), b.numpy(), lam, nm.numpy())
    for l in (1, 2, 3):
        for i in range(B):
            r = rel_l2(out[l, i].numpy(), ref[l, i])
            print(f"slerp N={N} lam={lam[l]} molecule {i}: rel_l2 {r:.2e} (bar 1e-6)")
            assert r <= 1e-6, (l, i, r)
    # a == b, and nearly parallel latents (sin theta below the documented 1e-6: the linear form)
    same = model.slerp(dev(a), dev(a), lam, dev(nm)).cpu()
    assert torch.equal(same[0], a) and torch.equal(same[4], a)
    assert all(rel_l2(same[l].numpy(), a.numpy()) <= 1e-6 for l in (1, 2, 3))
    near = a + 1e-7 * b
    o = model.slerp(dev(a), dev(near), [0.5], dev(nm)).cpu()
    r = rel_l2(o[0].numpy(), er.slerp_ref(a.numpy(), near.numpy(), [0.5], nm.numpy())[0])
    print(f"slerp N={N} nearly parallel: rel_l2 {r:.2e}")
    assert r <= 1e-6 and torch.all(o[:, ~nm.reshape(B, N)] == 0)
    # more frames than one launch carries
    many = [i / 69 for i in range(70)]
    om = model.slerp(dev(a), dev(b), many, dev(nm)).cpu()
    assert torch.equal(om[0], a) and torch.equal(om[69], b)
    assert rel_l2(om[66].numpy(), er.slerp_ref(a.numpy(), b.numpy(), [many[66]], nm.numpy())[0]) <= 1e-6


# ----------------------------------------------------------------------------- 12 - 13. list level and CLI

def _samples(sizes, seed=6):
    g = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(n, 3, generator=g), "h": torch.randn(n, 8, generator=g)} for n in sizes]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_interpolate_ends_in_the_reconstructions_of_its_inputs(precision):
    model, _, _, _ = setup(er.MAIN, 0, precision)
    a, b = _samples([5, 5])
    L = 4
    frames = model.interpolate(a, b, L, DEV, steps=7)
    assert len(frames) == L
    nm = torch.ones(1, 5, 1, dtype=torch.bool, device=DEV)
    for mol, fr in ((a, frames[0]), (b, frames[L - 1])):
        xc = mol["x"] - mol["x"].mean(0, keepdim=True)
        z = model.encode(dev(xc[None]), dev(mol["h"][None]), nm, steps=7)
        x, h = model.sample_from_latent(z, nm, steps=7, eta=0.0, fix_noise=True)
        assert torch.equal(x[0].cpu(), fr["x"]) and torch.equal(h[0].cpu(), fr["h"])
    for fr in frames:
        assert fr["x"].shape == (5, 3) and fr["h"].shape == (5, 8)
        assert torch.isfinite(fr["x"]).all() and torch.isfinite(fr["h"]).all()
        assert float(fr["x"].sum(0).abs().max()) <= 1e-4 * max(1.0, float(fr["x"].abs().max()))
    assert not torch.equal(frames[1]["x"], frames[2]["x"])


def test_vary_ids_follow_the_formula_and_the_cli_runs(tmp_path):
    from hierdiff_amd import sampler
    model, _, _, _ = setup(er.MAIN)
    mols = _samples([4, 2, 5])
    out = model.vary(mols, DEV, 12, n_variants=2, batch_size=4, sample_id_base=50, steps=5)
    assert len(out) == 6
    assert [tuple(o["x"].shape) for o in out] == [(4, 3), (4, 3), (2, 3), (2, 3), (5, 3), (5, 3)]
    assert all(torch.isfinite(o["x"]).all() and torch.isfinite(o["h"]).all() for o in out)
    assert not torch.equal(out[0]["x"], out[1]["x"])
    i, v = 1, 1                                   # variant v of input i alone, under its documented id
    alone = model.vary([mols[i]], DEV, 12, n_variants=1, sample_id_base=50 + i * 2 + v, steps=5)
    assert torch.equal(alone[0]["x"], out[i * 2 + v]["x"]) and torch.equal(alone[0]["h"], out[i * 2 + v]["h"])
    # the CLI, end to end on a tiny random-init model
    src, res = tmp_path / "mols.pkl", tmp_path / "out.pkl"
    sampler.write_results(str(src), _samples([4, 4, 3, 3]))
    from hierdiff_amd.weights import synthetic_state_dict
    ck = tmp_path / "diffusion.ckpt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(w.copy()) for k, w in synthetic_state_dict(9, 0, 32, 1, 2, True, 12, 0.02).items()}}, ck)
    tiny = ["--checkpoint", str(ck), "--hidden-nf", "32", "--n-layers", "1", "--timesteps", "10", "--out", str(res)]
    assert sampler.main(["--vary", str(src), "--t-start", "6", "--variants", "2", "--steps", "3", "--eta", "0.5"] + tiny) == 0
    got = pickle.load(open(res, "rb"))[0]
    assert len(got) == 8 and [g["x"].shape[0] for g in got] == [4, 4, 4, 4, 3, 3, 3, 3]
    assert sampler.main(["--interpolate", str(src), "--frames", "3", "--steps", "4"] + tiny) == 0
    got = pickle.load(open(res, "rb"))[0]
    assert len(got) == 6 and all(torch.isfinite(g["x"]).all() for g in got)      # pairs (0,1) and (2,3); (1,2) differs in size


# ----------------------------------------------------------------------------- 14. restrictions

def test_entry_points_refuse_what_the_header_says_they_refuse():
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _, _ = setup(er.MAIN)
    _, _, nm, _, _ = er.molecules(er.MAIN["n_list"])
    B, N = nm.shape[:2]
    h = model._lib_handle()
    model._schedule(rows=B)
    model.__dict__["_path_cache"] = None          # this test uploads paths behind the model's back
    topo = topo_of(model, nm)
    z = torch.zeros(B, N, 11, device=DEV)
    u, v = (C.c_int * 2)(0, 8), (C.c_int * 2)(8, 20)
    coef = (C.c_float * 8)(1.0, 0.1, 0.0, 0.0, 1.0, 0.1, 0.0, 0.0)
    noisy = (C.c_float * 8)(1.0, 0.1, 0.0, 0.0, 1.0, 0.1, 0.2, 0.0)
    assert lib.hd_set_path_up(h, 2, u, v, noisy) == -1 and b"draws nothing" in lib.hd_last_error()
    assert lib.hd_set_path_up(h, 2, v, u, coef) == -1                               # a descending pair
    assert lib.hd_set_path_up(h, 2, u, (C.c_int * 2)(8, 21), coef) == -1            # beyond T
    assert lib.hd_set_path(h, 2, u, v, coef, 1, None) == -1 and b"s_idx[k] < t_idx[k]" in lib.hd_last_error()
    assert lib.hd_set_path_up(h, 2, u, v, coef) == 0
    fm = torch.zeros(B * N, dtype=torch.uint8, device=DEV)
    args = (h, topo.ptr, z.data_ptr(), None, -1, 0, 2, None, None, B, 0, 0, 0, fm.data_ptr(), z.data_ptr(), 1, None)
    assert lib.hd_sample_path_inpaint(*args) == -1 and b"ascends" in lib.hd_last_error()
    raw = torch.zeros(B, N, 8, device=DEV)
    d_args = lambda rx, rh, rows: (h, topo.ptr, z.data_ptr(), 1.0, 0.5, rx, rh, rows, 0, 0, 0, 0, z.data_ptr(), None)
    assert lib.hd_diffuse(*d_args(raw.data_ptr(), None, B)) == -1 and b"go together" in lib.hd_last_error()
    assert lib.hd_diffuse(*d_args(None, None, 2)) == -1 and b"noise_rows" in lib.hd_last_error()
    lam = (C.c_float * 1)(0.5)
    out = torch.zeros(2, B, N, 11, device=DEV)
    assert lib.hd_slerp(h, topo.ptr, z.data_ptr(), z.data_ptr(), lam, 0, out.data_ptr(), None) == -1
    assert lib.hd_slerp(h, topo.ptr, z.data_ptr(), z.data_ptr(), lam, 1, z.data_ptr(), None) == -1 and b"alias" in lib.hd_last_error()
    assert lib.hd_slerp(h, topo.ptr, out[1].data_ptr(), z.data_ptr(), lam, 2, out.data_ptr(), None) == -1       # out overlaps za
    torch.cuda.synchronize()
    model.__dict__["_path_cache"] = None
