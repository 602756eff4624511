"""GPU tier (-m gpu) of second-order multistep sampling (solver="dpm2m"; hd_set_path_multistep, hd_multistep_step): the kernel
against float64, its bit identity with the eta = 0 update where c2 = 0, the convergence order on the analytic model through the
kernel, chains against the float64 reference (tests/solver_reference.py), and the loop's reproducibility: graph replay, split
ranges, shards, guidance.

Bars: 1e-5 relative L2 for the single kernel (the bar of the small elementwise kernels, tests/test_gpu_loss_kernels.py); 1e-3
relative L2 on the final x and h of a chain (`BAR` of tests/test_gpu_fewstep.py, the bar of compounded chains).  Measured values
are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests import solver_reference as sr
from tests.helpers import rel_l2
from tests.test_gpu_fewstep import BAR, N_LIST, context_for, dev, make_model, raw_draws
from tests.test_gpu_parity import PRECISIONS
from tests.test_inpaint_cpu import gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, L = 32, 2
KERNEL_BAR = 1e-5
MASKS = {"uneven": N_LIST, "one_node": [4, 1, 6], "wide": [30, 17]}     # N = 30: 330 elements, more than the 256 threads


def masks(name):
    nm, em = orc.canonical_masks(MASKS[name])
    return nm.bool(), em


def f32(row):
    return [float(np.float32(v)) for v in row]


def random_state(nm, seed, centred=True):
    """[B,N,11] normals, masked; the x part mean-free over the valid nodes when `centred`."""
    g = torch.Generator().manual_seed(seed)
    B, N = nm.shape[:2]
    rx, rh = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g)
    if centred:
        return orc.combined_noise(rx, rh, nm.float())
    return torch.cat([rx, rh], dim=2) * nm.float()


def step_on_device(lib, h, topo, row, zt, eps, x_prev, in_place=False):
    """hd_multistep_step -> (x^_k, z_s) on the device."""
    zt = zt.clone() if in_place else zt
    x_out = x_prev.clone() if (in_place and x_prev is not None) else torch.full_like(zt, float("nan"))
    zs = zt if in_place else torch.full_like(zt, float("nan"))
    xp = x_out if (in_place and x_prev is not None) else x_prev
    rc = lib.hd_multistep_step(h, topo.ptr, zt.data_ptr(), eps.data_ptr(), (C.c_float * 5)(*row), None if xp is None else xp.data_ptr(),
                               x_out.data_ptr(), zs.data_ptr(), None)
    assert rc == 0, lib.hd_last_error()
    return x_out, zs


@pytest.fixture(scope="module")
def small():
    from hierdiff_amd import _lib
    model, _, _ = make_model(H, L, 20)
    return _lib.load(), model, model._lib_handle()


# ----------------------------------------------------------------------------- B1. the kernel against float64

@pytest.mark.parametrize("name", list(MASKS))
def test_kernel_against_float64(small, name):
    lib, model, h = small
    nm, _ = masks(name)
    B, N = nm.shape[:2]
    topo = model.dynamics.topology(dev(nm), None, B, N)
    gg = gamma_grid_fp64(model, 20)
    rows = sr.multistep_rows(gg, sr.uniform_path(20, 7), lower_order_final=False)
    zt, eps, xp = random_state(nm, 1), random_state(nm, 2, centred=False), random_state(nm, 3)
    for k in (0, 3, 6):
        row = f32(rows[k])
        assert (row[2] == 0.0) == (k == 0)
        for in_place in (False, True):
            xk, zs = step_on_device(lib, h, topo, row, dev(zt), dev(eps), None if k == 0 else dev(xp), in_place)
            xo, zo = sr.step_ref(row, zt, eps, None if k == 0 else xp, nm)
            xk, zs = xk.cpu(), zs.cpu()
            ex, ez = rel_l2(xk.numpy(), xo.numpy()), rel_l2(zs.numpy(), zo.numpy())
            print(f"hd_multistep_step [{name}] row {k} in_place={in_place}: x^ rel_l2 {ex:.2e} z_s rel_l2 {ez:.2e} (bar {KERNEL_BAR:.0e})")
            assert ex < KERNEL_BAR and ez < KERNEL_BAR
            for v in (xk, zs):
                assert torch.isfinite(v).all() and torch.all(v[~nm.expand_as(v)] == 0)
                assert float(v[:, :, :3].sum(1).abs().max()) < 1e-3 * max(1.0, float(v[:, :, :3].abs().max()))
    # a row with c2 != 0 needs the history; overlapping outputs are refused
    z = dev(zt)
    bad = lib.hd_multistep_step(h, topo.ptr, z.data_ptr(), dev(eps).data_ptr(), (C.c_float * 5)(*f32(rows[3])), None,
                                torch.empty_like(z).data_ptr(), torch.empty_like(z).data_ptr(), None)
    assert bad == -1 and b"needs x_prev" in lib.hd_last_error()
    bad = lib.hd_multistep_step(h, topo.ptr, z.data_ptr(), dev(eps).data_ptr(), (C.c_float * 5)(*f32(rows[0])), None,
                                z.data_ptr(), z.data_ptr(), None)
    assert bad == -1 and b"alias" in lib.hd_last_error()


# ----------------------------------------------------------------------------- B2. bit identity with the first-order update

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [True, False])
def test_rows_without_correction_give_the_bits_of_eta_0(graph, precision):
    from hierdiff_amd import _lib, paths
    lib = _lib.load()
    T, K = 40, 9
    model, _, _ = make_model(H, L, T, precision=precision)
    model.use_graph = graph
    for name in MASKS:
        nm, _ = masks(name)
        nmd = dev(nm)
        B, N = nm.shape[:2]
        # one transition: the first row has no history
        a = model.sample_from_masks(nmd, None, None, sample_id_base=3, timesteps=[T, 0], eta=0.0)
        b = model.sample_from_masks(nmd, None, None, sample_id_base=3, timesteps=[T, 0], solver="dpm2m")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        # K transitions with every c2 forced to 0 at the C ABI
        zT = dev(random_state(nm, 5))
        want = model.path_steps(zT, nmd, steps=K, eta=0.0)
        hnd, tabs = model._lib_handle(), model._schedule(rows=B)
        pt = paths.path_tables(tabs["gamma"], paths.uniform_path(T, K), solver="dpm2m")
        coef = pt["coef"].clone()
        assert bool((coef[1:-1, 2] != 0).all())
        coef[:, 2] = 0.0
        ti, si, cf = (np.ascontiguousarray(v.numpy()) for v in (pt["t_idx"], pt["s_idx"], coef))
        model._path_cache = None                      # the handle's path is set behind the model's back
        assert lib.hd_set_path_multistep(hnd, K, ti.ctypes.data_as(C.POINTER(C.c_int)), si.ctypes.data_as(C.POINTER(C.c_int)),
                                         cf.ctypes.data_as(C.POINTER(C.c_float))) == 0, lib.hd_last_error()
        z = zT.clone()
        topo = model.dynamics.topology(nmd, None, B, N)
        assert lib.hd_sample_path(hnd, topo.ptr, z.data_ptr(), None, -1, 0, K, None, None, B, model.seed, 0, int(graph), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(z, want), name
        # and the real rows differ from first order
        assert not torch.equal(model.path_steps(zT, nmd, steps=K, solver="dpm2m"), want)


# ----------------------------------------------------------------------------- B3. convergence order through the kernel

def test_convergence_order_on_the_device(small):
    lib, model, h = small
    T, c2data = 1000, 4.0
    nm = torch.ones(2, 5, 1, dtype=torch.bool)
    topo = model.dynamics.topology(dev(nm), None, 2, 5)
    g = sr.analytic_grid(T)
    zT = random_state(nm, 7)                          # x part mean-free: eps* is linear, so every centring is the identity
    exact = sr.analytic_exact(g, T, zT.double(), c2data)
    err = {True: {}, False: {}}
    for second in (True, False):
        for K in (40, 80, 160):
            path = sr.uniform_path(T, K)
            rows = sr.multistep_rows(g, path)
            z, xp = dev(zT), None
            for k, t in enumerate(path[:-1]):
                row = f32(rows[k])
                if not second:
                    row[2] = 0.0
                a_t, s_t = sr.alpha_sigma(g[t])
                eps = z * float(s_t / (a_t * a_t * c2data + s_t * s_t))          # eps* from the current z, on the device
                xp, z = step_on_device(lib, h, topo, row, z, eps, xp if row[2] != 0.0 else None)
            err[second][K] = sr.rel_err(z.cpu(), exact)
    e2, e1 = err[True], err[False]
    for K in (40, 80, 160):
        print(f"device, K={K}: eta=0 {e1[K]:.2e}  2M {e2[K]:.2e}")
    for K in (40, 80):
        assert 3.0 <= e2[K] / e2[2 * K] <= 5.0, (K, e2[K] / e2[2 * K])
        assert 1.7 <= e1[K] / e1[2 * K] <= 2.3, (K, e1[K] / e1[2 * K])
    assert e2[80] < e1[80] / 10.0, (e2[80], e1[80])


# ----------------------------------------------------------------------------- B4 / B5. chains against the float64 reference

def check_chain(model, sd, cfg, T, nm, em, ctx, what, nan_path=False, **few):
    from hierdiff_amd import paths
    path = paths.build_path(T, few.get("steps"), few.get("spacing") or "uniform", few.get("timesteps"))
    K = len(path) - 1
    B, N = nm.shape[:2]
    raws = raw_draws(K + 2, B, N, seed=K)
    ref_raws = list(raws)
    if nan_path:                                      # the injected per-transition normals must never be read
        raws = [raws[0]] + [(torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))) for a, b in raws[1:K + 1]] + [raws[K + 1]]
    x, h = model.sample_from_masks(dev(nm), dev(em), dev(ctx), raw_noises=raws, solver="dpm2m", **few)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()
    gg = gamma_grid_fp64(model, T)
    zT = orc.combined_noise(ref_raws[0][0], ref_raws[0][1], nm.float())
    z0 = sr.chain_ref(sr.network_eps(sd, cfg, T, nm, em, ctx), gg, path, zT, nm.float())
    with torch.no_grad():
        xo, ho = orc.final_decode(sd, cfg, z0, nm, em, ctx, ref_raws[K + 1], gamma_0=gg[0].expand(B, 1))
    nmf = nm.float().numpy()
    rx, rh = rel_l2(x.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(h.cpu().numpy(), ho.numpy())
    print(f"dpm2m {what}: K={K}: x rel_l2 {rx:.2e} h rel_l2 {rh:.2e} (bar {BAR:.0e})")
    assert rx < BAR and rh < BAR, (what, rx, rh)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
def test_chain_vs_float64_T20_K7(C_, precision):
    T = 20
    model, sd, cfg = make_model(H, L, T, C_=C_, precision=precision)
    for name in MASKS:
        nm, em = masks(name)
        check_chain(model, sd, cfg, T, nm, em, context_for(nm) if C_ else None, f"T=20 ctx={C_} {name} [{precision}]", steps=7)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("few", [dict(steps=20), dict(steps=50), dict(steps=50, spacing="quadratic")], ids=["K20", "K50", "K50quadratic"])
def test_chain_vs_float64_T1000(few, precision):
    T = 1000
    model, sd, cfg = make_model(H, L, T, precision=precision)
    nm, em = masks("uneven")
    check_chain(model, sd, cfg, T, nm, em, None, f"T=1000 [{precision}]", **few)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_normal_is_read_on_the_path(precision):
    T = 40
    model, sd, cfg = make_model(H, L, T, precision=precision)
    nm, em = masks("uneven")
    check_chain(model, sd, cfg, T, nm, em, None, f"NaN normals on the path [{precision}]", nan_path=True, steps=10)


# ----------------------------------------------------------------------------- B6. graph replay and its cache

@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replay_equals_plain_launches_and_the_graph_is_cached(precision):
    from hierdiff_amd import _lib
    lib = _lib.load()
    model, _, _ = make_model(H, L, 60, precision=precision)
    nm, _ = masks("wide")
    nmd = dev(nm)
    B, N = nm.shape[:2]
    builds = lambda: int(lib.hd_path_graph_builds(model.dynamics.topology(nmd, None, B, N).ptr))
    res = {}
    for kw in ("dpm2m", "eta0"):
        few = dict(solver="dpm2m") if kw == "dpm2m" else dict(eta=0.0)
        for graph in (True, False):
            model.use_graph = graph
            res[kw, graph] = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, **few)
        assert torch.equal(res[kw, True][0], res[kw, False][0]) and torch.equal(res[kw, True][1], res[kw, False][1]), kw
    assert not torch.equal(res["dpm2m", True][0], res["eta0", True][0])
    model.use_graph = True
    a = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, solver="dpm2m")
    n0 = builds()
    assert n0 >= 1
    b = model.sample_from_masks(nmd, None, None, sample_id_base=77, steps=9, solver="dpm2m")
    assert builds() == n0, "another sample_id_base must replay the cached graph"
    assert not torch.equal(a[0], b[0]) and torch.equal(a[0], res["dpm2m", True][0]) and torch.equal(a[1], res["dpm2m", True][1])
    # eta = 0 and dpm2m in turn on one topology: one rebuild each way, each with its own bits
    e = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, eta=0.0)
    assert builds() == n0 + 1 and torch.equal(e[0], res["eta0", True][0]) and torch.equal(e[1], res["eta0", True][1])
    a2 = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, solver="dpm2m")
    assert builds() == n0 + 2 and torch.equal(a2[0], a[0]) and torch.equal(a2[1], a[1])
    # lower_order_final is part of the path-table key
    c = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=9, solver="dpm2m", lower_order_final=False)
    assert builds() == n0 + 3 and not torch.equal(c[0], a[0])


# ----------------------------------------------------------------------------- B7. split ranges and the continuity rule

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [True, False])
def test_split_ranges_give_the_bits_of_the_whole_and_need_their_history(graph, precision):
    from hierdiff_amd import _lib
    K = 9
    model, _, _ = make_model(H, L, 60, precision=precision)
    model.use_graph = graph
    nm, _ = masks("uneven")
    nmd = dev(nm)
    zT = dev(random_state(nm, 11))
    kw = dict(steps=K, solver="dpm2m")
    whole = model.path_steps(zT, nmd, **kw)
    for k in (1, 4, K - 1):
        cut = model.path_steps(model.path_steps(zT, nmd, k_hi=k, **kw), nmd, k_lo=k, **kw)
        assert torch.equal(whole, cut), k
    three = model.path_steps(model.path_steps(model.path_steps(zT, nmd, k_hi=2, **kw), nmd, k_lo=2, k_hi=5, **kw), nmd, k_lo=5, **kw)
    assert torch.equal(whole, three)
    # the last row (lower_order_final: c2 = 0) needs no history; an inner one does
    mid = model.path_steps(zT, nmd, k_hi=4, **kw)
    model.path_steps(mid, nmd, k_lo=K - 1, **kw)
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):      # a gap: the history is at K, not at 4
        model.path_steps(mid, nmd, k_lo=4, **kw)
    # the path was set again in between
    mid = model.path_steps(zT, nmd, k_hi=4, **kw)
    model.path_steps(zT, nmd, steps=K, eta=0.0)
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):
        model.path_steps(mid, nmd, k_lo=4, **kw)
    # a fresh topology has none
    nm2, _ = masks("one_node")
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):
        model.path_steps(dev(random_state(nm2, 2)), dev(nm2), k_lo=3, **kw)
    assert torch.equal(model.path_steps(zT, nmd, **kw), whole)                          # and nothing is left in a bad state


# ----------------------------------------------------------------------------- B8. shard independence

@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shard_with_its_global_ids_gives_its_rows_of_the_whole_batch(precision):
    T, K, B, lo, n = 1000, 20, 48, 16, 16
    model, _, _ = make_model(H, L, T, precision=precision)
    rng = np.random.default_rng(0)
    sizes = [int(v) for v in rng.integers(1, 13, size=B)]
    sizes[0] = 12                                 # the shard is padded to the batch's width below
    nm, _ = orc.canonical_masks(sizes)
    nm = nm.bool()
    x, h = model.sample_from_masks(dev(nm), None, None, sample_id_base=1000, steps=K, solver="dpm2m")
    xs, hs = model.sample_from_masks(dev(nm[lo:lo + n].contiguous()), None, None, sample_id_base=1000 + lo, steps=K, solver="dpm2m")
    assert torch.equal(x[lo:lo + n], xs) and torch.equal(h[lo:lo + n], hs)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()


# ----------------------------------------------------------------------------- B9. guidance

@pytest.mark.parametrize("precision", PRECISIONS)
def test_guidance_feeds_the_same_update(precision):
    from hierdiff_amd import _lib
    lib = _lib.load()
    T, K = 20, 7
    model, sd, cfg = make_model(H, L, T, C_=1, precision=precision)
    nm, em = masks("uneven")
    nmd = dev(nm)
    B, N = nm.shape[:2]
    ctx = context_for(nm)
    null = torch.zeros(B, N, 1)
    zT = random_state(nm, 13)
    kw = dict(steps=K, solver="dpm2m")
    guided_builds = lambda: int(lib.hd_guided_graph_builds(model.dynamics.topology(nmd, None, B, N).ptr))
    plain = model.path_steps(dev(zT), nmd, context=dev(ctx), **kw)
    g0 = guided_builds()
    one = model.path_steps(dev(zT), nmd, context=dev(ctx), guidance_scale=1.0, **kw)       # scalar 1.0: the unguided path
    assert guided_builds() == g0 and torch.equal(one, plain)
    for graph in (True, False):
        model.use_graph = graph
        rows = model.path_steps(dev(zT), nmd, context=dev(ctx), guidance_scale=torch.ones(B), guidance_context=dev(null), **kw)
        assert torch.equal(rows, plain), graph                                              # hd_sample_path_guided, w_b = 1
    assert guided_builds() == g0 + 1
    model.use_graph = True
    got = model.path_steps(dev(zT), nmd, context=dev(ctx), guidance_scale=2.0, guidance_context=dev(null), **kw).cpu()
    fn = sr.guided_eps(sr.network_eps(sd, cfg, T, nm, em, ctx), sr.network_eps(sd, cfg, T, nm, em, null), [2.0] * B, nm)
    ref = sr.chain_ref(fn, gamma_grid_fp64(model, T), sr.uniform_path(T, K), zT, nm.float())
    rx, rh = rel_l2(got[:, :, :3].numpy(), ref[:, :, :3].numpy()), rel_l2(got[:, :, 3:].numpy(), ref[:, :, 3:].numpy())
    print(f"dpm2m guided w=2 [{precision}]: z_0 x rel_l2 {rx:.2e} h rel_l2 {rh:.2e} (bar {BAR:.0e})")
    assert rx < BAR and rh < BAR
    assert not torch.equal(got, plain.cpu())
    # guided split ranges keep the history too
    cut = model.path_steps(model.path_steps(dev(zT), nmd, context=dev(ctx), guidance_scale=2.0, guidance_context=dev(null), k_hi=3, **kw),
                           nmd, context=dev(ctx), guidance_scale=2.0, guidance_context=dev(null), k_lo=3, **kw)
    assert torch.equal(cut.cpu(), got)


# ----------------------------------------------------------------------------- B10. list-level entry points, refusals

def test_list_level_entry_points_take_the_keyword():
    model, _, _ = make_model(H, 1, 30)

    def check(res):
        for r in res:
            assert torch.isfinite(r["x"]).all() and torch.isfinite(r["h"]).all()
            assert float(r["x"].sum(0).abs().max()) < 1e-3 * max(1.0, float(r["x"].abs().max()))
    torch.manual_seed(0)
    a = model.sample(3, DEV, sample_id_base=2, steps=5, solver="dpm2m")
    torch.manual_seed(0)
    model.sample_steps, model.sample_solver = 5, "dpm2m"           # the same through the attributes
    b = model.sample(3, DEV, sample_id_base=2)
    torch.manual_seed(0)
    first = model.sample(3, DEV, sample_id_base=2, solver="ddim", eta=0.0)
    model.sample_steps, model.sample_solver = None, None
    assert all(torch.equal(p["x"], q["x"]) and torch.equal(p["h"], q["h"]) for p, q in zip(a, b))
    assert not all(torch.equal(p["x"], q["x"]) for p, q in zip(a, first))
    check(a)
    torch.manual_seed(0)
    res, _ = model.sample_batches(2, 2, DEV, steps=5, spacing="quadratic", solver="dpm2m", lower_order_final=False)
    assert len(res) == 4
    check(res)
    var = model.vary(a, DEV, 20, n_variants=2, steps=4, solver="dpm2m")
    assert len(var) == 6 and all(v["x"].shape == a[i // 2]["x"].shape for i, v in enumerate(var))
    check(var)
    nm, _ = masks("uneven")
    z = model.diffuse(dev(torch.zeros(nm.shape[0], nm.shape[1], 3)), dev(torch.zeros(nm.shape[0], nm.shape[1], 8)), dev(nm), 20)
    x, h = model.sample_from_latent(z, dev(nm), t_start=20, steps=6, solver="dpm2m", sample_id_base=4)
    x, h = x.cpu(), h.cpu()
    assert torch.isfinite(x).all() and torch.isfinite(h).all()
    assert torch.all(x[~nm.expand_as(x)] == 0) and torch.all(h[~nm.expand_as(h)] == 0)
    assert float(x.sum(1).abs().max()) < 1e-3 * max(1.0, float(x.abs().max()))
    x0, _ = model.sample_from_latent(z, dev(nm), t_start=20, steps=6, eta=0.0, sample_id_base=4)
    assert not torch.equal(x0.cpu(), x)


def test_c_abi_refusals():
    from hierdiff_amd import _lib, paths
    lib = _lib.load()
    T, K = 8, 3
    model, _, _ = make_model(H, 1, T, C_=1)
    nm, _ = orc.canonical_masks([4, 3])
    nmd = dev(nm.bool())
    h = model._lib_handle()
    topo = model.dynamics.topology(nmd, None, 2, 4)
    z = torch.zeros(2, 4, 11, device=DEV)
    ctx = torch.zeros(8, 1, device=DEV)
    ti, si = (C.c_int * 3)(8, 5, 2), (C.c_int * 3)(5, 2, 0)
    rows = (C.c_float * 15)(*([1.0, 0.5, 0.0, 1.0, 0.5] * 3))
    assert lib.hd_set_path_multistep(h, K, ti, si, rows) == -4 and b"schedule not set" in lib.hd_last_error()
    tabs = model._schedule(rows=2)
    up_t, up_s = (C.c_int * 3)(0, 2, 5), (C.c_int * 3)(2, 5, 8)
    assert lib.hd_set_path_multistep(h, K, up_t, up_s, rows) == -1 and b"descends" in lib.hd_last_error()
    assert lib.hd_set_path_multistep(h, K, ti, (C.c_int * 3)(5, 3, 0), rows) == -1
    assert lib.hd_set_path_multistep(h, K, (C.c_int * 3)(9, 5, 2), si, rows) == -1
    bad = (C.c_float * 15)(*([1.0, 0.5, 0.1, 1.0, 0.5] * 3))
    assert lib.hd_set_path_multistep(h, K, ti, si, bad) == -1 and b"row 0" in lib.hd_last_error()
    pt = paths.path_tables(tabs["gamma"], [8, 5, 2, 0], solver="dpm2m", lower_order_final=False)
    cf = np.ascontiguousarray(pt["coef"].numpy())
    model._path_cache = None
    assert lib.hd_set_path_multistep(h, K, ti, si, cf.ctypes.data_as(C.POINTER(C.c_float))) == 0, lib.hd_last_error()
    fm = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert lib.hd_sample_path_inpaint(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 0, K, None, None, 2, 0, 0, 0, fm.data_ptr(),
                                      z.data_ptr(), 1, None) == -1 and b"ancestral rows only" in lib.hd_last_error()
    w = torch.ones(1, device=DEV)
    guided = lambda k_lo, fixed: lib.hd_sample_path_guided(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), w.data_ptr(), 1, 0.0,
                                                           k_lo, K, None, None, 2, 0, 0, 0, fixed, z.data_ptr() if fixed else None, 1, None)
    assert guided(0, fm.data_ptr()) == -1 and b"ancestral rows only" in lib.hd_last_error()
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 1, K, None, None, 2, 0, 0, 0, None) == -4    # no history yet
    assert b"needs the data prediction" in lib.hd_last_error()
    assert guided(2, None) == -4
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 0, 2, None, None, 2, 0, 0, 0, None) == 0
    assert guided(2, None) == 0                                          # continues the unguided call where it ended
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 2, K, None, None, 2, 0, 0, 0, None) == -4    # the history is at K now
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 2, 2, None, None, 2, 0, 0, 0, None) == 0     # an empty range asks nothing
    torch.cuda.synchronize()
