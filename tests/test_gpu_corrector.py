"""GPU tier (-m gpu) of predictor-corrector sampling: hd_langevin_step against the float64 restatement of
tests/corrector_reference.py, corrected chains against that restatement over the oracle, and the contracts of the device path: kept
bits, masked rows, graph replay, re-attaching, batch and chain cuts, the keyword switched off, refusals.

Bars.  The step: every element within 8 * 2^-23 of the sum of the absolute values of its terms (the magnitude array of the
restatement); the gains relative 1e-13 (the bar of the energy calls: they are double sums of the same fp32 values) wherever the
restatement sees the kernel's own normals, that is with injected ones.  The generator's normals are those of its host twin only to
3e-6 (device and host logf / sinf / cosf differ in the last bits: the bar of test_philox_device_matches_host_twin in
tests/test_gpu_parity.py), so there the gain is held to 1e-13 plus what normals 3e-6 apart can move it
(`corrector_reference.gain_slack`: 2 delta sum |xi~| / sum xi~^2, about 1e-5), and the elements to the same element-wise bar.
Chains: rel-L2 <= 1e-4 per state (tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: B = 5 molecules (ordinary, one valid node, no valid node, eps^ == 0, a NaN in eps^) of N in {5, 33} nodes at D in {4, 11};
chains at T = 8, K = 4, B = 4 (two groups of two equal masks) with C in {1, 2} on the models of tests/test_gpu_restraint.py.  The
chains draw from the generator (a corrected loop takes no injected noise); the restatement reads the same normals from its host twin."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.corrector import Corrector
from hierdiff_amd.diversity import Diversity
from hierdiff_amd.restraints import Restraints, feature_ratio
from oracle import egnn_oracle as orc
from tests import corrector_reference as cr
from tests import diversity_reference as dr
from tests import edit_reference as er
from tests import feature_reference as fr
from tests import guidance_reference as gr
from tests import restraint_reference as rr
from tests import sde_solver_reference as sd
from tests import solver_reference as sr
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_restraint import BOTH, DEV, T, Bare, dev, fresh as fresh_restraints, model_for, stream
from tests.test_inpaint_cpu import gamma_grid_fp64

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]
SEED, BASE = 99, 10
DRAW = (T + 2) * 2 + 3                                        # stream 2 of the layout, arrival s = T - 3


def fresh(model, graph=True):
    fresh_restraints(model, graph)
    model.particles = model.steer_scale = model.diversity = model.corrector = None
    return model


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- the kernel, on a bare handle (any D)

def run_step(bare, c, row, adaptive, raws, alias, draw=DRAW, rows=None):
    """(out, gains): injected normals `raws` = (raw_x, raw_h), or None for the generator at (SEED, BASE + b, draw) with `rows` rows."""
    zd, ed = dev(torch.from_numpy(c["z"])).contiguous(), dev(torch.from_numpy(c["eps"])).contiguous()
    out = zd if alias else torch.full_like(zd, 7.0)
    gain = torch.full((c["B"],), -1.0, device=DEV, dtype=torch.float64)
    rx = rh = None
    if raws is not None:
        rx, rh = dev(torch.from_numpy(np.ascontiguousarray(raws[0]))), dev(torch.from_numpy(np.ascontiguousarray(raws[1])))
        rows = rx.shape[0]
    rc = bare.lib.hd_langevin_step(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 3)(*row), adaptive,
                                   None if rx is None else rx.data_ptr(), None if rh is None else rh.data_ptr(), rows, SEED, BASE, draw,
                                   out.data_ptr(), gain.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), gain.cpu().numpy()


TWIN_DELTA = 3e-6                                             # |device normal - host twin| (tests/test_gpu_parity.py)


def check_step(what, c, row, adaptive, raws, got, gains, alias, twin=False):
    ref, A, g, kept = cr.langevin_ref(c["z"], c["eps"], c["nm"], row, adaptive, raws[0], raws[1])
    valid = c["nm"] != 0
    quiet = row[1] == 0.0
    if quiet and not alias:                                   # a row with q = 0 draws nothing and writes nothing
        assert (got == 7.0).all() and (gains == -1.0).all(), what
        return 0.0
    assert (bits(got[~valid]) == bits(c["z"][~valid] if alias else np.full_like(c["z"][~valid], 7.0))).all(), what      # masked rows: not written
    if quiet:
        assert (bits(got) == bits(c["z"])).all() and (gains == -1.0).all(), what
        return 0.0
    assert (kept == c["keeps"]).all(), what
    for b in np.flatnonzero(kept):                            # the molecule keeps its bits
        assert (bits(got[b][valid[b]]) == bits(c["z"][b][valid[b]])).all() and gains[b] == 0.0, (what, b)
    live = ~kept
    slack = cr.gain_slack(c["nm"], raws[0], raws[1], TWIN_DELTA) if twin else np.zeros(c["B"])
    gerr = np.abs(gains[live] - g[live]) / g[live]
    print(f"{what}: worst relative gain error {gerr.max():.2e} (bar {(1e-13 + slack[live]).min():.2e})")
    assert (gerr <= 1e-13 + slack[live]).all(), (what, gains, g)
    moved = np.zeros_like(valid)
    moved[live] = valid[live]
    r = cr.ratio(got, ref, A, moved)
    assert np.isfinite(got[moved]).all() and r <= cr.BOUND, (what, r)
    assert not (bits(got[0][valid[0]]) == bits(c["z"][0][valid[0]])).all()
    return r


@pytest.mark.parametrize("N,D", SHAPES)
def test_langevin_step_against_float64(N, D):
    c = cr.kernel_case(N, D)
    bare = Bare(D, torch.from_numpy(c["nm"]))
    lib = _lib.load()
    worst, n = 0.0, 0
    try:
        for name, row, adaptive in cr.kernel_rows():
            for rows in (c["B"], 1):                          # every molecule's own normals, one shared row
                raws = (c["raw_x"][:rows], c["raw_h"][:rows])
                what = f"hd_langevin_step N={N} D={D} '{name}' noise rows {rows}"
                got, gains = run_step(bare, c, row, adaptive, raws, alias=False)
                r = check_step(what, c, row, adaptive, raws, got, gains, False)
                got2, gains2 = run_step(bare, c, row, adaptive, raws, alias=True)      # in place
                check_step(what + " in place", c, row, adaptive, raws, got2, gains2, True)
                valid = c["nm"] != 0
                if row[1] != 0.0:
                    assert (bits(got2[valid]) == bits(got[valid])).all() and (gains2 == gains).all(), what
                worst, n = max(worst, r), n + 1
                # the generator against its host twin at a stream >= 1
                F = D - 3
                host = np.array([[lib.hd_philox_normal_host(SEED, BASE + b, DRAW, i) for i in range(N * D)] for b in range(rows)],
                                dtype=np.float32).reshape(rows, N, D)
                hr = (host[:, :, :3].copy(), host[:, :, 3:].copy())
                got3, gains3 = run_step(bare, c, row, adaptive, None, alias=False, rows=rows)
                r = check_step(what + " generator", c, row, adaptive, hr, got3, gains3, False, twin=True)
                worst = max(worst, r)
                if row[1] != 0.0 and row[0] != 0.0:           # the draw counts (sigma_t = 0 multiplies the noise away)
                    other, _ = run_step(bare, c, row, adaptive, None, alias=False, draw=DRAW + 1, rows=rows)
                    assert not (bits(other[0]) == bits(got3[0])).all()
        print(f"hd_langevin_step N={N} D={D}: worst err / (2^-23 A) over {n} cases {worst:.3f} (bar {cr.BOUND:g})")
    finally:
        bare.close()


def test_abi_refusals():
    c = cr.kernel_case(5, 4)
    bare = Bare(4, torch.from_numpy(c["nm"]))
    lib = bare.lib
    try:
        zd, ed = dev(torch.from_numpy(c["z"])).contiguous(), dev(torch.from_numpy(c["eps"])).contiguous()
        out = torch.full_like(zd, 7.0)
        r3 = (C.c_float * 3)(0.7, 0.05, math.inf)
        step = lambda z=zd.data_ptr(), e=ed.data_ptr(), row=r3, ad=1, rx=None, rh=None, rows=5, o=out.data_ptr(): lib.hd_langevin_step(
            bare.h, bare.topo, z, e, row, ad, rx, rh, rows, SEED, BASE, 1, o, None, stream())
        for bad in ((-0.1, 0.05, 1.0), (math.nan, 0.05, 1.0), (0.7, -1.0, 1.0), (0.7, math.inf, 1.0), (0.7, math.nan, 1.0), (0.7, 0.05, 0.0),
                    (0.7, 0.05, -1.0), (0.7, 0.05, math.nan)):
            assert step(row=(C.c_float * 3)(*bad)) == -1, bad
            assert b"hd_langevin_step" in lib.hd_last_error()
        assert step(ad=2) == -1 and step(z=None) == -1 and step(o=None) == -1 and step(rows=2) == -1
        assert step(rx=zd.data_ptr()) == -1 and b"go together" in lib.hd_last_error()
        assert step(o=ed.data_ptr()) == -1 and b"overlap eps" in lib.hd_last_error()
        assert step(o=zd.data_ptr() + 4) == -1 and b"shifted overlap" in lib.hd_last_error()
        torch.cuda.synchronize()
        assert (out.cpu() == 7.0).all()
        for bad in (0, 9, -1):
            assert lib.hd_corrector_attach(bare.topo, bad, 1, None) == -1 and b"hd_corrector_attach" in lib.hd_last_error()
        assert lib.hd_corrector_attach(bare.topo, 1, 2, None) == -1
        g = torch.zeros(5, dtype=torch.float64, device=DEV)
        assert lib.hd_corrector_read(bare.topo, g.data_ptr(), None) == -4
        assert lib.hd_set_corrector(bare.h, 1, r3) == -4          # no path
        assert lib.hd_corrector_attach(bare.topo, 8, 0, None) == 0 and lib.hd_corrector_detach(bare.topo) == 0
        assert step() == 0                                    # the single step needs no attachment
    finally:
        bare.close()
    wm = torch.zeros(1, 1490, dtype=torch.bool)               # 1490 * 11 floats are 24 bytes past 64 KiB
    wm[0, :2] = True
    wide = Bare(11, wm)
    try:
        z = torch.zeros(1, 1490, 11, device=DEV)
        o = torch.full_like(z, 7.0)
        e = torch.zeros_like(z)
        assert wide.lib.hd_langevin_step(wide.h, wide.topo, z.data_ptr(), e.data_ptr(), (C.c_float * 3)(0.7, 0.05, 1.0), 1, None, None, 1,
                                         SEED, BASE, 1, o.data_ptr(), None, stream()) == -1
        assert b"exceed one workgroup's LDS" in wide.lib.hd_last_error()
        torch.cuda.synchronize()
        assert (o.cpu() == 7.0).all()
    finally:
        wide.close()


def test_loop_refusals():
    """The path loop's new refusals, behind the old ones, with their codes and the process alive."""
    from hierdiff_amd._lib import HdConfig
    lib = _lib.load()
    B, N, F, K, T_ = 4, 5, 8, 4, 8
    D = 3 + F
    cfg = HdConfig(in_node_nf=F + 1, context_node_nf=0, n_dims=3, hidden_nf=32, n_layers=1, inv_sublayers=2, attention=1, tanh=1,
                   condition_time=1, norm_constant=0.0, normalization_factor=10.0, coords_range=30.0, precision=0, aggregation_mean=0)
    h, topo = C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, lib.hd_last_error()

    ok(lib.hd_create(C.byref(cfg), 0, C.byref(h)))
    nm = np.ones((B, N), dtype=np.uint8)
    ok(lib.hd_topology_create(h, nm.ctypes.data, None, B, N, C.byref(topo)))
    try:
        n = lib.hd_weight_count(h)
        blob = (np.random.default_rng(0).standard_normal(n) * 0.05).astype(np.float32)
        ok(lib.hd_set_weights(h, blob.ctypes.data, n, 0, None))
        rows = np.tile(np.array([0.9, 0.3, 0.5, 0.2], dtype=np.float32), (T_, 1))
        rows_p = rows.ctypes.data_as(C.POINTER(C.c_float))
        ok(lib.hd_set_schedule(h, T_, (C.c_float * (T_ + 1))(*np.linspace(0.0, 1.0, T_ + 1)), rows_p))
        ok(lib.hd_set_inpaint_schedule(h, T_, rows_p))
        i32 = lambda *v: (C.c_int * len(v))(*v)
        t_idx, s_idx = i32(8, 6, 4, 2), i32(6, 4, 2, 0)
        ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 0, rows_p))
        z = torch.zeros(B, N, D, device=DEV)
        fixed, known = torch.zeros(B, N, dtype=torch.uint8, device=DEV), torch.zeros(B, N, D, device=DEV)
        raw_x, raw_h = torch.zeros(K, B, N, 3, device=DEV), torch.zeros(K, B, N, F, device=DEV)
        one = (C.c_float * 1)(1.0)
        r3 = np.tile(np.array([0.5, 0.02, np.inf], dtype=np.float32), (K, 1))
        r3p = r3.ctypes.data_as(C.POINTER(C.c_float))
        r4 = np.tile(np.array([0.9, 0.3, 0.5, 0.2], dtype=np.float32), (K, 1))
        r4p = r4.ctypes.data_as(C.POINTER(C.c_float))
        run = lambda mol=-1, rows_=B, graph=1, rx=None, rh=None: lib.hd_sample_path(h, topo, z.data_ptr(), None, mol, 0, K, rx, rh, rows_, 7, 0,
                                                                                    graph, None)
        assert run() == 0
        ok(lib.hd_corrector_attach(topo, 2, 1, None))
        # rows not set for the current path
        assert run() == -4 and b"hd_set_corrector" in lib.hd_last_error()
        assert lib.hd_set_corrector(h, K + 1, r3p) == -1 and lib.hd_set_corrector(h, K, None) == -1
        bad = r3.copy()
        bad[2, 2] = 0.0
        assert lib.hd_set_corrector(h, K, bad.ctypes.data_as(C.POINTER(C.c_float))) == -1 and b"g_max_k > 0" in lib.hd_last_error()
        ok(lib.hd_set_corrector(h, K, r3p))
        assert run() == 0 and run(graph=0) == 0 and run(rows_=1) == 0
        # an inpainting call; mol_shape < N; injected noise; steering at the same time
        rc = lib.hd_sample_path_inpaint(h, topo, z.data_ptr(), None, -1, 0, K, None, None, B, 7, 0, 1, fixed.data_ptr(), known.data_ptr(), 2, None)
        assert rc == -1 and b"correctors" in lib.hd_last_error() and b"inpainting" in lib.hd_last_error()
        assert run(mol=3) == -1 and b"whole molecules" in lib.hd_last_error()
        assert run(rx=raw_x.data_ptr(), rh=raw_h.data_ptr()) == -1 and b"no injected noise" in lib.hd_last_error()
        ok(lib.hd_steer_attach(topo, 2, 0.5, 1, None))
        assert run() != 0                                     # (steering's own refusals come first: it needs restraints)
        ok(lib.hd_restraint_attach(topo, None, 1, 0, None, None, 1, 0, None, None, 1, 0, one, 1, 1.0, None))
        r3s = np.tile(np.array([0.9, 0.3, 0.5], dtype=np.float32), (K, 1))
        ok(lib.hd_set_restraint(h, K, r4p))
        ok(lib.hd_set_steer(h, K, r3s.ctypes.data_as(C.POINTER(C.c_float))))
        assert run() == -1 and b"correctors and steering" in lib.hd_last_error()
        ok(lib.hd_steer_detach(topo))
        ok(lib.hd_restraint_detach(topo))
        assert run() == 0
        # the every-step loops record nothing and run without the correctors
        assert lib.hd_sample_loop(h, topo, z.data_ptr(), None, -1, T_, 0, None, None, B, 7, 0, 1, None) == 0
        # a new path: the rows belong to the old one
        ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 1, None))
        assert run() == -4
        ok(lib.hd_corrector_detach(topo))
        assert run() == 0 and run(rx=raw_x.data_ptr(), rh=raw_h.data_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(z).all()
    finally:
        torch.cuda.synchronize()
        lib.hd_topology_destroy(topo)
        lib.hd_destroy(h)


# ----------------------------------------------------------------------------- chains against the restatement over the oracle

K = 4
MOLS = (7, 7, 4, 4)
CHAIN_BASE = 5
KINDS = ["eta1", "eta0", "dpm2m", "sde2m", "guided", "obstacles+band", "diversity", "x0", "latent"]
SNR = 0.5


def batch(C_=0):
    nm, em = orc.canonical_masks(list(MOLS))
    nm = nm.bool()
    ctx = None
    if C_:
        ctx = (torch.tensor([0.7, 0.7, -0.4, -0.4]).reshape(4, 1, 1).expand(4, nm.shape[1], 1) * nm.float()).contiguous()
    return nm, em, ctx


def predictor_for(kind, net_c, gg, path, nm):
    """predictor(k, z, eps, raw) of `corrector_reference.corrected_chain`, and the path keywords of the device call."""
    nmd = nm.to(torch.float64)
    if kind == "dpm2m":
        rows, hist = sr.multistep_rows(gg, path, True), {}

        def step(k, z, eps, raw):
            hist["x"], zs = sr.step_ref(rows[k], z, eps, hist.get("x"), nm.float())
            return zs
        return step, dict(solver="dpm2m")
    if kind == "sde2m":
        rows, hist = sd.sde_rows(gg, path, True), {}

        def step(k, z, eps, raw):
            hist["x"], zs = sd.step_ref(rows[k], z, eps, hist.get("x"), nm.float(), raw)
            return zs
        return step, dict(solver="sde2m")
    if kind == "eta0":
        def step(k, z, eps, raw):
            a, b, _ = er.down_row(float(gg[path[k + 1]]), float(gg[path[k]]), 0.0)
            return er._centre_x(a * z.double() - b * er._centre_x(eps.double(), nmd), nmd)
        return step, dict(eta=0.0)
    return (lambda k, z, eps, raw: gr.ancestral_on_eps(net_c, z, eps, path[k + 1], path[k], raw, gg)), dict(eta=1.0)


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("C_steps", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_corrected_chain_against_the_restatement(kind, C_steps, precision):
    guided = kind == "guided"
    Cx = 1 if guided else 0
    if kind == "obstacles+band":
        from tests.test_gpu_feature import model_for as feature_model
        model = feature_model(precision)
        sd_np, cfg = er.weights(*fr.CHAIN_SHAPES[precision])
    else:
        model, sd_np, cfg = model_for(precision, Cx)
    fresh(model)
    nm, em, ctx = batch(Cx)
    B, N = nm.shape[:2]
    nv0 = float(model.norm_values[0])
    gg = gamma_grid_fp64(model, T)
    t_start = 6 if kind == "latent" else T
    path = paths.partial_path(T, t_start, 3) if kind == "latent" else paths.build_path(T, K)
    Kp = len(path) - 1
    corr = Corrector(C_steps, snr=SNR, max_gain=0.5) if kind != "eta0" else Corrector(C_steps, mode="fixed", gain=[0.02, 0.01, 0.0, 0.005][:Kp])
    rows3 = cr.rows_from_grid(gg, path, corr.mode, corr.strength, corr.max_gain)
    raw0 = cr.normals_host(model.seed, CHAIN_BASE, 0, B, N, 8)
    z = orc.combined_noise(raw0[0], raw0[1], nm.float())
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
    kw = dict(steps=Kp, corrector=corr)
    rows4 = rr.rows_from_grid(gg, path, "score", 0.3, nv0)
    if kind == "obstacles+band":
        nv1, nb1 = float(model.norm_values[1]), float(model.norm_biases[1] or 0.0)
        ft = fr.chain_features()
        rs = Restraints(obstacles=fr.chain_obstacles(), features=ft)
        scale = torch.tensor(fr.CHAIN_SCALE)
        inner = fr.FeatNet(rr.RestrainedNet(inner, rs, scale, rows4, nv0), ft, scale, rows4, nv1, nb1, feature_ratio("score", nv0, nv1), nm=nm)
        kw.update(restraints=rs, restraint_scale=scale, restraint_clip=0.3)
    if kind == "diversity":
        dv = Diversity(particles=2, length=50.0, strength=2500.0, scale=[1.0, 0.5], clip=0.3)
        inner = dr.DiverseNet(inner, dv.P, dv.strength, dv.length, dv.scale, rows4, nv0)
        kw.update(diversity=dv)
    if guided:
        kw.update(guidance_scale=2.0)
    if kind == "latent":
        kw.update(t_start=t_start)
    predictor, pkw = predictor_for(kind, getattr(inner, "c", inner), gg, path, nm)
    kw.update(pkw)
    draws = cr.Draws(model.seed, CHAIN_BASE, T, B, N, 8)
    eps_log = []

    def eps_fn(zz, t):
        e = inner.net(zz, t)
        eps_log.append((zz, e, t))
        return e
    ref = cr.corrected_chain(eps_fn, predictor, path, z, nm, rows3, corr.adaptive, C_steps, draws)
    tag = f"corrected chain {kind} C={C_steps} [{precision}]"
    nmd, emd, ctxd = dev(nm), dev(em), dev(ctx)
    if kind == "x0":
        x, h, chain = model.sample_from_latent(dev(z), nmd, emd, ctxd, sample_id_base=CHAIN_BASE, keep_frames=Kp, record="x0", **kw)
        chain = chain.cpu()
        assert torch.isfinite(chain).all()
        pred_calls = eps_log[C_steps::C_steps + 1]            # the predictor's network call of every transition
        for k in range(Kp - 1):                               # transition k writes frame K - 1 - k; frame 0 is the result itself
            zz, e, t = pred_calls[k]
            want = rr.x0_f32(zz, e, rows4[int(t)][0], rows4[int(t)][1], nv0)
            r = rel_l2(chain[Kp - 1 - k][:, :, :3].numpy(), want.numpy())
            print(f"{tag} frame of transition {k + 1}/{Kp}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
            assert r < REL_L2_TOL, (k, r)
        x2, h2 = model.sample_from_latent(dev(z), nmd, emd, ctxd, sample_id_base=CHAIN_BASE, **kw)
        assert torch.equal(x2, x) and torch.equal(h2, h)       # recording changes no sample
    else:
        zz, worst = dev(z), 0.0
        for k in range(Kp):
            zz = model.latent_steps(zz, nmd, emd, ctxd, k_lo=k, k_hi=k + 1, sample_id_base=CHAIN_BASE, **kw)
            r = rel_l2(zz.cpu().numpy(), ref[k][1].numpy())
            worst = max(worst, r)
            print(f"{tag} state {k + 1}/{Kp}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
            assert torch.isfinite(zz).all() and r < REL_L2_TOL, (k, r)
        gains = model.corrector_last
        assert tuple(gains.shape) == (C_steps, B) and gains.dtype == torch.float64
        plain = model.latent_steps(dev(z), nmd, emd, ctxd, sample_id_base=CHAIN_BASE, **dict(kw, corrector=None))
        d = rel_l2(zz.cpu().numpy(), plain.cpu().numpy())
        print(f"{tag}: worst state {worst:.2e}; gains of the last transition {gains.numpy().round(5).tolist()}; distance from the "
              f"uncorrected z_0 {d:.2e}")
        assert d > 10 * REL_L2_TOL
    # the correctors moved z in every transition whose row asks for it: every state lies far outside the bar of the uncorrected chain
    # (the restatement with C = 0); a block's own move is printed (mode "snr" takes small steps where eps^ is large) and is not nothing
    off = cr.corrected_chain(lambda zz, t: inner.net(zz, t), predictor_for(kind, getattr(inner, "c", inner), gg, path, nm)[0], path, z, nm,
                             rows3, corr.adaptive, 0, draws)
    before = z
    for k in range(Kp):
        m = rel_l2(ref[k][0].numpy(), before.numpy())
        d = rel_l2(ref[k][1].numpy(), off[k][1].numpy())
        print(f"{tag} transition {k + 1}: the correctors moved z by rel_l2 {m:.2e}; distance of the state from the uncorrected one {d:.2e}")
        assert torch.equal(ref[k][0], before) == bool(rows3[k][1] == 0), (k, m)
        assert d > 10 * REL_L2_TOL, (k, d)
        before = ref[k][1]


# ----------------------------------------------------------------------------- bit for bit

def call(model, nmd, corr, base=3, **kw):
    if "solver" not in kw:
        kw.setdefault("eta", 0.5)
    return model.sample_from_masks(nmd, None, None, sample_id_base=base, corrector=corr, steps=4, **kw)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replay_reattaching_and_detaching():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    nm, _, _ = batch()
    nmd = dev(nm)
    c1, c2, cf = Corrector(1, snr=SNR), Corrector(2, snr=SNR), Corrector(1, mode="fixed", gain=0.01)
    fresh(model, graph=False)
    want = {k: call(model, nmd, c) for k, c in (("c1", c1), ("c2", c2), ("cf", cf), ("plain", None))}
    want["shared"] = call(model, nmd, c1, fix_noise=True)
    assert not same(want["c1"], want["plain"]) and not same(want["c1"], want["c2"]) and not same(want["c1"], want["cf"])
    assert not same(want["shared"], want["c1"])
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 4, nm.shape[1])
    assert same(call(model, nmd, None), want["plain"])        # a topology that never had it
    n0 = lib.hd_path_graph_builds(topo.ptr)
    assert same(call(model, nmd, c1), want["c1"])             # graph replay against plain launches
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 1
    assert same(call(model, nmd, Corrector(1, snr=SNR)), want["c1"])
    assert same(call(model, nmd, Corrector(1, snr=2 * SNR)), call(model, nmd, Corrector(1, snr=2 * SNR)))
    assert same(call(model, nmd, c1), want["c1"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 1       # the same C, rows of the same size: no graph is built
    assert same(call(model, nmd, c2), want["c2"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 2       # another C: one build
    assert same(call(model, nmd, c2), want["c2"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 2
    assert same(call(model, nmd, cf), want["cf"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 3       # another mode: one build
    assert same(call(model, nmd, c1, fix_noise=True), want["shared"])
    assert same(call(model, nmd, None), want["plain"])        # after detaching: the bits of a topology that never had it
    # all-zero rows and the keyword switched off are the call without it
    n1 = lib.hd_path_graph_builds(topo.ptr)
    plain = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=4, eta=0.5)
    assert same(plain, want["plain"])
    for off in (Corrector(0), Corrector(2, snr=0.0), Corrector(2, snr=[0.0] * 4), Corrector(1, mode="fixed", gain=0.0)):
        assert same(call(model, nmd, off), want["plain"])
    assert lib.hd_path_graph_builds(topo.ptr) == n1
    full = model.sample_from_masks(nmd, None, None, sample_id_base=3)      # ... also where that is the plain every-step loop
    assert same(model.sample_from_masks(nmd, None, None, sample_id_base=3, corrector=Corrector(0)), full)
    assert model.corrector_last is not None and tuple(model.corrector_last.shape) == (1, 4)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_molecule_depends_on_its_id_only_and_a_cut_chain_equals_the_whole(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    nm, _, _ = batch()
    nmd = dev(nm)
    corr = Corrector(2, snr=SNR)
    for kw in (dict(), dict(eta=0.0), dict(solver="dpm2m")):  # a batch against its two halves run alone, ids carried
        whole = call(model, nmd, corr, **kw)
        a = call(model, nmd[:2], corr, base=3, **kw)
        b = call(model, nmd[2:], corr, base=5, **kw)
        assert torch.equal(whole[0][:2], a[0]) and torch.equal(whole[0][2:], b[0]), kw
        assert torch.equal(whole[1][:2], a[1]) and torch.equal(whole[1][2:], b[1]), kw
    g = torch.Generator().manual_seed(3)
    z = orc.combined_noise(torch.randn(4, 7, 3, generator=g), torch.randn(4, 7, 8, generator=g), nm.float())
    for kw in (dict(eta=1.0), dict(eta=0.0), dict(solver="dpm2m"), dict(solver="sde2m")):     # path_steps cut in the middle
        whole = model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, corrector=corr, **kw)
        half = model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, k_lo=0, k_hi=2, corrector=corr, **kw)
        rest = model.path_steps(half, nmd, steps=4, sample_id_base=5, k_lo=2, k_hi=4, corrector=corr, **kw)
        assert torch.equal(whole, rest), kw
        assert not torch.equal(whole, model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, **kw))


def test_cli_round_trip(tmp_path):
    import pickle
    from hierdiff_amd import sampler
    out = str(tmp_path / "o.pkl")
    argv = ["--hidden-nf", "32", "--n-layers", "1", "--timesteps", "8", "--batch-size", "4", "--num-batches", "1", "--out", out,
            "--steps", "4", "--correctors", "2", "--corrector-snr", "0.2"]
    assert sampler.main(argv) == 0
    with open(out, "rb") as f:
        res, _ = pickle.load(f)
    assert len(res) == 4 and all(bool(torch.isfinite(r["x"]).all()) for r in res)
