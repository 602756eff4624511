"""GPU tier (-m gpu) of the feature restraints: hd_restrain_feat and hd_restraint_feature_energy against the float64 restatement of
tests/feature_reference.py, featured chains (plain, guided with obstacles, sde2m, recorded, framed inpainting, steered) against that
restatement over the oracle, and the contracts of the device path: bits of the columns the kernel never writes, graph replay,
re-attaching, batch and chain cuts, result entries, refusals.

Bars.  eps: the project's element-wise bar - every written element within 8 * 2^-23 of the sum of the absolute values of its terms
(tests/sampling_reference.py).  The energy call: 1e-13 relative of the float64 sum of its terms; the m_r within 1e-13 of the sum of
the absolute values of theirs.  Chains: rel-L2 <= 1e-4 per state (tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: B = 5 molecules (ordinary, s_b = 0, one valid node, no valid node, a NaN in one valid feature element) of N in {5, 33} nodes
with F in {1, 8} features, W < N and W = N, S in {0, 1, 8}; chains at T = 8, K = 4, B = 4 in fp32 and fp16x3 on models whose h is
normalised with nv1 = 1.7, nb1 = 0.3.  tests/test_feature_cpu.py asserts the input conditions of these cases and that every mutant
of the restatement misses these bars on them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from hierdiff_amd.restraints import Features, FeatureSum, Restraints, Template
from tests import feature_reference as fr
from tests import field_reference as fld
from tests import sampling_reference as sref
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_field import Bare
from tests.test_gpu_restraint import BOTH, DEV, dev, fresh, stream
from tests.test_gpu_steer import read_state
from tests.test_inpaint_cpu import SEED

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (5, 8), (33, 1), (33, 8)]


# ----------------------------------------------------------------------------- the kernels, on a bare handle (any D)

def feat_of(c):
    return (c.nv1, c.nb1, c.ratio)


def run_feat(bare, c, alias, rs=None, eps=None):
    rs = c.rs if rs is None else rs
    rs.attach(bare, c.scale, c.nv0, torch.device(DEV), stream(), feat=feat_of(c))
    zd, ed = dev(c.z).contiguous(), dev(c.eps if eps is None else eps).contiguous()
    out = ed if alias else torch.full_like(ed, 7.0)
    rc = bare.lib.hd_restrain_feat(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(*c.row), out.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    return out.cpu()


def others(N):
    """Obstacles, a field and a template for the `together` runs."""
    g = np.random.Generator(np.random.PCG64(N))
    tabs = Restraints(obstacles=[[0.2, 0.0, 0.1, 2.5, 2.0], [-1.0, 1.0, 0.5, 1.5, 1.0]])
    tabs = fld.with_fields(tabs, fld.make_fields(1, fr.B, N, 3, False, (0.0, 0.0, 0.0)))
    tabs.templates = [Template([0, 1, 2], g.normal(0.0, 1.5, (3, 3)), k=1.5)]
    return tabs


@pytest.mark.parametrize("N,F", SHAPES)
def test_restrain_feat_against_float64(N, F):
    what = f"hd_restrain_feat N={N} F={F}"
    bare, worst, cases = None, 0.0, 0
    try:
        for c in fr.kernel_cases(N, F):
            bare = Bare(c.D, c.nm) if bare is None else bare
            got = run_feat(bare, c, alias=False)
            assert torch.equal(got, run_feat(bare, c, alias=True)), c.name                 # in place
            ref, mag = fr.restrain_feat_ref(c.ft, c.z, c.eps, c.nm, c.scale, c.row, c.nv1, c.nb1, c.ratio)
            assert torch.isfinite(got).all(), c.name
            bound = sref.BOUND * sref.U * mag
            err = np.abs(got.double().numpy() - ref)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            print(f"{what} {c.name}: worst err / bound {ratio:.3f}")
            assert (err <= bound).all(), (what, c.name, ratio)
            worst = max(worst, ratio)
            cases += 1
            e, g_, valid = c.eps.numpy(), got.numpy(), c.nm.numpy()
            assert (g_[:, :, :3] == e[:, :, :3]).all() and (g_[~valid] == e[~valid]).all()   # position columns, masked rows
            assert (g_[1] == e[1]).all() and (g_[3] == e[3]).all()                          # s_b = 0; no valid node
            assert g_[fr.NAN_AT[0], fr.NAN_AT[1], 3 + fr.NAN_AT[2]] == e[fr.NAN_AT[0], fr.NAN_AT[1], 3 + fr.NAN_AT[2]]
            assert (g_[0] != e[0]).any(), c.name                                            # the ordinary molecule moved
            assert (ref[:, :, 3:][ref[:, :, 3:] == e[:, :, 3:].astype(np.float64)] == g_[:, :, 3:][ref[:, :, 3:] == e[:, :, 3:].astype(np.float64)]).all()
        print(f"{what}: worst err / bound over {cases} cases {worst:.3f}")
    finally:
        if bare is not None:
            bare.close()


@pytest.mark.parametrize("N,F", [(5, 8), (33, 1)])
def test_restrain_feat_together_with_obstacles_a_field_and_a_template(N, F):
    """The position update and the feature update touch disjoint columns: behind hd_restrain_eps on the same attachment the feature
    columns are those of the features alone, the position columns those of the others alone, bit for bit."""
    bare = None
    try:
        for c in list(fr.kernel_cases(N, F))[3:7]:
            bare = Bare(c.D, c.nm) if bare is None else bare
            alone = run_feat(bare, c, alias=False)
            both = others(N)
            both.features = c.ft
            both.attach(bare, c.scale, c.nv0, torch.device(DEV), stream(), feat=feat_of(c))
            zd = dev(torch.nan_to_num(c.z, nan=0.25)).contiguous()          # (a NaN position never occurs; the feature NaN is kept below)
            zd[:, :, 3:] = dev(c.z)[:, :, 3:]
            ed = dev(c.eps).contiguous()
            r4 = (C.c_float * 4)(*c.row)
            pos = torch.full_like(ed, 7.0)
            assert bare.lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, pos.data_ptr(), stream()) == 0, bare.lib.hd_last_error()
            out = pos.clone()
            assert bare.lib.hd_restrain_feat(bare.h, bare.topo, zd.data_ptr(), out.data_ptr(), r4, out.data_ptr(), stream()) == 0, bare.lib.hd_last_error()
            out, pos = out.cpu(), pos.cpu()
            assert not torch.equal(pos[:, :, :3], c.eps[:, :, :3]) and torch.equal(pos[:, :, 3:], c.eps[:, :, 3:])
            assert torch.equal(out[:, :, :3], pos[:, :, :3]) and torch.equal(out[:, :, 3:], alone[:, :, 3:]), c.name
    finally:
        if bare is not None:
            bare.close()


@pytest.mark.parametrize("N,F", SHAPES)
def test_restraint_feature_energy_against_float64(N, F):
    """On the data predictions of the kernel cases (fp32 features, so the restatement sees the same numbers)."""
    bare, wu, wm = None, 0.0, 0.0
    try:
        for c in fr.kernel_cases(N, F):
            if not math.isinf(c.row[3]):
                continue                                      # (the clip does not enter the energy)
            bare = Bare(c.D, c.nm) if bare is None else bare
            v = fr.v_f32(c.z, c.eps, c.row[0], c.row[1], c.nv1, c.nb1).contiguous()
            c.rs.attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream(), feat=(1.0, 0.0, 1.0))
            S = c.ft.S
            out = torch.full((fr.B, 2), -1.0, device=DEV, dtype=torch.float64)
            sums = torch.full((fr.B, max(S, 1)), -1.0, device=DEV, dtype=torch.float64)
            vd = dev(v)
            rc = bare.lib.hd_restraint_feature_energy(bare.h, bare.topo, vd.data_ptr(), out.data_ptr(), sums.data_ptr() if S else None, stream())
            assert rc == 0, bare.lib.hd_last_error()
            out2 = torch.full_like(out, -1.0)                 # sums may be NULL
            assert bare.lib.hd_restraint_feature_energy(bare.h, bare.topo, vd.data_ptr(), out2.data_ptr(), None, stream()) == 0
            assert torch.equal(out, out2)
            U, _, _, m, mm = fr.feature_energy_grad(c.ft, v.numpy(), c.nm)
            got, gm = out.cpu().numpy(), sums.cpu().numpy()[:, :S]
            assert np.isfinite(got).all() and np.isfinite(gm).all(), c.name
            assert (got[U == 0] == 0).all(), c.name
            ru = float((np.abs(got - U)[U > 0] / (1e-13 * U[U > 0])).max()) if (U > 0).any() else 0.0
            rm = float((np.abs(gm - m)[mm > 0] / (1e-13 * mm[mm > 0])).max()) if (mm > 0).any() else 0.0
            print(f"hd_restraint_feature_energy N={N} F={F} {c.name}: worst err / (1e-13 U) {ru:.3g}, err / (1e-13 sum |terms of m|) {rm:.3g}")
            assert (np.abs(got - U) <= 1e-13 * U).all(), (c.name, ru)
            assert (np.abs(gm - m) <= 1e-13 * mm).all() and (gm[mm == 0] == 0).all(), (c.name, rm)
            wu, wm = max(wu, ru), max(wm, rm)
        print(f"hd_restraint_feature_energy N={N} F={F}: worst err / (1e-13 U) {wu:.3g}, worst err / (1e-13 |m| terms) {wm:.3g}")
    finally:
        if bare is not None:
            bare.close()


def features_call(bare, W=2, S=1, band_rows=1, sum_rows=1, lo=0.0, hi=1.0, k=1.0, coef=1.0, sf=(0.0, 1.0, 1.0, 0.0), nv1=1.0, nb1=0.0, ratio=1.0,
                  null=()):
    F = 2
    nb, ns = max(1, abs(band_rows)) * max(1, W) * F, max(1, abs(sum_rows)) * max(1, S)
    arr = lambda v, n: (C.c_float * n)(*([v] * n))
    a = dict(lo=arr(lo, nb), hi=arr(hi, nb), k=arr(k, nb), coef=arr(coef, ns * F), sum_f=(C.c_float * (4 * ns))(*(list(sf) * ns)))
    for name in null:
        a[name] = None
    return bare.lib.hd_restraint_features(bare.topo, a["lo"], a["hi"], a["k"], band_rows, W, a["coef"], a["sum_f"], sum_rows, S,
                                          nv1, nb1, ratio, stream())


def test_abi_refusals_and_the_bits_without_features():
    N, F = 5, 2
    nm = fr.masks_for(N)
    bare = Bare(F + 3, nm)
    lib = bare.lib
    nan, inf = math.nan, math.inf
    try:
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert features_call(bare) == 0, lib.hd_last_error()
        assert features_call(bare, W=N, S=8, band_rows=5, sum_rows=5, lo=-inf, hi=inf) == 0, lib.hd_last_error()
        assert features_call(bare, W=0, null=("lo", "hi", "k")) == 0 and features_call(bare, S=0, null=("coef", "sum_f")) == 0
        bad = [dict(W=-1), dict(W=N + 1), dict(S=-1), dict(S=9), dict(band_rows=2), dict(band_rows=0), dict(sum_rows=3), dict(k=nan), dict(k=inf),
               dict(coef=nan), dict(coef=inf), dict(nv1=nan), dict(nv1=inf), dict(nb1=nan), dict(nb1=-inf), dict(ratio=nan), dict(ratio=inf),
               dict(lo=2.0, hi=1.0), dict(lo=nan), dict(hi=nan), dict(sf=(2.0, 1.0, 1.0, 0.0)), dict(sf=(nan, 1.0, 1.0, 0.0)), dict(sf=(0.0, nan, 1.0, 0.0)),
               dict(sf=(0.0, 1.0, nan, 0.0)), dict(sf=(0.0, 1.0, inf, 0.0)), dict(sf=(0.0, 1.0, 1.0, 2.0)), dict(sf=(0.0, 1.0, 1.0, 0.5)),
               dict(sf=(0.0, 1.0, 1.0, nan)), dict(null=("lo",)), dict(null=("hi",)), dict(null=("k",)), dict(null=("coef",)), dict(null=("sum_f",))]
        for kw in bad:
            assert features_call(bare, **kw) == -1, kw
            assert b"hd_restraint_features" in lib.hd_last_error()
        assert bare.lib.hd_restraint_features(None, None, None, None, 1, 0, None, None, 1, 0, 1.0, 0.0, 1.0, stream()) == -1
        # HD_E_STATE: restraints attached but no features; no restraints
        z = torch.randn(5, N, F + 3, device=DEV)
        e = torch.randn(5, N, F + 3, device=DEV)
        out = torch.full_like(e, 7.0)
        u = torch.full((5, 2), -1.0, device=DEV, dtype=torch.float64)
        r4 = (C.c_float * 4)(0.8, 0.5, 0.75, inf)
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), r4, out.data_ptr(), stream()) == -4
        assert lib.hd_restraint_feature_energy(bare.h, bare.topo, z.data_ptr(), u.data_ptr(), None, stream()) == -4
        assert features_call(bare) == 0
        assert features_call(bare, W=0, S=0) == 0             # ... which clears them
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), r4, out.data_ptr(), stream()) == -4
        assert features_call(bare) == 0
        assert lib.hd_restrain_feat(bare.h, bare.topo, None, e.data_ptr(), r4, out.data_ptr(), stream()) == -1
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), (C.c_float * 4)(0.0, 0.5, 0.75, inf), out.data_ptr(), stream()) == -1
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), r4, z.data_ptr(), stream()) == -1           # out overlaps z
        assert lib.hd_restraint_feature_energy(bare.h, bare.topo, None, u.data_ptr(), None, stream()) == -1
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), r4, out.data_ptr(), stream()) == 0, lib.hd_last_error()
        # a call of hd_restraint_attach alone forgets the features
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert lib.hd_restraint_feature_energy(bare.h, bare.topo, z.data_ptr(), u.data_ptr(), None, stream()) == -4
        assert (u.cpu() == -1.0).all() and lib.hd_restraint_detach(bare.topo) == 0
        assert features_call(bare) == -4 and b"hd_restraint_attach" in lib.hd_last_error()
        assert lib.hd_restrain_feat(bare.h, bare.topo, z.data_ptr(), e.data_ptr(), r4, out.data_ptr(), stream()) == -4
        # every k = 0: eps bit for bit
        c = next(iter(fr.kernel_cases(N, F)))
        k0 = Features(c.ft.lo, c.ft.hi, 0.0, [FeatureSum(r.coef, r.lo, r.hi, 0.0, r.reduce) for r in c.ft.sums] or [FeatureSum(np.ones(F), hi=0.0, k=0.0)])
        assert torch.equal(run_feat(bare, c, False, rs=Restraints(features=k0)), c.eps)
    finally:
        bare.close()


# ----------------------------------------------------------------------------- chains against the restatement over the oracle

K, T = fr.CHAIN_K, fr.CHAIN_T
RKW = dict(restraint_scale=torch.tensor(fr.CHAIN_SCALE), restraint_clip=fr.CHAIN_CLIP)


@functools.lru_cache(maxsize=None)
def model_for(precision, C_=0):
    """The models of tests/test_gpu_restraint.py with the normalisation constants of the chain references."""
    from hierdiff_amd import DiffusionQM9, default_config
    from tests import edit_reference as er
    H, L = fr.CHAIN_SHAPES[precision]
    sd_np, _ = er.weights(H, L, C_=C_)
    cfg = default_config(hidden_nf=H, n_layers=L, context_node_nf=C_, timesteps=T)
    cfg.norm_values, cfg.norm_biases = list(fr.CHAIN_NORM[0]), list(fr.CHAIN_NORM[1])
    m = DiffusionQM9(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd_np.items()})
    m.dynamics.precision = precision
    m = m.to(DEV)
    m.seed = SEED
    return m


def check_states(what, got, ref):
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        e = rel_l2(g.cpu().numpy(), r.numpy())
        worst = max(worst, e)
        print(f"featured chain {what} state {k + 1}/{len(ref)}: rel_l2 {e:.2e} (bar {REL_L2_TOL:.0e})")
        assert torch.isfinite(g).all()
        assert e <= REL_L2_TOL, (what, k, e)
    return worst


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("kind", ["features", "features+obstacles guided", "sde2m", "x0"])
def test_featured_chain_against_the_restatement(kind, precision):
    """T = 8, K = 4, B = 4 with injected normals: features only (eta = 1); features + obstacles under guidance with context; the sde2m
    solver; record="x0" (the frames show the featured data prediction)."""
    c = fr.chain_reference(kind, precision)
    model = fresh(model_for(precision, 1 if c["guided"] else 0))
    nm, em, ctx, raws = c["nm"], c["em"], c["ctx"], c["raws"]
    kw = dict(steps=K, restraints=c["rs"], **RKW)
    kw.update(dict(solver="sde2m") if kind == "sde2m" else dict(eta=1.0))
    if c["guided"]:
        kw.update(guidance_scale=2.0)
    if kind == "x0":
        x, h, chain = model.sample_from_latent(dev(c["z"]), dev(nm), dev(em), None, raw_noises=raws[1:], keep_frames=K, record="x0", **kw)
        assert torch.isfinite(chain).all() and torch.equal(chain[0], torch.cat([x, h], dim=2))
        worst = 0.0
        for k in range(K - 1):                                # transition k writes frame K - 1 - k; frame 0 is the decode
            r = rel_l2(chain[K - 1 - k].cpu().numpy(), c["frames"][k].numpy())
            worst = max(worst, r)
            print(f"featured chain x0 [{precision}] frame of transition {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
            assert r <= REL_L2_TOL, (k, r)
        x2, h2 = model.sample_from_latent(dev(c["z"]), dev(nm), dev(em), None, raw_noises=raws[1:], **kw)
        assert torch.equal(x2, x) and torch.equal(h2, h)       # recording changes no sample
    else:
        zz, got = dev(c["z"]), []
        for k in range(K):
            zz = model.latent_steps(zz, dev(nm), dev(em), dev(ctx), k_lo=k, k_hi=k + 1, raw_noises=[raws[1 + k]], **kw)
            got.append(zz)
        worst = check_states(f"{kind} [{precision}]", got, c["states"])
    d = rel_l2(c["states"][-1].numpy(), c["plain"].numpy())
    print(f"featured chain {kind} [{precision}]: worst {worst:.2e}; the features moved eps^ in {c['active']} of {c['calls']} network calls; "
          f"distance of the featured z_0 from the unfeatured one {d:.2e}")
    assert c["active"] == c["calls"] == K and d > 10 * REL_L2_TOL


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("R", [1, 2])
def test_featured_framed_inpainting_chain_against_the_restatement(R, precision):
    """sample_inpaint(restraint_frame="known") with features only: the term acts on every valid node, the replacement step overwrites
    the known elements afterwards."""
    c = fr.chain_reference(f"inpaint R={R}", precision)
    model = fresh(model_for(precision))
    nm, fm = c["nm"], c["fm"]
    x, h, chain, info = model.sample_inpaint(dev(nm), dev(fm), dev(c["xk"]), dev(c["hk"]), sample_id_base=fr.INPAINT_BASE, keep_frames=K,
                                             record="z", steps=K, resamplings=R, restraints=c["rs"], restraint_frame="known", **RKW)
    assert torch.isfinite(chain).all()
    nv, nb = c["norm"]
    worst = 0.0
    for k in range(K - 1):                                    # transition k arrives at position K - 1 - k
        ref = fr.unnormalize(c["states"][k], nm, nv[0], nv[1], nb[1])
        r = rel_l2(chain[K - 1 - k].cpu().numpy(), ref.numpy())
        worst = max(worst, r)
        print(f"featured framed inpainting R={R} [{precision}] state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
        assert r <= REL_L2_TOL, (R, precision, k, r)
    print(f"featured framed inpainting R={R} [{precision}]: worst state {worst:.2e}; the features moved eps^ in {c['active']} of {c['calls']}")
    assert c["calls"] == K * R and c["active"] == c["calls"]
    fe = info["restraint_feature_energy"].cpu()
    assert fe.shape == (4, 2) and fe.dtype == torch.float64 and info["feature_sums"].shape == (4, 2) and info["restraint_energy"].shape == (4, 3)
    U, _, _, m, _ = fr.feature_energy_grad(c["rs"].features, h.cpu().numpy(), nm)
    assert (np.abs(fe.numpy() - U) <= 1e-12 * np.maximum(U, 1.0)).all()
    assert (np.abs(info["feature_sums"].cpu().numpy() - m) <= 1e-12 * np.maximum(np.abs(m), 1.0)).all()


@pytest.mark.parametrize("precision", BOTH)
def test_featured_steered_chain_against_the_reference(precision):
    """P = 4, restraint_scale = 0: selection on U_feat alone.  Per state rel-L2 <= 1e-4; ancestors and roots of every transition
    exactly."""
    lib = _lib.load()
    c = fr.chain_reference("steered", precision)
    model = fresh(model_for(precision))
    nm, em = c["nm"], c["em"]
    B, N = nm.shape[:2]
    kw = dict(steps=K, eta=1.0, restraints=c["rs"], particles=fr.STEER_P, steer_scale=fr.STEER_BETA, steer_ess=fr.STEER_RHO,
              sample_id_base=fr.STEER_BASE, restraint_scale=0.0)
    model.seed = fr.STEER_SEED
    try:
        nmd, emd = dev(nm), dev(em)
        topo = model.dynamics.topology(nmd, emd, B, N)
        zz, worst = dev(c["z"]), 0.0
        roots = np.arange(B) % fr.STEER_P
        assert any(i["resampled"].any() for i in c["infos"])
        for k in range(K):
            zz = model.path_steps(zz, nmd, emd, k_lo=k, k_hi=k + 1, **kw)
            logw, uprev, root, anc, stats = read_state(lib, topo.ptr, B, B // fr.STEER_P)
            r = rel_l2(zz.cpu().numpy(), c["states"][k].numpy())
            worst = max(worst, r)
            print(f"featured steered chain [{precision}] state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e}), resampled "
                  f"{c['infos'][k]['resampled'].tolist()}")
            assert (anc == c["infos"][k]["anc"]).all(), (k, anc, c["infos"][k]["anc"])
            roots = roots[c["infos"][k]["anc"]]
            assert (root == roots).all(), k
            assert r <= REL_L2_TOL, (k, r)
        assert (root == c["state"].root).all() and (stats[:, 0] == c["state"].stats[:, 0]).all()
        print(f"featured steered chain [{precision}]: worst state {worst:.2e}; events {c['state'].stats[:, 0].tolist()}")
    finally:
        model.seed = SEED


# ----------------------------------------------------------------------------- graph behaviour

def test_graph_replay_reattaching_and_the_unfeatured_call():
    """On a topology of its own (masks no other test of this module uses: the buffers start empty).  The graph pass comes first;
    plain launches then reproduce every result bit for bit."""
    from tests import edit_reference as er
    lib = _lib.load()
    model = model_for("fp32")
    _, _, nm, em, _ = er.molecules([6, 5, 2])
    nmd, N = dev(nm), nm.shape[1]
    kw = dict(sample_id_base=3, steps=4, eta=0.5, restraint_scale=0.05, restraint_clip=0.3)
    obs = fr.chain_obstacles()
    cf = fr.chain_features
    sets = dict(a=Restraints(obs, features=cf()), b=Restraints(obs, features=cf(shift=0.25)), s1=Restraints(obs, features=cf(S=1)),
                w4=Restraints(obs, features=cf(W=4, S=1)), rows=Restraints(obs, features=cf(W=4, S=1, rows=3)),
                k0=Restraints(obs, features=Features.target(cf().lo, 0.0, 0.0, [FeatureSum(r.coef, r.lo, r.hi, 0.0, r.reduce) for r in cf().sums])),
                never=Restraints(obs), only=Restraints(features=cf()))
    call = lambda k, **more: model.sample_from_masks(nmd, None, None, restraints=sets[k], **{**kw, **more})
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 3, N)
    builds = lambda: lib.hd_path_graph_builds(topo.ptr)
    got, n0 = {}, builds()
    same = lambda out, k: torch.equal(out[0], got[k][0]) and torch.equal(out[1], got[k][1])
    got["a"] = call("a")
    assert builds() == n0 + 1
    assert same(call("a"), "a") and builds() == n0 + 1        # graph replay against the first run
    got["b"] = call("b")                                      # same-size tables: a copy, no rebuild
    assert same(call("a"), "a") and builds() == n0 + 1
    got["k0"] = call("k0")                                    # k = 0: the same sizes again
    assert builds() == n0 + 1
    got["s1"] = call("s1")                                    # another S: one rebuild
    assert builds() == n0 + 2
    got["w4"] = call("w4")                                    # another W: one rebuild
    assert builds() == n0 + 3
    got["rows"] = call("rows")                                # other row counts: one rebuild
    assert builds() == n0 + 4
    got["sigma"] = call("rows", restraint_schedule="sigma")   # another ratio (and other rows of the same K: a copy): one rebuild
    # (its bits may equal those of "score": under the clip of 0.3 every step of either schedule is the clipped one)
    assert builds() == n0 + 5
    got["never"] = call("never")                              # an unfeatured call afterwards rebuilds ...
    assert builds() == n0 + 6
    assert same(call("never"), "never") and builds() == n0 + 6
    assert same(call("rows"), "rows") and builds() == n0 + 7
    got["only"] = call("only")
    assert not same(got["b"], "a") and not same(got["never"], "a") and not same(got["s1"], "a") and not same(got["w4"], "s1")
    assert same(got["rows"], "w4")                            # the same rows, materialised per molecule
    assert same(got["k0"], "never")                           # every k = 0: the bits of the featureless call
    fresh(model, graph=False)                                 # graph replay equals plain launches bit for bit
    for k in sets:
        assert same(call(k), k), k
    assert same(call("rows", restraint_schedule="sigma"), "sigma")
    # ... and gives the bits of a topology that never had features
    _, _, nm2, _, _ = er.molecules([6, 5, 2, 1])
    fresh2 = model.sample_from_masks(dev(nm2), None, None, restraints=sets["never"], **kw)
    assert torch.equal(fresh2[0][:3, :N], got["never"][0]) and torch.equal(fresh2[1][:3, :N], got["never"][1])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_molecule_depends_on_its_id_and_its_own_rows_only_and_chains_may_be_cut(graph):
    from oracle import egnn_oracle as orc
    from tests import edit_reference as er
    model = fresh(model_for("fp32"), graph)
    _, _, nm, em, _ = er.molecules([7, 4, 1, 6])
    B, N = nm.shape[:2]
    g = np.random.Generator(np.random.PCG64(1))
    per = Features.target(g.normal(0.3, 1.5, (B, 4, 8)), 1.5, 0.25,
                          [FeatureSum(g.normal(0.0, 1.0, 8), lo=g.normal(0.0, 1.0, B) - 1.0, hi=g.normal(0.0, 1.0, B) + 1.0, reduce="mean")])
    rs = Restraints(obstacles=fr.chain_obstacles(), features=per)
    scale = torch.tensor([0.05, 0.03, 0.05, 0.08])
    kw = dict(steps=4, eta=1.0, restraint_clip=0.3)
    whole = model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=rs, restraint_scale=scale, **kw)
    for lo, hi in ((0, 1), (1, 2), (2, 4)):                   # batch cuts of one and of two molecules
        part = model.sample_from_masks(dev(nm[lo:hi]), None, None, sample_id_base=11 + lo, restraints=rs.slice(lo, hi),
                                       restraint_scale=scale[lo:hi], **kw)
        assert torch.equal(part[0], whole[0][lo:hi]) and torch.equal(part[1], whole[1][lo:hi]), (lo, hi)
    other = Restraints(obstacles=fr.chain_obstacles(), features=Features(per.lo + 0.5, per.hi + 0.5, per.k, per.sums))
    assert not torch.equal(model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=other, restraint_scale=scale, **kw)[1],
                           whole[1])
    # path_steps: one piece equals the pieces
    raws = er.raw_draws(1, B, N, seed=2)
    z = dev(orc.combined_noise(raws[0][0], raws[0][1], nm.float()))
    pk = dict(sample_id_base=5, steps=4, eta=1.0, restraints=rs, restraint_scale=scale, restraint_clip=0.3)
    one = model.path_steps(z, dev(nm), dev(em), k_lo=0, k_hi=4, **pk)
    zz = z
    for lo, hi in ((0, 1), (1, 3), (3, 4)):
        zz = model.path_steps(zz, dev(nm), dev(em), k_lo=lo, k_hi=hi, **pk)
    assert torch.equal(zz, one)


# ----------------------------------------------------------------------------- results

def test_results_carry_the_feature_entries():
    model = fresh(model_for("fp32"))
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]], features=fr.chain_features())
    torch.manual_seed(3)
    on = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    torch.manual_seed(3)
    bare = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]]),
                        restraint_scale=0.05, restraint_clip=0.3)
    assert all("restraint_feature_energy" not in r and "feature_sums" not in r and r["restraint_energy"].shape == (3,) for r in bare)
    for r in on:
        n = r["x"].shape[0]
        fe, fs = r["restraint_feature_energy"], r["feature_sums"]
        assert fe.shape == (2,) and fe.dtype == torch.float64 and fs.shape == (2,) and fs.dtype == torch.float64 and r["restraint_energy"].shape == (3,)
        U, _, _, m, _ = fr.feature_energy_grad(rs.features, r["h"].unsqueeze(0).numpy(), np.ones((1, n)))
        assert (np.abs(fe.numpy() - U[0]) <= 1e-12 * np.maximum(U[0], 1.0)).all() and (np.abs(fs.numpy() - m[0]) <= 1e-12 * np.maximum(np.abs(m[0]), 1.0)).all()
        cpu_U, cpu_m = rs.feature_energy(r["h"].unsqueeze(0), torch.ones(1, n, 1), return_sums=True)       # the CPU formulas of the product
        assert torch.allclose(fe, cpu_U[0], rtol=1e-9, atol=1e-12) and torch.allclose(fs, cpu_m[0], rtol=1e-9, atol=1e-12)
    var = model.vary(bare[:2], DEV, 4, n_variants=2, steps=2, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    assert len(var) == 4 and all(r["restraint_feature_energy"].shape == (2,) and r["feature_sums"].shape == (2,) for r in var)
