"""GPU tier (-m gpu) of the template restraints: the template term of hd_restrain_eps / hd_restrain_eps_framed and
hd_restraint_template_energy against the float64 restatement of tests/template_reference.py (rotation by SVD, not the kernel's
Jacobi), templated chains (plain, guided, sde2m, framed inpainting, steered) against that restatement over the oracle, and the
contracts of the device path: bits without templates, graph replay, re-attaching, batch and chain cuts, result entries, refusals.

Bars.  eps: the element-wise bar of tests/field_reference.py - every element within 8 * 2^-23 of the sum of the absolute values of
its terms.  The energy call: U relative 1e-13, R element-wise 1e-12 and |det R - 1| <= 1e-12 on the conditioned cases (conditioning
measure >= 0.05, asserted on the CPU by tests/test_template_cpu.py); the two named degenerate cases in energy and finiteness only.
The energy of the exact-fit case is a rounding residue of the fp32 template positions (~1e-13 in absolute terms), for which a
relative bar says nothing about the kernel: it is held to 1e-13 of the sum of the absolute terms instead, like the gradient.
Chains: rel-L2 < 1e-4 per state (tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: B = 5 molecules of N in {5, 33} nodes at D in {4, 11}, NT in {1, 2, 4} templates of M in {3, 20} rows; chains at T = 8, K = 4
on the models of tests/test_gpu_restraint.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.restraints import Restraints, Template
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import restraint_frame_reference as rf
from tests import restraint_reference as rr
from tests import sampling_reference as sref
from tests import steer_reference as st
from tests import template_reference as tr
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_field import Bare, run_eps, run_states
from tests.test_gpu_restraint import BOTH, DEV, T, batch_for, dev, model_for, reference_states, stream
from tests.test_gpu_restraint_frame import chain_case
from tests.test_gpu_steer import fresh, read_state
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]


# ----------------------------------------------------------------------------- the kernels, on a bare handle (any D)

def template_energy(bare, c, x):
    NT = c.rs.n_templates
    out = torch.full((c.B, NT), -1.0, device=DEV, dtype=torch.float64)
    fit = torch.full((c.B, NT, 16), -1.0, device=DEV, dtype=torch.float64)
    xd = dev(x).contiguous()
    rc = bare.lib.hd_restraint_template_energy(bare.h, bare.topo, xd.data_ptr(), out.data_ptr(), fit.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    out2 = torch.full_like(out, -1.0)                         # fit16 may be NULL
    assert bare.lib.hd_restraint_template_energy(bare.h, bare.topo, xd.data_ptr(), out2.data_ptr(), None, stream()) == 0
    assert torch.equal(out, out2)
    return out.cpu().numpy(), fit.cpu().numpy()


@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_restrain_eps_with_templates_against_float64(N, D, framed):
    what = f"{'hd_restrain_eps_framed' if framed else 'hd_restrain_eps'} N={N} D={D}"
    bare, worst, moved, cases = None, 0.0, 0, 0
    try:
        for c in tr.kernel_cases(N, D, framed):
            bare = Bare(D, c.nm) if bare is None else bare
            got = run_eps(bare, c, alias=False)
            assert torch.equal(got, run_eps(bare, c, alias=True))             # in place
            assert torch.isfinite(got).all(), c.name
            e, g_, valid = c.eps.numpy(), got.numpy(), c.nm.numpy()
            assert (g_[:, :, 3:] == e[:, :, 3:]).all() and (g_[~valid] == e[~valid]).all()
            if c.degenerate:                                  # R is not unique: the gradient may be any maximiser's
                continue
            ref, mag = tr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known)
            bound = sref.BOUND * sref.U * mag
            err = np.abs(got.double().numpy() - ref)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            print(f"{what} {c.name}: worst err / bound {ratio:.3f}")
            assert (err <= bound).all(), (what, c.name, ratio)
            worst = max(worst, ratio)
            cases += 1
            # the template term itself moved eps: the same call without the templates differs
            moved += int(not torch.equal(got, run_eps(bare, c, False, rs=tr.with_templates(c.rs, []))))
            if framed:
                assert (g_[2] == e[2]).all()                  # every valid node fixed: eps^ unchanged, bit for bit
                assert (g_[4] == e[4]).all()                  # one valid node: the projection removes its whole step
        print(f"{what}: worst err / bound over {cases} cases {worst:.3f}; the templates moved eps in {moved}")
        assert moved == cases
    finally:
        if bare is not None:
            bare.close()


@pytest.mark.parametrize("N", [5, 33])
def test_restraint_template_energy_against_float64(N):
    """On the data predictions of the kernel cases (fp32 positions, so the restatement sees the same numbers)."""
    bare, wu, wr, wd = None, 0.0, 0.0, 0.0
    try:
        for c in tr.kernel_cases(N, 11, False):
            if not math.isinf(c.row[3]):
                continue                                      # (the clip does not enter the energy)
            bare = Bare(11, c.nm) if bare is None else bare
            x = rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).contiguous()
            c.rs.attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
            got, fit = template_energy(bare, c, x)
            U, _, _, _, fits = tr.template_energy_grad(c.rs, x.numpy(), c.nm)
            assert np.isfinite(got).all() and np.isfinite(fit).all(), c.name
            if c.name == "exact fit":                         # a rounding residue (module docstring): 1e-13 of the absolute terms
                mags = np.array([[0.0 if f is None else 0.5 * t.k * float((f["w"] * (f["rm"] ** 2).sum(1)).sum())
                                  for f, t in zip(row, c.rs.templates)] for row in fits])
                assert (np.abs(got - U) <= 1e-13 * mags).all(), c.name
                assert got[0, 0] < 1e-10
            else:
                err = np.abs(got - U)
                assert (got[U == 0] == 0).all(), c.name
                ratio = float((err[U > 0] / (1e-13 * U[U > 0])).max()) if (U > 0).any() else 0.0
                wu = max(wu, ratio)
                print(f"hd_restraint_template_energy N={N} {c.name}: worst err / (1e-13 U) {ratio:.3g}")
                assert (err <= 1e-13 * U).all(), (c.name, ratio)
            for b in range(c.B):
                for j, f in enumerate(fits[b]):
                    R = fit[b, j, :9].reshape(3, 3)
                    wd = max(wd, abs(np.linalg.det(R) - 1.0))
                    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, (c.name, b, j)
                    if c.degenerate:
                        continue
                    want = tr.fit16(f)
                    wr = max(wr, float(np.abs(fit[b, j, :9] - want[:9]).max()))
                    assert (np.abs(fit[b, j, :9] - want[:9]) <= 1e-12).all(), (c.name, b, j)
                    assert (np.abs(fit[b, j, 9:] - want[9:]) <= 1e-12 * (1.0 + np.abs(want[9:]))).all(), (c.name, b, j)
        print(f"hd_restraint_template_energy N={N}: worst err / (1e-13 U) {wu:.3g}, worst |R - R_svd| {wr:.3g}, worst |det R - 1| {wd:.3g}")
    finally:
        if bare is not None:
            bare.close()


def templates_call(bare, NT=1, rows=1, M=3, idx=True, f=True, geom=(1.0, 0.0), y=(0.0, 0.0, 0.0), w=1.0):
    n = max(1, abs(rows)) * max(1, NT) * max(1, M)
    i = (C.c_int * n)(*([0] * n))
    fv = (C.c_float * (4 * n))(*(list(y) + [w]) * n)
    g = (C.c_float * len(geom))(*geom)
    return bare.lib.hd_restraint_templates(bare.topo, NT, rows, M, i if idx else None, fv if f else None, g, stream())


def test_bits_without_an_active_template_and_abi_refusals():
    N, D = 33, 4
    c = next(iter(tr.kernel_cases(N, D, False)))
    bare = Bare(D, c.nm)
    lib = bare.lib
    try:
        for pqa in (False, True):
            tabs = rr.random_tables(5, N, 7, 3, 2, 5, True)[0] if pqa else None
            base = tr.with_templates(tabs, [])
            want = run_eps(bare, c, False, rs=base)           # a topology that never had templates
            assert pqa == (not torch.equal(want, c.eps))
            live = tr.make_templates(2, 20, 5, N, 4, True)
            assert not torch.equal(run_eps(bare, c, False, rs=tr.with_templates(tabs, live)), want)
            # after hd_restraint_attach alone the templates of the previous call are gone
            assert torch.equal(run_eps(bare, c, False, rs=base), want)
            # k = 0; all weights 0: eps bit for bit
            k0 = [Template(t.index, t.positions, t.weights, k=0.0, fit=t.fit) for t in live]
            assert torch.equal(run_eps(bare, c, False, rs=tr.with_templates(tabs, k0)), want)
            w0 = [Template(t.index, t.positions, torch.zeros_like(t.weights), k=t.k, fit=t.fit) for t in live]
            assert torch.equal(run_eps(bare, c, False, rs=tr.with_templates(tabs, w0)), want)
            # hd_restraint_templates(NT = 0) clears them
            tr.with_templates(tabs, live).attach(bare, c.scale, c.nv0, torch.device(DEV), stream())
            assert lib.hd_restraint_templates(bare.topo, 0, 1, 0, None, None, None, stream()) == 0, lib.hd_last_error()
            zd, ed = dev(c.z).contiguous(), dev(c.eps).contiguous()
            out = torch.full_like(ed, 7.0)
            assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(*c.row), out.data_ptr(), stream()) == 0
            assert torch.equal(out.cpu(), want)
        # refusals: HD_E_INVALID for every bad argument, with restraints attached
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert templates_call(bare) == 0, lib.hd_last_error()
        assert templates_call(bare, rows=5, NT=4, M=20) == 0, lib.hd_last_error()
        bad = [dict(NT=-1), dict(NT=5), dict(M=0), dict(M=-3), dict(rows=2), dict(rows=0), dict(geom=(-1.0, 0.0)), dict(geom=(math.inf, 0.0)),
               dict(geom=(math.nan, 0.0)), dict(geom=(1.0, 2.0)), dict(geom=(1.0, 0.5)), dict(geom=(1.0, math.nan)), dict(w=-1.0), dict(w=math.inf),
               dict(w=math.nan), dict(y=(0.0, math.inf, 0.0)), dict(y=(math.nan, 0.0, 0.0)), dict(idx=False), dict(f=False)]
        for kw in bad:
            assert templates_call(bare, **kw) == -1, kw
            assert b"hd_restraint_templates" in lib.hd_last_error()
        # HD_E_STATE: no templates; no restraints
        x, out = torch.zeros(5, N, 3, device=DEV), torch.full((5, 4), -1.0, device=DEV, dtype=torch.float64)
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert lib.hd_restraint_template_energy(bare.h, bare.topo, x.data_ptr(), out.data_ptr(), None, stream()) == -4
        assert (out.cpu() == -1.0).all()                      # nothing written
        assert templates_call(bare) == 0
        assert lib.hd_restraint_template_energy(bare.h, bare.topo, None, out.data_ptr(), None, stream()) == -1
        assert lib.hd_restraint_detach(bare.topo) == 0
        assert templates_call(bare) == -4 and b"hd_restraint_attach" in lib.hd_last_error()
        assert lib.hd_restraint_template_energy(bare.h, bare.topo, x.data_ptr(), out.data_ptr(), None, stream()) == -4
    finally:
        bare.close()


# ----------------------------------------------------------------------------- chains against the restatement over the oracle

K = 4
SCALE = torch.tensor([0.05, 0.02, 0.05])
RKW = dict(restraint_scale=SCALE, restraint_clip=0.3)


def chain_templates(centre=(0.0, 0.0, 0.0), shift=0.0, M=5, NT=2, rows=None):
    """A rigid arrangement of the first M nodes and a translation-only triangle: in the molecules of 7, 4 and 1 nodes the first has
    every row active, the second loses the rows on nodes it lacks, the third keeps one row (nothing)."""
    g = np.random.Generator(np.random.PCG64(5))
    y = g.normal(0.0, 1.5, (M, 3)) + np.asarray(centre) + np.array([shift, 0.0, 0.0]) * np.arange(M)[:, None]
    w = g.uniform(0.5, 2.0, M)
    tri = g.normal(0.0, 1.5, (3, 3)) + np.asarray(centre)
    rep = (lambda a: a) if rows is None else (lambda a: np.broadcast_to(a, (rows,) + np.shape(a)).copy())
    return [Template(rep(np.arange(M)), rep(y), rep(w), k=1.5), Template([0, 2, 3], tri, k=1.0, fit="translation")][:NT]


def obstacles():
    return [[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]]


def check_states(what, got, ref):
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        e = rel_l2(g.cpu().numpy(), r.numpy())
        worst = max(worst, e)
        print(f"templated chain {what} state {k + 1}/{len(ref)}: rel_l2 {e:.2e} (bar {REL_L2_TOL:.0e})")
        assert torch.isfinite(g).all()
        assert e < REL_L2_TOL, (what, k, e)
    return worst


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("kind", ["template", "template+obstacles guided", "sde2m"])
def test_templated_chain_against_the_restatement(kind, precision):
    """T = 8, K = 4 with injected normals: templates only (eta = 1); templates + obstacles under guidance; the sde2m solver."""
    guided = "guided" in kind
    C_ = 1 if guided else 0
    model, sd_np, cfg = model_for(precision, C_)
    fresh(model)
    _, _, nm, em, ctx = batch_for((7, 4, 1), C_)
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 1, B, N, seed=K)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    rs = Restraints(obstacles=obstacles() if guided else None, templates=chain_templates())
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
    tnet = tr.TemplateNet(inner, rs, SCALE, rr.rows_from_grid(gg, path, "score", 0.3), nm=nm)
    off = tr.TemplateNet(inner, Restraints(), torch.zeros(B), {}, nm=nm)
    kw = dict(steps=K, restraints=rs, **RKW)
    if kind == "sde2m":
        from tests import sde_solver_reference as sd
        ref = [r[0] for r in sd.chain_ref(tnet.net, gg, path, z, nm.float(), raws[1:])]
        plain = [r[0] for r in sd.chain_ref(off.net, gg, path, z, nm.float(), raws[1:])]
        kw.update(solver="sde2m")
    else:
        ref = reference_states(tnet, gg, path, 1.0, z, nm, raws[1:], None)
        plain = reference_states(off, gg, path, 1.0, z, nm, raws[1:], None)
        kw.update(eta=1.0)
    if guided:
        kw.update(guidance_scale=2.0)
    got = run_states(model, z, nm, em, ctx, raws[1:], **kw)
    worst = check_states(f"{kind} [{precision}]", got, ref)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"templated chain {kind} [{precision}]: worst state {worst:.2e}; the templates moved eps^ in {tnet.active} of {tnet.calls} "
          f"network calls; distance of the templated z_0 from the unrestrained one {d:.2e}")
    assert tnet.active == tnet.calls == K
    assert d > 10 * REL_L2_TOL


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("R", [1, 2])
def test_templated_framed_inpainting_chain_against_the_restatement(R, precision):
    """sample_inpaint(restraint_frame="known") with templates: rows on fixed nodes take part in the fit, only free nodes gather."""
    lib = _lib.load()
    model, sd_np, cfg = model_for(precision)
    fresh(model)
    nm, em, ctx, fm, xk, hk = chain_case()
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    ids = [9 + b for b in range(B)]
    rs = Restraints(templates=chain_templates(centre=rf.CENTRE))
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    xh_known = torch.cat([xk, hk], dim=2) * fm.float()
    rows = rr.rows_from_grid(gg, path, "score", 0.3)
    tnet = tr.TemplateNet(net, rs, SCALE, rows, nm=nm, fm=fm, known=xh_known)
    off = tr.TemplateNet(net, Restraints(), torch.zeros(B), {}, nm=nm, fm=fm, known=xh_known)
    z = orc.combined_noise(*rf.philox_raw(lib, SEED, ids, 0, N), nm.float())
    ref = rf.inpaint_path_ref(lib, tnet, gg, path, T, z, nm, fm, xh_known, R, SEED, ids)
    plain = rf.inpaint_path_ref(lib, off, gg, path, T, z, nm, fm, xh_known, R, SEED, ids)
    x, h, chain, info = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), sample_id_base=9, keep_frames=K, record="z", steps=K,
                                             resamplings=R, restraints=rs, restraint_frame="known", **RKW)
    assert torch.isfinite(chain).all()
    worst = 0.0
    for k in range(K - 1):                                    # transition k arrives at position K - 1 - k
        r = rel_l2(chain[K - 1 - k].cpu().numpy(), ref[k].numpy())
        worst = max(worst, r)
        print(f"templated framed inpainting R={R} [{precision}] state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
        assert r < REL_L2_TOL, (R, precision, k, r)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"templated framed inpainting R={R} [{precision}]: worst state {worst:.2e}; the templates moved eps^ in {tnet.active} of "
          f"{tnet.calls} network calls; distance of the templated z_0 from the unrestrained one {d:.2e}")
    assert tnet.calls == K * R and tnet.active == tnet.calls
    assert d > 10 * REL_L2_TOL
    # the info dict: the template entries of the returned x next to the unchanged [B, 3]
    te = info["restraint_template_energy"].cpu()
    assert te.shape == (B, 2) and te.dtype == torch.float64 and info["restraint_energy"].shape == (B, 3)
    U = tr.template_energy_grad(rs, x.cpu().numpy(), nm)[0]
    assert (np.abs(te.numpy() - U) <= 1e-12 * np.maximum(U, 1.0)).all()
    assert info["template_rmsd"].shape == (B, 2) and info["x_template_frame"].shape == (B, N, 3)


def test_templated_steered_chain_against_the_reference():
    """P = 4, templates only: per state rel-L2 < 1e-4 against `SteeredNet` weighing on the total with U_tpl; ancestors and roots of
    every transition exactly."""
    lib = _lib.load()
    for precision in BOTH:
        model, _, _ = model_for(precision)
        fresh(model)
        states, infos, state, zT, (nm, em) = tr.steered_reference(precision)
        B, N = nm.shape[:2]
        G = B // st.CHAIN_P
        kw = dict(eta=1.0, restraints=Restraints(templates=tr.steer_templates()), particles=st.CHAIN_P, steer_scale=tr.STEER_BETA,
                  steer_ess=st.CHAIN_RHO, sample_id_base=tr.STEER_BASE, restraint_scale=tr.STEER_SCALE, restraint_clip=0.3)
        nmd, emd = dev(nm), dev(em)
        topo = model.dynamics.topology(nmd, emd, B, N)
        zz, worst = dev(zT), 0.0
        roots = np.arange(B) % st.CHAIN_P
        assert any(i["resampled"].any() for i in infos)
        for k in range(T):
            zz = model.path_steps(zz, nmd, emd, k_lo=k, k_hi=k + 1, **kw)
            logw, uprev, root, anc, stats = read_state(lib, topo.ptr, B, G)
            r = rel_l2(zz.cpu().numpy(), states[k].numpy())
            worst = max(worst, r)
            print(f"templated steered chain [{precision}] state {k + 1}/{T}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e}), resampled "
                  f"{infos[k]['resampled'].tolist()}")
            assert (anc == infos[k]["anc"]).all(), (k, anc, infos[k]["anc"])
            roots = roots[infos[k]["anc"]]
            assert (root == roots).all(), k
            assert r < REL_L2_TOL, (k, r)
        assert (root == state.root).all() and (stats[:, 0] == state.stats[:, 0]).all()
        print(f"templated steered chain [{precision}]: worst state {worst:.2e}; events {state.stats[:, 0].tolist()}")


# ----------------------------------------------------------------------------- graph behaviour

def test_graph_replay_reattaching_and_the_untemplated_call():
    """On a topology of its own (masks no other test of this module uses: the buffers start empty).  The graph pass comes first - a
    buffer that the launches had already grown would hide the rebuild - and plain launches then reproduce every result bit for bit."""
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    _, _, nm, em, _ = batch_for((6, 5, 2))
    nmd, N = dev(nm), nm.shape[1]
    kw = dict(sample_id_base=3, steps=4, eta=0.5, restraint_scale=0.05, restraint_clip=0.3)
    obs = obstacles()
    ct = chain_templates
    sets = dict(a=Restraints(obs, templates=ct()), b=Restraints(obs, templates=ct(shift=0.25)), one=Restraints(obs, templates=ct(NT=1)),
                short=Restraints(obs, templates=ct(M=4, NT=1)), rows=Restraints(obs, templates=ct(M=4, NT=1, rows=3)),
                k0=Restraints(obs, templates=[Template(t.index, t.positions, t.weights, k=0.0, fit=t.fit) for t in ct()]),
                never=Restraints(obs))
    call = lambda k: model.sample_from_masks(nmd, None, None, restraints=sets[k], **kw)
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 3, N)
    builds = lambda: lib.hd_path_graph_builds(topo.ptr)
    got, n0 = {}, builds()
    same = lambda out, k: torch.equal(out[0], got[k][0]) and torch.equal(out[1], got[k][1])
    got["a"] = call("a")
    assert builds() == n0 + 1
    got["b"] = call("b")                                      # same-size tables: a copy, no rebuild
    assert same(call("a"), "a") and builds() == n0 + 1
    got["k0"] = call("k0")                                    # k = 0: the same sizes again
    assert builds() == n0 + 1
    got["one"] = call("one")                                  # another NT: one rebuild
    assert builds() == n0 + 2
    got["short"] = call("short")                              # another M: one rebuild
    assert builds() == n0 + 3
    got["rows"] = call("rows")                                # other row counts: one rebuild
    assert builds() == n0 + 4
    got["never"] = call("never")                              # an untemplated call afterwards rebuilds ...
    assert builds() == n0 + 5
    assert same(call("never"), "never") and builds() == n0 + 5
    assert same(call("rows"), "rows") and builds() == n0 + 6
    assert not same(got["b"], "a") and not same(got["never"], "a") and not same(got["one"], "a") and not same(got["short"], "one")
    assert same(got["rows"], "short")                         # the same rows, materialised per molecule
    assert same(got["k0"], "never")                           # k = 0: the bits of the template-less call
    fresh(model, graph=False)                                 # graph replay equals plain launches bit for bit
    for k in sets:
        assert same(call(k), k), k
    # ... and gives the bits of a topology that never had templates
    _, _, nm2, _, _ = batch_for((6, 5, 2, 1))
    fresh2 = model.sample_from_masks(dev(nm2), None, None, restraints=sets["never"], **kw)
    assert torch.equal(fresh2[0][:3, :N], got["never"][0]) and torch.equal(fresh2[1][:3, :N], got["never"][1])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_molecule_depends_on_its_id_and_its_own_rows_only_and_chains_may_be_cut(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    _, _, nm, em, _ = batch_for((7, 4, 1, 6))
    B, N = nm.shape[:2]
    g = np.random.Generator(np.random.PCG64(1))
    per = Template(np.stack([g.permutation(4) for _ in range(B)]), g.normal(0.0, 1.5, (B, 4, 3)), g.uniform(0.5, 2.0, (B, 4)), k=1.5)
    rs = Restraints(obstacles=obstacles(), templates=[per, chain_templates()[1]])
    scale = torch.tensor([0.05, 0.03, 0.05, 0.08])
    kw = dict(steps=4, eta=1.0, restraint_clip=0.3)
    whole = model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=rs, restraint_scale=scale, **kw)
    for lo, hi in ((0, 1), (1, 2), (2, 4)):                   # batch cuts of one and of two molecules
        part = model.sample_from_masks(dev(nm[lo:hi]), None, None, sample_id_base=11 + lo, restraints=rs.slice(lo, hi),
                                       restraint_scale=scale[lo:hi], **kw)
        assert torch.equal(part[0], whole[0][lo:hi]) and torch.equal(part[1], whole[1][lo:hi]), (lo, hi)
    other = Restraints(obstacles=obstacles(), templates=[Template(per.index, per.positions * 1.25, per.weights, k=1.5), chain_templates()[1]])
    assert not torch.equal(model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=other, restraint_scale=scale, **kw)[0],
                           whole[0])
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

def test_results_carry_the_template_entries():
    model, _, _ = model_for("fp32")
    fresh(model)
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]], templates=chain_templates())
    torch.manual_seed(3)
    on = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    torch.manual_seed(3)
    bare = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]]),
                        restraint_scale=0.05, restraint_clip=0.3)
    assert all("restraint_template_energy" not in r and "x_template_frame" not in r and r["restraint_energy"].shape == (3,) for r in bare)
    for r in on:
        n = r["x"].shape[0]
        te, rm, xt = r["restraint_template_energy"], r["template_rmsd"], r["x_template_frame"]
        assert te.shape == (2,) and te.dtype == torch.float64 and rm.shape == (2,) and r["restraint_energy"].shape == (3,)
        assert xt.shape == (n, 3) and xt.dtype == torch.float64
        x1, one = r["x"].unsqueeze(0), np.ones((1, n))
        U, _, _, _, fits = tr.template_energy_grad(rs, x1.numpy(), one)
        assert (np.abs(te.numpy() - U[0]) <= 1e-12 * np.maximum(U[0], 1.0)).all()
        f0 = fits[0][0]
        if f0 is not None and f0["cond"] >= tr.COND_MIN:
            want = (x1[0].double().numpy() - f0["cx"]) @ f0["R"] + f0["cy"]
            assert np.abs(xt.numpy() - want).max() < 1e-9
            assert abs(float(rm[0]) - math.sqrt(f0["q"] / f0["W"])) < 1e-10
        cpu_U, _ = rs.template_energy(x1, torch.ones(1, n, 1))                 # the CPU formulas of the product
        assert torch.allclose(te, cpu_U[0], rtol=1e-9, atol=1e-12)
        assert torch.allclose(r["restraint_energy"], rs.energy(x1.double(), torch.ones(1, n, 1))[0], rtol=1e-9, atol=1e-12)
    var = model.vary(bare[:2], DEV, 4, n_variants=2, steps=2, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    assert len(var) == 4 and all(r["restraint_template_energy"].shape == (2,) and r["x_template_frame"].shape == r["x"].shape for r in var)
    g = torch.Generator().manual_seed(4)
    known = [{"x": torch.tensor(rf.CENTRE) + torch.randn(k, 3, generator=g), "h": torch.randn(k, 8, generator=g)} for k in (3, 2)]
    grown = model.sample_grow(known, [7, 4], DEV, sample_id_base=2, steps=4, restraints=Restraints(templates=chain_templates(centre=rf.CENTRE)),
                              restraint_scale=0.05, restraint_clip=0.3, restraint_frame="known")
    assert all(r["restraint_template_energy"].shape == (2,) and r["frame_shift"].shape == (3,) and r["x_template_frame"].shape == r["x"].shape
               for r in grown)
