"""GPU tier (-m gpu) of the field restraints: the field term of hd_restrain_eps / hd_restrain_eps_framed and
hd_restraint_field_energy[_framed] against the float64 restatement of tests/field_reference.py, fielded chains (plain, guided and
recorded, sde2m, framed inpainting, steered) against that restatement over the oracle, and the contracts of the device path: bits
without fields, graph replay, re-attaching, batch independence, result entries, refusals.

Bars (the project's own).  eps: the element-wise bar of tests/sampling_reference.py - every element within 8 * 2^-23 of the sum of
the absolute values of its terms.  Energies: 1e-12 of the sum of the absolute values of their terms; tau: 1e-12 of mean_F|x| +
mean_F|x_known|.  Chains: rel-L2 < 1e-4 per state (tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: B = 3 (framed: 5) molecules of N in {5, 33} nodes at D in {4, 11}, NF in {1, 3, 8} fields on (2,2,2) and (3,4,5) lattices;
chains at T = 8 on the models of tests/test_gpu_restraint.py.  tests/test_field_cpu.py asserts that these inputs keep every node off
the lattice planes and that every mutant of the restatement misses these bars on them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.restraints import Field, Restraints
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import field_reference as fr
from tests import guidance_reference as gr
from tests import restraint_frame_reference as rf
from tests import restraint_reference as rr
from tests import sampling_reference as sref
from tests import steer_reference as st
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_restraint import BOTH, DEV, T, Bare, batch_for, dev, model_for, reference_states, stream
from tests.test_gpu_restraint_frame import chain_case, u8
from tests.test_gpu_steer import fresh, read_state
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]


# ----------------------------------------------------------------------------- the kernels, on a bare handle (any D)

class Bare(Bare):
    """... which also knows its N, as the topologies of the model do: the field weights are materialised per node."""

    def __init__(self, D, nm):
        super().__init__(D, nm)
        self.N = int(nm.shape[1])


def run_eps(bare, c, alias, rs=None):
    rs = c.rs if rs is None else rs
    rs.attach(bare, c.scale, c.nv0, torch.device(DEV), stream())
    zd, ed = dev(c.z).contiguous(), dev(c.eps).contiguous()
    out = ed if alias else torch.full_like(ed, 7.0)
    r4 = (C.c_float * 4)(*c.row)
    if c.fm is None:
        rc = bare.lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream())
    else:
        kd, fd = dev(c.known).contiguous(), u8(c.fm)
        rc = bare.lib.hd_restrain_eps_framed(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, fd.data_ptr(), kd.data_ptr(),
                                             out.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    return out.cpu()


def check_eps(bare, c, what):
    ref, mag = fr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known)
    got = run_eps(bare, c, alias=False)
    assert torch.equal(got, run_eps(bare, c, alias=True))     # out aliased to eps
    bound = sref.BOUND * sref.U * mag
    err = np.abs(got.double().numpy() - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what} {c.name}: worst err / bound {ratio:.3f}")
    assert (err <= bound).all(), (what, c.name, ratio)
    e, g_, valid = c.eps.numpy(), got.numpy(), c.nm.numpy()
    assert (g_[:, :, 3:] == e[:, :, 3:]).all() and (g_[~valid] == e[~valid]).all()
    return ratio, got


@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_restrain_eps_with_fields_against_float64(N, D, framed):
    what = "hd_restrain_eps_framed" if framed else "hd_restrain_eps"
    bare, worst, moved, cases = None, 0.0, 0, 0
    try:
        for c in fr.kernel_cases(N, D, framed):
            bare = Bare(D, c.nm) if bare is None else bare
            ratio, got = check_eps(bare, c, f"{what} N={N} D={D}")
            worst = max(worst, ratio)
            cases += 1
            # the field term itself moved eps: the same call on the tables alone differs
            moved += int(not torch.equal(got, run_eps(bare, c, False, rs=fr.with_fields(c.rs, []))))
            if framed:
                e, g_ = c.eps.numpy(), got.numpy()
                assert (g_[2] == e[2]).all()                  # every valid node fixed: eps^ unchanged, bit for bit
                assert (g_[4] == e[4]).all()                  # one valid node: the projection removes its whole step
        print(f"{what} N={N} D={D}: worst err / bound over {cases} cases {worst:.3f}; the fields moved eps in {moved}")
        assert moved == cases
    finally:
        if bare is not None:
            bare.close()


def test_restrain_eps_on_the_exact_points():
    """Nodes exactly on a lattice point, on the upper boundary, outside each face, a NaN coordinate (alpha = 1, sigma = 0, nv0 = 1:
    x^0 = z bit for bit, u exact)."""
    c = fr.exact_case()
    bare = Bare(c.D, c.nm)
    try:
        check_eps(bare, c, "hd_restrain_eps")
        got = run_eps(bare, c, False)
        assert torch.isfinite(got).all()
        # the energy of the same points, NaN node included
        x = c.z[:, :, :3].contiguous()
        c.rs.attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        out = torch.full((1,), -1.0, device=DEV, dtype=torch.float64)
        assert bare.lib.hd_restraint_field_energy(bare.h, bare.topo, dev(x).data_ptr(), out.data_ptr(), stream()) == 0, bare.lib.hd_last_error()
        U, Um, _, _ = fr.field_energy_grad(c.rs, x.numpy(), c.nm)
        assert math.isfinite(float(out[0])) and abs(float(out[0]) - U[0]) <= 1e-12 * Um[0]
    finally:
        bare.close()


def field_energy(bare, c, x, framed):
    out = torch.full((c.B,), -1.0, device=DEV, dtype=torch.float64)
    xd = dev(x).contiguous()
    if not framed:
        rc = bare.lib.hd_restraint_field_energy(bare.h, bare.topo, xd.data_ptr(), out.data_ptr(), stream())
        assert rc == 0, bare.lib.hd_last_error()
        return out.cpu().numpy(), None
    sh = torch.full((c.B, 3), -1.0, device=DEV, dtype=torch.float64)
    kd, fd = dev(c.x_known).contiguous(), u8(c.fm)
    rc = bare.lib.hd_restraint_field_energy_framed(bare.h, bare.topo, xd.data_ptr(), fd.data_ptr(), kd.data_ptr(), out.data_ptr(),
                                                   sh.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    out2 = torch.full_like(out, -1.0)                         # shift3 may be NULL
    assert bare.lib.hd_restraint_field_energy_framed(bare.h, bare.topo, xd.data_ptr(), fd.data_ptr(), kd.data_ptr(), out2.data_ptr(),
                                                     None, stream()) == 0
    assert torch.equal(out, out2)
    return out.cpu().numpy(), sh.cpu().numpy()


@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
@pytest.mark.parametrize("N", [5, 33])
def test_restraint_field_energy_against_float64(N, framed):
    """On the data predictions of the kernel cases (fp32 positions, so the restatement sees the same numbers)."""
    bare, worst, worst_t = None, 0.0, 0.0
    try:
        for c in fr.kernel_cases(N, 11, framed):
            if not math.isinf(c.row[3]):
                continue                                      # (the clip does not enter the energy)
            bare = Bare(11, c.nm) if bare is None else bare
            x = rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).contiguous()
            c.rs.attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
            got, sh = field_energy(bare, c, x, framed)
            if framed:
                U, Um, tau = fr.field_energy_framed(c.rs, x.numpy(), c.x_known.numpy(), c.nm, c.fm)
                _, tmag = rf.frame_shift_ref(x.numpy(), c.x_known.numpy(), c.nm, c.fm)
                terr = np.abs(sh - tau)
                worst_t = max(worst_t, float((terr / np.maximum(1e-12 * tmag, 1e-300)).max()))
                assert (terr <= 1e-12 * tmag).all() and (sh[[1, 4]] == 0).all()
            else:
                U, Um, _, _ = fr.field_energy_grad(c.rs, x.numpy(), c.nm)
            err = np.abs(got - U)
            ratio = float((err / np.maximum(1e-12 * Um, 1e-300)).max())
            worst = max(worst, ratio)
            print(f"hd_restraint_field_energy{'_framed' if framed else ''} N={N} {c.name}: worst err / (1e-12 sum|terms|) {ratio:.3g}")
            assert (err <= 1e-12 * Um).all(), (c.name, ratio)
            # the three-component energy does not see the fields
            e3 = torch.full((c.B, 3), -1.0, device=DEV, dtype=torch.float64)
            assert bare.lib.hd_restraint_energy(bare.h, bare.topo, dev(x).data_ptr(), e3.data_ptr(), stream()) == 0
            fr.with_fields(c.rs, []).attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
            e3b = torch.full((c.B, 3), -1.0, device=DEV, dtype=torch.float64)
            assert bare.lib.hd_restraint_energy(bare.h, bare.topo, dev(x).data_ptr(), e3b.data_ptr(), stream()) == 0
            assert torch.equal(e3, e3b)
            # ... and without fields the field energy is 0
            z0, _ = field_energy(bare, c, x, framed)
            assert (z0 == 0).all()
        print(f"hd_restraint_field_energy{'_framed' if framed else ''} N={N}: worst err / (1e-12 sum|terms|) {worst:.3g}, tau {worst_t:.3g}")
    finally:
        if bare is not None:
            bare.close()


def fields_call(bare, NF=1, values=True, off=(0, 8), dims=(2, 2, 2), geom=(0, 0, 0, 1, 1, 1, 1, 0), weights=True, w_rows=1):
    lib, N = bare.lib, bare.N
    v = torch.zeros(max(1, off[-1]), device=DEV)
    w = torch.ones(max(1, abs(w_rows)) * max(1, NF) * N, device=DEV)
    o = (C.c_longlong * len(off))(*off)
    d = (C.c_int * len(dims))(*dims)
    g = (C.c_float * len(geom))(*geom)
    return lib.hd_restraint_fields(bare.topo, NF, v.data_ptr() if values else None, o, d, g, w.data_ptr() if weights else None, w_rows,
                                   stream())


def test_bits_without_an_active_field_and_abi_refusals():
    N, D = 33, 4
    nm = fr.masks_for(N)
    bare = Bare(D, nm)
    lib = bare.lib
    try:
        c = next(iter(fr.kernel_cases(N, D, False)))
        for pqa in (False, True):
            tabs = rr.random_tables(3, N, 7, 3, 2, 5, True)[0] if pqa else None
            base = fr.with_fields(tabs, [])
            want = run_eps(bare, c, False, rs=base)           # a topology that never had fields
            assert pqa == (not torch.equal(want, c.eps))
            live = fr.make_fields(3, 3, N, 4, True)
            assert not torch.equal(run_eps(bare, c, False, rs=fr.with_fields(tabs, live)), want)
            # after hd_restraint_attach alone the fields of the previous call are gone
            assert torch.equal(run_eps(bare, c, False, rs=base), want)
            # k = 0; all weights 0: eps bit for bit
            k0 = fr.make_fields(3, 3, N, 4, True, k=0.0)
            assert torch.equal(run_eps(bare, c, False, rs=fr.with_fields(tabs, k0)), want)
            w0 = [Field(f.values, f.origin, f.spacing, f.k, f.wall, weights=torch.zeros(3, N)) for f in live]
            assert torch.equal(run_eps(bare, c, False, rs=fr.with_fields(tabs, w0)), want)
            # hd_restraint_fields(NF = 0) clears them
            fr.with_fields(tabs, live).attach(bare, c.scale, c.nv0, torch.device(DEV), stream())
            assert lib.hd_restraint_fields(bare.topo, 0, None, None, None, None, None, 1, stream()) == 0, lib.hd_last_error()
            zd, ed = dev(c.z).contiguous(), dev(c.eps).contiguous()
            out = torch.full_like(ed, 7.0)
            assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(*c.row), out.data_ptr(), stream()) == 0
            assert torch.equal(out.cpu(), want)
        # refusals: HD_E_INVALID for every bad argument, with restraints attached
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert fields_call(bare) == 0, lib.hd_last_error()
        assert fields_call(bare, w_rows=3) == 0, lib.hd_last_error()
        bad = [dict(NF=-1), dict(NF=9), dict(dims=(1, 2, 2), off=(0, 4)), dict(dims=(2, 2, 0), off=(0, 0)),
               dict(geom=(0, 0, 0, 0, 1, 1, 1, 0)), dict(geom=(0, 0, 0, 1, -1, 1, 1, 0)), dict(geom=(0, 0, 0, 1, 1, math.inf, 1, 0)),
               dict(geom=(0, 0, 0, 1, 1, math.nan, 1, 0)), dict(geom=(0, 0, 0, 1, 1, 1, -1, 0)), dict(geom=(0, 0, 0, 1, 1, 1, math.nan, 0)),
               dict(geom=(0, 0, 0, 1, 1, 1, 1, -0.5)), dict(geom=(0, 0, 0, 1, 1, 1, 1, math.inf)), dict(off=(0, 7)), dict(off=(1, 9)),
               dict(w_rows=2), dict(w_rows=0), dict(values=False), dict(weights=False)]
        for kw in bad:
            assert fields_call(bare, **kw) == -1, kw
            assert b"hd_restraint_fields" in lib.hd_last_error()
        assert lib.hd_restraint_fields(bare.topo, 1, torch.zeros(8, device=DEV).data_ptr(), None, None, None, None, 1, stream()) == -1
        two = dict(NF=2, off=(0, 8, 68), dims=(2, 2, 2, 3, 4, 5), geom=(0, 0, 0, 1, 1, 1, 1, 0) * 2)
        assert fields_call(bare, **two) == 0, lib.hd_last_error()
        assert fields_call(bare, **dict(two, off=(0, 8, 67))) == -1
        # HD_E_STATE without attached restraints
        assert lib.hd_restraint_detach(bare.topo) == 0
        assert fields_call(bare) == -4 and b"hd_restraint_attach" in lib.hd_last_error()
        x, out = torch.zeros(3, N, 3, device=DEV), torch.zeros(3, device=DEV, dtype=torch.float64)
        fm = torch.zeros(3 * N, dtype=torch.uint8, device=DEV)
        assert lib.hd_restraint_field_energy(bare.h, bare.topo, x.data_ptr(), out.data_ptr(), stream()) == -4
        assert lib.hd_restraint_field_energy_framed(bare.h, bare.topo, x.data_ptr(), fm.data_ptr(), x.data_ptr(), out.data_ptr(), None,
                                                    stream()) == -4
        Restraints().attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
        assert lib.hd_restraint_field_energy(bare.h, bare.topo, None, out.data_ptr(), stream()) == -1
        assert lib.hd_restraint_field_energy_framed(bare.h, bare.topo, x.data_ptr(), None, x.data_ptr(), out.data_ptr(), None, stream()) == -1
    finally:
        bare.close()


# ----------------------------------------------------------------------------- chains against the restatement over the oracle

K = 4
SCALE = torch.tensor([0.05, 0.02, 0.05])
RKW = dict(restraint_scale=SCALE, restraint_clip=0.3)


def chain_fields(centre=(0.0, 0.0, 0.0), shift=0.0, shape=(4, 5, 3), weights=(1.0, 0.0, 2.0, 1.0), wall2=0.0):
    """A non-cubic lattice with a wall over the region the molecules live in and a (2,2,2) one around it with per-node weights (and
    no wall unless `wall2`: with synthetic weights the data predictions of the noisy levels lie outside it)."""
    g = np.random.Generator(np.random.PCG64(5))
    o = np.array([-3.0 + shift, -2.5, -3.5]) + np.asarray(centre)
    h = (6.0 / (shape[0] - 1), 5.0 / (shape[1] - 1), 7.0 / (shape[2] - 1))
    return [Field(g.normal(0.0, 2.0, shape), o.tolist(), h, k=1.5, wall=0.5),
            Field(g.normal(0.0, 2.0, (2, 2, 2)), (o - 1.0).tolist(), 8.0, k=1.0, wall=wall2, weights=torch.as_tensor(weights))]


def obstacles():
    return [[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]]


def check_states(what, got, ref):
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        e = rel_l2(g.cpu().numpy(), r.numpy())
        worst = max(worst, e)
        print(f"fielded chain {what} state {k + 1}/{len(ref)}: rel_l2 {e:.2e} (bar {REL_L2_TOL:.0e})")
        assert torch.isfinite(g).all()
        assert e < REL_L2_TOL, (what, k, e)
    return worst


def run_states(model, z, nm, em, ctx, raws, **kw):
    zz, out = dev(z), []
    for k in range(len(raws)):
        zz = model.latent_steps(zz, dev(nm), dev(em), dev(ctx), k_lo=k, k_hi=k + 1, raw_noises=None if raws[k] is None else [raws[k]], **kw)
        out.append(zz)
    return out


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("kind", ["field", "field+obstacles guided", "sde2m"])
def test_fielded_chain_against_the_restatement(kind, precision):
    """T = 8, K = 4 with injected normals: a field only (eta = 1); field + obstacles under guidance; the sde2m solver."""
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
    rs = Restraints(obstacles=obstacles() if guided else None, fields=chain_fields())
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
    fnet = fr.FieldNet(inner, rs, SCALE, rr.rows_from_grid(gg, path, "score", 0.3), nm=nm)
    off = fr.FieldNet(inner, Restraints(), torch.zeros(B), {}, nm=nm)
    kw = dict(steps=K, restraints=rs, **RKW)
    if kind == "sde2m":
        from tests import sde_solver_reference as sd
        ref = [r[0] for r in sd.chain_ref(fnet.net, gg, path, z, nm.float(), raws[1:])]
        plain = [r[0] for r in sd.chain_ref(off.net, gg, path, z, nm.float(), raws[1:])]
        kw.update(solver="sde2m")
    else:
        ref = reference_states(fnet, gg, path, 1.0, z, nm, raws[1:], None)
        plain = reference_states(off, gg, path, 1.0, z, nm, raws[1:], None)
        kw.update(eta=1.0)
    if guided:
        kw.update(guidance_scale=2.0)
    got = run_states(model, z, nm, em, ctx, raws[1:], **kw)
    worst = check_states(f"{kind} [{precision}]", got, ref)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"fielded chain {kind} [{precision}]: worst state {worst:.2e}; the field moved eps^ in {fnet.active} of {fnet.calls} network "
          f"calls; distance of the fielded z_0 from the unrestrained one {d:.2e}")
    assert fnet.active == fnet.calls == K
    assert d > 10 * REL_L2_TOL
    if guided:                                                # recorded: record = "x0" shows the fielded data prediction, changes no sample
        call = lambda **k: model.sample_from_masks(dev(nm), None, dev(ctx), sample_id_base=6, steps=K, eta=0.0, guidance_scale=2.0, **k)
        xg, hg, chain = call(keep_frames=K, record="x0", restraints=rs, **RKW)
        assert chain.shape[0] == K and torch.isfinite(chain).all() and torch.equal(chain[0], torch.cat([xg, hg], dim=2))
        x2, h2 = call(restraints=rs, **RKW)
        assert torch.equal(x2, xg) and torch.equal(h2, hg)
        _, _, other = call(keep_frames=K, record="x0", restraints=Restraints(obstacles=obstacles()), **RKW)
        assert not torch.equal(other[K - 1], chain[K - 1])


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("R", [1, 2])
def test_fielded_framed_inpainting_chain_against_the_restatement(R, precision):
    """sample_inpaint(restraint_frame="known") with a field in the coordinates of the known fragments: per state rel-L2 < 1e-4
    against the inpainting chain (host twin of the generator) with the framed update on eps^."""
    lib = _lib.load()
    model, sd_np, cfg = model_for(precision)
    fresh(model)
    nm, em, ctx, fm, xk, hk = chain_case()
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    ids = [9 + b for b in range(B)]
    c0 = ((xk[0] * fm[0]).sum(0) / fm[0].sum()).tolist()
    rs = Restraints(fields=chain_fields(centre=c0))
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    xh_known = torch.cat([xk, hk], dim=2) * fm.float()
    rows = rr.rows_from_grid(gg, path, "score", 0.3)
    fnet = fr.FieldNet(net, rs, SCALE, rows, nm=nm, fm=fm, known=xh_known)
    off = fr.FieldNet(net, Restraints(), torch.zeros(B), {}, nm=nm, fm=fm, known=xh_known)
    z = orc.combined_noise(*rf.philox_raw(lib, SEED, ids, 0, N), nm.float())
    ref = rf.inpaint_path_ref(lib, fnet, gg, path, T, z, nm, fm, xh_known, R, SEED, ids)
    plain = rf.inpaint_path_ref(lib, off, gg, path, T, z, nm, fm, xh_known, R, SEED, ids)
    x, h, chain, info = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), sample_id_base=9, keep_frames=K, record="z", steps=K,
                                             resamplings=R, restraints=rs, restraint_frame="known", **RKW)
    assert torch.isfinite(chain).all()
    worst = 0.0
    for k in range(K - 1):                                    # transition k arrives at position K - 1 - k
        r = rel_l2(chain[K - 1 - k].cpu().numpy(), ref[k].numpy())
        worst = max(worst, r)
        print(f"fielded framed inpainting R={R} [{precision}] state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
        assert r < REL_L2_TOL, (R, precision, k, r)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"fielded framed inpainting R={R} [{precision}]: worst state {worst:.2e}; the field moved eps^ in {fnet.active} of {fnet.calls} "
          f"network calls; distance of the fielded z_0 from the unrestrained one {d:.2e}")
    assert fnet.calls == K * R and 2 * fnet.active >= fnet.calls
    assert d > 10 * REL_L2_TOL
    # the info dict: the field energy of the returned x in the known frame, next to the unchanged [B, 3]
    fe = info["restraint_field_energy"].cpu()
    assert fe.shape == (B,) and fe.dtype == torch.float64 and info["restraint_energy"].shape == (B, 3)
    want = rs.field_energy(x.cpu(), nm, fixed_mask=fm, x_known=xk)
    assert torch.allclose(fe, want, rtol=1e-9, atol=1e-9)
    U, Um, _ = fr.field_energy_framed(rs, x.cpu().numpy(), xk.numpy(), nm, fm)
    assert (np.abs(fe.numpy() - U) <= 1e-12 * Um).all()


def test_fielded_steered_chain_against_the_reference():
    """P = 4, a field only: per state rel-L2 < 1e-4 against `SteeredNet` weighing on the total with U_fld; ancestors and roots of every
    transition exactly (tests/test_field_cpu.py asserts the reference's margins)."""
    lib = _lib.load()
    for precision in BOTH:
        model, _, _ = model_for(precision)
        fresh(model)
        states, infos, state, zT, (nm, em) = fr.steered_reference(precision)
        B, N = nm.shape[:2]
        G = B // st.CHAIN_P
        kw = dict(eta=1.0, restraints=Restraints(fields=fr.steer_fields()), particles=st.CHAIN_P, steer_scale=fr.STEER_BETA,
                  steer_ess=st.CHAIN_RHO, sample_id_base=fr.STEER_BASE, restraint_scale=fr.STEER_SCALE, restraint_clip=0.3)
        nmd, emd = dev(nm), dev(em)
        topo = model.dynamics.topology(nmd, emd, B, N)
        zz, worst = dev(zT), 0.0
        roots = np.arange(B) % st.CHAIN_P
        assert any(i["resampled"].any() for i in infos) and not all(i["resampled"].all() for i in infos)
        for k in range(T):
            zz = model.path_steps(zz, nmd, emd, k_lo=k, k_hi=k + 1, **kw)
            logw, uprev, root, anc, stats = read_state(lib, topo.ptr, B, G)
            r = rel_l2(zz.cpu().numpy(), states[k].numpy())
            worst = max(worst, r)
            print(f"fielded steered chain [{precision}] state {k + 1}/{T}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e}), resampled "
                  f"{infos[k]['resampled'].tolist()}")
            assert (anc == infos[k]["anc"]).all(), (k, anc, infos[k]["anc"])
            roots = roots[infos[k]["anc"]]
            assert (root == roots).all(), k
            assert r < REL_L2_TOL, (k, r)
        assert (root == state.root).all() and (stats[:, 0] == state.stats[:, 0]).all()
        print(f"fielded steered chain [{precision}]: worst state {worst:.2e}; events {state.stats[:, 0].tolist()}")


# ----------------------------------------------------------------------------- graph behaviour

def test_graph_replay_reattaching_and_the_unfielded_call():
    """On a topology of its own (masks no other test of this module uses: the buffers start empty).  The graph pass comes first - a
    buffer that the launches had already grown would hide the rebuild - and plain launches then reproduce every result bit for bit."""
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    _, _, nm, em, _ = batch_for((6, 5, 2))
    nmd, N = dev(nm), nm.shape[1]
    kw = dict(sample_id_base=3, steps=4, eta=0.5, restraint_scale=0.05, restraint_clip=0.3)
    obs = obstacles()
    cf = lambda **k: chain_fields(wall2=0.25, **k)             # (both fields act on the far-out data predictions)
    sets = dict(a=Restraints(obs, fields=cf()), b=Restraints(obs, fields=cf(shift=0.25)),
                big=Restraints(obs, fields=cf(shape=(9, 8, 7))), one=Restraints(obs, fields=cf()[:1]),
                rows=Restraints(obs, fields=cf(weights=torch.tensor([[1.0, 0.0, 2.0, 1.0]] * 3))), never=Restraints(obs))
    call = lambda k: model.sample_from_masks(nmd, None, None, restraints=sets[k], **kw)
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 3, N)
    builds = lambda: lib.hd_path_graph_builds(topo.ptr)
    got, n0 = {}, builds()
    same = lambda out, k: torch.equal(out[0], got[k][0]) and torch.equal(out[1], got[k][1])
    got["a"] = call("a")
    assert builds() == n0 + 1
    got["b"] = call("b")                                      # same-size fields: a copy, no rebuild
    assert same(call("a"), "a") and builds() == n0 + 1
    got["big"] = call("big")                                  # a larger lattice outgrows the pool: one rebuild
    assert builds() == n0 + 2
    assert same(call("big"), "big") and same(call("a"), "a") and builds() == n0 + 2
    got["one"] = call("one")                                  # another NF: one rebuild
    assert builds() == n0 + 3
    got["rows"] = call("rows")                                # NF and the weights' rows change together: one rebuild
    assert builds() == n0 + 4
    got["never"] = call("never")                              # an unfielded call afterwards rebuilds ...
    assert builds() == n0 + 5
    assert same(call("never"), "never") and builds() == n0 + 5
    assert same(call("rows"), "rows") and builds() == n0 + 6
    assert not same(got["b"], "a") and not same(got["never"], "a") and not same(got["big"], "a") and not same(got["one"], "a")
    assert same(got["rows"], "a")                             # the same weights, materialised per molecule
    fresh(model, graph=False)                                 # graph replay equals plain launches bit for bit
    for k in sets:
        assert same(call(k), k), k
    # ... and gives the bits of a topology that never had fields
    _, _, nm2, _, _ = batch_for((6, 5, 2, 1))
    fresh2 = model.sample_from_masks(dev(nm2), None, None, restraints=sets["never"], **kw)
    assert torch.equal(fresh2[0][:3, :N], got["never"][0]) and torch.equal(fresh2[1][:3, :N], got["never"][1])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_molecule_depends_on_its_id_its_own_rows_and_its_own_weights_only(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    _, _, nm, em, _ = batch_for((7, 4, 1, 6))
    B, N = nm.shape[:2]
    g = torch.Generator().manual_seed(1)
    obs = torch.cat([torch.randn(B, 3, 3, generator=g), torch.full((B, 3, 1), 1.5), torch.full((B, 3, 1), 2.0)], dim=2)
    w = torch.rand(B, N, generator=g) + 0.25
    w[:, 2] = 0.0
    fields = chain_fields()
    fields[0] = Field(fields[0].values, fields[0].origin, fields[0].spacing, 1.5, 0.5, weights=w)
    rs = Restraints(obstacles=obs, fields=fields)
    scale = torch.tensor([0.05, 0.03, 0.05, 0.08])
    kw = dict(steps=4, eta=1.0, restraint_clip=0.3)
    whole = model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=rs, restraint_scale=scale, **kw)
    for lo, hi in ((0, 1), (1, 2), (2, 4)):                   # batch cuts of one and of two molecules
        part = model.sample_from_masks(dev(nm[lo:hi]), None, None, sample_id_base=11 + lo, restraints=rs.slice(lo, hi),
                                       restraint_scale=scale[lo:hi], **kw)
        assert torch.equal(part[0], whole[0][lo:hi]) and torch.equal(part[1], whole[1][lo:hi]), (lo, hi)
    other = Restraints(obstacles=obs, fields=[Field(fields[0].values, fields[0].origin, fields[0].spacing, 1.5, 0.5, weights=w * 2.0), fields[1]])
    assert not torch.equal(model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=other, restraint_scale=scale, **kw)[0],
                           whole[0])


# ----------------------------------------------------------------------------- results

def test_results_carry_the_field_energy():
    model, _, _ = model_for("fp32")
    fresh(model)
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]], fields=chain_fields())
    torch.manual_seed(3)
    on = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    torch.manual_seed(3)
    bare = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]]),
                        restraint_scale=0.05, restraint_clip=0.3)
    assert all("restraint_field_energy" not in r and r["restraint_energy"].shape == (3,) for r in bare)
    for r in on:
        n = r["x"].shape[0]
        fe = r["restraint_field_energy"]
        assert fe.shape == () and fe.dtype == torch.float64 and r["restraint_energy"].shape == (3,)
        x1, one = r["x"].unsqueeze(0), torch.ones(1, n, 1)
        assert torch.allclose(fe, rs.field_energy(x1, one)[0], rtol=1e-9, atol=1e-9)          # field_energy of the returned x (CPU formulas)
        U, Um, _, _ = fr.field_energy_grad(rs, x1.numpy(), np.ones((1, n)))
        assert abs(float(fe) - U[0]) <= 1e-12 * Um[0]
        assert torch.allclose(r["restraint_energy"], rs.energy(x1.double(), one)[0], rtol=1e-9, atol=1e-12)
    # ... and through the device entry of field_energy itself
    got = rs.field_energy(dev(on[0]["x"].unsqueeze(0)), torch.ones(1, on[0]["x"].shape[0], 1), model=model)
    assert got.device.type == "cuda" and torch.allclose(got[0].cpu(), on[0]["restraint_field_energy"], rtol=1e-12, atol=1e-12)
    var = model.vary(bare[:2], DEV, 4, n_variants=2, steps=2, restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    assert len(var) == 4 and all(r["restraint_field_energy"].shape == () and r["restraint_energy"].shape == (3,) for r in var)
    g = torch.Generator().manual_seed(4)
    known = [{"x": torch.tensor(rf.CENTRE) + torch.randn(k, 3, generator=g), "h": torch.randn(k, 8, generator=g)} for k in (3, 2)]
    grown = model.sample_grow(known, [7, 4], DEV, sample_id_base=2, steps=4, restraints=Restraints(fields=chain_fields(centre=rf.CENTRE)),
                              restraint_scale=0.05, restraint_clip=0.3, restraint_frame="known")
    assert all(r["restraint_field_energy"].shape == () and r["frame_shift"].shape == (3,) for r in grown)
