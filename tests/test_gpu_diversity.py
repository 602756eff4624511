"""GPU tier (-m gpu) of diverse sampling: hd_diverse_eps and hd_diversity_energy against the float64 restatement of
tests/diversity_reference.py (rotation by SVD, not the kernel's Jacobi), diverse chains against that restatement over the oracle, and
the contracts of the device path: exact zeros, graph replay, re-attaching, batch and chain cuts, the keyword switched off, the direction
of the update, refusals.

Bars.  eps: the element-wise bar of the restraint kernels - every element within 8 * 2^-23 of the sum of the absolute values of its
terms.  The energy call: Phi and the RMSD matrix relative 1e-13 on the conditioned cases (conditioning measure >= 0.05, asserted on the
CPU by tests/test_diversity_cpu.py); the two degenerate cases in d2 (relative 1e-13) and finiteness only.  The RMSD of two identical
rows is a rounding residue in the restatement and exactly 0 in the kernel: asserted as such.  Chains: rel-L2 < 1e-4 per state
(tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: G = 3 groups of P in {2, 4, 8} rows (one case of P = 32) of N in {5, 33} nodes at D in {4, 11}; chains at T = 8, K = 4, B = 8 as
2 groups of 4 on the models of tests/test_gpu_restraint.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.diversity import Diversity
from hierdiff_amd.restraints import Field, Restraints, Template
from oracle import egnn_oracle as orc
from tests import diversity_reference as dr
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import restraint_reference as rr
from tests import template_reference as tr
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_restraint import BOTH, DEV, T, Bare, dev, fresh as fresh_restraints, model_for, reference_states, stream
from tests.test_inpaint_cpu import gamma_grid_fp64

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]


def fresh(model, graph=True):
    fresh_restraints(model, graph)
    model.particles = model.steer_scale = model.diversity = None
    return model


# ----------------------------------------------------------------------------- the kernels, on a bare handle (any D)

def attach(bare, c, scale=None, P=None, kappa=None, length=None):
    s = np.ascontiguousarray((c.scale if scale is None else torch.as_tensor(scale, dtype=torch.float32)).reshape(-1).numpy())
    return bare.lib.hd_diversity_attach(bare.topo, c.P if P is None else P, c.kappa if kappa is None else kappa,
                                        c.length if length is None else length, s.ctypes.data_as(C.POINTER(C.c_float)), int(s.shape[0]),
                                        c.nv0, stream())


def run_eps(bare, c, alias, eps=None, row=None):
    assert attach(bare, c) == 0, bare.lib.hd_last_error()
    zd, ed = dev(c.z).contiguous(), dev(c.eps if eps is None else eps).contiguous()
    out = ed if alias else torch.full_like(ed, 7.0)
    r4 = (C.c_float * 4)(*(c.row if row is None else row))
    rc = bare.lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    return out.cpu()


def energy(bare, c, x, want_rmsd=True):
    assert attach(bare, c) == 0, bare.lib.hd_last_error()
    phi = torch.full((c.G,), -1.0, device=DEV, dtype=torch.float64)
    rm = torch.full((c.G, c.P, c.P), -1.0, device=DEV, dtype=torch.float64)
    xd = dev(x).contiguous()
    rc = bare.lib.hd_diversity_energy(bare.h, bare.topo, xd.data_ptr(), phi.data_ptr(), rm.data_ptr() if want_rmsd else None, stream())
    assert rc == 0, bare.lib.hd_last_error()
    return phi.cpu().numpy(), rm.cpu().numpy()


def check_eps(bare, c, what, eps=None):
    e_in = c.eps if eps is None else eps
    ref, mag = dr.diverse_ref(c.z, e_in, c.nm, c.P, c.kappa, c.length, c.scale, c.row, c.nv0)
    got = run_eps(bare, c, alias=False, eps=eps)
    assert torch.equal(got, run_eps(bare, c, alias=True, eps=eps))              # in place
    e, g_, valid = e_in.numpy(), got.numpy(), c.nm.numpy()
    # exact zeros: feature columns, masked rows, groups with scale 0
    assert (g_[:, :, 3:].view(np.int32) == e[:, :, 3:].view(np.int32)).all() and (g_[~valid].view(np.int32) == e[~valid].view(np.int32)).all()
    s = np.broadcast_to(c.scale.numpy(), (c.G,))
    for g in range(c.G):
        if s[g] == 0:
            assert (g_[g * c.P:(g + 1) * c.P].view(np.int32) == e[g * c.P:(g + 1) * c.P].view(np.int32)).all(), c.name
    assert np.isfinite(g_[np.isfinite(e)]).all(), c.name
    if c.degenerate:                                          # R is not unique: the gradient may be any maximiser's
        return None, got
    bound = dr.BOUND * dr.U * mag
    ok = np.isfinite(bound)                                   # (the NaN coordinate itself has no magnitude; its eps is not touched)
    err = np.abs(got.double().numpy() - ref)
    ratio = float((err[ok] / np.maximum(bound[ok], 1e-300)).max())
    print(f"{what} {c.name}: worst err / bound {ratio:.3f}")
    assert (err[ok] <= bound[ok]).all(), (what, c.name, ratio)
    return ratio, got


@pytest.mark.parametrize("N,D", SHAPES)
def test_diverse_eps_against_float64(N, D):
    what = f"hd_diverse_eps N={N} D={D}"
    worst, moved, cases = 0.0, 0, 0
    bares = {}
    try:
        for c in dr.kernel_cases(N, D):
            key = (c.P, c.nm.numpy().tobytes())
            bare = bares.get(key) or bares.setdefault(key, Bare(D, c.nm))
            ratio, got = check_eps(bare, c, what)
            e, g_ = c.eps.numpy(), got.numpy()
            P = c.P
            if c.kind == "identical rows" and P == 2:         # r = 0 exactly: the group keeps its bits
                assert (g_[:2].view(np.int32) == e[:2].view(np.int32)).all()
            if c.kind == "one common node, none":
                assert (g_[P + 1].view(np.int32) == e[P + 1].view(np.int32)).all()     # a row that shares no node with any other
                if P == 2:                                    # n = 1, n = 0: neither group moves
                    assert (g_[:4].view(np.int32) == e[:4].view(np.int32)).all()
            if c.kind == "unequal masks":
                assert (g_[2 * P - 1].view(np.int32) == e[2 * P - 1].view(np.int32)).all()      # the masked row
            if c.kind == "nan coordinate":                    # every pair with row 1 contributes to neither side
                assert (g_[1].view(np.int32) == e[1].view(np.int32)).all()
                if P == 2:
                    assert (g_[0].view(np.int32) == e[0].view(np.int32)).all()
            if ratio is None:
                continue
            worst = max(worst, ratio)
            cases += 1
            moved += int(not torch.equal(got, c.eps))
        print(f"{what}: worst err / bound over {cases} cases {worst:.3f}; the term moved eps in {moved}")
        assert moved == cases
    finally:
        for b in bares.values():
            b.close()


def test_diverse_eps_with_32_rows_per_group():
    c = dr.big_case()
    bare = Bare(c.D, c.nm)
    try:
        ratio, got = check_eps(bare, c, "hd_diverse_eps")
        assert not torch.equal(got, c.eps)
        x = torch.from_numpy(dr.data_prediction(c)).float()
        phi, rm = energy(bare, c, x)
        rphi, rrm, _, _, _ = dr.phi_grad(x.numpy(), c.nm.numpy(), c.P, c.kappa, c.length)
        assert (np.abs(phi - rphi) <= 1e-13 * rphi).all() and (np.abs(rm - rrm) <= 1e-13 * rrm).all()
        print(f"P = 32: eps worst err / bound {ratio:.3f}; Phi rel {float((np.abs(phi - rphi) / rphi).max()):.2e}")
    finally:
        bare.close()


@pytest.mark.parametrize("N,D", [(5, 4), (33, 11)])
def test_diverse_eps_behind_the_restraint_update(N, D):
    """hd_restrain_eps with obstacles, a field and a template, then hd_diverse_eps on its output: the restatement on the same fp32
    input."""
    g = np.random.Generator(np.random.PCG64(5))
    rs = Restraints(obstacles=[[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]],
                    fields=[Field(g.normal(0.0, 2.0, (4, 5, 3)), [-3.0, -2.5, -3.5], (2.0, 1.25, 3.5), k=1.5, wall=0.5)],
                    templates=[Template([0, 1, 2], g.normal(0.0, 1.5, (3, 3)), k=1.5)])
    for P, clip in ((4, math.inf), (8, 0.05)):
        c = dr.conditioned_case(3, P, N, D, kind="partly masked", clip=clip, scale=[1.0, 0.6, 0.8], seed=11)
        bare = Bare(D, c.nm)
        bare.N = N
        try:
            rs.attach(bare, torch.full((1,), 0.1), c.nv0, torch.device(DEV), stream())
            zd, ed = dev(c.z).contiguous(), dev(c.eps).contiguous()
            mid = torch.full_like(ed, 7.0)
            r4 = (C.c_float * 4)(*c.row[:3], math.inf)
            assert bare.lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, mid.data_ptr(), stream()) == 0
            mid = mid.cpu()
            assert not torch.equal(mid, c.eps)
            # the restrained data prediction is another arrangement: its pairs must be conditioned too
            c2 = dr.Case()
            c2.__dict__.update(c.__dict__)
            c2.eps = mid
            assert dr.worst_cond(c2) >= dr.COND_MIN
            ratio, got = check_eps(bare, c, f"behind hd_restrain_eps N={N} D={D}", eps=mid)
            assert not torch.equal(got, mid)
        finally:
            bare.close()


@pytest.mark.parametrize("N", [5, 33])
def test_diversity_energy_against_float64(N):
    """On the data predictions of the kernel cases (fp32 positions, so the restatement sees the same numbers)."""
    wp, wr = 0.0, 0.0
    bares = {}
    try:
        for c in dr.kernel_cases(N, 4):
            key = (c.P, c.nm.numpy().tobytes())
            bare = bares.get(key) or bares.setdefault(key, Bare(4, c.nm))
            x = torch.from_numpy(dr.data_prediction(c)).float().contiguous()
            phi, rm = energy(bare, c, x)
            phi2, _ = energy(bare, c, x, want_rmsd=False)     # rmsd may be NULL
            assert (phi == phi2).all()
            rphi, rrm, _, _, _ = dr.phi_grad(x.double().numpy(), c.nm.numpy(), c.P, c.kappa, c.length)
            # symmetric bit for bit, zero diagonal, NaN exactly where the restatement has none
            assert (rm.view(np.int64) == rm.transpose(0, 2, 1).view(np.int64)).all(), c.name
            assert (rm[:, np.arange(c.P), np.arange(c.P)] == 0).all() and (np.isnan(rm) == np.isnan(rrm)).all(), c.name
            assert np.isfinite(phi).all()
            live = ~np.isnan(rrm) & (rrm > 1e-9)
            if c.kind == "identical rows":
                assert rm[0, 0, 1] == 0.0 and rrm[0, 0, 1] < 1e-12
            if c.degenerate:                                  # d2 is unique although R is not
                d2, rd2 = rm[live] ** 2, rrm[live] ** 2
                r = float((np.abs(d2 - rd2) / rd2).max())
                print(f"hd_diversity_energy N={N} {c.name}: worst d2 rel {r:.3g}")
                assert r <= 1e-13, (c.name, r)
                continue
            r_rm = float((np.abs(rm[live] - rrm[live]) / rrm[live]).max()) if live.any() else 0.0
            ok = rphi > 0
            assert (phi[~ok] == 0).all(), c.name
            r_phi = float((np.abs(phi[ok] - rphi[ok]) / rphi[ok]).max()) if ok.any() else 0.0
            wp, wr = max(wp, r_phi), max(wr, r_rm)
            print(f"hd_diversity_energy N={N} {c.name}: Phi rel {r_phi:.3g}, rmsd rel {r_rm:.3g}")
            assert r_phi <= 1e-13 and r_rm <= 1e-13, (c.name, r_phi, r_rm)
        print(f"hd_diversity_energy N={N}: worst Phi rel {wp:.3g}, worst rmsd rel {wr:.3g} (bar 1e-13)")
    finally:
        for b in bares.values():
            b.close()


def test_the_update_moves_the_rows_apart():
    """One transition, the clip inactive: the mean pairwise aligned RMSD of x^0 from the updated eps^ exceeds that from the given one."""
    for P in (2, 4):
        c = dr.conditioned_case(3, P, 33, 4, kind="full", clip=math.inf, seed=21, kappa=0.2)
        bare = Bare(4, c.nm)
        try:
            got = run_eps(bare, c, alias=False)
            x_old = rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).contiguous()
            x_new = rr.x0_f32(c.z, got, c.row[0], c.row[1], c.nv0).contiguous()
            iu = np.triu_indices(P, 1)
            old = energy(bare, c, x_old)[1][:, iu[0], iu[1]].mean(1)
            new = energy(bare, c, x_new)[1][:, iu[0], iu[1]].mean(1)
            print(f"direction P={P}: mean pairwise aligned RMSD {old} -> {new}")
            assert (new > old).all()
        finally:
            bare.close()


def test_abi_refusals():
    c = dr.make_case(3, 4, 5, 4)
    bare = Bare(4, c.nm)
    lib = bare.lib
    try:
        zd, ed = dev(c.z).contiguous(), dev(c.eps).contiguous()
        out = torch.full_like(ed, 7.0)
        r4 = (C.c_float * 4)(*c.row)
        phi = torch.full((3,), -1.0, device=DEV, dtype=torch.float64)
        # HD_E_STATE: nothing attached
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream()) == -4
        assert lib.hd_diversity_energy(bare.h, bare.topo, zd.data_ptr(), phi.data_ptr(), None, stream()) == -4
        assert (out.cpu() == 7.0).all() and (phi.cpu() == -1.0).all()
        for kw in (dict(P=1), dict(P=33), dict(P=5), dict(P=0), dict(kappa=-1.0), dict(kappa=math.inf), dict(kappa=math.nan), dict(length=0.0),
                   dict(length=-1.0), dict(length=math.inf), dict(length=math.nan), dict(scale=[1.0, 2.0]), dict(scale=[1.0] * 12),
                   dict(scale=[math.nan]), dict(scale=[1.0, math.inf, 1.0])):
            assert attach(bare, c, **kw) == -1, kw
            assert b"hd_diversity_attach" in lib.hd_last_error()
        one = (C.c_float * 1)(1.0)
        assert lib.hd_diversity_attach(bare.topo, 4, 1.0, 1.0, None, 1, 1.0, stream()) == -1
        for nv0 in (0.0, -1.0, math.inf, math.nan):
            assert lib.hd_diversity_attach(bare.topo, 4, 1.0, 1.0, one, 1, nv0, stream()) == -1
        assert attach(bare, c) == 0 and attach(bare, c, scale=[1.0, 0.0, 2.0]) == 0 and attach(bare, c, P=2, scale=[1.0] * 6) == 0
        assert attach(bare, c) == 0
        # the rows and the aliasing rules of hd_restrain_eps
        for bad in ((0.0, 0.5, 1.0, 1.0), (0.8, -0.5, 1.0, 1.0), (0.8, 0.5, math.nan, 1.0), (0.8, 0.5, 1.0, 0.0), (0.8, 0.5, 1.0, math.nan)):
            assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(*bad), out.data_ptr(), stream()) == -1
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, zd.data_ptr(), stream()) == -1
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, ed.data_ptr() + 4, stream()) == -1
        assert lib.hd_diverse_eps(bare.h, bare.topo, None, ed.data_ptr(), r4, out.data_ptr(), stream()) == -1
        assert lib.hd_diversity_energy(bare.h, bare.topo, None, phi.data_ptr(), None, stream()) == -1
        assert (out.cpu() == 7.0).all()
        # lambda = 0 and kappa = 0: nothing is written / eps bit for bit
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(0.8, 0.5, 0.0, 1.0), out.data_ptr(), stream()) == 0
        assert torch.equal(out.cpu(), c.eps)
        assert attach(bare, c, kappa=0.0) == 0
        out.fill_(7.0)
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream()) == 0
        assert torch.equal(out.cpu(), c.eps)
        assert lib.hd_diversity_detach(bare.topo) == 0
        assert lib.hd_diverse_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream()) == -4
    finally:
        bare.close()
    # one workgroup's LDS: 32 rows of 50 nodes and 496 pair records do not fit, 2 rows do
    wide = Bare(4, torch.ones(32, 50, dtype=torch.bool))
    try:
        assert attach(wide, c, P=32) == -1 and b"LDS" in wide.lib.hd_last_error()
        assert attach(wide, c, P=2) == 0
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
        one = (C.c_float * 1)(1.0)
        r4 = np.tile(np.array([0.9, 0.3, 0.5, 0.2], dtype=np.float32), (K, 1))
        r4p = r4.ctypes.data_as(C.POINTER(C.c_float))
        run = lambda mol=-1, rows_=B, graph=1: lib.hd_sample_path(h, topo, z.data_ptr(), None, mol, 0, K, None, None, rows_, 7, 0, graph, None)
        assert run() == 0
        ok(lib.hd_diversity_attach(topo, 2, 1.0, 1.0, one, 1, 1.0, None))
        # rows not set for the current path
        assert run() == -4 and b"hd_set_diversity" in lib.hd_last_error()
        assert lib.hd_set_diversity(h, K + 1, r4p) == -1 and lib.hd_set_diversity(h, K, None) == -1
        ok(lib.hd_set_diversity(h, K, r4p))
        assert run() == 0 and run(graph=0) == 0
        # an inpainting call; mol_shape < N; shared noise on rows that draw; steering at the same time
        rc = lib.hd_sample_path_inpaint(h, topo, z.data_ptr(), None, -1, 0, K, None, None, B, 7, 0, 1, fixed.data_ptr(), known.data_ptr(), 2, None)
        assert rc == -1 and b"diversity" in lib.hd_last_error() and b"inpainting" in lib.hd_last_error()
        assert run(mol=3) == -1 and b"whole molecules" in lib.hd_last_error()
        assert run(rows_=1) == -1 and b"shared row of noise" in lib.hd_last_error()
        ok(lib.hd_steer_attach(topo, 2, 0.5, 1, None))
        assert run() != 0                                     # (steering's own refusals come first: it needs restraints)
        ok(lib.hd_restraint_attach(topo, None, 1, 0, None, None, 1, 0, None, None, 1, 0, one, 1, 1.0, None))
        r3 = np.tile(np.array([0.9, 0.3, 0.5], dtype=np.float32), (K, 1))
        ok(lib.hd_set_restraint(h, K, r4p))
        ok(lib.hd_set_steer(h, K, r3.ctypes.data_as(C.POINTER(C.c_float))))
        assert run() == -1 and b"diversity and steering" in lib.hd_last_error()
        ok(lib.hd_steer_detach(topo))
        ok(lib.hd_restraint_detach(topo))
        assert run() == 0
        # a new path: the rows belong to the old one
        ok(lib.hd_set_path(h, K, t_idx, s_idx, rows_p, 1, None))
        assert run() == -4
        # linear rows with c = 0 draw nothing: shared noise is allowed there
        det = np.tile(np.array([0.9, 0.3, 0.0, 0.0], dtype=np.float32), (K, 1))
        ok(lib.hd_set_path(h, K, t_idx, s_idx, det.ctypes.data_as(C.POINTER(C.c_float)), 1, None))
        ok(lib.hd_set_diversity(h, K, r4p))
        assert run(rows_=1) == 0
        ok(lib.hd_diversity_detach(topo))
        assert run() == 0
        torch.cuda.synchronize()
        assert torch.isfinite(z).all()
    finally:
        torch.cuda.synchronize()
        lib.hd_topology_destroy(topo)
        lib.hd_destroy(h)


# ----------------------------------------------------------------------------- chains against the restatement over the oracle

K = 4
MOLS = (7, 7, 7, 7, 4, 4, 4, 4)
# (with synthetic weights the data predictions of the noisy levels are hundreds of units wide - the aligned RMSD of the first
# transition is about 300 - so a length of 50 keeps the Gaussian alive on the whole path; kappa = length^2 makes the step e r / n)
DV = dict(particles=4, length=50.0, strength=2500.0, scale=[1.0, 0.5], clip=0.3)


def batch(C_=0):
    nm, em = orc.canonical_masks(list(MOLS))
    nm = nm.bool()
    ctx = None
    if C_:                                                    # one context value per group
        ctx = (torch.tensor([0.7, -0.4]).repeat_interleave(4).reshape(8, 1, 1).expand(8, nm.shape[1], 1) * nm.float()).contiguous()
    return nm, em, ctx


def run_states(model, z, nm, em, ctx, raws, **kw):
    zz, out = dev(z), []
    for k in range(len(raws)):
        zz = model.latent_steps(zz, dev(nm), dev(em), dev(ctx), k_lo=k, k_hi=k + 1, raw_noises=None if raws[k] is None else [raws[k]], **kw)
        out.append(zz)
    return out


def check_states(what, got, ref):
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        e = rel_l2(g.cpu().numpy(), r.numpy())
        worst = max(worst, e)
        print(f"diverse chain {what} state {k + 1}/{len(ref)}: rel_l2 {e:.2e} (bar {REL_L2_TOL:.0e})")
        assert torch.isfinite(g).all()
        assert e < REL_L2_TOL, (what, k, e)
    return worst


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("kind", ["eta1", "eta0", "dpm2m", "sde2m", "guided", "obstacles+template"])
def test_diverse_chain_against_the_restatement(kind, precision):
    """T = 8, K = 4, B = 8 as 2 groups of 4, with injected normals where the update draws."""
    guided = kind == "guided"
    C_ = 1 if guided else 0
    model, sd_np, cfg = model_for(precision, C_)
    fresh(model)
    nm, em, ctx = batch(C_)
    B, N = nm.shape[:2]
    nv0 = float(model.norm_values[0])
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 1, B, N, seed=K)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    dv = Diversity(**DV)
    rows = rr.rows_from_grid(gg, path, "score", 0.3, nv0)
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    inner = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0) if guided else net
    kw = dict(steps=K, diversity=dv)
    if kind == "obstacles+template":
        g = np.random.Generator(np.random.PCG64(5))
        rs = Restraints(obstacles=[[0.5, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0, 0.5, 1.0, 1.0]],
                        templates=[Template([0, 1, 2, 3], g.normal(0.0, 1.5, (4, 3)), k=1.5)])
        inner = tr.TemplateNet(inner, rs, torch.tensor([0.05]), rows, nv0, nm=nm)
        kw.update(restraints=rs, restraint_scale=0.05, restraint_clip=0.3)
    dnet = dr.DiverseNet(inner, dv.P, dv.strength, dv.length, dv.scale, rows, nv0)
    off = dr.DiverseNet(inner, dv.P, 0.0, dv.length, dv.scale, {}, nv0)
    noisy = kind in ("eta1", "sde2m", "guided", "obstacles+template")
    if kind == "sde2m":
        from tests import sde_solver_reference as sd
        ref = [r[0] for r in sd.chain_ref(dnet.net, gg, path, z, nm.float(), raws[1:])]
        plain = [r[0] for r in sd.chain_ref(off.net, gg, path, z, nm.float(), raws[1:])]
        kw.update(solver="sde2m")
    elif kind == "dpm2m":
        ref = reference_states(dnet, gg, path, 0.0, z, nm, raws[1:], "dpm2m")
        plain = reference_states(off, gg, path, 0.0, z, nm, raws[1:], "dpm2m")
        kw.update(solver="dpm2m")
    else:
        eta = 0.0 if kind == "eta0" else 1.0
        ref = reference_states(dnet, gg, path, eta, z, nm, raws[1:], None)
        plain = reference_states(off, gg, path, eta, z, nm, raws[1:], None)
        kw.update(eta=eta)
    if guided:
        kw.update(guidance_scale=2.0)
    got = run_states(model, z, nm, em, ctx, raws[1:] if noisy else [None] * K, **kw)
    worst = check_states(f"{kind} [{precision}]", got, ref)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"diverse chain {kind} [{precision}]: worst state {worst:.2e}; the term moved eps^ in {dnet.active} of {dnet.calls} network "
          f"calls; distance of the diverse z_0 from the plain one {d:.2e}")
    assert dnet.active == dnet.calls == K                     # the term is on in every network call
    assert d > 10 * REL_L2_TOL                                # not a no-op: the plain chain lies far outside the bar


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("record", ["x0", "z"])
def test_recorded_diverse_chain_from_a_latent(record, precision):
    """sample_from_latent with keep_frames: the states ("z"), or the data predictions, which show the update ("x0")."""
    model, sd_np, cfg = model_for(precision)
    fresh(model)
    nm, em, _ = batch()
    B, N = nm.shape[:2]
    nv0 = float(model.norm_values[0])
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 2, B, N, seed=K)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    dv = Diversity(**DV)
    rows = rr.rows_from_grid(gg, path, "score", 0.3, nv0)
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    dnet = dr.DiverseNet(net, dv.P, dv.strength, dv.length, dv.scale, rows, nv0)
    ref, want, bare_x0 = [], [], []
    zz = z
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):     # the ancestral chain, keeping every eps^
        eps_plain = net.net(zz, t)
        eps = dnet.net(zz, t)
        al, sg = rows[int(t)][0], rows[int(t)][1]
        want.append(rr.x0_f32(zz, eps, al, sg, nv0))
        bare_x0.append(rr.x0_f32(zz, eps_plain, al, sg, nv0))
        zz = gr.ancestral_on_eps(net, zz, eps, s, t, raws[1 + k], gg).float()
        ref.append(zz)
    x, h, chain = model.sample_from_latent(dev(z), dev(nm), dev(em), None, steps=K, eta=1.0, raw_noises=raws[1:], keep_frames=K,
                                           record=record, diversity=dv)
    chain = chain.cpu()
    assert torch.isfinite(chain).all()
    for k in range(K - 1):                                    # transition k writes frame K - 1 - k; frame 0 is the result itself
        fr_ = chain[K - 1 - k]
        if record == "z":                                     # (frames are in data units: the x columns times nv0)
            e = rel_l2(fr_[:, :, :3].numpy() / nv0, ref[k][:, :, :3].numpy())
        else:
            e = rel_l2(fr_[:, :, :3].numpy(), want[k].numpy())
            # the recorded x^0 shows the update: the data prediction of the network's own eps^ lies at least 100 times farther from
            # the restatement than the frame does (the clipped step is small next to an x^0 that is hundreds of units wide)
            assert rel_l2(bare_x0[k].numpy(), want[k].numpy()) > 100 * max(e, 2.0 ** -23), (k, e)
        print(f"recorded diverse chain record={record} [{precision}] frame of transition {k + 1}/{K}: rel_l2 {e:.2e}")
        assert e < REL_L2_TOL, (record, k, e)
    res = model.diversity_last
    assert tuple(res.phi.shape) == (2,) and tuple(res.rmsd.shape) == (2, 4, 4) and bool(torch.isfinite(res.mean_rmsd).all())
    want_rm = dr.phi_grad(x.cpu().double().numpy(), nm.reshape(B, N).numpy(), 4, dv.strength, dv.length)[1]
    assert np.allclose(res.rmsd.numpy(), want_rm, rtol=1e-10, atol=1e-12)


# ----------------------------------------------------------------------------- bit for bit

def call(model, nmd, dv, base=3, **kw):
    if "solver" not in kw:
        kw.setdefault("eta", 0.5)
    return model.sample_from_masks(nmd, None, None, sample_id_base=base, diversity=dv, steps=4, **kw)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replay_reattaching_and_detaching():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    nm, _, _ = batch()
    nmd = dev(nm)
    dv, dv2, dvg = Diversity(**DV), Diversity(**dict(DV, particles=2, scale=1.0)), Diversity(**dict(DV, scale=1.0))
    fresh(model, graph=False)
    want = {k: call(model, nmd, d) for k, d in (("dv", dv), ("dv2", dv2), ("dvg", dvg), ("plain", None))}
    assert not same(want["dv"], want["plain"]) and not same(want["dv"], want["dv2"]) and not same(want["dv"], want["dvg"])
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 8, nm.shape[1])
    assert same(call(model, nmd, None), want["plain"])        # a topology that never had it
    n0 = lib.hd_path_graph_builds(topo.ptr)
    assert same(call(model, nmd, dv), want["dv"])             # graph replay against plain launches
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 1
    assert same(call(model, nmd, Diversity(**DV)), want["dv"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 1       # same sizes: no graph is built
    assert same(call(model, nmd, dv2), want["dv2"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 2       # another P: one build
    assert same(call(model, nmd, dv2), want["dv2"])
    assert lib.hd_path_graph_builds(topo.ptr) == n0 + 2
    assert same(call(model, nmd, dvg), want["dvg"])
    assert same(call(model, nmd, dv), want["dv"])             # scale rows 1 -> G: one build each way
    assert same(call(model, nmd, None), want["plain"])        # after detaching: the bits of a topology that never had it
    # the keyword switched off is the call without it
    n1 = lib.hd_path_graph_builds(topo.ptr)
    plain = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=4, eta=0.5)
    assert same(plain, want["plain"])
    for off in (Diversity(1, 1.0), Diversity(4, 1.0, strength=0.0), Diversity(4, 1.0, scale=[0.0, 0.0])):
        assert same(call(model, nmd, off), want["plain"])
    assert lib.hd_path_graph_builds(topo.ptr) == n1
    full = model.sample_from_masks(nmd, None, None, sample_id_base=3)      # ... also where that is the plain every-step loop
    assert same(model.sample_from_masks(nmd, None, None, sample_id_base=3, diversity=Diversity(1, 1.0)), full)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_group_depends_on_its_own_rows_only_and_a_cut_chain_equals_the_whole(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    nm, _, _ = batch()
    nmd = dev(nm)
    dv = Diversity(**DV)
    for kw in (dict(), dict(eta=0.0), dict(solver="dpm2m")):  # a batch of 2 groups against its two groups run alone
        whole = call(model, nmd, dv, **kw)
        a = call(model, nmd[:4], dv.slice(0, 1), base=3, **kw)
        b = call(model, nmd[4:], dv.slice(1, 2), base=7, **kw)
        assert torch.equal(whole[0][:4], a[0]) and torch.equal(whole[0][4:], b[0]), kw
        assert torch.equal(whole[1][:4], a[1]) and torch.equal(whole[1][4:], b[1]), kw
    # path_steps cut in the middle
    g = torch.Generator().manual_seed(3)
    z = orc.combined_noise(torch.randn(8, 7, 3, generator=g), torch.randn(8, 7, 8, generator=g), nm.float())
    for kw in (dict(eta=1.0), dict(eta=0.0), dict(solver="sde2m")):
        whole = model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, diversity=dv, **kw)
        half = model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, k_lo=0, k_hi=2, diversity=dv, **kw)
        rest = model.path_steps(half, nmd, steps=4, sample_id_base=5, k_lo=2, k_hi=4, diversity=dv, **kw)
        assert torch.equal(whole, rest)
        assert not torch.equal(whole, model.path_steps(dev(z), nmd, steps=4, sample_id_base=5, **kw))


def test_cli_round_trip(tmp_path):
    import pickle
    from hierdiff_amd import sampler
    out = str(tmp_path / "o.pkl")
    argv = ["--hidden-nf", "32", "--n-layers", "1", "--timesteps", "8", "--batch-size", "4", "--num-batches", "1", "--out", out,
            "--steps", "4", "--eta", "0", "--diverse", "2", "--diverse-length", "1.0", "--diverse-strength", "0.5", "--diverse-clip", "0.3",
            "--diverse-schedule", "sigma"]
    assert sampler.main(argv) == 0
    with open(out, "rb") as f:
        res, _ = pickle.load(f)
    assert len(res) == 4 and [int(r["diversity_group"]) for r in res] == [0, 0, 1, 1]
    assert all(tuple(r["diversity_rmsd"].shape) == (2,) for r in res)


def test_list_level_results():
    model, _, _ = model_for("fp32")
    fresh(model)
    dv = Diversity(particles=4, length=1.0, clip=0.3)
    out = model.sample(8, DEV, steps=4, eta=0.0, diversity=dv)
    assert len(out) == 8 and [int(r['diversity_group']) for r in out] == [0] * 4 + [1] * 4
    assert len({r['x'].shape[0] for r in out[:4]}) == 1 and len({r['x'].shape[0] for r in out[4:]}) == 1      # one size per group
    for i, r in enumerate(out):
        assert r['diversity_rmsd'].dtype == torch.float64 and tuple(r['diversity_rmsd'].shape) == (4,) and float(r['diversity_rmsd'][i % 4]) == 0.0
    res = model.diversity_last
    assert torch.equal(res.rmsd[1, 2], out[6]['diversity_rmsd'])
    # vary: the variants of one input form its group
    mol = {"x": out[0]['x'], "h": out[0]['h']}
    var = model.vary([mol, mol], DEV, 4, n_variants=4, steps=2, diversity=dv)
    assert [int(r['diversity_group']) for r in var] == [0] * 4 + [1] * 4 and all(tuple(r['diversity_rmsd'].shape) == (4,) for r in var)
    n = out[0]['x'].shape[0]
    nmask = torch.ones(4, n, 1, dtype=torch.bool)
    rm = Diversity(4, 1.0).energy(torch.stack([r['x'] for r in var[:4]]).to(DEV), nmask.to(DEV), model=model)[1].cpu()
    assert torch.equal(rm[0, 1], var[1]['diversity_rmsd'])
