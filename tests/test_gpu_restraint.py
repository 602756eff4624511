"""GPU tier (-m gpu) of restraint-guided sampling: hd_restrain_eps and hd_restraint_energy against the float64 restatement of
tests/restraint_reference.py, the restrained path loop against `RestrainedNet` over the oracle with injected normals, and its
reproducibility: a zero scale, graph replay, batch split, chain cuts, guidance, recorded trajectories, refusals.

Bars.  hd_restrain_eps: the element-wise bar of tests/sampling_reference.py - every element within 8 * 2^-23 of the sum of the
absolute values of its terms.  hd_restraint_energy: 1e-12 of the sum of the absolute values of its terms (double rounding times a few
hundred terms in a fixed order).  Chain parity: rel-L2 < 1e-4 per state (tests/helpers.py REL_L2_TOL).  Measured figures are printed.
Shapes: B = 3 molecules of N in {5, 33} nodes at D in {4, 11}; chains at T = 8, H = 32, L = 2 (fp16x3: H = 128, L = 1)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from hierdiff_amd.restraints import Restraints
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import restraint_reference as rr
from tests import sampling_reference as sref
from tests import solver_reference as sr
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_parity import build_diffusion
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 8
SHAPES = {"fp32": (32, 2), "fp16x3": (128, 1)}
BOTH = ["fp32", "fp16x3"]


def dev(t):
    return None if t is None else t.to(DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ----------------------------------------------------------------------------- the kernels, on a bare handle (any D)

class Bare:
    """A handle of feature width D - 3 and a topology for `nm` [B,N] straight from the C ABI (the kernels need no weights)."""

    def __init__(self, D, nm):
        self.lib = lib = _lib.load()
        cfg = _lib.HdConfig(in_node_nf=D - 3 + 1, context_node_nf=0, n_dims=3, hidden_nf=32, n_layers=1, inv_sublayers=1, attention=1,
                            tanh=1, condition_time=1, norm_constant=0.0, normalization_factor=1.0, coords_range=15.0, precision=0,
                            aggregation_mean=0)
        self.h, self.topo = C.c_void_p(), C.c_void_p()
        assert lib.hd_create(C.byref(cfg), 0, C.byref(self.h)) == 0, lib.hd_last_error()
        m = np.ascontiguousarray(nm.numpy().astype(np.uint8))
        assert lib.hd_topology_create(self.h, m.ctypes.data, None, m.shape[0], m.shape[1], C.byref(self.topo)) == 0, lib.hd_last_error()
        self.ptr = self.topo                                  # `Restraints.attach` takes anything with .ptr

    def close(self):
        torch.cuda.synchronize()
        self.lib.hd_topology_destroy(self.topo)
        self.lib.hd_destroy(self.h)


def masks_for(N):
    nm = torch.zeros(3, N, dtype=torch.bool)
    for b, n in enumerate((N, (N + 1) // 2, 1)):              # a full molecule, a partly masked one, one valid node
        nm[b, :n] = True
    return nm


def run_restrain(bare, rs, scale, z, eps, row, nv0, alias):
    rs.attach(bare, scale, nv0, torch.device(DEV), stream())
    zd, ed = dev(z).contiguous(), dev(eps).contiguous()
    out = ed if alias else torch.full_like(ed, 7.0)
    r4 = (C.c_float * 4)(*row)
    rc = bare.lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, out.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    return out.cpu()


PQA = [(P, Q, A) for P in (0, 1, 7, 70) for Q in (0, 3) for A in (0, 2)]


@pytest.mark.parametrize("N,D", [(5, 4), (5, 11), (33, 4), (33, 11)])
def test_restrain_eps_against_float64(N, D):
    nm = masks_for(N)
    B = 3
    bare = Bare(D, nm)
    g = torch.Generator().manual_seed(N * 100 + D)
    z = torch.randn(B, N, D, generator=g)
    eps = torch.randn(B, N, D, generator=g)                   # masked rows hold values too: they must come back untouched
    scale = torch.tensor([1.0, 0.5, 2.0])
    nv0 = 1.7
    valid = nm.numpy()
    worst_all, moved = 0.0, 0
    try:
        for (P, Q, A) in PQA:
            for per in (False, True):
                rs, _ = rr.random_tables(B, N, P, Q, A, seed=P + 10 * Q + 100 * A + int(per), per_molecule=per)
                for clip in (math.inf, 0.2):
                    row = (0.8, 0.6, 0.75, clip)
                    ref, mag = rr.restrain_ref(rs, z, eps, nm, scale, row, nv0)
                    got = run_restrain(bare, rs, scale, z, eps, row, nv0, alias=False)
                    ali = run_restrain(bare, rs, scale, z, eps, row, nv0, alias=True)
                    assert torch.equal(got, ali)
                    err = np.abs(got.double().numpy() - ref)
                    ratio = float((err / (sref.BOUND * sref.U * np.maximum(mag, 1e-300))).max())
                    worst_all = max(worst_all, ratio)
                    print(f"hd_restrain_eps N={N} D={D} P={P} Q={Q} A={A} {'rows' if per else 'shared'} clip={clip}: "
                          f"worst err / bound {ratio:.3f}")
                    assert (err <= sref.BOUND * sref.U * mag).all(), (P, Q, A, per, clip, ratio)
                    e = eps.numpy()
                    g_ = got.numpy()
                    assert (g_[:, :, 3:] == e[:, :, 3:]).all() and (g_[~valid] == e[~valid]).all()
                    assert (g_[2] == e[2]).all()              # one valid node: eps unchanged
                    moved += int(not (g_[:2, :, :3] == e[:2, :, :3]).all())
        # clip active AND inactive within one call (the reference decides which nodes)
        rs, _ = rr.random_tables(B, N, 7, 3, 2, seed=5, per_molecule=True)
        x0 = rr.x0_f32(z, eps, 0.8, 0.6, nv0).numpy()
        gg_ = rr.energy_grad(rs, x0, nm)[2] * (scale.numpy().reshape(B, 1, 1) * 0.75)
        ln = np.sqrt((gg_ * gg_).sum(-1))[valid]
        ln = np.unique(ln[ln > 0])
        assert ln.size >= 2
        mid = float(np.float32(0.5 * (ln[ln.size // 2 - 1] + ln[ln.size // 2])))
        ref, mag = rr.restrain_ref(rs, z, eps, nm, scale, (0.8, 0.6, 0.75, mid), nv0)
        got = run_restrain(bare, rs, scale, z, eps, (0.8, 0.6, 0.75, mid), nv0, alias=True)
        assert (np.abs(got.double().numpy() - ref) <= sref.BOUND * sref.U * mag).all()
        # lambda = 0 and s_b = 0: bit-identical, aliased or not
        for sc, row in ((scale, (0.8, 0.6, 0.0, math.inf)), (torch.zeros(3), (0.8, 0.6, 0.75, 0.2)), (torch.zeros(1), (0.8, 0.6, 0.75, 0.2))):
            for alias in (False, True):
                assert torch.equal(run_restrain(bare, rs, sc, z, eps, row, nv0, alias), eps)
        part = run_restrain(bare, rs, torch.tensor([0.0, 1.0, 1.0]), z, eps, (0.8, 0.6, 0.75, 0.2), nv0, False)
        assert torch.equal(part[0], eps[0]) and not torch.equal(part[1], eps[1])
        # satisfied restraints leave eps's bits (-0.0 included)
        sat = Restraints(obstacles=[[100.0, 0, 0, 1.0, 5.0]], pairs=[[0, 1, 0.0, 1e6, 5.0]], anchors=[[0, 0, 0, 0, 1e6, 5.0]])
        e0 = eps.clone()
        e0[0, 0, 0] = -0.0
        out = run_restrain(bare, sat, scale, z, e0, (0.8, 0.6, 0.75, math.inf), nv0, False)
        assert (out.numpy().view(np.uint32) == e0.numpy().view(np.uint32)).all()
        # a node exactly on an obstacle's centre (alpha = 1, sigma = 0, nv0 = 1: x^0 = z): energy, no gradient, nothing non-finite
        c = z[0, 2, :3].tolist()
        onc = Restraints(obstacles=[c + [1.5, 2.0]])
        ref, mag = rr.restrain_ref(onc, z, eps, nm, scale, (1.0, 0.0, 0.75, math.inf), 1.0)
        got = run_restrain(bare, onc, scale, z, eps, (1.0, 0.0, 0.75, math.inf), 1.0, False)
        assert torch.isfinite(got).all()
        assert (np.abs(got.double().numpy() - ref) <= sref.BOUND * sref.U * mag).all()
        # argument errors
        lib, r4 = bare.lib, (C.c_float * 4)(0.8, 0.6, 0.75, 0.2)
        zd, ed = dev(z).contiguous(), dev(eps).contiguous()
        assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, zd.data_ptr(), stream()) == -1
        assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(0.0, 0.6, 1, 1), ed.data_ptr(), stream()) == -1
        assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 4)(0.8, 0.6, 1, -1), ed.data_ptr(), stream()) == -1
        assert lib.hd_restraint_detach(bare.topo) == 0
        assert lib.hd_restrain_eps(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), r4, ed.data_ptr(), stream()) == -4
        print(f"hd_restrain_eps N={N} D={D}: worst err / bound over all cases {worst_all:.3f}; eps moved in {moved} of {4 * len(PQA)}")
        assert moved >= len(PQA)                              # the cases are not no-ops
    finally:
        bare.close()


@pytest.mark.parametrize("N", [5, 33])
def test_restraint_energy_against_float64(N):
    nm = masks_for(N)
    B = 3
    bare = Bare(11, nm)
    g = torch.Generator().manual_seed(N)
    x = (torch.randn(B, N, 3, generator=g) * 1.5).contiguous()
    try:
        for (P, Q, A) in PQA:
            for per in (False, True):
                rs, centre = rr.random_tables(B, N, P, Q, A, seed=P + 10 * Q + 100 * A + int(per), per_molecule=per)
                xx = x.clone()
                if centre is not None:
                    xx[0, 2] = torch.from_numpy(centre.astype(np.float32))
                rs.attach(bare, torch.ones(1), 1.0, torch.device(DEV), stream())
                out = torch.full((B, 3), -1.0, device=DEV, dtype=torch.float64)
                xd = dev(xx).contiguous()
                assert bare.lib.hd_restraint_energy(bare.h, bare.topo, xd.data_ptr(), out.data_ptr(), stream()) == 0, bare.lib.hd_last_error()
                U, mag, _, _ = rr.energy_grad(rs, xx.numpy(), nm)
                err = np.abs(out.cpu().numpy() - U)
                print(f"hd_restraint_energy N={N} P={P} Q={Q} A={A} {'rows' if per else 'shared'}: worst err / (1e-12 sum|terms|) "
                      f"{float((err / np.maximum(1e-12 * mag, 1e-300)).max()):.3g}")
                assert (err <= 1e-12 * mag).all()
        assert bare.lib.hd_restraint_detach(bare.topo) == 0
        assert bare.lib.hd_restraint_energy(bare.h, bare.topo, xd.data_ptr(), out.data_ptr(), stream()) == -4
    finally:
        bare.close()


# ----------------------------------------------------------------------------- the models of the chain tests

@functools.lru_cache(maxsize=None)
def model_for(precision, C_=0):
    H, L = SHAPES[precision]
    sd_np, cfg = er.weights(H, L, C_=C_)
    model = build_diffusion(sd_np, H, L, C_=C_, T=T, precision=precision)
    model.seed = SEED
    return model, sd_np, cfg


@functools.lru_cache(maxsize=None)
def batch_for(mols, C_=0):
    return er.molecules(list(mols), C_=C_)


def fresh(model, graph=True):
    model.use_graph = graph
    model.restraints, model.restraint_scale, model.restraint_schedule, model.restraint_clip = None, None, "score", None
    model.guidance_scale, model.guidance_context, model.guidance_rescale = None, None, 0.0
    model.eval()
    return model


def tables(N, shift=0.0, P=2):
    obs = [[0.5 + shift, 0.0, 0.0, 1.5, 2.0], [-1.0, 1.0 + shift, 0.5, 1.0, 1.0]] + [[3.0 + p, shift, 0.0, 1.0, 1.0] for p in range(P - 2)]
    return Restraints(obstacles=obs, pairs=[[0, 1, 2.0 + shift, 2.5 + shift, 1.0], [2, 3, 0.0, 0.5, 1.0], [1, N + 3, 0.0, 1.0, 1.0]],
                      anchors=[[0, 1.0, 1.0 + shift, 1.0, 0.25, 1.5]])


RKW = dict(restraint_scale=0.05, restraint_clip=0.3)          # clipped: lambda = sigma / alpha is large at the noisy end


# ----------------------------------------------------------------------------- scale 0 is the unrestrained call, bit for bit

@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
@pytest.mark.parametrize("few", [dict(), dict(steps=4, eta=0.0)], ids=["identity", "K4eta0"])
def test_scale_zero_is_the_unrestrained_call_bit_for_bit(few, graph, precision):
    model, _, _ = model_for(precision)
    fresh(model, graph)
    x, h, nm, em, _ = batch_for((7, 4, 1))
    nmd, N = dev(nm), nm.shape[1]
    rs = tables(N)
    plain = model.sample_from_masks(nmd, None, None, sample_id_base=5, **few)
    for sc in (0, 0.0, torch.zeros(3), None):
        got = model.sample_from_masks(nmd, None, None, sample_id_base=5, restraints=rs, restraint_scale=sc, restraint_clip=0.3, **few)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # inside the kernel: molecules with s_b = 0 keep their bits while the others move
    part = model.sample_from_masks(nmd, None, None, sample_id_base=5, restraints=rs, restraint_scale=torch.tensor([0.0, 0.05, 0.0]),
                                   restraint_clip=0.3, **few)
    assert torch.equal(part[0][0], plain[0][0]) and torch.equal(part[0][2], plain[0][2]) and torch.equal(part[1][0], plain[1][0])
    assert not torch.equal(part[0][1], plain[0][1])
    again = model.sample_from_masks(nmd, None, None, sample_id_base=5, **few)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])


# ----------------------------------------------------------------------------- chain parity with injected normals

def reference_states(rnet, gg, path, eta, z, nm, raws, solver):
    """The state after every transition (fp32, rounded once per transition as the device loop keeps it)."""
    states = []
    if solver == "dpm2m":
        rows = sr.multistep_rows(gg, path, True)
        x_prev = None
        for k, t in enumerate(path[:-1]):
            x_prev, zs = sr.step_ref(rows[k], z, rnet.net(z, t), x_prev, nm.float())
            z = zs.float()
            states.append(z)
        return states
    nmd = nm.to(torch.float64)
    for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
        eps = rnet.net(z, t)
        if eta == 1.0:
            z = gr.ancestral_on_eps(rnet.c, z, eps, s, t, raws[k], gg).float()
        else:
            a, b, c = er.down_row(float(gg[s]), float(gg[t]), eta)
            z = er._centre_x(a * z.double() - b * er._centre_x(eps.double(), nmd), nmd).float()
        states.append(z)
    return states


@pytest.mark.parametrize("case", ["K4eta1", "KTeta1", "K4eta0", "KTeta0", "K4dpm2m", "KTdpm2m"])
def test_restrained_chain_parity_with_injected_normals(case):
    """Per state: rel-L2 < 1e-4 against `RestrainedNet` over the oracle."""
    steps = 4 if case.startswith("K4") else None
    solver = "dpm2m" if case.endswith("dpm2m") else None
    eta = 1.0 if case.endswith("eta1") else 0.0
    model, sd_np, cfg = model_for("fp32")
    fresh(model)
    x, h, nm, em, _ = batch_for((7, 4, 1))
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, steps)
    K = len(path) - 1
    raws = er.raw_draws(K + 1, B, N, seed=K)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    rs = tables(N)
    scale = torch.tensor([0.05, 0.02, 0.05])
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    rnet = rr.RestrainedNet(net, rs, scale, rr.rows_from_grid(gg, path, "score", 0.3))
    ref = reference_states(rnet, gg, path, eta, z, nm, raws[1:], solver)
    plain = reference_states(rr.RestrainedNet(net, rs, torch.zeros(B), {}), gg, path, eta, z, nm, raws[1:], solver)
    kw = dict(steps=steps, restraints=rs, restraint_scale=scale, restraint_clip=0.3)
    kw.update(dict(solver="dpm2m") if solver else dict(eta=eta))
    zz, worst = dev(z), 0.0
    for k in range(K):
        rn = None if (solver or eta == 0.0) else [raws[1 + k]]
        zz = model.latent_steps(zz, dev(nm), dev(em), None, k_lo=k, k_hi=k + 1, raw_noises=rn, **kw)
        r = rel_l2(zz.cpu().numpy(), ref[k].numpy())
        worst = max(worst, r)
        print(f"restrained parity {case} state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
        assert torch.isfinite(zz).all()
        assert r < REL_L2_TOL, (case, k, r)
    d = rel_l2(ref[-1].numpy(), plain[-1].numpy())
    print(f"restrained parity {case}: worst state {worst:.2e}; distance of the restrained z_0 from the unrestrained one {d:.2e}")
    assert d > 10 * REL_L2_TOL                                # not a no-op: the unrestrained chain lies far outside the bar


# ----------------------------------------------------------------------------- graph replay

def test_graph_replay_equals_launches_and_reattaching_does_not_rebuild():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    x, h, nm, em, _ = batch_for((7, 4, 1))
    nmd, N = dev(nm), nm.shape[1]
    kw = dict(sample_id_base=3, steps=4, eta=0.5, **RKW)
    a, b, big = tables(N), tables(N, shift=0.25), tables(N, P=9)
    fresh(model, graph=False)
    want = {k: model.sample_from_masks(nmd, None, None, restraints=r, **kw) for k, r in (("a", a), ("b", b), ("big", big))}
    want["plain"] = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=4, eta=0.5)
    assert not torch.equal(want["a"][0], want["b"][0]) and not torch.equal(want["a"][0], want["plain"][0])
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, 3, N)
    same = lambda got, k: torch.equal(got[0], want[k][0]) and torch.equal(got[1], want[k][1])
    n0 = lib.hd_path_graph_builds(topo.ptr)
    assert same(model.sample_from_masks(nmd, None, None, restraints=a, **kw), "a")
    n1 = lib.hd_path_graph_builds(topo.ptr)
    assert n1 == n0 + 1
    assert same(model.sample_from_masks(nmd, None, None, restraints=b, **kw), "b")            # equal sizes: a copy, no rebuild
    assert same(model.sample_from_masks(nmd, None, None, restraints=a, **dict(kw, restraint_scale=torch.full((3,), 0.05))), "a")
    assert lib.hd_path_graph_builds(topo.ptr) == n1 + 1                                       # (scale rows 1 -> 3: one rebuild)
    assert same(model.sample_from_masks(nmd, None, None, restraints=b, **dict(kw, restraint_scale=torch.full((3,), 0.05))), "b")
    assert lib.hd_path_graph_builds(topo.ptr) == n1 + 1
    assert same(model.sample_from_masks(nmd, None, None, restraints=big, **dict(kw, restraint_scale=torch.full((3,), 0.05))), "big")
    assert lib.hd_path_graph_builds(topo.ptr) == n1 + 2                                       # a grown P rebuilds once
    assert same(model.sample_from_masks(nmd, None, None, restraints=big, **dict(kw, restraint_scale=torch.full((3,), 0.05))), "big")
    assert lib.hd_path_graph_builds(topo.ptr) == n1 + 2
    assert same(model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=4, eta=0.5), "plain")   # unrestrained afterwards
    assert same(model.sample_from_masks(nmd, None, None, restraints=a, **kw), "a")


def check_row_setter_and_the_captured_graph(steer):
    """hd_set_restraint (`steer`: hd_set_steer) between graph-replayed hd_sample_path calls at the C ABI, B = 4, N = 5, K = 3, hidden 32:
    rows of the same K land in the table the captured transition already reads - no graph is built and the rows that were set are the
    ones that act - and rows of another K (which takes a path of that K) cost exactly one build."""
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    fresh(model, graph=True)
    _, _, nm, _, _ = batch_for((5, 4, 3, 1))
    nmd = dev(nm)
    B, N = nm.shape[:2]
    hnd, tabs = model._lib_handle(), model._schedule(rows=B)
    topo = model.dynamics.topology(nmd, None, B, N)
    g = torch.Generator().manual_seed(11)
    zT = dev(orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float()))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda v: np.ascontiguousarray(v.numpy()).ctypes.data_as(C.POINTER(C.c_int))

    def set_path(K):
        pt = paths.path_tables(tabs["gamma"], paths.uniform_path(T, K), eta=0.5)
        coef = np.ascontiguousarray(pt["coef"].numpy())
        assert lib.hd_set_path(hnd, K, ip(pt["t_idx"]), ip(pt["s_idx"]), fp(coef), pt["form"], None) == 0, lib.hd_last_error()

    def set_rows(K, strength):
        rows4 = np.ascontiguousarray(np.tile(np.array([0.8, 0.6, 0.0 if steer else strength, 0.3], dtype=np.float32), (K, 1)))
        assert lib.hd_set_restraint(hnd, K, fp(rows4)) == 0, lib.hd_last_error()
        if steer:
            rows3 = np.ascontiguousarray(np.tile(np.array([0.8, 0.6, strength], dtype=np.float32), (K, 1)))
            assert lib.hd_set_steer(hnd, K, fp(rows3)) == 0, lib.hd_last_error()

    def run(K):
        z = zT.clone()
        assert lib.hd_sample_path(hnd, topo.ptr, z.data_ptr(), None, -1, 0, K, None, None, B, SEED, 3, 1, stream()) == 0, lib.hd_last_error()
        torch.cuda.synchronize()
        return z

    builds = lambda: lib.hd_path_graph_builds(topo.ptr)
    rs, _ = rr.random_tables(B, N, 3, 2, 2, seed=4, per_molecule=False)
    model._path_cache = None                                  # the handle's path and rows are set behind the model's back
    try:
        rs.attach(topo, torch.ones(1), 1.0, torch.device(DEV), stream())
        if steer:
            assert lib.hd_steer_attach(topo.ptr, 2, 0.5, 1, stream()) == 0, lib.hd_last_error()
        set_path(3)
        set_rows(3, 0.05)
        n0 = builds()
        first = run(3)
        assert builds() == n0 + 1
        set_rows(3, 0.4)
        other = run(3)
        assert builds() == n0 + 1, "rows of the same K rebuilt the captured transition"
        if not steer:
            assert not torch.equal(other, first), "the captured transition did not read the new rows"
        if steer:
            assert lib.hd_steer_attach(topo.ptr, 2, 0.5, 1, stream()) == 0, lib.hd_last_error()
        set_rows(3, 0.05)
        assert torch.equal(run(3), first) and builds() == n0 + 1
        set_path(2)
        set_rows(2, 0.05)
        if steer:
            assert lib.hd_steer_attach(topo.ptr, 2, 0.5, 1, stream()) == 0, lib.hd_last_error()
        run(2)
        assert builds() == n0 + 2, "rows of another K (and their path) cost exactly one build"
        set_rows(2, 0.4)
        run(2)
        assert builds() == n0 + 2
    finally:
        lib.hd_steer_detach(topo.ptr)
        lib.hd_restraint_detach(topo.ptr)
        model._path_cache = model._row_caches = None


def test_restraint_rows_of_the_same_K_keep_the_captured_graph_and_another_K_builds_one():
    check_row_setter_and_the_captured_graph(steer=False)


# ----------------------------------------------------------------------------- independence of batch and chain cuts

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_molecule_depends_on_its_id_and_its_own_rows_only(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    x, h, nm, em, _ = batch_for((7, 4, 1, 6))
    B, N = nm.shape[:2]
    g = torch.Generator().manual_seed(1)
    obs = torch.cat([torch.randn(B, 3, 3, generator=g), torch.full((B, 3, 1), 1.5), torch.full((B, 3, 1), 2.0)], dim=2)
    anc = torch.cat([torch.zeros(B, 1, 1), torch.randn(B, 1, 3, generator=g), torch.full((B, 1, 1), 0.25), torch.ones(B, 1, 1)], dim=2)
    rs = Restraints(obstacles=obs, pairs=[[0, 1, 2.0, 2.5, 1.0]], anchors=anc)
    scale = torch.tensor([0.05, 0.03, 0.05, 0.08])
    kw = dict(steps=4, eta=1.0, restraint_clip=0.3)
    whole = model.sample_from_masks(dev(nm), None, None, sample_id_base=11, restraints=rs, restraint_scale=scale, **kw)
    for b in range(B):
        one = model.sample_from_masks(dev(nm[b:b + 1]), None, None, sample_id_base=11 + b, restraints=rs.slice(b, b + 1),
                                      restraint_scale=scale[b:b + 1], **kw)
        assert torch.equal(one[0][0], whole[0][b]) and torch.equal(one[1][0], whole[1][b]), b


@pytest.mark.parametrize("solver", [None, "dpm2m"])
def test_a_cut_chain_equals_the_whole(solver):
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, _ = batch_for((7, 4, 1))
    B, N = nm.shape[:2]
    raw = er.raw_draws(1, B, N, seed=2)[0]
    z = dev(orc.combined_noise(raw[0], raw[1], nm.float()))
    kw = dict(steps=6, restraints=tables(N), sample_id_base=4, **RKW)
    kw.update(dict(solver="dpm2m") if solver else dict(eta=0.5))
    whole = model.path_steps(z, dev(nm), **kw)
    cut = model.path_steps(model.path_steps(z, dev(nm), k_hi=2, **kw), dev(nm), k_lo=2, **kw)
    assert torch.equal(cut, whole)
    assert not torch.equal(whole, model.path_steps(z, dev(nm), steps=6, sample_id_base=4, **({"solver": "dpm2m"} if solver else {"eta": 0.5})))


# ----------------------------------------------------------------------------- combinations

def test_restrained_and_guided():
    model, sd_np, cfg = model_for("fp32", 1)
    x, h, nm, em, ctx = batch_for((7, 4, 1), 1)
    N = nm.shape[1]
    kw = dict(sample_id_base=2, steps=4, eta=1.0, guidance_scale=2.0)
    out = {}
    for graph in (False, True):
        fresh(model, graph)
        out[graph] = (model.sample_from_masks(dev(nm), None, dev(ctx), restraints=tables(N), **kw, **RKW),
                      model.sample_from_masks(dev(nm), None, dev(ctx), **kw))
    assert torch.equal(out[True][0][0], out[False][0][0]) and torch.equal(out[True][1][0], out[False][1][0])
    assert torch.isfinite(out[True][0][0]).all() and not torch.equal(out[True][0][0], out[True][1][0])
    # one transition against the restatement: guided, then restrained
    fresh(model)
    B = nm.shape[0]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, 4)
    raws = er.raw_draws(2, B, N, seed=8)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    net_c, net_u = er.RefNet(sd_np, cfg, T, nm, em, ctx), er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm))
    rnet = rr.RestrainedNet(gr.GuidedNet(net_c, net_u, 2.0, 0.0), tables(N), torch.tensor([0.05]), rr.rows_from_grid(gg, path, "score", 0.3))
    ref = gr.ancestral_on_eps(net_c, z, rnet.net(z, path[0]), path[1], path[0], raws[1], gg)
    got = model.latent_steps(dev(z), dev(nm), dev(em), dev(ctx), steps=4, eta=1.0, guidance_scale=2.0, k_hi=1, raw_noises=[raws[1]],
                             restraints=tables(N), **RKW)
    r = rel_l2(got.cpu().numpy(), ref.numpy())
    print(f"restrained + guided, one transition: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e})")
    assert r < REL_L2_TOL


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_keep_frames_with_x0_under_restraints(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    x, h, nm, em, _ = batch_for((7, 4, 1))
    N = nm.shape[1]
    kw = dict(sample_id_base=6, steps=4, eta=0.0, restraints=tables(N), **RKW)
    xg, hg, chain = model.sample_from_masks(dev(nm), None, None, keep_frames=4, record="x0", **kw)
    assert chain.shape[0] == 4 and torch.isfinite(chain).all()
    assert torch.equal(chain[0], torch.cat([xg, hg], dim=2))                       # frame 0 is the call's own output
    x2, h2 = model.sample_from_masks(dev(nm), None, None, **kw)                    # recording changes no sample
    assert torch.equal(x2, xg) and torch.equal(h2, hg)
    _, _, plain = model.sample_from_masks(dev(nm), None, None, sample_id_base=6, steps=4, eta=0.0, keep_frames=4, record="x0")
    assert not torch.equal(plain[3], chain[3])                                     # the frames show the restrained prediction


def test_list_level_results_carry_the_energy():
    """Reported, not asserted: the mean restraint energy of a restrained B = 8 run against the same ids unrestrained (synthetic
    weights: says nothing chemical)."""
    model, _, _ = model_for("fp32")
    fresh(model)
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]], pairs=[[0, 1, 3.0, 4.0, 1.0]], anchors=[[2, 3.0, 0.0, 0.0, 0.5, 1.0]])
    torch.manual_seed(3)
    on = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, **RKW)
    torch.manual_seed(3)
    off = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, restraint_scale=1e-30, restraint_clip=0.3)
    torch.manual_seed(3)
    plain = model.sample(8, DEV, sample_id_base=40, steps=8)
    assert all(r["restraint_energy"].shape == (3,) and r["restraint_energy"].dtype == torch.float64 for r in on)
    assert all("restraint_energy" not in r for r in plain)
    e_on = torch.stack([r["restraint_energy"] for r in on]).sum(1)
    e_off = torch.stack([r["restraint_energy"] for r in off]).sum(1)
    print(f"mean restraint energy, B = 8, synthetic weights: restrained {float(e_on.mean()):.4g}, unrestrained {float(e_off.mean()):.4g}")
    assert torch.isfinite(e_on).all() and torch.isfinite(e_off).all()
    # the energy is that of the returned x, by the CPU formulas
    for r in on:
        n = r["x"].shape[0]
        want = rs.energy(r["x"].double().unsqueeze(0), torch.ones(1, n, 1))[0]
        assert torch.allclose(r["restraint_energy"], want, rtol=1e-9, atol=1e-12)
    var = model.vary(plain[:2], DEV, 4, n_variants=2, steps=2, restraints=rs, **RKW)
    assert len(var) == 4 and all(r["restraint_energy"].shape == (3,) for r in var)


# ----------------------------------------------------------------------------- refusals on the device path

def test_device_path_refusals():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, _ = batch_for((7, 4, 1))
    B, N = nm.shape[:2]
    nmd = dev(nm)
    z = torch.zeros(B, N, 11, device=DEV)
    want = model.path_steps(z, nmd, steps=4, sample_id_base=1)                     # sets the path; no restraint rows for it yet
    hnd, topo = model._lib_handle(), model.dynamics.topology(nmd, None, B, N)
    rs = tables(N)
    rs.attach(topo, torch.ones(1), 1.0, torch.device(DEV), stream())
    try:
        zz = z.clone()
        fm = torch.zeros(B, N, dtype=torch.uint8, device=DEV)
        args = (hnd, topo.ptr, zz.data_ptr(), None, -1, 0, 4, None, None, B, SEED, 1, 1)
        assert lib.hd_sample_path_inpaint(*args, fm.data_ptr(), zz.data_ptr(), 1, stream()) == -1
        assert b"restraints are attached" in lib.hd_last_error()
        model._row_caches = None
        rows = (C.c_float * 16)(*([0.8, 0.6, 0.5, 0.3] * 4))
        assert lib.hd_set_restraint(hnd, 3, rows) == -1 and b"K differs" in lib.hd_last_error()
        assert lib.hd_set_restraint(hnd, 4, (C.c_float * 16)(*([0.8, 0.6, 0.5, 0.0] * 4))) == -1
        assert lib.hd_set_restraint(hnd, 4, rows) == 0, lib.hd_last_error()
        assert lib.hd_sample_path(hnd, topo.ptr, zz.data_ptr(), None, N - 1, 0, 4, None, None, B, SEED, 1, 1, stream()) == -1
        assert b"whole molecules" in lib.hd_last_error()
    finally:
        Restraints.detach(topo)
    model.path_steps(z, nmd, steps=3, sample_id_base=1)                             # a new path without new rows: HD_E_STATE, not stale rows
    rs.attach(topo, torch.ones(1), 1.0, torch.device(DEV), stream())
    try:
        zz = z.clone()
        assert lib.hd_sample_path(hnd, topo.ptr, zz.data_ptr(), None, -1, 0, 3, None, None, B, SEED, 1, 1, stream()) == -4
        assert b"hd_set_restraint" in lib.hd_last_error()
        # the every-step loop ignores attached restraints
        za, zb = z.clone(), z.clone()
        assert lib.hd_sample_loop(hnd, topo.ptr, za.data_ptr(), None, -1, T, T - 2, None, None, B, SEED, 1, 1, stream()) == 0
    finally:
        Restraints.detach(topo)
    assert lib.hd_sample_loop(hnd, topo.ptr, zb.data_ptr(), None, -1, T, T - 2, None, None, B, SEED, 1, 1, stream()) == 0
    assert torch.equal(za, zb)
    model._row_caches = None
    assert torch.equal(model.path_steps(z, nmd, steps=4, sample_id_base=1), want)
    with pytest.raises(NotImplementedError, match="restraints"):
        model.sample_inpaint(nmd, nmd, z[:, :, :3], z[:, :, 3:], restraints=rs)
