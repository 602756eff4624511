"""CPU tier of the field restraints: the float64 restatement of tests/field_reference.py against float64 autograd of
`restraints.field_energy_terms`, hand-computed values at exact points, the conditioning of the kernel test's inputs (no coordinate on
a lattice plane; every mutant of the restatement misses the GPU bars there), `Field.from_obstacles` against the sphere energy, the
restrained chain over the oracle with the field term, and the host API: argument errors, steering groups, JSON, the C ABI without a
device, the CLI."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths, restraints, steering
from hierdiff_amd.restraints import Field, Restraints
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import field_reference as fr
from tests import guidance_reference as gr
from tests import restraint_frame_reference as rf
from tests import restraint_reference as rr
from tests import sampling_reference as sref
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_inpaint_cpu import gamma_grid_fp64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 4), (5, 11), (33, 4), (33, 11)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def first_cases(N, D, framed, every=5):
    """A thinned walk through the kernel cases (every `every`-th: all NF, both weight kinds, both table settings, both clips occur)."""
    return [c for i, c in enumerate(fr.kernel_cases(N, D, framed)) if i % every == 0]


# ----------------------------------------------------------------------------- the restatement

def autograd(rs, x, nm):
    with torch.enable_grad():
        xv = torch.as_tensor(x).clone().double().requires_grad_(True)
        U = restraints.field_energy_terms(rs, xv, torch.as_tensor(nm).reshape(xv.shape[0], -1, 1))
        U.sum().backward()
    return U.detach().numpy(), xv.grad.numpy()


@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
def test_hand_derived_gradient_equals_float64_autograd(framed):
    """Away from the lattice planes (asserted below) the interpolant is smooth: the restatement and autograd of the product's torch
    formulas agree to double rounding."""
    n = 0
    for c in first_cases(33, 4, framed):
        x, valid = fr.data_prediction(c)
        U, Um, g, ga = fr.field_energy_grad(c.rs, x, valid)
        Ut, gt = autograd(c.rs, x, valid)
        assert np.abs(U - Ut).max() <= 1e-12 * max(1.0, Um.max()), c.name
        assert (np.abs(g - gt) <= 1e-12 * np.maximum(ga, 1e-300)).all(), c.name
        assert np.abs(g).max() > 0
        n += 1
    assert n >= 4


def test_exact_points_by_hand():
    c = fr.exact_case()
    v = c.values
    f0, f1 = c.rs.fields                                      # k = 1, wall = 0; k = 0.5, wall = 2
    h = np.array([0.5, 1.0, 2.0])
    x = c.z[0, :, :3].double().numpy()
    zero = np.zeros(3)
    # a node exactly on the interior lattice point (1, 1, 1): the value, and the right-hand cell's gradient
    e, _, g, _ = fr.field_node(f0, x[0], zero)
    assert e == v[1, 1, 1]
    assert (g == np.array([v[2, 1, 1] - v[1, 1, 1], v[1, 2, 1] - v[1, 1, 1], v[1, 1, 2] - v[1, 1, 1]]) / h).all()
    # exactly on the upper boundary, every axis: the value, and the LAST cell's gradient with t = 1
    e, _, g, _ = fr.field_node(f0, x[1], zero)
    assert e == v[2, 3, 4]
    assert (g == np.array([v[2, 3, 4] - v[1, 3, 4], v[2, 3, 4] - v[2, 2, 4], v[2, 3, 4] - v[2, 3, 3]]) / h).all()
    # outside each of the six faces by (1, 1, 1/2, 1/2, 1/2, 1/2) cells: the boundary's bilinear value, no in-box gradient along
    # that axis, the wall 1/2 wall out^2 with out = cells x h in data units
    faces = [(0, -0.5, v[0, 1:3, 2:4]), (0, 0.5, v[2, 1:3, 2:4]), (1, -0.5, v[0:2, 0, 2:4]), (1, 0.5, v[0:2, 3, 2:4]),
             (2, -1.0, v[0:2, 1:3, 0]), (2, 1.0, v[0:2, 1:3, 4])]
    for i, (axis, out, slab) in enumerate(faces):
        for f in (f0, f1):
            e, _, g, _ = fr.field_node(f, x[2 + i], zero)
            assert e == pytest.approx(slab.mean() + 0.5 * f.wall * out * out, abs=1e-14), (i, f.wall)
            assert g[axis] == f.wall * out, (i, f.wall)       # only the wall; 0 with wall = 0
            others = [a for a in range(3) if a != axis]
            want = [(slab[1, :].mean() - slab[0, :].mean()) / h[others[0]], (slab[:, 1].mean() - slab[:, 0].mean()) / h[others[1]]]
            assert g[others] == pytest.approx(want, abs=1e-14)
    # inside cell (0, 1, 2) at t = (1/2, 1/2, 1/2): the mean of the 8 corners
    e, _, g, _ = fr.field_node(f0, x[8], zero)
    cube = v[0:2, 1:3, 2:4]
    assert e == pytest.approx(cube.mean(), abs=1e-14)
    assert g == pytest.approx([(cube[1].mean() - cube[0].mean()) / 0.5, (cube[:, 1].mean() - cube[:, 0].mean()) / 1.0,
                               (cube[:, :, 1].mean() - cube[:, :, 0].mean()) / 2.0], abs=1e-14)
    # a NaN coordinate: neither energy nor gradient
    assert fr.field_node(f0, x[9], zero) is None
    U, _, gg, _ = fr.field_energy_grad(c.rs, x[None], c.nm)
    assert np.isfinite(U).all() and (gg[0, 9] == 0).all()
    # the product's CPU formulas give the same numbers, the NaN node included
    Up = c.rs.field_energy(torch.from_numpy(x[None]), c.nm.reshape(1, -1, 1))
    assert Up.dtype == torch.float64 and Up.shape == (1,)
    assert float(Up[0]) == pytest.approx(float(U[0]), rel=1e-14)
    parts = [k * (fr.field_node(f, x[i], zero)[0]) for f, k in ((f0, 1.0), (f1, 0.5)) for i in range(9)]
    assert float(U[0]) == pytest.approx(sum(parts), rel=1e-14)
    # the whole update on these points is finite, and the NaN node's x^0 stays out of every other node's step
    out, _ = fr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0)
    assert np.isfinite(out).all()


# ----------------------------------------------------------------------------- conditioning of the kernel test's inputs

@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_no_generated_coordinate_lies_on_a_lattice_plane(N, D, framed):
    worst = math.inf
    for c in fr.kernel_cases(N, D, framed):
        x, valid = fr.data_prediction(c)
        worst = min(worst, fr.plane_distance(c.rs, x, valid))
    print(f"N={N} D={D} {'known' if framed else 'model'} frame: smallest distance from a lattice plane {worst:.3g} cell widths")
    assert worst > 1e-6


def bar_ratio(c, mutant):
    ref, mag = fr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known)
    mut, _ = fr.restrain_ref(c.rs, c.z, c.eps, c.nm, c.scale, c.row, c.nv0, c.fm, c.known, mutant=mutant)
    return float((np.abs(mut - ref) / (sref.BOUND * sref.U * np.maximum(mag, 1e-300))).max())


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_every_mutant_misses_the_gpu_bars_on_the_kernel_inputs(mutant):
    """The eps bar (8 * 2^-23 of the sum of the absolute terms) on the cases of the kernel test; for the mutants that change the
    energy, the energy bar (1e-12 of the sum of the absolute terms) too."""
    framed = mutant == "tau_sign"                             # tau is 0 in the model's frame
    cases = first_cases(5, 4, framed, every=7) + [fr.exact_case()]
    worst = max(bar_ratio(c, mutant) for c in cases)
    print(f"mutant {mutant}: worst eps error / bar {worst:.3g}")
    assert worst > 1.0
    if mutant in ("no_inv_h", "no_cap"):                      # gradient-only mistakes
        return
    eworst = 0.0
    for c in cases:
        x0 = rr.x0_f32(c.z, c.eps, c.row[0], c.row[1], c.nv0).numpy().astype(np.float64)
        if c.fm is None:
            U, Um, _, _ = fr.field_energy_grad(c.rs, x0, c.nm)
            Ub, _, _, _ = fr.field_energy_grad(c.rs, x0, c.nm, mutant=mutant)
        else:
            xk = c.x_known.double().numpy()
            U, Um, _ = fr.field_energy_framed(c.rs, x0, xk, c.nm, c.fm)
            Ub, _, _ = fr.field_energy_framed(c.rs, x0, xk, c.nm, c.fm, mutant=mutant)
        eworst = max(eworst, float((np.abs(U - Ub) / np.maximum(1e-12 * Um, 1e-300)).max()))
    print(f"mutant {mutant}: worst energy error / bar {eworst:.3g}")
    assert eworst > 1.0


# ----------------------------------------------------------------------------- from_obstacles

def test_from_obstacles_equals_the_sphere_energy_at_lattice_points():
    obs = [[0.5, 0.2, -0.3, 1.5, 2.0], [-1.0, 0.0, 0.25, 1.0, 3.0], [0.0, 0.0, 0.0, 0.0, 1.0]]
    o, shape, h = [-2.0, -1.5, -1.0], (9, 5, 4), (0.5, 0.75, 1.0)
    f = Field.from_obstacles(obs, o, shape, h, k=1.0)
    assert tuple(f.values.shape) == shape and f.values.dtype == torch.float32
    rs_o = Restraints(obstacles=obs)
    one = torch.ones(1, 1, 1)
    hit = 0
    for i in range(shape[0]):
        for j in range(shape[1]):
            for k in range(shape[2]):
                y = torch.tensor([[[o[0] + i * h[0], o[1] + j * h[1], o[2] + k * h[2]]]], dtype=torch.float64)
                want = float(rs_o.energy(y, one)[0, 0])
                assert float(f.values[i, j, k]) == float(np.float32(want)), (i, j, k)       # its one fp32 rounding
                hit += int(want > 0)
                # ... and the field read at the lattice point gives that value back
                assert float(Restraints(fields=f).field_energy(y, one)[0]) == float(np.float32(want))
    assert hit > 10
    with pytest.raises(ValueError):
        Field.from_obstacles(obs, o, (9, 5, 1), h)
    with pytest.raises(ValueError):
        Field.from_obstacles(torch.ones(2, 1, 5), o, shape, h)
    with pytest.raises(ValueError):
        Field.from_obstacles(obs, o, shape, 0.0)


# ----------------------------------------------------------------------------- the restrained chain over the oracle

T = 8


def chain_fields(centre=(0.0, 0.0, 0.0)):
    g = np.random.Generator(np.random.PCG64(5))
    o = np.array([-3.0, -2.5, -3.5]) + np.asarray(centre)
    return [Field(g.normal(0.0, 2.0, (4, 5, 3)), o.tolist(), (2.0, 1.25, 3.5), k=1.5, wall=0.5),
            Field(g.normal(0.0, 2.0, (2, 2, 2)), (o - 1.0).tolist(), 8.0, k=1.0, weights=[1.0, 0.0, 2.0, 1.0])]


@pytest.mark.parametrize("framed", [False, True], ids=["model", "known"])
def test_restrained_chain_with_a_field_moves_the_sample(framed):
    """T = 8, K = 4 over the oracle: the chain with the field term ends more than 10x the chain bar away from the unrestrained one,
    and the field moved eps^ in every restrained network call."""
    sd_np, cfg = er.weights(32, 2)
    x, h, nm, em, _ = er.molecules([7, 4, 5])
    model = er.cpu_diffusion(sd_np, 32, 2, T)
    gg = gamma_grid_fp64(model, T)
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    B, N = nm.shape[:2]
    path = paths.build_path(T, 4)
    rows = rr.rows_from_grid(gg, path, "score", 0.3)
    scale = torch.tensor([0.05, 0.02, 0.05])
    if not framed:
        raws = er.raw_draws(len(path), B, N, seed=6)
        z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
        fnet = fr.FieldNet(net, Restraints(fields=chain_fields()), scale, rows)
        plain = gr.guided_chain_ref(gr.GuidedNet(net, net, 1.0, 0.0), gg, path, 1.0, z, nm, raws)[2]
        on = gr.guided_chain_ref(fnet, gg, path, 1.0, z, nm, raws)[2]
    else:
        lib = _lib.load()
        fm = torch.zeros(B, N, 1, dtype=torch.bool)
        fm[0, 1:4] = True
        fm[2, :2] = True
        g = torch.Generator().manual_seed(3)
        known = torch.randn(B, N, 11, generator=g)
        known[:, :, :3] = torch.tensor(rf.CENTRE) + torch.randn(B, N, 3, generator=g) * 1.5
        known = known * nm.float()
        raw = er.raw_draws(1, B, N, seed=6)[0]
        z = orc.combined_noise(raw[0], raw[1], nm.float())
        fnet = fr.FieldNet(net, Restraints(fields=chain_fields(rf.CENTRE)), scale, rows, nm=nm, fm=fm, known=known)
        ids = list(range(B))
        off = fr.FieldNet(net, Restraints(), torch.zeros(B), rows, nm=nm, fm=fm, known=known)      # scale 0: eps^ itself
        plain = rf.inpaint_path_ref(lib, off, gg, path, T, z, nm, fm, known, 1, 7, ids)[-1]
        on = rf.inpaint_path_ref(lib, fnet, gg, path, T, z, nm, fm, known, 1, 7, ids)[-1]
    d = rel_l2(on.numpy(), plain.numpy())
    print(f"{'known' if framed else 'model'} frame: distance of the fielded z_0 from the unrestrained one {d:.3g}; the field moved eps^ in "
          f"{fnet.active} of {fnet.calls} network calls")
    assert torch.isfinite(on).all()
    assert d > 10 * REL_L2_TOL
    assert fnet.calls == 4 and fnet.active == fnet.calls


# ----------------------------------------------------------------------------- the containers

V222 = np.arange(8.0).reshape(2, 2, 2)


def test_field_and_restraints_accept_the_documented_forms():
    f = Field(V222, [0, 0, 0], 1.0)
    assert (f.k, f.wall, f.weights, f.rows) == (1.0, 0.0, None, 1) and f.spacing.tolist() == [1.0, 1.0, 1.0]
    f3 = Field(torch.from_numpy(V222), (1, 2, 3), (0.5, 1, 2), k=2, wall=0.5, weights=[1.0, 0.0])
    assert f3.spacing.tolist() == [0.5, 1.0, 2.0] and f3.weights.shape == (1, 2)
    assert f3.node_weights(4).tolist() == [[1.0, 0.0, 0.0, 0.0]]          # nodes i >= W take 0
    assert f3.node_weights(1).tolist() == [[1.0]]
    fb = Field(V222, [0, 0, 0], 1.0, weights=torch.ones(3, 5))
    rs = Restraints(obstacles=[[0, 0, 0, 1, 2]], fields=[f, fb])
    assert rs.n_fields == 2 and rs.sizes == (1, 0, 0) and rs.rows() == (1, 1, 1) and rs.field_rows() == 3
    assert Restraints(fields=f).n_fields == 1 and Restraints().n_fields == 0
    assert rs.field_weights(4).shape == (3, 2, 4)
    rs.check_batch(3)
    with pytest.raises(ValueError, match="field weights hold rows for 3 molecules"):
        rs.check_batch(4)
    s = rs.slice(1, 3)
    assert s.n_fields == 2 and s.field_rows() == 2 and s.fields[0] is f and s.fields[1].values is fb.values
    # `energy` keeps its [B, 3]; the field energy is its own [B] float64
    x, nm = torch.zeros(3, 2, 3, dtype=torch.float64), torch.ones(3, 2, 1)
    assert rs.energy(x, nm).shape == (3, 3)
    e = rs.field_energy(x, nm)
    assert e.shape == (3,) and e.dtype == torch.float64 and e.tolist() == [0.0, 0.0, 0.0]   # v[0,0,0] = 0
    # in the known frame: x - tau
    xk = torch.full((3, 2, 3), 5.0, dtype=torch.float64)
    fm = torch.ones(3, 2, 1)
    shifted = Restraints(fields=Field(V222, [5.0, 5.0, 5.0], 1.0))
    assert shifted.field_energy(x + 0.5, nm).tolist() == [0.0] * 3                          # outside, wall 0: v[0,0,0]
    got = shifted.field_energy(x, nm, fixed_mask=fm, x_known=xk + 0.5)                      # tau = -5.5: p = 5.5, t = 1/2
    assert got.tolist() == [2 * V222.mean()] * 3
    with pytest.raises(ValueError, match="go together"):
        shifted.field_energy(x, nm, fixed_mask=fm)


@pytest.mark.parametrize("kw", [
    dict(values=np.zeros((2, 2))), dict(values=np.zeros((1, 2, 2))), dict(values=np.full((2, 2, 2), np.nan)), dict(values="abc"),
    dict(values=np.full((2, 2, 2), 1e39)),
    dict(origin=[0, 0]), dict(origin=[0, 0, float("inf")]), dict(origin="x"),
    dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=[1, 1]), dict(spacing=[1, 0, 1]), dict(spacing=float("nan")),
    dict(k=-1.0), dict(k=float("inf")), dict(k="1"), dict(k=True), dict(wall=-0.5), dict(wall=float("nan")),
    dict(weights=[-1.0]), dict(weights=[float("nan")]), dict(weights=np.zeros((2, 2, 2))), dict(weights=[]), dict(weights="w")])
def test_field_rejects_malformed_arguments(kw):
    args = dict(values=V222, origin=[0, 0, 0], spacing=1.0)
    args.update(kw)
    with pytest.raises(ValueError):
        Field(**args)


def test_restraints_reject_bad_field_lists():
    f = Field(V222, [0, 0, 0], 1.0)
    with pytest.raises(ValueError, match="fields"):
        Restraints(fields=V222)
    with pytest.raises(ValueError, match="fields"):
        Restraints(fields=[f, V222])
    with pytest.raises(ValueError, match="at most 8"):
        Restraints(fields=[f] * 9)
    with pytest.raises(ValueError, match="must agree"):
        Restraints(fields=[Field(V222, [0, 0, 0], 1.0, weights=np.ones((2, 3))), Field(V222, [0, 0, 0], 1.0, weights=np.ones((3, 3)))])
    assert Restraints(fields=[f] * 8).n_fields == 8


def test_check_groups_compares_the_field_weights():
    st = steering.Steer(2, 1.0, 0.5, None)
    nm = torch.ones(4, 3, 1)
    w = torch.ones(4, 3)
    w[2:] = 2.0                                               # equal inside each group of 2
    steering.check_groups(st, nm, None, Restraints(fields=Field(V222, [0, 0, 0], 1.0, weights=w)))
    steering.check_groups(st, nm, None, Restraints(fields=Field(V222, [0, 0, 0], 1.0, weights=[1.0, 2.0])))
    w[1, 0] = 3.0
    with pytest.raises(ValueError, match="field weights"):
        steering.check_groups(st, nm, None, Restraints(fields=Field(V222, [0, 0, 0], 1.0, weights=w)))


def test_json_file_with_fields(tmp_path):
    (tmp_path / "sub").mkdir()
    np.save(tmp_path / "sub" / "pocket.npy", V222.astype(np.float32))
    p = tmp_path / "r.json"
    p.write_text(json.dumps({"obstacles": [[0, 0, 0, 1, 2]],
                             "fields": [{"file": "sub/pocket.npy", "origin": [1, 2, 3], "spacing": 0.5},
                                        {"file": "sub/pocket.npy", "origin": [0, 0, 0], "spacing": [1, 2, 3], "k": 2.0, "wall": 0.25,
                                         "weights": [1.0, 0.0]}]}))
    rs = Restraints.from_json(str(p))
    assert rs.sizes == (1, 0, 0) and rs.n_fields == 2
    assert rs.fields[0].origin.tolist() == [1.0, 2.0, 3.0] and (rs.fields[0].k, rs.fields[0].wall) == (1.0, 0.0)
    assert rs.fields[1].spacing.tolist() == [1.0, 2.0, 3.0] and (rs.fields[1].k, rs.fields[1].wall) == (2.0, 0.25)
    assert torch.equal(rs.fields[1].values, torch.from_numpy(V222.astype(np.float32)))
    p.write_text(json.dumps({"spheres": []}))
    with pytest.raises(ValueError, match="obstacles / pairs / anchors / fields"):
        Restraints.from_json(str(p))
    for bad in ({"fields": {}}, {"fields": [{"file": "sub/pocket.npy", "origin": [0, 0, 0]}]},
                {"fields": [{"file": "nope.npy", "origin": [0, 0, 0], "spacing": 1}]},
                {"fields": [{"file": "sub/pocket.npy", "origin": [0, 0, 0], "spacing": 1, "colour": 1}]},
                {"fields": [{"file": "sub/pocket.npy", "origin": [0, 0, 0], "spacing": -1}]}):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            Restraints.from_json(str(p))
    # a pickled array is not read
    import pickle
    (tmp_path / "evil.npy").write_bytes(pickle.dumps([1, 2, 3]))
    p.write_text(json.dumps({"fields": [{"file": "evil.npy", "origin": [0, 0, 0], "spacing": 1}]}))
    with pytest.raises(ValueError):
        Restraints.from_json(str(p))


# ----------------------------------------------------------------------------- C ABI

NEW_SYMBOLS = ["hd_restraint_fields", "hd_restraint_field_energy", "hd_restraint_field_energy_framed"]


def test_field_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} not declared in the header"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+HD_MAX_FIELDS\s+8\b", hdr) and restraints.MAX_FIELDS == 8
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays


def test_field_entry_points_reject_bad_arguments_without_a_gpu(lib):
    off, dims, geom = (C.c_longlong * 2)(0, 8), (C.c_int * 3)(2, 2, 2), (C.c_float * 8)(0, 0, 0, 1, 1, 1, 1, 0)
    assert lib.hd_restraint_fields(None, 1, None, off, dims, geom, None, 1, None) == -1
    assert b"hd_restraint_fields: null topology" in lib.hd_last_error()
    assert lib.hd_restraint_fields(None, 0, None, None, None, None, None, 1, None) == -1
    assert lib.hd_restraint_field_energy(None, None, None, None, None) == -1
    assert b"hd_restraint_field_energy: null" in lib.hd_last_error()
    assert lib.hd_restraint_field_energy_framed(None, None, None, None, None, None, None, None) == -1
    assert b"hd_restraint_field_energy_framed: null" in lib.hd_last_error()


# ----------------------------------------------------------------------------- the Python entry points and the CLI

def test_fielded_calls_keep_the_refusals_and_reach_the_device_check():
    from hierdiff_amd import EnVariationalDiffusion, default_config
    m = EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=20))
    nm = torch.ones(2, 3, 1, dtype=torch.bool)
    rs = Restraints(fields=Field(V222, [0, 0, 0], 1.0))
    z3, z8 = torch.zeros(2, 3, 3), torch.zeros(2, 3, 8)
    with pytest.raises(NotImplementedError, match="sample_inpaint: restraints"):
        m.sample_inpaint(nm, nm, z3, z8, restraints=rs)               # unframed inpainting
    with pytest.raises(NotImplementedError, match="encode: restraints"):
        m.encode(z3, z8, nm, restraints=rs)
    with pytest.raises(NotImplementedError, match="pocket"):
        m.sample_from_masks(nm, None, None, pocket=(None,) * 4, restraints=rs, restraint_scale=1.0)
    with pytest.raises(ValueError, match="field weights hold rows"):
        m.sample_from_masks(nm, None, None, restraints=Restraints(fields=Field(V222, [0, 0, 0], 1.0, weights=np.ones((3, 3)))),
                            restraint_scale=1.0)
    with pytest.raises(_lib.HierDiffHipError, match="MI355X"):
        m.sample_from_masks(nm, None, None, restraints=rs, restraint_scale=1.0)


def test_sampler_cli_takes_a_json_with_fields(tmp_path):
    from hierdiff_amd import sampler
    np.save(tmp_path / "pocket.npy", V222.astype(np.float32))
    p = tmp_path / "r.json"
    p.write_text(json.dumps({"fields": [{"file": "pocket.npy", "origin": [0, 0, 0], "spacing": 1.0, "wall": 1.0}]}))
    a = sampler.parse_args(["--restraints", str(p), "--restraint-scale", "0.5", "--particles", "4", "--steer-scale", "1.0", "--batch-size", "8"])
    assert a.restraints == str(p) and a.particles == 4
    assert Restraints.from_json(a.restraints).n_fields == 1       # what the sampler does with the argument
    a = sampler.parse_args(["--restraints", str(p), "--restraint-frame", "known", "--known", "k.pkl", "--grow", "2"])
    assert a.restraint_frame == "known"


# ----------------------------------------------------------------------------- the steered fixture of the GPU tier

@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_steered_reference_is_far_from_every_boundary(precision):
    """The steered chain with a field only (tests/field_reference.steered_reference): some transitions resample and some do not, and
    every resampling point and ESS threshold lies MARGIN_FACTOR times further from a boundary than the reference moves when its
    network runs in float64 instead of fp32 - the noise a device network within the chain bar can have."""
    from tests import steer_reference as st
    a = fr.steered_reference(precision)
    b = fr.steered_reference(precision, dtype=torch.float64)
    noise, same = st.cumulative_difference(a[1], b[1])
    margin = min(min(i["margin"], i["margin_ess"]) for i in a[1])
    res = [i["resampled"].tolist() for i in a[1]]
    print(f"steered field fixture [{precision}]: resampled {res}; smallest margin {margin:.3g}, fp32-vs-float64 noise {noise:.3g}")
    assert same and margin > st.MARGIN_FACTOR * noise
    assert any(any(r) for r in res) and not all(all(r) for r in res)
    assert all(np.isfinite(i["U"]).all() for i in a[1])
