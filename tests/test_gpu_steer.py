"""GPU tier (-m gpu) of steered sampling: hd_steer_step against the float64 restatement of tests/steer_reference.py, the steered path
loop against `SteeredNet` over the oracle with the generator's own noise, its reproducibility contract (graph replay, batch cuts at
group boundaries, chain cuts, zero-energy tables, no rebuild), the direction of the selection, result entries and the CLI.

Bars.  Ancestors and lineage roots: exact, on fixtures whose margins tests/test_steer_cpu.py asserts.  Energies: 1e-12 of the sum of
the absolute values of their terms (the bar of hd_restraint_energy), times beta for the log-weights.  Moved rows: bit for bit.  Chain
states: rel-L2 < 1e-4 (tests/helpers.py REL_L2_TOL).  Measured figures are printed."""
import ctypes as C
import json
import math
import pickle

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from hierdiff_amd.restraints import Restraints
from tests import restraint_reference as rr
from tests import steer_reference as st
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_restraint import Bare, batch_for, check_row_setter_and_the_captured_graph, dev, model_for, stream, tables
from tests.test_inpaint_cpu import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 8


def fresh(model, graph=True):
    model.use_graph = graph
    model.restraints, model.restraint_scale, model.restraint_schedule, model.restraint_clip = None, None, "score", None
    model.guidance_scale, model.guidance_context, model.guidance_rescale = None, None, 0.0
    model.particles, model.steer_scale, model.steer_ess = None, None, None
    model.eval()
    return model


def read_state(lib, topo, B, G):
    logw, uprev = (torch.empty(B, device=DEV, dtype=torch.float64) for _ in range(2))
    root, anc = (torch.empty(B, device=DEV, dtype=torch.int32) for _ in range(2))
    stats = torch.empty((G, 3), device=DEV, dtype=torch.float64)
    assert lib.hd_steer_read(topo, logw.data_ptr(), uprev.data_ptr(), root.data_ptr(), anc.data_ptr(), stats.data_ptr(), stream()) == 0, \
        lib.hd_last_error()
    return tuple(t.cpu().numpy() for t in (logw, uprev, root, anc, stats))


def bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the kernels, on a bare handle

@pytest.mark.parametrize("P,N,D", st.STEP_SHAPES)
def test_steer_step_against_the_reference(P, N, D):
    worst_u, worst_lw = 0.0, 0.0
    for c in st.step_cases():
        if c[:3] != (P, N, D):
            continue
        case = st.step_case(*c)
        ref = st.step_reference(case)
        nm, rs, B = case["nm"], case["rs"], case["nm"].shape[0]
        bare = Bare(D, nm)
        lib = bare.lib
        try:
            rs.attach(bare, torch.zeros(1), st.STEP_NV0, torch.device(DEV), stream())
            assert lib.hd_steer_attach(bare.topo, P, case["rho"], 1, stream()) == 0, lib.hd_last_error()
            for (z, eps, row3, draw), (zr, er_, info, state) in zip(case["stages"], ref):
                zd, ed = dev(z).contiguous(), dev(eps).contiguous()
                # the energy of the same positions through hd_restraint_energy (x^0 is exact in fp32 on these inputs)
                x0 = ((z[:, :, :3] - 0.5 * eps[:, :, :3]) * 2.0 * 2.0).contiguous()
                assert torch.equal(x0, rr.x0_f32(z, eps, row3[0], row3[1], st.STEP_NV0))
                e3 = torch.empty((B, 3), device=DEV, dtype=torch.float64)
                assert lib.hd_restraint_energy(bare.h, bare.topo, dev(x0).data_ptr(), e3.data_ptr(), stream()) == 0, lib.hd_last_error()
                e3 = e3.cpu().numpy()
                U_dev = (e3[:, 0] + e3[:, 1]) + e3[:, 2]
                rc = lib.hd_steer_step(bare.h, bare.topo, zd.data_ptr(), ed.data_ptr(), (C.c_float * 3)(*row3), draw, st.STEP_SEED,
                                       st.STEP_BASE, stream())
                assert rc == 0, lib.hd_last_error()
                logw, uprev, root, anc, stats = read_state(lib, bare.topo, B, 2)
                assert (anc == info["anc"]).all(), (c, anc, info["anc"])
                assert (root == state.root).all(), c
                # moved rows are their sources bit for bit, unmoved rows keep their bits
                src = torch.from_numpy(info["anc"])
                assert torch.equal(bits(zd.cpu()), bits(z[src])) and torch.equal(bits(ed.cpu()), bits(eps[src])), c
                # U_prev: the doubles of hd_restraint_energy, gathered; and within the energy bar of the reference
                assert (uprev == U_dev[info["anc"]]).all(), c
                fin = np.isfinite(state.uprev)
                assert (uprev[~fin] == state.uprev[~fin]).all()
                err_u = np.abs(uprev[fin] - state.uprev[fin])
                assert (err_u <= 1e-12 * state.umag[fin]).all(), c
                lfin = np.isfinite(state.logw)
                assert (logw[~lfin] == state.logw[~lfin]).all(), c
                err_l = np.abs(logw[lfin] - state.logw[lfin])
                assert (err_l <= 1e-12 * state.lwmag[lfin]).all(), (c, err_l.max())
                if fin.any() and state.umag[fin].max() > 0:
                    worst_u = max(worst_u, float((err_u / np.maximum(1e-12 * state.umag[fin], 1e-300)).max()))
                nz = lfin & (state.lwmag > 0)
                if nz.any():
                    worst_lw = max(worst_lw, float((np.abs(logw[nz] - state.logw[nz]) / (1e-12 * state.lwmag[nz])).max()))
                assert (stats[:, 0] == state.stats[:, 0]).all() and (stats[:, 2] == state.stats[:, 2]).all(), c
                assert np.allclose(stats[:, 1], state.stats[:, 1], rtol=1e-9, atol=0), c
        finally:
            bare.close()
    print(f"hd_steer_step P={P} N={N} D={D}: worst U_prev err / (1e-12 sum|terms|) {worst_u:.3g}, worst logw err / (1e-12 beta "
          f"sum|terms|) {worst_lw:.3g}")


def test_steer_abi_argument_errors():
    nm = torch.ones(6, 5, dtype=torch.bool)
    bare = Bare(4, nm)
    lib = bare.lib
    try:
        z, eps = torch.zeros(6, 5, 4, device=DEV), torch.zeros(6, 5, 4, device=DEV)
        r3 = (C.c_float * 3)(0.5, 0.5, 1.0)
        step = lambda zz, ee, row=r3: lib.hd_steer_step(bare.h, bare.topo, zz.data_ptr(), ee.data_ptr(), row, 1, 1, 0, stream())
        assert step(z, eps) == -4 and b"hd_steer_attach" in lib.hd_last_error()
        for P, ess in ((1, 0.5), (257, 0.5), (4, 0.5), (3, 0.0), (3, 1.5), (3, float("nan"))):
            assert lib.hd_steer_attach(bare.topo, P, ess, 1, stream()) == -1, (P, ess)
        assert lib.hd_steer_read(bare.topo, None, None, None, None, None, stream()) == -4
        assert lib.hd_steer_attach(bare.topo, 3, 0.5, 0, stream()) == -4 and b"reset = 0" in lib.hd_last_error()
        assert lib.hd_steer_attach(bare.topo, 3, 0.5, 1, stream()) == 0, lib.hd_last_error()
        assert step(z, eps) == -4 and b"hd_restraint_attach" in lib.hd_last_error()
        Restraints(obstacles=[[0, 0, 0, 1, 1]]).attach(bare, torch.zeros(1), 1.0, torch.device(DEV), stream())
        assert step(z, z) == -1 and b"overlap" in lib.hd_last_error()
        for row in ((0.0, 0.5, 1.0), (0.5, -0.1, 1.0), (0.5, 0.5, -1.0), (0.5, 0.5, float("inf"))):
            assert step(z, eps, (C.c_float * 3)(*row)) == -1
        assert step(z, eps) == 0, lib.hd_last_error()
        assert lib.hd_steer_attach(bare.topo, 2, 0.5, 0, stream()) == -4                 # another P continues nothing
        assert lib.hd_steer_attach(bare.topo, 3, 1.0, 0, stream()) == 0
        assert lib.hd_steer_detach(bare.topo) == 0 and step(z, eps) == -4
    finally:
        bare.close()


# ----------------------------------------------------------------------------- chains against SteeredNet

def chain_kw(eta, restrained, base=st.CHAIN_BASE):
    N = max(st.CHAIN_MOLS)
    kw = dict(eta=eta, restraints=st.chain_tables(N), particles=st.CHAIN_P, steer_scale=st.CHAIN_BETA, steer_ess=st.CHAIN_RHO,
              sample_id_base=base)
    if restrained:
        kw.update(st.CHAIN_RKW)
    return kw


@pytest.mark.parametrize("precision,eta,restrained", st.CHAIN_CASES)
def test_steered_chain_against_the_reference(precision, eta, restrained):
    """Per state rel-L2 < 1e-4 against `SteeredNet` over the oracle; ancestors and roots of every transition exactly."""
    lib = _lib.load()
    model, _, _ = model_for(precision)
    fresh(model)
    states, infos, state, zT, (nm, em) = st.chain_reference(precision, eta, restrained)
    B, N = nm.shape[:2]
    G = B // st.CHAIN_P
    kw = chain_kw(eta, restrained)
    nmd, emd = dev(nm), dev(em)
    topo = model.dynamics.topology(nmd, emd, B, N)
    zz, worst = dev(zT), 0.0
    ref_state = st.State(B, st.CHAIN_P)
    assert any(i["resampled"].any() for i in infos) and not all(i["resampled"].all() for i in infos)
    for k in range(T):
        zz = model.path_steps(zz, nmd, emd, k_lo=k, k_hi=k + 1, **kw)
        logw, uprev, root, anc, stats = read_state(lib, topo.ptr, B, G)
        r = rel_l2(zz.cpu().numpy(), states[k].numpy())
        worst = max(worst, r)
        print(f"steered chain {precision} eta={eta} restrained={restrained} state {k + 1}/{T}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e}), "
              f"resampled {infos[k]['resampled'].tolist()}")
        assert (anc == infos[k]["anc"]).all(), (k, anc, infos[k]["anc"])
        ref_state.root = ref_state.root[infos[k]["anc"]]
        assert (root == ref_state.root).all(), k
        assert r < REL_L2_TOL, (k, r)
    assert (root == state.root).all() and (stats[:, 0] == state.stats[:, 0]).all()
    assert np.allclose(model.steer_last.min_ess.numpy(), state.stats[:, 1], rtol=1e-3)
    print(f"steered chain {precision} eta={eta} restrained={restrained}: worst state {worst:.2e}; events {state.stats[:, 0].tolist()}")


# ----------------------------------------------------------------------------- bit equalities

def steer_batch(groups):
    mols = tuple(n for n in groups for _ in range(st.CHAIN_P))
    return batch_for(mols)


SKW = dict(steps=6, eta=1.0, particles=st.CHAIN_P, steer_scale=st.CHAIN_BETA, **st.CHAIN_RKW)


def test_steer_rows_of_the_same_K_keep_the_captured_graph_and_another_K_builds_one():
    check_row_setter_and_the_captured_graph(steer=True)


def test_graph_replay_equals_launches_and_a_second_call_builds_no_graph():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    x, h, nm, em, _ = steer_batch((7, 4))
    nmd, N, B = dev(nm), nm.shape[1], nm.shape[0]
    kw = dict(sample_id_base=3, restraints=tables(N), **SKW)
    fresh(model, graph=False)
    want = model.sample_from_masks(nmd, None, None, **kw)
    want_state = model.steer_last
    plain = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=6, eta=1.0, restraints=tables(N), **st.CHAIN_RKW)
    assert int(want_state.events.sum()) >= 1 and not torch.equal(want[0], plain[0])
    fresh(model, graph=True)
    topo = model.dynamics.topology(nmd, None, B, N)
    n0 = lib.hd_path_graph_builds(topo.ptr)
    got = model.sample_from_masks(nmd, None, None, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(model.steer_last.root, want_state.root) and torch.equal(model.steer_last.logw, want_state.logw)
    assert torch.equal(model.steer_last.events, want_state.events)
    n1 = lib.hd_path_graph_builds(topo.ptr)
    assert n1 == n0 + 1
    again = model.sample_from_masks(nmd, None, None, **dict(kw, restraints=tables(N, shift=0.25)))       # same P, same sizes: a copy
    assert lib.hd_path_graph_builds(topo.ptr) == n1 and not torch.equal(again[0], want[0])
    got = model.sample_from_masks(nmd, None, None, **kw)
    assert torch.equal(got[0], want[0]) and lib.hd_path_graph_builds(topo.ptr) == n1
    got = model.sample_from_masks(nmd, None, None, sample_id_base=3, steps=6, eta=1.0, restraints=tables(N), **st.CHAIN_RKW)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])                               # unsteered afterwards


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_a_group_depends_on_its_ids_and_its_own_rows_only(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    x, h, nm, em, _ = steer_batch((7, 4, 6, 1))
    B, N = nm.shape[:2]
    P = st.CHAIN_P
    g = torch.Generator().manual_seed(1)
    obs = torch.cat([torch.randn(4, 3, 3, generator=g), torch.full((4, 3, 1), 1.5), torch.full((4, 3, 1), 2.0)], dim=2)
    rs = Restraints(obstacles=obs.repeat_interleave(P, dim=0), pairs=[[0, 1, 2.0, 2.5, 1.0]])
    whole = model.sample_from_masks(dev(nm), None, None, sample_id_base=40, restraints=rs, **SKW)
    ws = model.steer_last
    assert int(ws.events.sum()) >= 1
    for lo in (0, 2 * P):
        half = model.sample_from_masks(dev(nm[lo:lo + 2 * P]), None, None, sample_id_base=40 + lo, restraints=rs.slice(lo, lo + 2 * P), **SKW)
        assert torch.equal(half[0], whole[0][lo:lo + 2 * P]) and torch.equal(half[1], whole[1][lo:lo + 2 * P]), lo
        assert torch.equal(model.steer_last.root, ws.root[lo:lo + 2 * P]) and torch.equal(model.steer_last.logw, ws.logw[lo:lo + 2 * P])
        assert torch.equal(model.steer_last.events, ws.events[lo // P:lo // P + 2])


def test_a_cut_chain_equals_the_whole_and_duplicates_diverge():
    lib = _lib.load()
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, _ = steer_batch((7, 4))
    B, N = nm.shape[:2]
    raw = st.normals_host(SEED, 4, 0, B, N, 8)
    from oracle import egnn_oracle as orc
    z = dev(orc.combined_noise(raw[0], raw[1], nm.float()))
    kw = dict(restraints=tables(N), sample_id_base=4, **SKW)
    whole = model.path_steps(z, dev(nm), **kw)
    ws = model.steer_last
    cut = model.path_steps(model.path_steps(model.path_steps(z, dev(nm), k_hi=2, **kw), dev(nm), k_lo=2, k_hi=3, **kw), dev(nm), k_lo=3, **kw)
    assert torch.equal(cut, whole)
    assert torch.equal(model.steer_last.root, ws.root) and torch.equal(model.steer_last.events, ws.events)
    assert torch.equal(model.steer_last.logw, ws.logw) and int(ws.events.sum()) >= 1
    # a resampling transition: rows that received another row's state differ from their source behind the step
    topo = model.dynamics.topology(dev(nm), None, B, N)
    zz, seen = z, 0
    for k in range(6):
        zz = model.path_steps(zz, dev(nm), k_lo=k, k_hi=k + 1, **kw)
        anc = read_state(lib, topo.ptr, B, B // st.CHAIN_P)[3]
        for b in np.nonzero(anc != np.arange(B))[0]:
            seen += 1
            assert not torch.equal(zz[b], zz[int(anc[b])])
    assert seen >= 1 and torch.equal(zz, whole)
    # a piece that continues nothing is refused, not run on stale state
    other = dev(steer_batch((6, 5))[2])
    with pytest.raises(_lib.HierDiffHipError, match="reset = 0"):
        model.path_steps(z[:, :6].contiguous(), other, k_lo=2, **dict(kw, restraints=tables(6)))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_zero_energy_tables_equal_the_unsteered_restrained_call(graph):
    model, _, _ = model_for("fp32")
    fresh(model, graph)
    x, h, nm, em, _ = steer_batch((7, 4))
    sat = Restraints(obstacles=[[1e4, 0, 0, 1.0, 5.0]], pairs=[[0, 1, 0.0, 1e9, 5.0]], anchors=[[0, 0, 0, 0, 1e9, 5.0]])
    kw = dict(sample_id_base=9, steps=6, eta=1.0, restraints=sat, **st.CHAIN_RKW)
    plain = model.sample_from_masks(dev(nm), None, None, **kw)
    got = model.sample_from_masks(dev(nm), None, None, particles=st.CHAIN_P, steer_scale=1.0, **kw)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    s = model.steer_last
    assert int(s.events.sum()) == 0 and torch.equal(s.root, torch.arange(8) % st.CHAIN_P) and (s.min_ess == st.CHAIN_P).all()
    assert torch.allclose(s.logw, torch.full((8,), -math.log(st.CHAIN_P), dtype=torch.float64))
    for off in (dict(particles=1, steer_scale=1.0), dict(particles=st.CHAIN_P, steer_scale=0), dict(particles=None, steer_scale=1.0)):
        got = model.sample_from_masks(dev(nm), None, None, **off, **kw)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


# ----------------------------------------------------------------------------- direction

def test_steering_lowers_the_mean_restraint_energy():
    """G = 8 groups of P = 8 on the seven-node case with an obstacle through the molecule's centre, T = 8: the mean final restraint
    energy with steering is below the mean of the same seeds without.  An ordering only (synthetic weights: says nothing chemical).
    Measured on an MI355X: see EXPERIMENTS.md."""
    model, _, _ = model_for("fp32")
    fresh(model)
    rs0, _, _ = rr.seven_node_case()
    obs = torch.cat([rs0.obs[0].double(), torch.tensor([[0.0, 0.0, 0.0, 2.0, 3.0]], dtype=torch.float64)])
    rs = Restraints(obstacles=obs, pairs=torch.cat([rs0.pair_idx[0].double(), rs0.pair_f[0].double()], dim=1),
                    anchors=torch.cat([rs0.anc_idx[0].double().unsqueeze(1), rs0.anc_f[0].double()], dim=1))
    x, h, nm, em, _ = batch_for((7,) * 64)
    nmd = dev(nm)
    kw = dict(sample_id_base=500, restraints=rs)
    on = model.sample_from_masks(nmd, None, None, particles=8, steer_scale=st.CHAIN_BETA, **kw)
    events = int(model.steer_last.events.sum())
    off = model.sample_from_masks(nmd, None, None, restraint_scale=0.0, **kw)
    plain = model.sample_from_masks(nmd, None, None, sample_id_base=500)
    assert torch.equal(off[0], plain[0])
    e_on = rs.energy(on[0], nmd, model=model).sum(1).cpu()
    e_off = rs.energy(off[0], nmd, model=model).sum(1).cpu()
    print(f"direction: mean final restraint energy steered {float(e_on.mean()):.6g}, unsteered {float(e_off.mean()):.6g} "
          f"({events} resampling events in 8 groups)")
    assert events >= 1 and torch.isfinite(e_on).all() and torch.isfinite(e_off).all()
    assert float(e_on.mean()) < float(e_off.mean())


# ----------------------------------------------------------------------------- results and the CLI

def test_result_entries_and_statistics():
    model, _, _ = model_for("fp32")
    fresh(model)
    rs = Restraints(obstacles=[[0.0, 0.0, 0.0, 2.0, 1.0]], pairs=[[0, 1, 3.0, 4.0, 1.0]])
    torch.manual_seed(3)
    out = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, particles=4, steer_scale=st.CHAIN_BETA)
    assert len(out) == 8
    for i, r in enumerate(out):
        assert r["steer_logw"].dtype == torch.float64 and int(r["steer_group"]) == i // 4 and 0 <= int(r["steer_root"]) < 4
        assert r["restraint_energy"].shape == (3,)
        assert r["x"].shape[0] == out[4 * (i // 4)]["x"].shape[0]                  # one size per group
    for g in range(2):
        lw = torch.stack([r["steer_logw"] for r in out[4 * g:4 * g + 4]])
        assert abs(float(torch.logsumexp(lw, 0))) < 1e-12
    s = model.steer_last
    assert s.events.shape == (2,) and s.min_ess.shape == (2,) and (s.min_ess > 0).all() and (s.min_ess <= 4).all()
    torch.manual_seed(3)
    plain = model.sample(8, DEV, sample_id_base=40, steps=8, restraints=rs, restraint_scale=0.0)
    assert all("steer_logw" not in r for r in plain)
    var = model.vary(plain[:2], DEV, 4, n_variants=4, steps=2, restraints=rs, particles=2, steer_scale=st.CHAIN_BETA)
    assert len(var) == 8 and [int(r["steer_group"]) for r in var] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert all(r["x"].shape == plain[i // 4]["x"].shape and "restraint_energy" in r for i, r in enumerate(var))
    two = model.vary(plain[:2], DEV, 4, n_variants=4, batch_size=4, steps=2, restraints=rs, particles=2, steer_scale=st.CHAIN_BETA)
    for a, b in zip(var, two):
        assert torch.equal(a["x"], b["x"]) and torch.equal(a["steer_logw"], b["steer_logw"]) and int(a["steer_group"]) == int(b["steer_group"])


def test_cli_round_trip(tmp_path):
    from hierdiff_amd import sampler
    rj, out = str(tmp_path / "r.json"), str(tmp_path / "o.pkl")
    with open(rj, "w") as f:
        json.dump({"obstacles": [[0.0, 0.0, 0.0, 2.0, 1.0]]}, f)
    argv = ["--hidden-nf", "32", "--n-layers", "1", "--timesteps", "8", "--batch-size", "4", "--num-batches", "1", "--out", out,
            "--restraints", rj, "--particles", "2", "--steer-scale", "1e-4"]
    assert sampler.main(argv) == 0
    with open(out, "rb") as f:
        res, _ = pickle.load(f)
    assert len(res) == 4 and [int(r["steer_group"]) for r in res] == [0, 0, 1, 1]
    assert all("steer_logw" in r and "steer_root" in r and "restraint_energy" in r for r in res)
