"""GPU tier (-m gpu) of stochastic second-order multistep sampling (solver="sde2m"; hd_set_path_multistep_sde,
hd_multistep_sde_step): the kernel against float64, its bit identity with the ancestral linear rows where c2 = 0, chains against
the float64 restatement (tests/sde_solver_reference.py) with injected normals - plain, with context, guided, restrained, recorded -
the loop's reproducibility (graph replay, split ranges, shards), the steered chain, whose history must follow the lineage, and the
refusals of the C ABI.

Bars.  The kernel: every element within 8 * 2^-23 of the sum of the absolute values of its terms (tests/sampling_reference.py);
masked entries exactly 0.  Chains: rel-L2 < 1e-4 per state (tests/helpers.py REL_L2_TOL).  Ancestors and roots of the steered chain:
exact, on a fixture whose margins the test asserts on the reference side first.  Measured figures are printed.
Shapes: B = 3 molecules of 1, 7 and 30 nodes (N = 30, F = 8: 330 elements, the strided loops wrap), F = 1, B = 1, a pocket case
with mol < N; networks H = 32 (2 layers) and 64 (1 layer), T = 20 with K = 7, and one T = 1000, K = 20 chain at B = 4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests import restraint_reference as rr
from tests import sde_solver_reference as sd
from tests import steer_reference as st
from tests.helpers import REL_L2_TOL, rel_l2
from tests.test_gpu_parity import PRECISIONS, build_diffusion
from tests.test_gpu_restraint import RKW, Bare, stream, tables
from tests.test_gpu_steer import read_state
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, K = 20, 7
SIZES = (1, 7, 30)
SHAPES = {"fp32": (32, 2), "fp16x3": (64, 1)}
KSEED, KBASE, KDRAW = 99, 10, 5
BOUND = 8.0
SKW = dict(solver="sde2m", steps=K)


def dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def model_for(precision, C_=0, T_=T, HL=None):
    H, L = HL or SHAPES[precision]
    sd_np, cfg = er.weights(H, L, C_=C_)
    model = build_diffusion(sd_np, H, L, C_=C_, T=T_, precision=precision)
    model.seed = SEED
    return model, sd_np, cfg


@functools.lru_cache(maxsize=None)
def batch_for(mols, C_=0):
    return er.molecules(list(mols), C_=C_)


def fresh(model, graph=True):
    model.use_graph = graph
    model.restraints, model.restraint_scale, model.restraint_schedule, model.restraint_clip = None, None, "score", None
    model.guidance_scale, model.guidance_context, model.guidance_rescale = None, None, 0.0
    model.particles, model.steer_scale, model.steer_ess = None, None, None
    model.sample_solver, model.sample_steps = None, None
    model.eval()
    return model


def f32(row):
    return [float(np.float32(v)) for v in row]


def bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the kernel against float64

def kernel_case(name):
    """(nm [B,N] bool, F, mol): masks are zero-padded prefixes; `mol` < N is the pocket form (rows >= mol are left alone)."""
    sizes, N, F, mol = {"wrap": (SIZES, 30, 8, None), "F1": ((9, 4, 1), 9, 1, None), "B1": ((6,), 8, 8, None),
                        "pocket": ((8, 5), 12, 8, 8)}[name]
    nm = torch.zeros(len(sizes), N, dtype=torch.bool)
    for b, n in enumerate(sizes):
        nm[b, :n] = True
    if mol is not None:
        nm[:, mol:] = True                                    # the pocket's rows are valid nodes of the topology
    return nm, F, mol


def kernel_inputs(nm, F, seed):
    """zt with a centre-of-mass offset (the final re-centring counts), eps not mean-free, a history; all zero at masked nodes."""
    g = torch.Generator().manual_seed(seed)
    B, N = nm.shape
    m = nm.float().unsqueeze(-1)
    zt = torch.randn(B, N, 3 + F, generator=g) * m
    zt[:, :, :3] += torch.tensor([3.0, -2.0, 1.0]) * m
    eps = torch.randn(B, N, 3 + F, generator=g) * m
    xp = torch.randn(B, N, 3 + F, generator=g) * m
    return zt, eps, xp


def sde_step(bare, row, zt, eps, xp, raw, noise_rows, mol, share=0, alias=False, sentinel=7.0):
    """hd_multistep_sde_step -> (x^_k, z_s) on the host; outputs pre-filled with `sentinel`."""
    ztd, epd = dev(zt).clone(), dev(eps)
    xpd = None if xp is None else dev(xp).clone()
    x_out = xpd if (alias and xpd is not None) else torch.full_like(ztd, sentinel)
    zs = ztd if alias else torch.full_like(ztd, sentinel)
    rx, rh = (None, None) if raw is None else (dev(raw[0]).contiguous(), dev(raw[1]).contiguous())
    rc = bare.lib.hd_multistep_sde_step(bare.h, bare.topo, ztd.data_ptr(), epd.data_ptr(), (C.c_float * 6)(*row),
                                        None if xpd is None else xpd.data_ptr(), x_out.data_ptr(),
                                        None if rx is None else rx.data_ptr(), None if rh is None else rh.data_ptr(), noise_rows,
                                        KSEED, KBASE, KDRAW, share, -1 if mol is None else mol, zs.data_ptr(), stream())
    assert rc == 0, bare.lib.hd_last_error()
    torch.cuda.synchronize()
    return x_out.cpu(), zs.cpu()


@pytest.mark.parametrize("name", ["wrap", "F1", "B1", "pocket"])
def test_kernel_against_float64(name):
    """Rows with c2 = 0 and c2 != 0; injected normals per molecule and one shared row; the generator against its host twin, per
    molecule and shared; zt with a centre-of-mass offset; aliased outputs.  Measured on an MI355X: see EXPERIMENTS.md."""
    nm, F, mol = kernel_case(name)
    B, N = nm.shape
    n = N if mol is None else mol
    rows = sd.sde_rows(sd.analytic_grid(T), sd.uniform_path(T, K), lower_order_final=False)
    zt, eps, xp = kernel_inputs(nm, F, 1)
    g = torch.Generator().manual_seed(2)
    raw_b = (torch.randn(B, n, 3, generator=g), torch.randn(B, n, F, generator=g))
    host = st.normals_host(KSEED, KBASE, KDRAW, B, N, F)
    host = (host[0][:, :n].contiguous(), host[1][:, :n].contiguous())
    sources = [("injected", raw_b, B, raw_b, 0), ("shared row", (raw_b[0][:1], raw_b[1][:1]), 1, (raw_b[0][:1], raw_b[1][:1]), 0),
               ("generator", None, B, host, 0), ("generator, shared", None, B, (host[0][:1], host[1][:1]), 1)]
    bare = Bare(3 + F, nm)
    worst = 0.0
    try:
        for k in (0, 3, K - 1):
            row = f32(rows[k])
            assert (row[3] == 0.0) == (k == 0) and row[2] != 0.0
            hist = None if k == 0 else xp
            for what, raw, noise_rows, ref_raw, share in sources:
                xk, zs = sde_step(bare, row, zt, eps, hist, raw, noise_rows, mol, share)
                xo, zo, Ax, Az = sd.step_ref(row, zt, eps, hist, nm, ref_raw, mol=n, magnitudes=True)
                for tag, got, ref, A in (("x^", xk, xo, Ax), ("z_s", zs, zo, Az)):
                    r, nonzero = sd.ratio(got[:, :n].numpy(), ref.numpy(), A.numpy(), nm[:, :n].numpy())
                    worst = max(worst, r)
                    print(f"hd_multistep_sde_step [{name}] row {k} {what} {tag}: worst |err| / (2^-23 A) = {r:.3g} (bound {BOUND:g})")
                    assert torch.isfinite(got).all() and nonzero == 0, (name, k, what, tag)
                    assert r <= BOUND, (name, k, what, tag, r)
                    assert torch.all(got[:, n:] == 7.0), "rows >= mol_shape are left alone"
                single = np.flatnonzero(nm[:, :n].sum(1).numpy() == 1)
                assert torch.all(zs[single][:, :n, :3] == 0), "the x row of a one-node molecule is exactly 0"
                if mol is None:
                    xa, za = sde_step(bare, row, zt, eps, hist, raw, noise_rows, mol, share, alias=True)
                    assert torch.equal(bits(za), bits(zs)), "zs == zt gives other bits"
                    if hist is not None:
                        assert torch.equal(bits(xa), bits(xk)), "x_out == x_prev gives other bits"
    finally:
        bare.close()
    print(f"hd_multistep_sde_step [{name}]: worst multiple of 2^-23 A over all rows and noise sources {worst:.3g} (bound {BOUND:g})")


# ----------------------------------------------------------------------------- c2 = 0 rows give the bits of form 1

def set_path(lib, hnd, fn, pt, coef, *extra):
    ti, si, cf = (np.ascontiguousarray(v.numpy()) for v in (pt["t_idx"], pt["s_idx"], coef))
    rc = fn(hnd, pt["K"], ti.ctypes.data_as(C.POINTER(C.c_int)), si.ctypes.data_as(C.POINTER(C.c_int)),
            cf.ctypes.data_as(C.POINTER(C.c_float)), *extra)
    assert rc == 0, lib.hd_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_rows_without_correction_give_the_bits_of_the_ancestral_linear_rows(graph, precision):
    lib = _lib.load()
    model, _, _ = model_for(precision)
    fresh(model, graph)
    _, _, nm, em, _ = batch_for(SIZES)
    nmd = dev(nm)
    B, N = nm.shape[:2]
    raw = st.normals_host(SEED, 0, 0, B, N, 8)
    zT = dev(orc.combined_noise(raw[0], raw[1], nm.float()))
    hnd, tabs = model._lib_handle(), model._schedule(rows=B)
    pt = paths.path_tables(tabs["gamma"], paths.uniform_path(T, K), solver="sde2m")
    assert bool((pt["coef"][1:-1, 3] != 0).all()) and bool((pt["coef"][:, 2] != 0).all())
    topo = model.dynamics.topology(nmd, None, B, N)
    run = lambda z: lib.hd_sample_path(hnd, topo.ptr, z.data_ptr(), None, -1, 0, K, None, None, B, model.seed, 3, int(graph), None)
    model._path_cache = None                          # the handle's path is set behind the model's back
    lin = torch.cat([pt["coef"][:, :3], torch.zeros(K, 1)], dim=1).contiguous()
    set_path(lib, hnd, lib.hd_set_path, pt, lin, 1, None)
    want = zT.clone()
    assert run(want) == 0, lib.hd_last_error()
    flat = pt["coef"].clone()
    flat[:, 3] = 0.0
    set_path(lib, hnd, lib.hd_set_path_multistep_sde, pt, flat)
    got = zT.clone()
    assert run(got) == 0, lib.hd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    model._path_cache = None
    # the real rows differ from first order (eta = 1 through the keywords runs the ancestral row FORMAT, form 0: other bits)
    assert not torch.equal(model.path_steps(zT, nmd, sample_id_base=3, **SKW), want)


# ----------------------------------------------------------------------------- chains against float64 on the oracle

def run_states(model, z, nm, em, ctx, raws, **kw):
    """The state behind every transition, one call each (the history is the topology's), and the same range in one call."""
    zz, out = dev(z), []
    for k in range(len(raws)):
        zz = model.latent_steps(zz, dev(nm), dev(em), dev(ctx), k_lo=k, k_hi=k + 1, raw_noises=[raws[k]], **kw)
        out.append(zz)
    whole = model.latent_steps(dev(z), dev(nm), dev(em), dev(ctx), raw_noises=raws, **kw)
    assert torch.equal(whole, out[-1]), "a chain cut into single transitions gives other bits than the whole"
    return out


def check_states(what, got, ref):
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        e = rel_l2(g.cpu().numpy(), r.numpy())
        worst = max(worst, e)
        assert torch.isfinite(g).all()
        assert e < REL_L2_TOL, (what, k, e)
    print(f"sde2m chain {what}: worst state rel_l2 {worst:.2e} over {len(ref)} transitions (bar {REL_L2_TOL:.0e})")
    return worst


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["plain", "context", "guided"])
def test_chain_against_float64_T20_K7(kind, precision):
    C_ = 0 if kind == "plain" else 1
    model, sd_np, cfg = model_for(precision, C_)
    fresh(model)
    _, _, nm, em, ctx = batch_for(SIZES, C_)
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 1, B, N, seed=K)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    net = er.RefNet(sd_np, cfg, T, nm, em, ctx)
    kw = dict(SKW)
    if kind == "guided":
        net = gr.GuidedNet(net, er.RefNet(sd_np, cfg, T, nm, em, gr.null_ctx(nm)), 2.0, 0.0)
        kw["guidance_scale"] = 2.0
    for lof in (True, False):
        ref = sd.chain_ref(net.net, gg, path, z, nm.float(), raws[1:], lof)
        got = run_states(model, z, nm, em, ctx, raws[1:], lower_order_final=lof, **kw)
        check_states(f"{kind} lower_order_final={lof} [{precision}]", got, [r[0] for r in ref])
    first = sd.chain_ref(net.net, gg, path, z, nm.float(), raws[1:], rows=sd.ancestral_rows(gg, path))
    assert rel_l2(first[-1][0].numpy(), ref[-1][0].numpy()) > 10 * REL_L2_TOL       # not a no-op: first order lies outside the bar


def test_chain_against_float64_T1000_K20():
    T_, K_ = 1000, 20
    model, sd_np, cfg = model_for("fp32", 0, T_, (64, 1))
    fresh(model)
    _, _, nm, em, _ = batch_for((8, 5, 7, 3))
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T_)
    for spacing in ("uniform", "quadratic"):
        path = paths.build_path(T_, K_, spacing)
        raws = er.raw_draws(K_ + 1, B, N, seed=K_)
        z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
        ref = sd.chain_ref(er.RefNet(sd_np, cfg, T_, nm, em, None).net, gg, path, z, nm.float(), raws[1:])
        got = run_states(model, z, nm, em, None, raws[1:], solver="sde2m", steps=K_, spacing=spacing)
        check_states(f"T=1000 K=20 {spacing}", got, [r[0] for r in ref])


def test_restrained_chain_against_float64():
    model, sd_np, cfg = model_for("fp32")
    fresh(model)
    _, _, nm, em, _ = batch_for(SIZES)
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 1, B, N, seed=K + 1)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    rs, scale = tables(N), torch.tensor([0.05, 0.02, 0.05])
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    rnet = rr.RestrainedNet(net, rs, scale, rr.rows_from_grid(gg, path, "score", 0.3))
    ref = sd.chain_ref(rnet.net, gg, path, z, nm.float(), raws[1:])
    plain = sd.chain_ref(net.net, gg, path, z, nm.float(), raws[1:])
    got = run_states(model, z, nm, em, None, raws[1:], restraints=rs, restraint_scale=scale, restraint_clip=0.3, **SKW)
    check_states("restrained", got, [r[0] for r in ref])
    assert rel_l2(ref[-1][0].numpy(), plain[-1][0].numpy()) > 10 * REL_L2_TOL       # the restraints move the chain


# ----------------------------------------------------------------------------- recording

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_recorded_frames_against_the_reference(graph):
    model, sd_np, cfg = model_for("fp32")
    fresh(model, graph)
    _, _, nm, em, _ = batch_for(SIZES)
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    raws = er.raw_draws(K + 2, B, N, seed=K + 2)
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    ref = sd.chain_ref(er.RefNet(sd_np, cfg, T, nm, em, None).net, gg, path, z, nm.float(), raws[1:K + 1], False)
    kw = dict(raw_noises=raws, lower_order_final=False, **SKW)
    x, h = model.sample_from_masks(dev(nm), dev(em), None, **kw)
    cf = paths.chain_frames(K, K, path)
    for record, col in (("z", 0), ("x0", 1)):
        xr, hr, chain = model.sample_from_masks(dev(nm), dev(em), None, keep_frames=K, record=record, **kw)
        assert torch.equal(xr, x) and torch.equal(hr, h), "recording changes the sample"
        assert torch.equal(chain[0], torch.cat([x, h], dim=2))
        worst = 0.0
        for k, f in enumerate(cf.frame_of):
            if f == 0:
                continue                                  # overwritten by the decode
            v = ref[k][col].float()
            want = torch.cat(model.unnormalize(v[:, :, :3], v[:, :, 3:], nm.float()), dim=2)
            e = rel_l2(chain[f].cpu().numpy(), want.numpy())
            worst = max(worst, e)
            assert e < REL_L2_TOL, (record, k, e)
            assert torch.all(chain[f].cpu()[~nm.expand_as(v)] == 0)
        print(f"sde2m record={record!r} graph={graph}: worst frame rel_l2 {worst:.2e} (bar {REL_L2_TOL:.0e})")


# ----------------------------------------------------------------------------- graph replay, split ranges, shards

@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replay_equals_plain_launches_and_the_graph_is_cached(precision):
    lib = _lib.load()
    model, _, _ = model_for(precision)
    _, _, nm, _, _ = batch_for(SIZES)
    nmd = dev(nm)
    B, N = nm.shape[:2]
    builds = lambda: int(lib.hd_path_graph_builds(model.dynamics.topology(nmd, None, B, N).ptr))
    res = {}
    for graph in (False, True):
        fresh(model, graph)
        res[graph] = model.sample_from_masks(nmd, None, None, sample_id_base=40, **SKW)
        res[graph, "fix"] = model.sample_from_masks(nmd, None, None, sample_id_base=40, fix_noise=True, **SKW)
    for key in (True, (True, "fix")):
        other = False if key is True else (False, "fix")
        assert torch.equal(res[key][0], res[other][0]) and torch.equal(res[key][1], res[other][1]), key
        assert torch.isfinite(res[key][0]).all() and torch.isfinite(res[key][1]).all()
    assert not torch.equal(res[True][0], res[True, "fix"][0])
    a = model.sample_from_masks(nmd, None, None, sample_id_base=40, **SKW)
    n0 = builds()
    assert n0 >= 1 and torch.equal(a[0], res[True][0]) and torch.equal(a[1], res[True][1])
    b = model.sample_from_masks(nmd, None, None, sample_id_base=77, **SKW)
    assert builds() == n0, "another sample_id_base must replay the cached graph"
    assert not torch.equal(a[0], b[0])
    c = model.sample_from_masks(nmd, None, None, sample_id_base=40, solver="sde2m", steps=5)
    assert builds() == n0 + 1, "a new path rebuilds once"
    c2 = model.sample_from_masks(nmd, None, None, sample_id_base=40, solver="sde2m", steps=5)
    assert builds() == n0 + 1 and torch.equal(c[0], c2[0])
    e = model.sample_from_masks(nmd, None, None, sample_id_base=40, steps=K, eta=1.0)          # the ancestral chain, its own bits
    assert not torch.equal(e[0], a[0])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
def test_split_ranges_give_the_bits_of_the_whole_and_need_their_history(graph, precision):
    model, _, _ = model_for(precision)
    fresh(model, graph)
    _, _, nm, _, _ = batch_for(SIZES)
    nmd = dev(nm)
    B, N = nm.shape[:2]
    raw = st.normals_host(SEED, 7, 0, B, N, 8)
    zT = dev(orc.combined_noise(raw[0], raw[1], nm.float()))
    kw = dict(sample_id_base=7, **SKW)
    whole = model.path_steps(zT, nmd, **kw)
    for k in (1, 4, K - 1):
        cut = model.path_steps(model.path_steps(zT, nmd, k_hi=k, **kw), nmd, k_lo=k, **kw)
        assert torch.equal(whole, cut), k
    # the last row (lower_order_final: c2 = 0) needs no history; an inner one does
    mid = model.path_steps(zT, nmd, k_hi=4, **kw)
    model.path_steps(mid, nmd, k_lo=K - 1, **kw)
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):      # a gap: the history is at K, not at 4
        model.path_steps(mid, nmd, k_lo=4, **kw)
    mid = model.path_steps(zT, nmd, k_hi=4, **kw)
    model.path_steps(zT, nmd, steps=K, eta=1.0, sample_id_base=7)                        # another path in between
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):
        model.path_steps(mid, nmd, k_lo=4, **kw)
    _, _, nm2, _, _ = batch_for((4, 1, 6))                                               # fresh masks: a topology without history
    with pytest.raises(_lib.HierDiffHipError, match="needs the data prediction"):
        model.path_steps(torch.zeros(3, 6, 11, device=DEV), dev(nm2), k_lo=3, **kw)
    assert torch.equal(model.path_steps(zT, nmd, **kw), whole)                           # and nothing is left in a bad state


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shard_with_its_global_ids_gives_its_rows_of_the_whole_batch(precision):
    B, lo, n = 12, 4, 4
    model, _, _ = model_for(precision)
    fresh(model)
    rng = np.random.default_rng(0)
    sizes = [int(v) for v in rng.integers(1, 13, size=B)]
    sizes[0] = 12                                 # the shard is padded to the batch's width below
    nm, _ = orc.canonical_masks(sizes)
    nm = nm.bool()
    x, h = model.sample_from_masks(dev(nm), None, None, sample_id_base=1000, **SKW)
    xs, hs = model.sample_from_masks(dev(nm[lo:lo + n].contiguous()), None, None, sample_id_base=1000 + lo, **SKW)
    assert torch.equal(x[lo:lo + n], xs) and torch.equal(h[lo:lo + n], hs)
    assert torch.isfinite(x).all() and torch.isfinite(h).all()


# ----------------------------------------------------------------------------- steering: the history follows the lineage

ST_P, ST_MOLS, ST_BETA, ST_RHO, ST_BASE = 4, (7, 7, 7, 7, 4, 4, 4, 4), 3e-4, 0.5, 24
ST_MARGIN = 1e-3                # of S and of P; the fp32 and the float64 oracle differ by 1.6e-6 in the normalised prefix sums here


@functools.lru_cache(maxsize=None)
def steered_reference(gather=True):
    model, sd_np, cfg = model_for("fp32")
    _, _, nm, em, _ = batch_for(ST_MOLS)
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.build_path(T, K)
    rs = st.chain_tables(N)
    net = er.RefNet(sd_np, cfg, T, nm, em, None)
    inner = rr.RestrainedNet(net, rs, torch.tensor([RKW["restraint_scale"]]), rr.rows_from_grid(gg, path, "score", RKW["restraint_clip"]))
    raw = st.normals_host(SEED, ST_BASE, 0, B, N, 8)
    z = orc.combined_noise(raw[0], raw[1], nm.float()).float()
    return sd.steered_chain_ref(inner, rs, gg, path, ST_BETA, ST_P, ST_RHO, SEED, ST_BASE, T, 8, z, False, gather) + (z,)


def steer_kw(N, base=ST_BASE):
    return dict(restraints=st.chain_tables(N), particles=ST_P, steer_scale=ST_BETA, steer_ess=ST_RHO, sample_id_base=base,
                lower_order_final=False, **RKW, **SKW)


def test_steered_chain_against_the_reference():
    """G = 2 groups of P = 4, K = 7, lower_order_final=False.  The float64 reference alone resamples with duplicated rows at
    transitions 1 <= k <= K - 2 (asserted first, with its margins), and the chain that leaves the history in its row lies far
    outside the bar: this test fails when x^_{k-1} does not follow the lineage."""
    lib = _lib.load()
    states, xs, infos, state, zT = steered_reference()
    wrong = steered_reference(False)[0]
    _, _, nm, em, _ = batch_for(ST_MOLS)
    B, N = nm.shape[:2]
    moved = [k for k, i in enumerate(infos) if (i["anc"] != np.arange(B)).any()]
    assert any(1 <= k <= K - 2 for k in moved), moved
    assert min(i["margin"] for i in infos) >= ST_MARGIN and min(i["margin_ess"] for i in infos) >= ST_MARGIN
    # (rows cloned at transition 0 share x^_0, so a later move among them shows nothing: look for the first move that does)
    away = [rel_l2(w.numpy(), s.numpy()) for w, s in zip(wrong, states)]
    k1 = min(k for k in range(K) if away[k] > 0.0)
    print(f"steered sde2m reference: rows move at transitions {moved}; without the history gather state {k1 + 1} is {away[k1]:.2e} away")
    assert 1 <= k1 <= K - 2 and k1 in moved and away[k1] > 10 * REL_L2_TOL
    model, _, _ = model_for("fp32")
    fresh(model)
    nmd, emd = dev(nm), dev(em)
    topo = model.dynamics.topology(nmd, emd, B, N)
    kw = steer_kw(N)
    zz, worst, root_ref = dev(zT), 0.0, np.arange(B) % ST_P
    for k in range(K):
        zz = model.path_steps(zz, nmd, emd, k_lo=k, k_hi=k + 1, **kw)
        logw, uprev, root, anc, stats = read_state(lib, topo.ptr, B, B // ST_P)
        r = rel_l2(zz.cpu().numpy(), states[k].numpy())
        worst = max(worst, r)
        print(f"steered sde2m state {k + 1}/{K}: rel_l2 {r:.2e} (bar {REL_L2_TOL:.0e}), resampled {infos[k]['resampled'].tolist()}")
        assert (anc == infos[k]["anc"]).all(), (k, anc, infos[k]["anc"])
        root_ref = root_ref[infos[k]["anc"]]
        assert (root == root_ref).all(), k
        assert r < REL_L2_TOL, (k, r)
    assert (root == state.root).all() and (stats[:, 0] == state.stats[:, 0]).all()
    assert np.allclose(model.steer_last.min_ess.numpy(), state.stats[:, 1], rtol=1e-3)
    assert torch.equal(model.steer_last.root, torch.from_numpy(state.root).to(torch.int64))
    print(f"steered sde2m: worst state {worst:.2e}; events {state.stats[:, 0].tolist()}")


def test_steered_groups_are_independent_and_graph_replay_equals_launches():
    model, _, _ = model_for("fp32")
    _, _, nm, _, _ = batch_for(ST_MOLS)
    B, N = nm.shape[:2]
    kw = steer_kw(N)
    out = {}
    for graph in (False, True):
        fresh(model, graph)
        out[graph] = (model.sample_from_masks(dev(nm), None, None, **kw), model.steer_last)
    (want, ws), (got, gs) = out[False], out[True]
    assert int(ws.events.sum()) >= 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(gs.root, ws.root) and torch.equal(gs.logw, ws.logw) and torch.equal(gs.events, ws.events)
    for lo in (0, ST_P):                              # a group alone, with its global ids: the other group is removed
        half = model.sample_from_masks(dev(nm[lo:lo + ST_P].contiguous()), None, None, **dict(kw, sample_id_base=ST_BASE + lo))
        assert torch.equal(half[0], got[0][lo:lo + ST_P]) and torch.equal(half[1], got[1][lo:lo + ST_P]), lo
        assert torch.equal(model.steer_last.root, gs.root[lo:lo + ST_P]) and torch.equal(model.steer_last.logw, gs.logw[lo:lo + ST_P])
        assert torch.equal(model.steer_last.events, gs.events[lo // ST_P:lo // ST_P + 1])
    cut = model.path_steps(model.path_steps(dev(steered_reference()[4]), dev(nm), k_hi=3, **kw), dev(nm), k_lo=3, **kw)
    assert torch.equal(cut, model.path_steps(dev(steered_reference()[4]), dev(nm), **kw))
    with pytest.raises(ValueError, match="dpm2m"):
        model.sample_from_masks(dev(nm), None, None, **dict(kw, solver="dpm2m"))


# ----------------------------------------------------------------------------- list-level entry points

def test_list_level_entry_points_take_the_keyword():
    model, _, _ = model_for("fp32")
    fresh(model)

    def check(res):
        for r in res:
            assert torch.isfinite(r["x"]).all() and torch.isfinite(r["h"]).all()
            assert float(r["x"].sum(0).abs().max()) < 1e-3 * max(1.0, float(r["x"].abs().max()))
    torch.manual_seed(0)
    a = model.sample(3, DEV, sample_id_base=2, steps=5, solver="sde2m")
    torch.manual_seed(0)
    model.sample_steps, model.sample_solver = 5, "sde2m"           # the same through the attributes
    b = model.sample(3, DEV, sample_id_base=2)
    torch.manual_seed(0)
    first = model.sample(3, DEV, sample_id_base=2, solver="ddim", eta=1.0)
    model.sample_steps, model.sample_solver = None, None
    assert all(torch.equal(p["x"], q["x"]) and torch.equal(p["h"], q["h"]) for p, q in zip(a, b))
    assert not all(torch.equal(p["x"], q["x"]) for p, q in zip(a, first))
    check(a)
    torch.manual_seed(0)
    res, _ = model.sample_batches(2, 2, DEV, steps=5, spacing="quadratic", solver="sde2m", lower_order_final=False)
    assert len(res) == 4
    check(res)
    var = model.vary(a, DEV, 10, n_variants=2, steps=4, solver="sde2m")
    assert len(var) == 6
    check(var)
    # the reference's signatures
    from hierdiff_amd import EnVariationalDiffusion
    _, _, nm, _, _ = batch_for(SIZES)
    nmd = dev(nm)
    x, h = EnVariationalDiffusion.sample(model, 3, 30, nmd, None, None, steps=5, solver="sde2m")
    want = model.sample_from_masks(nmd, None, None, steps=5, solver="sde2m", keep_frames=5)
    assert torch.equal(x, want[0]) and torch.equal(h, want[1])
    flat = EnVariationalDiffusion.sample_chain(model, 3, 30, nmd, None, None, keep_frames=5, steps=5, solver="sde2m")
    assert tuple(flat.shape) == (15, 30, 11) and torch.equal(flat, want[2].reshape(15, 30, 11))


# ----------------------------------------------------------------------------- C-ABI refusals

def test_c_abi_refusals():
    lib = _lib.load()
    T_, K_ = 8, 3
    sd_np, _ = er.weights(32, 1, C_=1)
    model = build_diffusion(sd_np, 32, 1, C_=1, T=T_)
    nm, _ = orc.canonical_masks([4, 3])
    nmd = dev(nm.bool())
    h = model._lib_handle()
    topo = model.dynamics.topology(nmd, None, 2, 4)
    z = torch.zeros(2, 4, 11, device=DEV)
    ctx = torch.zeros(8, 1, device=DEV)
    ti, si = (C.c_int * 3)(8, 5, 2), (C.c_int * 3)(5, 2, 0)
    rows = (C.c_float * 18)(*([1.0, 0.5, 0.1, 0.0, 1.0, 0.5] * 3))
    assert lib.hd_set_path_multistep_sde(h, K_, ti, si, rows) == -4 and b"schedule not set" in lib.hd_last_error()
    tabs = model._schedule(rows=2)
    assert lib.hd_set_path_multistep_sde(h, K_, (C.c_int * 3)(0, 2, 5), (C.c_int * 3)(2, 5, 8), rows) == -1 and b"descends" in lib.hd_last_error()
    assert lib.hd_set_path_multistep_sde(h, K_, ti, (C.c_int * 3)(5, 3, 0), rows) == -1
    assert lib.hd_set_path_multistep_sde(h, K_, None, si, rows) == -1 and lib.hd_set_path_multistep_sde(h, K_, ti, si, None) == -1
    bad = (C.c_float * 18)(*([1.0, 0.5, 0.1, 0.2, 1.0, 0.5] * 3))
    assert lib.hd_set_path_multistep_sde(h, K_, ti, si, bad) == -1 and b"row 0" in lib.hd_last_error()
    pt = paths.path_tables(tabs["gamma"], [8, 5, 2, 0], solver="sde2m", lower_order_final=False)
    model._path_cache = None
    set_path(lib, h, lib.hd_set_path_multistep_sde, pt, pt["coef"])
    fm = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert lib.hd_sample_path_inpaint(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 0, K_, None, None, 2, 0, 0, 0, fm.data_ptr(),
                                      z.data_ptr(), 1, None) == -1 and b"ancestral rows only" in lib.hd_last_error()
    w = torch.ones(1, device=DEV)
    guided = lambda k_lo, fixed: lib.hd_sample_path_guided(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), w.data_ptr(), 1, 0.0,
                                                           k_lo, K_, None, None, 2, 0, 0, 0, fixed, z.data_ptr() if fixed else None, 1, None)
    assert guided(0, fm.data_ptr()) == -1 and b"ancestral rows only" in lib.hd_last_error()
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 1, K_, None, None, 2, 0, 0, 0, None) == -4    # no history yet
    assert b"needs the data prediction" in lib.hd_last_error()
    assert guided(2, None) == -4
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 0, 2, None, None, 2, 0, 0, 0, None) == 0
    assert guided(2, None) == 0                                          # continues the unguided call where it ended
    assert lib.hd_sample_path(h, topo.ptr, z.data_ptr(), ctx.data_ptr(), -1, 2, K_, None, None, 2, 0, 0, 0, None) == -4    # the history is at K now
    torch.cuda.synchronize()
    # the single update: null arguments, a missing history, overlaps, the LDS limit
    r6 = (C.c_float * 6)(1.0, 0.5, 0.1, 0.0, 1.0, 0.5)
    c6 = (C.c_float * 6)(1.0, 0.5, 0.1, 0.2, 1.0, 0.5)
    out, xo = torch.empty_like(z), torch.empty_like(z)
    step = lambda row, zt, eps, xp, xout, zs, rx=None, rh=None, rows_=2: lib.hd_multistep_sde_step(
        h, topo.ptr, zt, eps, row, xp, xout, rx, rh, rows_, 0, 0, 0, 0, -1, zs, None)
    e = torch.zeros_like(z)
    assert step(r6, None, e.data_ptr(), None, xo.data_ptr(), out.data_ptr()) == -1 and b"null tensor" in lib.hd_last_error()
    assert step(c6, z.data_ptr(), e.data_ptr(), None, xo.data_ptr(), out.data_ptr()) == -1 and b"needs x_prev" in lib.hd_last_error()
    assert step(r6, z.data_ptr(), e.data_ptr(), None, z.data_ptr(), z.data_ptr()) == -1 and b"alias" in lib.hd_last_error()
    assert step(r6, z.data_ptr(), e.data_ptr(), None, xo.data_ptr(), out.data_ptr(), e.data_ptr(), None) == -1 and b"go together" in lib.hd_last_error()
    assert step(r6, z.data_ptr(), e.data_ptr(), None, xo.data_ptr(), out.data_ptr(), rows_=3) == -1 and b"noise_rows" in lib.hd_last_error()
    assert step(r6, z.data_ptr(), e.data_ptr(), None, xo.data_ptr(), out.data_ptr()) == 0, lib.hd_last_error()
    torch.cuda.synchronize()
    N_big = 1490                                         # 1490 * 11 floats are 24 bytes past 64 KiB
    big = torch.zeros(1, N_big, dtype=torch.bool)
    big[0, :2] = True
    bare = Bare(11, big)
    try:
        zb = torch.zeros(1, N_big, 11, device=DEV)
        ob, xb = torch.full_like(zb, float("nan")), torch.full_like(zb, float("nan"))
        rc = lib.hd_multistep_sde_step(bare.h, bare.topo, zb.data_ptr(), zb.data_ptr(), r6, None, xb.data_ptr(), None, None, 1, 0, 0, 0, 0,
                                       -1, ob.data_ptr(), None)
        assert rc == -1 and b"N * D floats exceed one workgroup's LDS" in lib.hd_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(ob).all()) and bool(torch.isnan(xb).all()), "a refused call writes nothing"
    finally:
        bare.close()
