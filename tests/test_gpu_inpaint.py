"""GPU tier (-m gpu) of fragment-constrained sampling: the HIP loop (hd_sample_loop_inpaint) against the CPU restatement of
tests/test_inpaint_cpu.py, the exactness of the known part, reproducibility across batch / graph replay / neighbours, and the
absence of host round trips inside the loop.

Bounds: the project's own parity bar (tests/helpers.py: rel-L2 < 1e-4, max-abs < 1e-4 * max(1, |ref|)) for a single step and for
the short chains.  A chain that misses it is held against the PLAIN chain's error on the same model, T and masks, measured in the
same test: at most twice that (resamplings multiply the network calls that feed back into the trajectory), never above the 1e-3
trajectory bar of test_full_length_chain_vs_oracle."""
import pickle

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as orc
from tests.helpers import MAX_ABS_TOL, REL_L2_TOL, assert_parity, fixture_model, load, rel_l2
from tests.test_gpu_parity import PRECISIONS, build_diffusion
from tests.test_inpaint_cpu import (SEED, gamma_grid_fp64, inpaint_chain_ref, inpaint_steps_ref, philox_raw)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXTURE = {32: "f7_h32_l2", 64: "f7_h64_l2"}
N_LIST = [8, 5, 7, 3, 6]
N_FIXED = [0, 1, 3, 3, 6]              # none, one, some, all (3 of 3), all (6 of 6)


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import _lib
    return _lib.load()


def make_model(H, T, C_=0, precision="fp32", norm=None):
    from hierdiff_amd import DiffusionQM9, default_config
    fx = load(FIXTURE[H])
    sd_np, sd, cfg = fixture_model(fx, context_node_nf=C_)
    if norm is None:
        model = build_diffusion(sd_np, H, int(fx["n_layers"]), C_=C_, T=T, precision=precision)
    else:
        c = default_config(hidden_nf=H, n_layers=int(fx["n_layers"]), context_node_nf=C_, timesteps=T)
        c.norm_values, c.norm_biases = norm
        model = DiffusionQM9(c)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd_np.items()})
        model.dynamics.precision = precision
        model = model.to(DEV)
    model.seed = SEED
    return model, sd, cfg


def make_case(n_list=N_LIST, n_fixed=N_FIXED, seed=0, C_=0, n_max=None):
    nm, em = orc.canonical_masks(n_list, n_max)
    B, N = nm.shape[:2]
    fm = torch.zeros(B, N, 1, dtype=torch.bool)
    for b, k in enumerate(n_fixed):
        fm[b, :k] = True
    g = torch.Generator().manual_seed(100 + seed)
    xk = torch.randn(B, N, 3, generator=g) + torch.tensor([3.0, -2.0, 1.0])     # an arbitrary frame: only the shape matters
    hk = torch.cat([torch.randint(0, 5, (B, N, 5), generator=g).float(), torch.randn(B, N, 3, generator=g)], dim=2)
    ctx = torch.randn(B, 1, 1, generator=g).expand(B, N, 1).contiguous() * nm.float() if C_ else None
    return nm.bool(), em, fm, xk, hk, ctx


def dev(t):
    return None if t is None else t.to(DEV)


def errors(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return rel_l2(got, ref), float(np.max(np.abs(got - ref))), MAX_ABS_TOL * max(1.0, float(np.max(np.abs(ref))))


# ----------------------------------------------------------------------------- 1. no-op identity

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", [32, 64])
def test_no_fixed_nodes_is_plain_sampling_bit_for_bit(H, precision):
    model, _, _ = make_model(H, 12, precision=precision)
    nm, em, fm, xk, hk, _ = make_case()
    x0, h0 = model.sample_from_masks(dev(nm), None, None, sample_id_base=17)
    x1, h1 = model.sample_inpaint(dev(nm), dev(torch.zeros_like(fm)), dev(xk), dev(hk), sample_id_base=17)
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    model.use_graph = False
    x2, h2 = model.sample_inpaint(dev(nm), dev(torch.zeros_like(fm)), dev(xk), dev(hk), sample_id_base=17)
    assert torch.equal(x0, x2) and torch.equal(h0, h2)


# ----------------------------------------------------------------------------- 2. parity with the restatement

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("H", [32, 64])
def test_single_step_matches_the_restatement(lib, H, r, C_, precision):
    T, s = 20, 9
    model, sd, cfg = make_model(H, T, C_=C_, precision=precision)
    gg = gamma_grid_fp64(model, T)
    nm, em, fm, xk, hk, ctx = make_case(C_=C_)
    B, N = nm.shape[:2]
    ids = [5 + b for b in range(B)]
    g = torch.Generator().manual_seed(1)
    z_t = orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float())
    xh_known = torch.cat([xk, hk], dim=2) * fm.float()
    ref = inpaint_steps_ref(lib, sd, cfg, T, gg, z_t, s + 1, s, nm.float(), em, ctx, fm.float(), xh_known, r, SEED, ids)
    for graph in (True, False):
        model.use_graph = graph
        got = model.inpaint_steps(dev(z_t), s + 1, s, dev(nm), dev(fm), dev(xk), dev(hk), context=dev(ctx), resamplings=r,
                                  sample_id_base=5)
        rl, ma, bound = errors(got.cpu().numpy(), ref.numpy())
        print(f"single step H={H} r={r} ctx={C_} [{precision}] graph={graph}: rel_l2 {rl:.2e} max_abs {ma:.2e} (bound {bound:.2e})")
        assert_parity(got.cpu().numpy(), ref.numpy(), f"inpaint step H={H} r={r}")
        assert torch.all(got.cpu()[~nm.expand_as(got).bool()] == 0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C_", [0, 1])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("H", [32, 64])
def test_chain_matches_the_restatement(lib, H, r, C_, precision):
    T = 20
    model, sd, cfg = make_model(H, T, C_=C_, precision=precision)
    gg = gamma_grid_fp64(model, T)
    nm, em, fm, xk, hk, ctx = make_case(C_=C_)
    B, N = nm.shape[:2]
    ids = [30 + b for b in range(B)]
    x, h = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), context=dev(ctx), resamplings=r, sample_id_base=30)
    xr, hr, _ = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, ctx, fm, xk, hk, r, SEED, ids)
    ex, eh = errors(x.cpu().numpy(), xr.numpy()), errors(h.cpu().numpy(), hr.numpy())
    print(f"chain T={T} H={H} r={r} ctx={C_} [{precision}]: x rel_l2 {ex[0]:.2e} max_abs {ex[1]:.2e} (bound {ex[2]:.2e}); "
          f"h rel_l2 {eh[0]:.2e} max_abs {eh[1]:.2e} (bound {eh[2]:.2e})")
    assert torch.isfinite(x).all() and torch.isfinite(h).all()
    if all(e[0] < REL_L2_TOL and e[1] < e[2] for e in (ex, eh)):
        return
    # missed the per-chain bar: hold it against the plain chain on the same model, T and masks
    raws = [philox_raw(lib, SEED, ids, d, N) for d in range(T + 2)]
    xo, ho = orc.sample_chain(sd, cfg, T, nm.float(), em, ctx, raws, gamma_grid=gg)
    xp, hp = model.sample_from_masks(dev(nm), None, dev(ctx), sample_id_base=30)
    px, ph = errors(xp.cpu().numpy(), xo.numpy()), errors(hp.cpu().numpy(), ho.numpy())
    print(f"  plain chain on the same model: x rel_l2 {px[0]:.2e} max_abs {px[1]:.2e}; h rel_l2 {ph[0]:.2e} max_abs {ph[1]:.2e}")
    for e, p, what in ((ex, px, "x"), (eh, ph, "h")):
        assert e[0] <= min(2 * p[0], 1e-3) or e[0] < REL_L2_TOL, f"{what}: rel_l2 {e[0]:.3e} vs plain chain {p[0]:.3e}"
        assert e[1] <= 2 * p[1] or e[1] < e[2], f"{what}: max_abs {e[1]:.3e} vs plain chain {p[1]:.3e}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_with_non_unit_norm_values_matches_the_restatement(lib, precision):
    T, r = 12, 2
    norm = ([2.0, 4.0, 1.0], [None, 0.5, 0.0])
    model, sd, cfg = make_model(64, T, precision=precision, norm=norm)
    gg = gamma_grid_fp64(model, T)
    nm, em, fm, xk, hk, _ = make_case(seed=2)
    ids = [b for b in range(nm.shape[0])]
    x, h = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r)
    xr, hr, _ = inpaint_chain_ref(lib, sd, cfg, T, gg, nm, em, None, fm, xk, hk, r, SEED, ids, norm_values=norm[0],
                                  norm_biases=norm[1])
    assert_parity(x.cpu().numpy(), xr.numpy(), "norm x")
    assert_parity(h.cpu().numpy(), hr.numpy(), "norm h")
    assert torch.equal(h.cpu()[fm.expand_as(hk)], hk[fm.expand_as(hk)])


# ----------------------------------------------------------------------------- 3. exactness of the known part

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("r", [1, 3])
def test_known_part_is_returned_exactly(r, precision):
    model, _, _ = make_model(64, 16, precision=precision)
    nm, em, fm, xk, hk, _ = make_case(seed=3)
    x, h = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=9)
    model.debug_checks = True          # the loop's own centre-of-gravity check after every step (asserts inside)
    xd, hd = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=9)
    model.debug_checks = False
    assert torch.equal(x, xd) and torch.equal(h, hd)          # a chain cut into single steps gives the bits of the whole
    x, h = x.cpu(), h.cpu()
    assert torch.equal(h[fm.expand_as(h)], hk[fm.expand_as(h)])
    for b, k in enumerate(N_FIXED):
        if k < 2:
            continue
        got = x[b, :k, None, :] - x[b, None, :k, :]
        want = xk[b, :k, None, :] - xk[b, None, :k, :]
        mag = max(float(x[b, :k].abs().max()), float(xk[b, :k].abs().max()))
        assert float((got - want).abs().max()) <= 2 * float(np.spacing(np.float32(mag))), b
    assert torch.all(x[~nm.expand_as(x)] == 0) and torch.all(h[~nm.expand_as(h)] == 0)


# ----------------------------------------------------------------------------- 4. reproducibility

@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_molecule_depends_on_its_own_id_masks_and_known_values_only(precision):
    T, r, n, k, gid = 10, 2, 6, 2, 1234
    model, _, _ = make_model(32, T, precision=precision)
    g = torch.Generator().manual_seed(8)
    xk1, hk1 = torch.randn(1, n, 3, generator=g), torch.randn(1, n, 8, generator=g)
    nm1 = torch.ones(1, n, 1, dtype=torch.bool)
    fm1 = torch.zeros(1, n, 1, dtype=torch.bool)
    fm1[0, :k] = True
    xa, ha = model.sample_inpaint(dev(nm1), dev(fm1), dev(xk1), dev(hk1), resamplings=r, sample_id_base=gid)
    # a batch of 8, the molecule at row 5 with the same global id, padded to 9 nodes
    row, sizes = 5, [9, 4, 7, 3, 8, n, 5, 9]
    nm, em, fm, xk, hk, _ = make_case(sizes, [0, 2, 3, 3, 1, k, 0, 9], seed=4)
    fm[row] = False
    fm[row, :k] = True
    xk[row, :n], hk[row, :n] = xk1[0], hk1[0]
    outs = []
    for graph in (True, False):
        model.use_graph = graph
        outs.append(model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r, sample_id_base=gid - row))
    model.use_graph = True
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # graph replay on / off
    xb, hb = outs[0]
    assert torch.equal(xb[row, :n], xa[0]) and torch.equal(hb[row, :n], ha[0])               # alone vs in the batch
    fm2 = fm.clone()                                                                         # the neighbours' fixed sets change
    fm2[0, :4] = True
    fm2[1] = False
    fm2[7, 3:] = False
    xc, hc = model.sample_inpaint(dev(nm), dev(fm2), dev(xk), dev(hk), resamplings=r, sample_id_base=gid - row)
    assert torch.equal(xc[row], xb[row]) and torch.equal(hc[row], hb[row])
    assert not torch.equal(xc[0], xb[0])


# ----------------------------------------------------------------------------- 5. the known values matter

@pytest.mark.parametrize("r", [1, 3])
def test_known_values_reach_the_free_nodes_of_their_molecule_only(r):
    model, _, _ = make_model(64, 16)
    nm, em, fm, xk, hk, _ = make_case(seed=5)
    x1, h1 = model.sample_inpaint(dev(nm), dev(fm), dev(xk), dev(hk), resamplings=r)
    xk2 = xk.clone()
    xk2[2, 1] += torch.tensor([0.7, -0.4, 0.9])          # molecule 2: 3 of 7 nodes fixed
    x2, h2 = model.sample_inpaint(dev(nm), dev(fm), dev(xk2), dev(hk), resamplings=r)
    free = slice(N_FIXED[2], N_LIST[2])
    assert not torch.equal(x1[2, free], x2[2, free]) and not torch.equal(h1[2, free], h2[2, free])
    for b in (0, 1, 3, 4):
        assert torch.equal(x1[b], x2[b]) and torch.equal(h1[b], h2[b])


# ----------------------------------------------------------------------------- 6. no host round trip

@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("r", [1, 3])
def test_loop_runs_library_kernels_only(r, graph):
    from torch.profiler import ProfilerActivity, profile
    T = 8
    model, _, _ = make_model(64, T)
    model.use_graph = graph
    nm, em, fm, xk, hk, _ = make_case(seed=6)
    args = [dev(nm), dev(fm), dev(xk), dev(hk)]
    model.sample_inpaint(*args, resamplings=r)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        model.sample_inpaint(*args, resamplings=r)
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name for e in evs if not e.name.lower().startswith(("memcpy", "memset"))]
    steps = [i for i, n in enumerate(names) if "k_post_step" in n]
    assert len(steps) == T * r, (len(steps), names[:60])
    window = names[steps[0]:steps[-1] + 1]
    assert sum("k_inpaint_replace" in n for n in names) == T * r
    assert sum("k_inpaint_jump" in n for n in names) == T * (r - 1)
    foreign = [n for n in window if "at::native" in n or "k_" not in n]
    assert not foreign, foreign[:20]


# ----------------------------------------------------------------------------- 7. CLI round trip

def test_cli_grows_known_fragments(tmp_path):
    from hierdiff_amd import sampler
    from hierdiff_amd.weights import synthetic_state_dict
    syn = synthetic_state_dict(9, 0, 32, 1, 2, True, 12, 1.0)
    ck = tmp_path / "diffusion.ckpt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v.copy()) for k, v in syn.items()}}, ck)
    plain, known, out = tmp_path / "plain.pkl", tmp_path / "known.pkl", tmp_path / "grown.pkl"
    common = ["--checkpoint", str(ck), "--hidden-nf", "32", "--n-layers", "1", "--timesteps", "6"]
    assert sampler.main(common + ["--out", str(plain), "--batch-size", "8", "--num-batches", "1"]) == 0
    res = [m for m in pickle.load(open(plain, "rb"))[0] if m["x"].shape[0] >= 3][:4]
    assert len(res) == 4
    frag = [{"x": m["x"][:3].clone(), "h": m["h"][:3].clone()} for m in res]
    sampler.write_results(str(known), frag)
    assert sampler.main(common + ["--out", str(out), "--known", str(known), "--grow", "5", "--resamplings", "2",
                                  "--batch-size", "3"]) == 0
    grown, names = pickle.load(open(out, "rb"))
    assert names == [] and len(grown) == 4
    for m, f in zip(grown, frag):
        assert tuple(m["x"].shape) == (8, 3) and tuple(m["h"].shape) == (8, 8)
        assert torch.isfinite(m["x"]).all() and torch.isfinite(m["h"]).all()
        assert torch.equal(m["h"][:3], f["h"])
        d = m["x"][:3] - f["x"]
        mag = max(float(m["x"][:3].abs().max()), float(f["x"].abs().max()))
        assert float((d - d[0]).abs().max()) <= 2 * float(np.spacing(np.float32(mag)))
