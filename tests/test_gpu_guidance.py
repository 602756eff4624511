"""GPU tier (-m gpu) of classifier-free guidance: hd_guide_combine against its float64 restatement, the guided path loop
(hd_sample_path_guided) against the unguided loops at w = 1 / w = 0 (bit for bit) and against `guided_chain_ref` of
tests/guidance_reference.py with injected normals, and its reproducibility across graph replay, batch split, chain cuts, inpainting,
variations, merged batches; context dropout in training.

Bar of the parity cases: tests/test_gpu_fewstep.py's rel-L2 < 1e-3 on the final x and h (and here z_0), the bar the unguided chain of
the same (T, K, eta) is held to; tests/test_guidance_cpu.py shows that the restatement's own fp32 / fp64 gap stays below a tenth of it
for every case.  Measured distances are printed.  Shapes: T = 20, H = 32, L = 2 (fp16x3: H = 128, L = 1), molecules [7, 4, 1] (a
one-node molecule) and [30, 17] (N * D = 330 > 256: the kernel's strided loops wrap)."""
import functools

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests.helpers import rel_l2
from tests.test_gpu_parity import build_diffusion
from tests.test_inpaint_cpu import SEED, gamma_grid_fp64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 20
SHAPES = {"fp32": (32, 2), "fp16x3": (128, 1)}          # the cases marked "both precisions" run fp16x3 at H = 128, L = 1
BOTH = ["fp32", "fp16x3"]
FEWS = {"identity": dict(eta=1.0), "K7eta0": dict(steps=7, eta=0.0), "K5eta05": dict(steps=5, eta=0.5)}


def dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def model_for(precision):
    H, L = SHAPES[precision]
    sd_np, cfg = er.weights(H, L, C_=1)
    model = build_diffusion(sd_np, H, L, C_=1, T=T, precision=precision)
    model.seed = SEED
    return model, sd_np, cfg


@functools.lru_cache(maxsize=None)
def batch_for(mols):
    x, h, nm, em, ctx = er.molecules(list(mols), C_=1)
    return x, h, nm, em, ctx, gr.null_ctx(nm, 0.0)


def few_kw(few):
    return {k: v for k, v in few.items()}


def fresh(model):
    model.use_graph = True
    model.guidance_scale, model.guidance_context, model.guidance_rescale, model.null_context = None, None, 0.0, 0.0
    model.merge_batches = 4096
    model.context_drop_prob = 0.0
    model.eval()
    return model


# ----------------------------------------------------------------------------- the kernel

def test_guide_combine_against_float64():
    model, _, _ = model_for("fp32")
    fresh(model)
    lib = _lib.load()
    nm, _ = orc.canonical_masks([30, 17, 7, 4, 1, 9])
    nm = nm.bool()
    B, N, D = nm.shape[0], nm.shape[1], 11
    g = torch.Generator().manual_seed(2)
    ec = torch.randn(B, N, D, generator=g) * nm.float()
    eu = torch.randn(B, N, D, generator=g) * nm.float()
    eu[4, 0, :3] = ec[4, 0, :3] = 0.0                       # the one-node molecule: a mean-free x part is exactly 0
    w = torch.tensor([0.0, 1.0, 2.5, -0.5, 1.7, 0.3])
    nmd = dev(nm)
    topo = model.dynamics.topology(nmd, None, B, N)
    h = model._lib_handle()
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    ecd, eud, wd = dev(ec).contiguous(), dev(eu).contiguous(), dev(w).contiguous()
    valid = nm.expand(B, N, D)

    def run(phi, wt, out=None, src=None):
        src = ecd if src is None else src
        out = torch.full((B, N, D), 7.0, device=DEV) if out is None else out
        rc = lib.hd_guide_combine(h, topo.ptr, src.data_ptr(), eud.data_ptr(), wt.data_ptr(), wt.numel(), phi, out.data_ptr(), stream)
        assert rc == 0, lib.hd_last_error()
        return out

    for phi in (0.0, 0.7):
        out = run(phi, wd).cpu()
        assert torch.equal(out[1], ec[1]) and torch.equal(out[0], eu[0])          # copies, phi ignored
        assert bool((out[~valid] == 0).all())
        alias_buf = ecd.clone()
        aliased = run(phi, wd, out=alias_buf, src=alias_buf).cpu()
        assert torch.equal(aliased, out)
        ref = gr.combine_ref(ec, eu, w, phi, nm)                                    # float64
        if phi == 0.0:
            bound = 2.0 ** -23 * (eu.double().abs() + 2 * w.double().abs().view(B, 1, 1) * (ec.double() - eu.double()).abs())
            err = (out.double() - ref).abs()
            print(f"hd_guide_combine phi=0: max err / bound {float((err / bound.clamp(min=1e-300))[valid].max()):.3f}")
            assert bool((err <= bound)[valid].all())
        else:
            for b in range(B):
                r = rel_l2(out[b].numpy(), ref[b].numpy())
                print(f"hd_guide_combine phi=0.7 molecule {b} (w = {float(w[b])}): rel_l2 {r:.2e}")
                assert r < 1e-6
    # a shared scale
    shared = run(0.0, dev(torch.tensor([2.5]))).cpu()
    assert rel_l2(shared.numpy(), gr.combine_ref(ec, eu, 2.5, 0.0, nm).numpy()) < 1e-6
    # argument errors
    bad = torch.empty(B, N, D, device=DEV)
    assert lib.hd_guide_combine(h, topo.ptr, ecd.data_ptr(), eud.data_ptr(), wd.data_ptr(), 2, 0.0, bad.data_ptr(), stream) == -1
    assert lib.hd_guide_combine(h, topo.ptr, ecd.data_ptr(), eud.data_ptr(), wd.data_ptr(), B, 1.5, bad.data_ptr(), stream) == -1
    assert lib.hd_guide_combine(h, topo.ptr, ecd.data_ptr(), eud.data_ptr(), wd.data_ptr(), B, -0.1, bad.data_ptr(), stream) == -1
    assert lib.hd_guide_combine(h, topo.ptr, ecd.data_ptr(), eud.data_ptr(), wd.data_ptr(), B, 0.0, eud.data_ptr(), stream) == -1
    assert lib.hd_guided_graph_builds(None) == -1


# ----------------------------------------------------------------------------- w = 1 / w = 0: the unguided loops, bit for bit

@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
@pytest.mark.parametrize("few", ["identity", "K7eta0"])
def test_scale_one_and_zero_are_the_unguided_loop_bit_for_bit(few, graph, precision):
    model, _, _ = model_for(precision)
    fresh(model).use_graph = graph
    for mols in ((7, 4, 1), (30, 17)):
        x, h, nm, em, ctx, ctx0 = batch_for(mols)
        B = nm.shape[0]
        gctx = (ctx * 0.5 + 0.25 * nm.float()).contiguous()
        kw = few_kw(FEWS[few])
        nmd = dev(nm)
        plain_c = model.sample_from_masks(nmd, None, dev(ctx), sample_id_base=5, **kw)
        plain_u = model.sample_from_masks(nmd, None, dev(gctx), sample_id_base=5, **kw)
        assert not torch.equal(plain_c[0], plain_u[0])
        for phi in (0.0, 0.7):
            one = model.sample_from_masks(nmd, None, dev(ctx), sample_id_base=5, guidance_scale=torch.ones(B),
                                          guidance_context=dev(gctx), guidance_rescale=phi, **kw)
            zero = model.sample_from_masks(nmd, None, dev(ctx), sample_id_base=5, guidance_scale=torch.zeros(B),
                                           guidance_context=dev(gctx), guidance_rescale=phi, **kw)
            assert torch.equal(one[0], plain_c[0]) and torch.equal(one[1], plain_c[1])
            assert torch.equal(zero[0], plain_u[0]) and torch.equal(zero[1], plain_u[1])


# ----------------------------------------------------------------------------- parity with injected normals

@functools.lru_cache(maxsize=None)
def reference(name, precision, t_start=T):
    case = {c[0]: c for c in gr.PARITY}[name]
    _, mols, few, w, phi = case
    model, sd_np, cfg = model_for(precision)
    x, h, nm, em, ctx, ctx0 = batch_for(tuple(mols))
    B, N = nm.shape[:2]
    gg = gamma_grid_fp64(model, T)
    path = paths.partial_path(T, t_start, few.get("steps"))
    raws = er.raw_draws(len(path) + 1, B, N, seed=len(path))
    z = orc.combined_noise(raws[0][0], raws[0][1], nm.float())
    net_c, net_u = er.RefNet(sd_np, cfg, T, nm, em, ctx), er.RefNet(sd_np, cfg, T, nm, em, ctx0)
    out = gr.guided_chain_ref(gr.GuidedNet(net_c, net_u, gr.scale_for(w, B), phi), gg, path, few["eta"], z, nm, raws[1:])
    return out, z, raws


def check_parity(name, precision, t_start=T):
    _, mols, few, w, phi = {c[0]: c for c in gr.PARITY}[name]
    model, _, _ = model_for(precision)
    fresh(model)
    x, h, nm, em, ctx, ctx0 = batch_for(tuple(mols))
    B = nm.shape[0]
    (xo, ho, zo), z, raws = reference(name, precision, t_start)
    K = len(raws) - 2
    kw = dict(t_start=t_start, steps=few.get("steps"), eta=few["eta"], guidance_scale=gr.scale_for(w, B), guidance_rescale=phi)
    z0 = model.latent_steps(dev(z), dev(nm), dev(em), dev(ctx), raw_noises=raws[1:K + 1], **kw)
    xg, hg = model.sample_from_latent(dev(z), dev(nm), dev(em), dev(ctx), raw_noises=raws[1:], **kw)
    nmf = nm.float().numpy()
    rx, rh = rel_l2(xg.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(hg.cpu().numpy(), ho.numpy())
    rz = rel_l2(z0.cpu().numpy(), zo.numpy())
    print(f"guided parity {name} [{precision}] t_start={t_start}: x {rx:.2e} h {rh:.2e} z0 {rz:.2e} (bar {gr.BAR:.0e})")
    assert torch.isfinite(xg).all() and torch.isfinite(hg).all()
    assert max(rx, rh, rz) < gr.BAR, (name, rx, rh, rz)
    return (xg, hg, z0), kw, (z, raws, K)


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("name", [c[0] for c in gr.PARITY])
def test_guided_chain_parity_with_injected_normals(name, precision):
    (xg, hg, z0), kw, (z, raws, K) = check_parity(name, precision)
    _, mols, few, w, phi = {c[0]: c for c in gr.PARITY}[name]
    if not isinstance(w, list):                       # not a no-op: the w = 1 chain lies further away than the bar
        model, _, _ = model_for(precision)
        x, h, nm, em, ctx, ctx0 = batch_for(tuple(mols))
        kw1 = dict(kw, guidance_scale=None, guidance_rescale=None)
        x1, h1 = model.sample_from_latent(dev(z), dev(nm), dev(em), dev(ctx), raw_noises=raws[1:], **kw1)
        d = max(rel_l2(xg.cpu().numpy(), x1.cpu().numpy()), rel_l2(hg.cpu().numpy(), h1.cpu().numpy()))
        print(f"   distance of the w = 2.5 result from the w = 1 result: {d:.2e}")
        assert d > gr.BAR


def test_sample_from_masks_guided_matches_the_reference():
    """The same chain through `sample_from_masks` (z_T from the injected pair, the identity path chosen by the guided call itself)."""
    name = "wrap-identity-w2.5-phi0.7"
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, ctx, ctx0 = batch_for((30, 17))
    (xo, ho, zo), z, raws = reference(name, "fp32")
    xg, hg = model.sample_from_masks(dev(nm), dev(em), dev(ctx), raw_noises=raws, guidance_scale=2.5, guidance_rescale=0.7)
    nmf = nm.float().numpy()
    rx, rh = rel_l2(xg.cpu().numpy() * nmf, xo.numpy() * nmf), rel_l2(hg.cpu().numpy(), ho.numpy())
    print(f"sample_from_masks guided: x {rx:.2e} h {rh:.2e}")
    assert rx < gr.BAR and rh < gr.BAR


@pytest.mark.parametrize("precision", BOTH)
def test_partial_path_variations_match_the_reference(precision):
    check_parity("main-K5eta05-w2.5-phi0.7", precision, t_start=8)
    check_parity("wrap-identity-wrows-phi0.0", precision, t_start=8)


# ----------------------------------------------------------------------------- graph replay, cache keys, interleaving

def test_graph_replay_equals_plain_launches_and_the_cache_keys():
    model, _, _ = model_for("fp32")
    fresh(model)
    lib = _lib.load()
    x, h, nm, em, ctx, ctx0 = batch_for((30, 17))
    B, N = nm.shape[:2]
    nmd, ctxd = dev(nm), dev(ctx)
    topo = model.dynamics.topology(nmd, None, B, N)
    builds = lambda: lib.hd_guided_graph_builds(topo.ptr)
    kw = dict(steps=7, eta=0.5, guidance_scale=2.5, guidance_rescale=0.7, sample_id_base=3)
    a = model.sample_from_masks(nmd, None, ctxd, **kw)
    n0 = builds()
    assert n0 >= 1
    model.use_graph = False
    b = model.sample_from_masks(nmd, None, ctxd, **kw)
    model.use_graph = True
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and builds() == n0
    # new values of w, of the contexts and of sample_id_base replay the cached graph
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, guidance_scale=1.7))
    model.sample_from_masks(nmd, None, dev(ctx * 0.5), **kw)
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, guidance_context=dev(ctx * 0.25)))
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, sample_id_base=11))
    assert builds() == n0
    a2 = model.sample_from_masks(nmd, None, ctxd, **kw)
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    # a new phi, a new w_rows and a new path each instantiate once
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, guidance_rescale=0.2))
    assert builds() == n0 + 1
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, guidance_rescale=0.2, guidance_scale=torch.tensor([2.5, 0.3])))
    assert builds() == n0 + 2
    model.sample_from_masks(nmd, None, ctxd, **dict(kw, guidance_rescale=0.2, guidance_scale=torch.tensor([2.5, 0.3]), steps=5))
    assert builds() == n0 + 3
    # unguided -> guided -> unguided -> guided on one topology: each returns its first bits
    un = dict(steps=7, eta=0.5, sample_id_base=3)
    u1 = model.sample_from_masks(nmd, None, ctxd, **un)
    g1 = model.sample_from_masks(nmd, None, ctxd, **kw)
    p0 = lib.hd_path_graph_builds(topo.ptr)
    u2 = model.sample_from_masks(nmd, None, ctxd, **un)
    g2 = model.sample_from_masks(nmd, None, ctxd, **kw)
    assert torch.equal(u1[0], u2[0]) and torch.equal(u1[1], u2[1])
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1]) and torch.equal(g1[0], a[0])
    assert lib.hd_path_graph_builds(topo.ptr) == p0          # the guided graph did not evict the unguided one
    assert not torch.equal(u1[0], g1[0])


def test_shard_independence_and_chain_cuts():
    model, _, _ = model_for("fp32")
    fresh(model)
    mols = (7, 4, 1, 30, 17, 5, 9, 3)
    x, h, nm, em, ctx, ctx0 = batch_for(mols)
    B, N = nm.shape[:2]
    w = torch.tensor([2.5, 1.0, 0.3, -0.5, 1.7, 0.0, 3.0, 2.0])
    kw = dict(steps=7, eta=1.0, guidance_rescale=0.7)
    full = model.sample_from_masks(dev(nm), None, dev(ctx), sample_id_base=20, guidance_scale=w, **kw)
    part = model.sample_from_masks(dev(nm[2:5].contiguous()), None, dev(ctx[2:5].contiguous()), sample_id_base=22,
                                   guidance_scale=w[2:5], **kw)
    assert torch.equal(full[0][2:5], part[0]) and torch.equal(full[1][2:5], part[1])
    # a chain cut with path_steps(k_lo, k_hi) gives the bits of the whole
    g = torch.Generator().manual_seed(8)
    z = orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm.float())
    pk = dict(steps=7, eta=0.5, guidance_scale=w, guidance_rescale=0.7, sample_id_base=20)
    whole = model.path_steps(dev(z), dev(nm), None, dev(ctx), **pk)
    cut = model.path_steps(dev(z), dev(nm), None, dev(ctx), k_lo=0, k_hi=3, **pk)
    cut = model.path_steps(cut, dev(nm), None, dev(ctx), k_lo=3, k_hi=7, **pk)
    assert torch.equal(whole, cut)
    plain = model.path_steps(dev(z), dev(nm), None, dev(ctx), steps=7, eta=0.5, sample_id_base=20)
    assert not torch.equal(whole, plain)


# ----------------------------------------------------------------------------- inpainting, variations, merged batches

@pytest.mark.parametrize("r", [1, 2])
def test_guided_inpainting(r):
    from tests.test_gpu_inpaint import make_case
    model, _, _ = model_for("fp32")
    fresh(model)
    nm, em, fm, xk, hk, ctx = make_case(C_=1)
    B = nm.shape[0]
    args = (dev(nm), dev(fm), dev(xk), dev(hk))
    for few in (dict(), dict(steps=7)):
        plain = model.sample_inpaint(*args, context=dev(ctx), resamplings=r, sample_id_base=21, **few)
        one = model.sample_inpaint(*args, context=dev(ctx), resamplings=r, sample_id_base=21, guidance_scale=torch.ones(B),
                                   guidance_rescale=0.7, **few)
        assert torch.equal(one[0], plain[0]) and torch.equal(one[1], plain[1])
        xg, hg = model.sample_inpaint(*args, context=dev(ctx), resamplings=r, sample_id_base=21, guidance_scale=2.5, **few)
        xg, hg = xg.cpu(), hg.cpu()
        fmb = fm.expand(-1, -1, 3)
        free = (nm & ~fm)
        assert torch.equal(hg[fm.expand(-1, -1, 8)], hk[fm.expand(-1, -1, 8)])
        for b in range(B):                                # the fixed rows: the known ones translated as one block
            if int(fm[b].sum()) == 0:
                continue
            shift = (xg[b] - xk[b])[fmb[b]].reshape(-1, 3)
            assert float((shift - shift[0:1]).abs().max()) < 1e-5
        assert not torch.equal(xg[free.expand(-1, -1, 3)], plain[0].cpu()[free.expand(-1, -1, 3)])
    with pytest.raises(ValueError):
        model.sample_inpaint(*args, context=dev(ctx), eta=0.5, guidance_scale=2.5)


def test_guided_vary_and_merged_batches():
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, ctx, ctx0 = batch_for((7, 4, 1))
    mols = [{"x": x[i, :n].clone(), "h": h[i, :n].clone(), "context": ctx[i, :n].clone()} for i, n in enumerate((7, 4, 1))]
    plain = model.vary(mols, DEV, 8, n_variants=2, sample_id_base=4, steps=4)
    one = model.vary(mols, DEV, 8, n_variants=2, sample_id_base=4, steps=4, guidance_scale=torch.ones(6), guidance_rescale=0.7)
    strong = model.vary(mols, DEV, 8, n_variants=2, sample_id_base=4, steps=4, guidance_scale=2.5)
    assert all(torch.equal(a["x"], b["x"]) and torch.equal(a["h"], b["h"]) for a, b in zip(plain, one))
    assert any(not torch.equal(a["x"], b["x"]) for a, b in zip(plain, strong))
    # sample_batches with one scale per batch: the merged device batch gives the bits of the loop over batches
    runs = []
    for merge in (4096, 0):
        model.merge_batches = merge
        torch.manual_seed(3)
        runs.append(model.sample_batches(2, 2, DEV, context_range=[0.3, -0.2], sample_id_base=6, steps=5, guidance_scale=[2.5, 0.5],
                                         guidance_rescale=0.7)[0])
    model.merge_batches = 4096
    assert len(runs[0]) == len(runs[1]) == 4
    assert all(torch.equal(a["x"], b["x"]) and torch.equal(a["h"], b["h"]) for a, b in zip(*runs))
    torch.manual_seed(3)
    unguided = model.sample_batches(2, 2, DEV, context_range=[0.3, -0.2], sample_id_base=6, steps=5)[0]
    assert any(not torch.equal(a["x"], b["x"]) for a, b in zip(runs[0], unguided))


# ----------------------------------------------------------------------------- training: context dropout

def test_context_dropout_in_training(monkeypatch):
    from hierdiff_amd import guidance
    model, _, _ = model_for("fp32")
    fresh(model)
    x, h, nm, em, ctx, ctx0 = batch_for((7, 4, 1))
    B, N = nm.shape[:2]
    nmf = nm.float()
    xc = orc.remove_mean_with_mask(x * nmf, nmf)
    g = torch.Generator().manual_seed(12)
    noise = lambda: orc.combined_noise(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nmf)
    replay = dict(t_int=torch.tensor([[3.0], [11.0], [17.0]]), eps=noise(), eps0=noise())

    def loss(context, p, null=0.0):
        model.context_drop_prob, model.null_context = p, null
        batch = dict(positions=dev(xc), atom_mask=dev(nm), edge_mask=dev(em), node_feature=dev(h * nmf), context=dev(context))
        return model.forward(batch, **{k: dev(v) for k, v in replay.items()})["loss"].detach().cpu()

    model.train()
    try:
        base = loss(ctx, 0.0)
        with monkeypatch.context() as mp:                 # p = 0 is today's path: the dropout is not even called
            mp.setattr(guidance, "drop_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("dropout called")))
            assert torch.equal(loss(ctx, 0.0), base)
        null = 0.5
        dropped = loss(ctx, 1.0, null)
        assert torch.equal(dropped, loss(gr.null_ctx(nm, null), 0.0))
        assert not torch.equal(dropped, base)
        model.eval()
        ev = loss(ctx, 1.0, null)
        model.context_drop_prob = 0.0
        assert torch.equal(ev, loss(ctx, 0.0))            # eval mode never drops
    finally:
        fresh(model)
