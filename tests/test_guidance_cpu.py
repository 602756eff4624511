"""CPU tier of classifier-free guidance: the restatement of tests/guidance_reference.py against the unguided restatements and the
oracle, the fp32 / fp64 gap of every GPU parity case against its bar, `combine_ref`'s rescale, context dropout, and every argument
error of the Python entry points (raised before a device is looked at)."""
import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, guidance, paths
from oracle import egnn_oracle as orc
from tests import edit_reference as er
from tests import guidance_reference as gr
from tests.helpers import rel_l2
from tests.test_inpaint_cpu import gamma_grid_fp64

T = 20


def setup(n_list, H=32, L=2, dtype=torch.float32, null=0.0):
    sd_np, cfg = er.weights(H, L, C_=1)
    x, h, nm, em, ctx = er.molecules(n_list, C_=1)
    model = er.cpu_diffusion(sd_np, H, L, T, C_=1)
    gg = gamma_grid_fp64(model, T)
    ctx_u = gr.null_ctx(nm, null)
    net_c = er.RefNet(sd_np, cfg, T, nm, em, ctx, dtype=dtype)
    net_u = er.RefNet(sd_np, cfg, T, nm, em, ctx_u, dtype=dtype)
    return model, gg, nm, em, ctx, ctx_u, net_c, net_u


def start_state(nm, seed=9):
    B, N = nm.shape[:2]
    raw = er.raw_draws(1, B, N, seed)[0]
    return orc.combined_noise(raw[0], raw[1], nm.float())


@pytest.mark.parametrize("few", [dict(eta=1.0), dict(steps=7, eta=0.0), dict(steps=5, eta=0.5)], ids=["identity", "K7eta0", "K5eta05"])
def test_scale_one_and_zero_are_the_unguided_chains(few):
    model, gg, nm, em, ctx, ctx_u, net_c, net_u = setup([7, 4, 1])
    B, N = nm.shape[:2]
    path = paths.build_path(T, few.get("steps"))
    eta = few["eta"]
    raws = er.raw_draws(len(path), B, N, seed=3)
    z = start_state(nm)
    for w, net in ((1.0, net_c), (0.0, net_u)):
        for phi in (0.0, 0.7):                                   # phi is ignored for these two values
            got = gr.guided_chain_ref(gr.GuidedNet(net_c, net_u, torch.full((B,), w), phi), gg, path, eta, z, nm, raws)
            # the decode of the w = 0 chain runs under the null context too: partial_chain_ref on net_u
            ref = er.partial_chain_ref(net, gg, path, eta, z, nm, raws)
            for a, b in zip(got, ref):
                assert torch.equal(a, b)


def test_identity_path_is_the_oracles_own_posterior_chain():
    model, gg, nm, em, ctx, ctx_u, net_c, net_u = setup([30, 17])
    B, N = nm.shape[:2]
    path = list(range(T, -1, -1))
    raws = er.raw_draws(T + 1, B, N, seed=4)
    z = start_state(nm)
    got = gr.guided_chain_ref(gr.GuidedNet(net_c, net_u, 1.0, 0.0), gg, path, 1.0, z, nm, raws)
    zz = z
    with torch.no_grad():
        for k, (t, s) in enumerate(zip(path[:-1], path[1:])):
            s_arr, t_arr = torch.full((B, 1), s, dtype=torch.int64), torch.full((B, 1), t, dtype=torch.int64)
            zz = orc.posterior_step(net_c.sd, net_c.cfg, s_arr / T, t_arr / T, zz, nm, em, ctx, raws[k], mol_shape=N,
                                    gammas=(gg[s].expand(B, 1), gg[t].expand(B, 1)))
        x, h = orc.final_decode(net_c.sd, net_c.cfg, zz, nm, em, ctx, raws[T], gamma_0=gg[0].expand(B, 1))
    assert torch.equal(got[2], zz) and torch.equal(got[0], x) and torch.equal(got[1], h)


def chain_pair(mols, few, w, phi, H, L):
    out = []
    for dtype in (torch.float32, torch.float64):
        model, gg, nm, em, ctx, ctx_u, net_c, net_u = setup(mols, H, L, dtype)
        B, N = nm.shape[:2]
        path = paths.build_path(T, few.get("steps"))
        raws = er.raw_draws(len(path), B, N, seed=len(path))
        z = start_state(nm)
        out.append(gr.guided_chain_ref(gr.GuidedNet(net_c, net_u, gr.scale_for(w, B), phi), gg, path, few["eta"], z, nm, raws))
    return out, nm


@pytest.mark.parametrize("H,L", [(32, 2), (128, 1)], ids=["H32L2", "H128L1"])
@pytest.mark.parametrize("case", gr.PARITY, ids=[c[0] for c in gr.PARITY])
def test_fp32_and_fp64_restatements_differ_by_a_tenth_of_the_bar(case, H, L):
    """Guidance amplifies round-off by about |w| + |w - 1|: a parity case whose own fp32 / fp64 gap came near the bar would test the
    arithmetic of the restatement, not the device.  Every GPU parity case must stay below a tenth of its bar here."""
    name, mols, few, w, phi = case
    (f32, f64), nm = chain_pair(mols, few, w, phi, H, L)
    nmf = nm.float().numpy()
    rx = rel_l2(f32[0].numpy() * nmf, f64[0].numpy() * nmf)
    rh = rel_l2(f32[1].numpy(), f64[1].numpy())
    rz = rel_l2(f32[2].numpy(), f64[2].numpy())
    print(f"{name} H={H}: fp32 vs fp64 x {rx:.2e} h {rh:.2e} z0 {rz:.2e} (bar / 10 = {gr.BAR / 10:.0e})")
    assert max(rx, rh, rz) < gr.BAR / 10


def test_combine_ref_rescale_and_degenerate_molecules():
    g = torch.Generator().manual_seed(1)
    nm, _ = orc.canonical_masks([7, 4, 1, 5])
    B, N = nm.shape[:2]
    ec = torch.randn(B, N, 11, generator=g, dtype=torch.float64) * nm.double()
    eu = torch.randn(B, N, 11, generator=g, dtype=torch.float64) * nm.double()
    eu[3] = ec[3]                                     # g == eps_c for any w ...
    ec[3] = ec[3, 0:1, 0:1] * nm[3].double()          # ... and constant over its valid entries: S_g = S_c = 0 -> factor 1
    eu[3] = ec[3]
    w = torch.tensor([2.5, -0.5, 3.0, 1.7])
    out1 = gr.combine_ref(ec, eu, w, 1.0, nm)
    out0 = gr.combine_ref(ec, eu, w, 0.0, nm)
    plain = (eu + w.double().view(B, 1, 1) * (ec - eu)) * nm.double()
    assert torch.allclose(out0, plain, rtol=0, atol=0)
    for b in range(3):
        valid = nm[b].expand(N, 11).bool()
        sd_c = float(torch.sqrt(((ec[b][valid] - ec[b][valid].mean()) ** 2).sum()))
        sd_o = float(torch.sqrt(((out1[b][valid] - out1[b][valid].mean()) ** 2).sum()))
        assert abs(sd_o - sd_c) <= 1e-12 * sd_c, (b, sd_o, sd_c)
        assert bool((out1[b][~valid] == 0).all())
    assert torch.equal(out1[3], plain[3])             # S_g = 0: factor 1
    # w = 1 / w = 0 ignore phi
    assert torch.equal(gr.combine_ref(ec, eu, 1.0, 0.7, nm), ec * nm.double())
    assert torch.equal(gr.combine_ref(ec, eu, 0.0, 0.7, nm), eu * nm.double())


def test_drop_context():
    nm, _ = orc.canonical_masks([7, 4, 1, 5, 6, 3])
    nm = nm.bool()
    B, N = nm.shape[:2]
    ctx = (torch.arange(1, B + 1).float().view(B, 1, 1).expand(B, N, 1) * nm.float()).contiguous()
    assert guidance.drop_context(ctx, 0.0, 0.0, nm) is ctx
    null = -2.5
    full = guidance.drop_context(ctx, 1.0, null, nm)
    assert torch.equal(full, torch.full((B, N, 1), null) * nm.float())
    a = guidance.drop_context(ctx, 0.5, null, nm, torch.Generator().manual_seed(11))
    b = guidance.drop_context(ctx, 0.5, null, nm, torch.Generator().manual_seed(11))
    assert torch.equal(a, b)
    kinds = set()
    for i in range(B):                                # whole molecules: every row of one is its own context or the null one
        own, dropped = torch.equal(a[i], ctx[i]), torch.equal(a[i], torch.full((N, 1), null) * nm[i].float())
        assert own or dropped
        kinds.add(dropped)
    assert kinds == {True, False}                     # seed 11 at p = 0.5 over six molecules draws both
    assert bool((a[~nm.expand(B, N, 1)] == 0).all())
    vec = guidance.drop_context(ctx.expand(B, N, 1), 1.0, [4.0], nm)
    assert torch.equal(vec, torch.full((B, N, 1), 4.0) * nm.float())
    with pytest.raises(ValueError):
        guidance.drop_context(ctx, 1.5, 0.0, nm)


def test_training_forward_drops_only_in_training_mode(monkeypatch):
    sd_np, _ = er.weights(32, 2, C_=1)
    model = er.cpu_diffusion(sd_np, 32, 2, T, C_=1)
    assert model.context_drop_prob == 0.0 and model.null_context == 0.0
    seen = []
    monkeypatch.setattr(type(model), "nll", lambda self, x, h, nm, em, context=None, mol_shape=None, **kw: (seen.append(context), torch.zeros(x.shape[0]))[1])
    x, h, nm, em, ctx = er.molecules([7, 4, 1], C_=1)
    batch = dict(positions=x, atom_mask=nm, edge_mask=em, node_feature=h, context=ctx)
    model.train()
    model.forward(batch)
    assert seen[-1] is ctx                            # p = 0: the very object
    model.context_drop_prob, model.null_context = 1.0, 0.5
    model.forward(batch)
    assert torch.equal(seen[-1], torch.full_like(ctx, 0.5) * nm.float())
    model.eval()
    model.forward(batch)
    assert seen[-1] is ctx                            # eval mode never drops


def test_python_entry_points_raise_on_bad_arguments_before_touching_the_gpu(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    sd_np, _ = er.weights(32, 2, C_=1)
    model = er.cpu_diffusion(sd_np, 32, 2, T, C_=1)
    x, h, nm, em, ctx = er.molecules([7, 4, 1], C_=1)
    B, N = nm.shape[:2]
    z = torch.zeros(B, N, 11)
    fm = torch.zeros(B, N, 1, dtype=torch.bool)
    mols = [{"x": x[i, :n], "h": h[i, :n], "context": ctx[i, :n]} for i, n in enumerate([7, 4, 1])]
    calls = {
        "sample_from_masks": lambda **kw: model.sample_from_masks(nm, None, ctx, **kw),
        "path_steps": lambda **kw: model.path_steps(z, nm, None, ctx, **kw),
        "sample_inpaint": lambda **kw: model.sample_inpaint(nm, fm, x, h, context=ctx, **kw),
        "sample_grow": lambda **kw: model.sample_grow([{"x": x[0, :2], "h": h[0, :2]}], 4, "cpu", context=0.3, **kw),
        "sample_from_latent": lambda **kw: model.sample_from_latent(z, nm, None, ctx, t_start=5, **kw),
        "vary": lambda **kw: model.vary(mols, "cpu", 5, **kw),
        "sample": lambda **kw: model.sample(B, "cpu", context=0.3, **kw),
        "sample_batches": lambda **kw: model.sample_batches(2, 2, "cpu", context_range=[0.1, 0.2], **kw),
    }
    for name, call in calls.items():
        for bad in (dict(guidance_scale=2.0, guidance_rescale=1.5), dict(guidance_scale=2.0, guidance_rescale=-0.1),
                    dict(guidance_scale=float("nan")), dict(guidance_scale=float("inf")), dict(guidance_scale=True),
                    dict(guidance_scale=torch.ones(2, 2))):
            with pytest.raises(ValueError):
                call(**bad)
        if name in ("sample_from_masks", "path_steps", "sample_inpaint", "sample_from_latent", "sample"):
            with pytest.raises(ValueError):
                call(guidance_scale=torch.ones(B + 1))            # one scale per molecule
            with pytest.raises(ValueError):
                call(guidance_scale=2.0, guidance_context=torch.zeros(B, N, 2))
        model.noise_mode = "torch"
        with pytest.raises(NotImplementedError):
            call(guidance_scale=2.0)
        model.noise_mode = "philox"
        model.dynamics.mode = "gnn_dynamics"
        with pytest.raises(NotImplementedError):
            call(guidance_scale=2.0)
        model.dynamics.mode = "egnn_dynamics"
        model.pocket = True
        with pytest.raises((NotImplementedError, ValueError)) as ei:
            call(guidance_scale=2.0)
        model.pocket = False
        if name in ("sample_from_masks", "path_steps", "sample", "sample_batches", "sample_grow"):
            assert ei.type is NotImplementedError
    # eta < 1 together with inpainting, as today
    with pytest.raises(ValueError):
        model.sample_inpaint(nm, fm, x, h, context=ctx, eta=0.5, guidance_scale=2.0)
    # the EDM signature
    from hierdiff_amd import EnVariationalDiffusion, default_config
    edm = EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=2, context_node_nf=1, timesteps=T))
    with pytest.raises(ValueError):
        edm.sample(B, N, nm, None, ctx, guidance_scale=2.0, guidance_rescale=2.0)
    # a model without context
    plain = er.cpu_diffusion(er.weights(32, 2)[0], 32, 2, T)
    with pytest.raises(ValueError):
        plain.sample_from_masks(nm, None, None, guidance_scale=2.0)
    with pytest.raises(ValueError):
        plain.sample(B, "cpu", guidance_scale=2.0)
    # a null context of the wrong width
    model.null_context = [0.0, 1.0]
    with pytest.raises(ValueError):
        model.sample_from_masks(nm, None, ctx, guidance_scale=2.0)


class _Reached(Exception):
    pass


def test_unguided_defaults_reach_no_guided_call(monkeypatch):
    """guidance_scale None and a scalar 1.0 take today's path: the stub library answers the unguided entry point and would fail on
    the guided one."""
    sd_np, _ = er.weights(32, 2, C_=1)
    model = er.cpu_diffusion(sd_np, 32, 2, T, C_=1)
    x, h, nm, em, ctx = er.molecules([7, 4, 1], C_=1)
    seen = []

    class Stub:
        def __getattr__(self, name):
            def f(*a):
                seen.append(name)
                if name in ("hd_sample_loop", "hd_sample_path", "hd_sample_path_guided"):
                    raise _Reached(name)
                return 0
            return f

    class FakeMask:                                       # a node mask that claims to live on a GPU
        def __init__(self, t):
            self.t = t
            self.shape, self.device = t.shape, torch.device("cuda", 0)

        def dim(self):
            return self.t.dim()

    monkeypatch.setattr(_lib, "load", lambda: Stub())
    monkeypatch.setattr(type(model), "_lib_handle", lambda self, synced=False: 1)
    monkeypatch.setattr(type(model), "_schedule", lambda self, rows=1: {"gamma": gamma_grid_fp64(model, T), "decode": torch.zeros(3)})
    monkeypatch.setattr(type(model), "_path_tables", lambda self, h, tabs, path, eta: {"K": len(path) - 1})
    monkeypatch.setattr(type(model.dynamics), "topology", lambda self, *a: type("Topo", (), {"ptr": 1})())
    monkeypatch.setattr(type(model), "_guide_device", lambda self, gd, nm_, dev: type("G", (), dict(
        ctx_u=torch.zeros(1), w=torch.zeros(1), rows=gd.rows, phi=gd.rescale))())
    import hierdiff_amd.diffusion as dmod
    monkeypatch.setattr(dmod, "_stream", lambda dev: 0)
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: torch.zeros(*a, **{k: v for k, v in kw.items() if k != "device"}))

    def run(**kw):
        seen.clear()
        with pytest.raises(_Reached) as ei:
            model.sample_from_masks(FakeMask(nm), None, type("Ctx", (), {"to": lambda self, *a: ctx})(), **kw)
        return str(ei.value)

    assert run() == "hd_sample_loop"
    assert run(guidance_scale=None) == "hd_sample_loop"
    assert run(guidance_scale=1.0) == "hd_sample_loop"
    assert run(guidance_scale=1.0, steps=5) == "hd_sample_path"
    assert run(guidance_scale=2.5) == "hd_sample_path_guided"
    assert run(guidance_scale=torch.ones(3)) == "hd_sample_path_guided"       # per molecule: a guided call even at 1
    assert run(guidance_scale=1.0, guidance_context=torch.zeros(3, 7, 1)) == "hd_sample_path_guided"
    model.guidance_scale = 2.5                             # the model's attribute is the keywords' default
    assert run() == "hd_sample_path_guided"


def test_cli_rejects_guidance_without_context():
    from hierdiff_amd.sampler import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--guidance", "2.0"])
    with pytest.raises(SystemExit):
        parse_args(["--context", "0.5", "--guidance-rescale", "0.5"])
    with pytest.raises(SystemExit):
        parse_args(["--context", "0.5", "--guidance", "2.0", "--guidance-rescale", "1.5"])
    args = parse_args(["--context", "0.5", "--guidance", "2.0", "--guidance-rescale", "0.7", "--null-context", "0.1", "--steps", "50"])
    assert args.guidance == 2.0 and args.guidance_rescale == 0.7 and args.null_context == [0.1] and args.steps == 50


def test_header_and_binding_declare_the_guidance_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hierdiff_hip.h")).read()
    for name in ("hd_guide_combine", "hd_sample_path_guided", "hd_guided_graph_builds"):
        assert name + "(" in header and name in _lib.SIGNATURES
    assert "#define HD_ABI_VERSION 12" in header
    assert "guided loops draw what their unguided loop draws" in header
