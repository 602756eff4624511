"""Stage-2 training on the GPU: the backward of E_GCL (hd_egcl_forward_train / hd_egcl_backward through
hierdiff_amd.stage2.E_GCL under autograd), Edge_denoise.training_forward and the EdgeDenoise training module, against
torch.autograd through the CPU oracles (oracle/egnn_oracle.py:e_gcl_forward, oracle/edge_denoise_oracle.py:forward)."""
import copy

import numpy as np
import pytest
import torch

from oracle import edge_denoise_oracle as edo
from oracle import egnn_oracle as orc
from tests.helpers import load

pytestmark = [pytest.mark.gpu, pytest.mark.autograd]

DEV = "cuda:0"
TOL = 1e-4
F15 = ["f15_egcl_full_h64", "f15_egcl_full_h256", "f15_egcl_focal_h64", "f15_egcl_edge_h64", "f15_egcl_ctx_h64",
       "f15_egcl_geo_h64"]


def _close(got, ref, what, scale, tol=TOL):
    """rel-L2 bar with the absolute floor of tests/test_gpu_training.py:_compare_grads for tensors whose gradient is ~0."""
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    err = np.linalg.norm(got - ref)
    bound = tol * np.linalg.norm(ref) + 1e-7 * scale * np.sqrt(ref.size)
    assert err <= bound, f"{what}: |diff| {err:.3e} > {bound:.3e} (|ref| {np.linalg.norm(ref):.3e})"


def _layer_case(name):
    """(layer kwargs, state dict, inputs) of an F15 fixture, or of the tanh=False / recurrent=False variant of full_h64."""
    from hierdiff_amd.stage2 import synthetic_egcl_state_dict
    plain = name.endswith(":plain")
    fx = load(name.split(":")[0])
    H, De, ctx = int(fx["hidden_nf"]), int(fx["edges_in_d"]), int(fx["context_nf"])
    att, eu = bool(int(fx["attention"])), bool(int(fx["edge_update"]))
    geo = bool(int(fx.get("geo", 0)))
    sd_np = synthetic_egcl_state_dict(H, De, ctx, att, eu, int(fx["weight_seed"]), coord_gain=0.3)
    kw = dict(context_nf=ctx, edges_in_d=De, attention=att, tanh=not plain, coords_range=30, edge_update=eu, geo=geo,
              recurrent=not plain)
    cfg = orc.EGCLCfg(hidden_nf=H, edges_in_d=De, context_nf=ctx, attention=att, edge_update=eu, geo=geo, tanh=not plain,
                      recurrent=not plain)
    nm = torch.from_numpy(fx["node_mask"]) if int(fx["masked"]) else None
    em = torch.from_numpy(fx["edge_mask"]) if int(fx["has_edge_mask"]) else None
    inp = dict(h=torch.from_numpy(fx["h"]), x=torch.from_numpy(fx["x"]), ea=torch.from_numpy(fx["edge_attr"]),
               row=torch.from_numpy(fx["row"]).long(), col=torch.from_numpy(fx["col"]).long(), nm=nm, em=em)
    return H, kw, cfg, sd_np, inp


def _hip_layer(H, kw, sd_np):
    from hierdiff_amd.stage2 import E_GCL
    m = E_GCL(H, H, H, **kw)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
    return m.to(DEV)


def _run_hip(m, inp, ups):
    g = lambda t: None if t is None else t.to(DEV)
    h, x, ea = (inp[k].to(DEV).requires_grad_(True) for k in ("h", "x", "ea"))
    outs = m(h, [g(inp["row"]), g(inp["col"])], x, edge_attr=ea, node_mask=g(inp["nm"]), edge_mask=g(inp["em"]))
    loss = sum((o * u.to(DEV)).sum() for o, u in zip(outs, ups))
    m.zero_grad(set_to_none=True)
    loss.backward()
    return outs, (h.grad, x.grad, ea.grad), {k: p.grad for k, p in m.named_parameters()}


def _upstream(outs, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)) for o in outs]


@pytest.mark.parametrize("name", F15 + ["f15_egcl_full_h64:plain"])
def test_layer_gradients_match_autograd_through_the_oracle(name):
    H, kw, cfg, sd_np, inp = _layer_case(name)
    sd = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in sd_np.items()}
    h, x, ea = (inp[k].clone().requires_grad_(True) for k in ("h", "x", "ea"))
    ref = [o for o in orc.e_gcl_forward(sd, cfg, h, inp["row"], inp["col"], x, ea, inp["nm"], inp["em"]) if o is not None]
    ups = _upstream(ref, 7)
    sum((o * u).sum() for o, u in zip(ref, ups)).backward()
    m = _hip_layer(H, kw, sd_np)
    outs, gin, gpar = _run_hip(m, inp, ups)
    assert len(outs) == len(ref)
    scale = max(float(v.grad.abs().max()) for v in sd.values())
    for what, got, r in zip(("h", "x", "edge_attr"), gin, (h.grad, x.grad, ea.grad)):
        _close(got, r, f"{name} d{what}", scale)
    for k, v in sd.items():
        assert gpar[k] is not None, k
        _close(gpar[k], v.grad, f"{name} d[{k}]", scale)


@pytest.mark.parametrize("name", ["f15_egcl_full_h256", "f15_egcl_ctx_h64", "f15_egcl_edge_h64"])
def test_forward_under_autograd_is_the_inference_forward_and_backward_is_deterministic(name):
    H, kw, cfg, sd_np, inp = _layer_case(name)
    m = _hip_layer(H, kw, sd_np)
    g = lambda t: None if t is None else t.to(DEV)
    args = (inp["h"].to(DEV), [g(inp["row"]), g(inp["col"])], inp["x"].to(DEV))
    kwargs = dict(edge_attr=inp["ea"].to(DEV), node_mask=g(inp["nm"]), edge_mask=g(inp["em"]))
    with torch.no_grad():
        value = m(*args, **kwargs)
    ups = _upstream(value, 11)
    outs1, gin1, gpar1 = _run_hip(m, inp, ups)
    outs2, gin2, gpar2 = _run_hip(m, inp, ups)
    assert all(o.grad_fn is not None for o in outs1)
    assert all(torch.equal(a, b) for a, b in zip(outs1, value)), "forward_train must give the inference bits"
    assert all(torch.equal(a, b) for a, b in zip(gin1, gin2))
    assert all(torch.equal(gpar1[k], gpar2[k]) for k in gpar1)


def test_gradients_accumulate_over_repeated_applications():
    """One layer applied twice in a chain (what Edge_denoise does with gcl_edge / gcl_denoise along the breadth-first layers)."""
    H, kw, cfg, sd_np, inp = _layer_case("f15_egcl_edge_h64")
    sd = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in sd_np.items()}
    h = inp["h"].clone().requires_grad_(True)
    h1, x1, _ = orc.e_gcl_forward(sd, cfg, h, inp["row"], inp["col"], inp["x"], inp["ea"], inp["nm"], inp["em"])
    h2, x2, _ = orc.e_gcl_forward(sd, cfg, h1, inp["col"], inp["row"], x1, inp["ea"], inp["nm"], inp["em"])
    (h2.square().sum() + x2.sum()).backward()
    m = _hip_layer(H, kw, sd_np)
    g = lambda t: None if t is None else t.to(DEV)
    hg = inp["h"].to(DEV).requires_grad_(True)
    ea = inp["ea"].to(DEV)
    a1, b1 = m(hg, [g(inp["row"]), g(inp["col"])], inp["x"].to(DEV), edge_attr=ea, node_mask=g(inp["nm"]))
    a2, b2 = m(a1, [g(inp["col"]), g(inp["row"])], b1, edge_attr=ea, node_mask=g(inp["nm"]))
    (a2.square().sum() + b2.sum()).backward()
    scale = max(float(v.grad.abs().max()) for v in sd.values())
    _close(hg.grad, h.grad, "dh", scale)
    for k, p in m.named_parameters():
        _close(p.grad, sd[k].grad, f"d[{k}]", scale)


# ----------------------------------------------------------------------------- whole model
FWD = ["f17_fwd_h64", "f17_fwd_h256", "f17_fwd_ctx_h64", "f17_fwd_array_h64", "f17_fwd_first_edges_h64"]


def _fx_model(name, tmp_path):
    from tests.test_edge_denoise import _array_dict, _cfg, _module, _train_batch, _weights
    fx = load(name)
    return fx, _module(fx, tmp_path), _train_batch(fx), _weights(fx), _cfg(fx), _array_dict(fx)


@pytest.mark.parametrize("name", FWD)
def test_model_gradients_match_autograd_through_the_oracle(name, tmp_path):
    fx, m, batch, w, cfg, ad = _fx_model(name, tmp_path)
    sd = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in w.items()}
    ref = edo.forward.__wrapped__(sd, cfg, copy.deepcopy(batch), array_dict=ad)
    ref["total_loss"].backward()
    m = m.to(DEV).train()
    out = m.training_forward(copy.deepcopy(batch))
    out["total_loss"].backward()
    for k in ("focal_loss", "edge_loss", "node_loss", "total_loss"):
        assert abs(float(out[k].detach()) - float(ref[k].detach())) <= 1e-4 * max(1.0, abs(float(ref[k]))), k
    scale = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    for k, p in m.named_parameters():
        r = sd[k].grad
        if r is None:                    # no path from this parameter to the loss in the reference (e.g. the last focal layer's edge model)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        _close(p.grad, r, f"{name} d[{k}]", scale)


@pytest.mark.parametrize("name", ["f17_fwd_h64", "f17_fwd_ctx_h64"])
def test_training_forward_losses_agree_with_forward(name, tmp_path):
    fx, m, batch, *_ = _fx_model(name, tmp_path)
    m = m.to(DEV)
    with torch.no_grad():
        val = m.eval()(copy.deepcopy(batch))
    tr = m.train().training_forward(copy.deepcopy(batch))
    assert tr["total_loss"].requires_grad
    for k in val:
        a, b = float(tr[k]), float(val[k])
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (k, a, b)


def test_edge_denoise_module_trains(tmp_path):
    """Five optimisation steps of the training module on one batch (trainer.ddp_step, clip 1.0 as conf/trainer/default.yaml),
    from the module's own initialisation - the reference's (torch defaults, coord_mlp.2 at xavier gain 0.001) - like a run of
    train_edge_denoise_pl.py starts."""
    from hierdiff_amd.edge_denoise_train import CLIP_VAL, EdgeDenoise
    from hierdiff_amd.trainer import ddp_step
    from tests.test_edge_denoise import _kw
    fx, m0, batch, w, *_ = _fx_model("f17_fwd_h64", tmp_path)
    torch.manual_seed(0)
    mod = EdgeDenoise({"model": dict(array_dict=None, full_softmax=True, focal_loss=5, edge_loss=1, node_loss=2, **_kw(fx))})
    mod = mod.to(DEV)
    [opt], [sched] = mod.configure_optimizers()
    losses = []
    for _ in range(5):
        r = ddp_step(mod, copy.deepcopy(batch), opt, clip_val=CLIP_VAL, overlap=False)
        losses.append(float(r["loss"]))
        assert np.isfinite(float(r["grad_norm"]))
        assert all(torch.isfinite(p.grad).all() for p in mod.parameters() if p.grad is not None)
    assert losses[-1] < losses[0], losses
    mod.training_epoch_end([])
    assert opt.param_groups[0]["lr"] == pytest.approx(4e-4)


def test_stage2_step_launches_no_blas_library_kernel(tmp_path):
    from torch.profiler import ProfilerActivity, profile
    fx, m, batch, *_ = _fx_model("f17_fwd_h64", tmp_path)
    m = m.to(DEV).train()
    m.training_forward(copy.deepcopy(batch))["total_loss"].backward()          # warm-up: graphs, weight images
    m.zero_grad(set_to_none=True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        m.training_forward(copy.deepcopy(batch))["total_loss"].backward()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    blas = [n for n in names if n.startswith("Cijk_") or "rocblas" in n.lower() or "hipblas" in n.lower()]
    assert not blas, blas
    for k in ("k_tgemm", "k_egcl_bgate", "k_egcl_bgeo", "k_egcl_bnode_out"):
        assert any(k in n for n in names), k
