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


# ----------------------------------------------------------------------------- the layer's backward at training sizes
# (tests/fuzz_egcl_grads.py: generated cases against torch.autograd through the oracle in float64)
def _sweep(*args):
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_egcl_grads.py"), *args], cwd=root, capture_output=True,
                          text=True, timeout=900)
    tail = "\n".join(proc.stdout.splitlines()[-6:])
    print(tail)
    assert proc.returncode == 0, tail + proc.stderr[-2000:]
    assert "failures 0, skipped 0" in tail, tail


def test_randomised_layer_gradient_sweep():
    """tests/fuzz_egcl_grads.py, default tier (40 cases, seed 17: M <= 40, E <= 4 M) and `big` tier (12 cases, seed 23: E around 512,
    1024, 8192 and 20,000..30,000 rows, M up to 1,100 - split-K weight gradients, the LDS-tiled GEMM on edge rows, node reductions in
    slabs): every gradient within `_close` of float64 autograd, forward values within 1e-5.  The float32 oracle passes the same cases
    at one tenth of these bars (profiles/fuzz_egcl_grads_oracle_only.log), so the inputs leave the tolerance to the kernels.
    Measured on an MI355X (profiles/fuzz_egcl_grads_gpu.log): worst gradient rel-L2 2.15e-6 (default) / 2.05e-6 (big), worst value
    rel-L2 4.9e-7 / 9.2e-7; 6.5 s of wall time for both tiers (1 s + 2 s in the cases, the rest starting two interpreters), next to
    17 s for every earlier GPU test of this file, test_gpu_training.py and test_gpu_refine.py together."""
    _sweep("40", "17")
    _sweep("12", "23", "big")


def _edge_case(kind, n, lean, seed=0):
    """Deterministic graphs at the sizes where hd_egcl_backward changes path, H = 64.  lean: De = 1, no edge / coordinate update."""
    from tests import fuzz_egcl_grads as fz
    rng = np.random.Generator(np.random.PCG64([77, n, int(lean), seed]))
    if kind == "E":                  # split-K of the edge-row weight gradients starts at 512 rows and reaches 32 slabs at 8192
        M = 96
        row, col = fz.sparse_graph(rng, M, n, self_edges=True)
    elif kind == "M":                # the node-level weight gradients split at M >= 512
        M = n
        row, col = fz.sparse_graph(rng, M, 2 * M + 3, self_edges=True)
    else:                            # "hub": isolated / send-only / receive-only nodes and a hub on 40 % of about 3,000 edges
        M = 300
        row, col = fz.ragged_graph(rng, M, n, self_edges=True)
    kw = dict(H=64, De=1, eu=False, cu=False) if lean else dict(H=64, De=64, eu=True, cu=True)
    return fz.make_case(rng, ctx=2, att=True, rec=True, tanh=True, M=M, row=row, col=col, nm=True, em=True, weight_seed=400 + n, **kw)


def _check_case(c, name):
    from tests import fuzz_egcl_grads as fz
    routs, ref = fz.oracle_grads(c)
    outs, got = fz.hip_grads(c)
    assert len(outs) == len(routs) and set(got) == set(ref)
    for i, (a, b) in enumerate(zip(outs, routs)):
        r = float((a.double() - b).norm() / max(float(b.norm()), 1e-30))
        assert r <= 1e-5, f"{name} output {i}: rel-L2 {r:.2e}"
    scale = fz.grad_scale(c, ref)
    for k, r in ref.items():
        _close(got[k], r, f"{name} d[{k}]", scale)
    return got, ref


EDGE_CASES = ([("E", n, lean) for n in (511, 512, 513, 8191, 8192, 8193) for lean in (False, True)]
              + [("M", n, False) for n in (511, 512, 513, 1025)] + [("hub", 3001, False)])


@pytest.mark.parametrize("kind,n,lean", EDGE_CASES)
def test_layer_gradients_at_the_path_changes(kind, n, lean):
    """E in {511, 512, 513, 8191, 8192, 8193} with every option on and again with De = 1 and no edge / coordinate update, M in
    {511, 512, 513, 1025} with about 2 M edges, and the hub / isolated-node graph at E = 3,001."""
    c = _edge_case(kind, n, lean)
    if kind == "hub":
        deg = torch.bincount(torch.cat([c["row"], c["col"]]), minlength=c["M"])
        assert int((deg == 0).sum()) > 0 and int(deg.max()) >= c["E"] // 3
        assert int((torch.bincount(c["row"], minlength=c["M"]) == 0).sum()) > int((deg == 0).sum())
    _check_case(c, f"{kind}={n}{' lean' if lean else ''}")


def test_backward_is_bit_reproducible_with_split_k():
    """The header's "deterministic" at a size where every edge-row weight gradient is a split-K sum of 32 slabs (E = 8193)."""
    from tests import fuzz_egcl_grads as fz
    c = _edge_case("E", 8193, False)
    m = fz.hip_layer(c)
    _, g1 = fz.hip_grads(c, m)
    _, g2 = fz.hip_grads(c, m)
    _, g3 = fz.hip_grads(c, fz.hip_layer(c))              # ... and across two handles / graphs
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and torch.equal(g1[k], g3[k]), k


def _abi_layer_step(m, c, douts, want_dea=True, null_edges=False):
    """hd_egcl_forward_train + hd_egcl_backward through ctypes.  douts: dh_out, dx_out, dedge_attr_out device tensors or None (NULL).
    The gradient buffers start as NaN.  null_edges: NULL for every zero-length edge tensor (E = 0)."""
    from hierdiff_amd import _lib
    lib = _lib.load()
    hd = m._handle()
    m._sync_weights()
    g = m._graph(c["row"], c["col"], c["M"])
    d = lambda t: None if t is None else t.to(DEV).reshape(-1).contiguous()
    h, x, ea, nm, em = c["h"].to(DEV), c["x"].to(DEV), c["ea"].to(DEV), d(c["nm"]), d(c["em"])
    saved = torch.empty(int(lib.hd_egcl_saved_floats(hd, g.M, g.E)), device=DEV)
    h_out, x_out = torch.full_like(h, float("nan")), torch.full_like(x, float("nan"))
    ea_out = torch.full((g.E, c["H"]), float("nan"), device=DEV) if c["eu"] else None
    p = lambda t: None if t is None or (null_edges and t.numel() == 0) else t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hd_egcl_forward_train(hd, g._h, p(h), p(x), p(ea), p(nm), p(em), p(h_out), p(x_out), p(ea_out), p(saved), s),
               "hd_egcl_forward_train")
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    dh, dx, dw = nan(*h.shape), nan(*x.shape), nan(int(lib.hd_egcl_weight_count(hd)))
    dea = nan(*ea.shape) if want_dea else None
    _lib.check(lib.hd_egcl_backward(hd, g._h, p(h), p(x), p(ea), p(nm), p(em), p(saved), p(douts[0]), p(douts[1]), p(douts[2]),
                                    p(dh), p(dx), p(dea), p(dw), s), "hd_egcl_backward")
    torch.cuda.synchronize()
    grads = {"h": dh, "x": dx}
    if want_dea:
        grads["edge_attr"] = dea
    off = 0
    for k, q in m.named_parameters():
        grads[k] = dw[off:off + q.numel()].view(q.shape)
        off += q.numel()
    assert off == dw.numel()
    return [o for o in (h_out, x_out, ea_out) if o is not None], grads


@pytest.mark.parametrize("full", [True, False])
def test_c_abi_null_upstream_gradients_are_zeros(full):
    """include/hierdiff_hip.h: dh_out, dx_out and dedge_attr_out "may be NULL = zero".  torch.autograd always hands tensors, so only
    the C ABI takes these branches: each NULL in turn (and none) on NaN-filled result buffers - every element written, the bits of
    the call with an explicit zero tensor, and the float64 oracle's gradients - for a layer with every option on and one with none."""
    from tests import fuzz_egcl_grads as fz
    rng = np.random.Generator(np.random.PCG64([78, int(full)]))
    M, E = 50, 300
    row, col = fz.sparse_graph(rng, M, E, self_edges=True)
    if full:
        c = fz.make_case(rng, H=64, De=64, ctx=2, att=True, eu=True, cu=True, rec=True, tanh=True, M=M, row=row, col=col, nm=True,
                         em=True, weight_seed=31)
    else:
        c = fz.make_case(rng, H=64, De=1, ctx=0, att=False, eu=False, cu=False, rec=False, tanh=False, M=M, row=row, col=col,
                         weight_seed=32)
    m = fz.hip_layer(c)
    ups = [u.to(DEV) for u in c["ups"]]
    n_out = len(ups)
    for missing in [None] + list(range(n_out)):
        given = [u if i != missing else None for i, u in enumerate(ups)] + [None] * (3 - n_out)
        zeros = [u if i != missing else torch.zeros_like(u) for i, u in enumerate(ups)] + [None] * (3 - n_out)
        outs_a, ga = _abi_layer_step(m, c, given)
        outs_b, gb = _abi_layer_step(m, c, zeros)
        c["only"] = None if missing is None else tuple(i for i in range(n_out) if i != missing)
        routs, ref = fz.oracle_grads(c)
        scale = fz.grad_scale(c, ref)
        for a, b in zip(outs_a, routs):
            assert float((a.cpu().double() - b).norm()) <= 1e-5 * float(b.norm())
        assert set(ga) == set(ref)
        for k in ga:
            assert bool(torch.isfinite(ga[k]).all()), f"missing={missing} d[{k}]: an element was left unwritten"
            assert torch.equal(ga[k], gb[k]), f"missing={missing} d[{k}]: NULL and an explicit zero tensor differ"
            _close(ga[k], ref[k], f"missing={missing} d[{k}]", scale)


@pytest.mark.parametrize("full", [True, False])
def test_layer_on_a_graph_without_edges(full):
    """E = 0 (a valid hd_egcl_graph): only the node model has a gradient - every edge-model, coordinate-model and attention parameter
    gradient is exactly 0, dx = dx_out * node_mask - through the Python layer (zero-length tensors: NULL data pointers) and through
    the C ABI with NULL for the zero-length edge tensors."""
    from tests import fuzz_egcl_grads as fz
    rng = np.random.Generator(np.random.PCG64([79, int(full)]))
    M = 37
    none = torch.zeros(0, dtype=torch.long)
    kw = dict(H=64, De=64, eu=True, ctx=2) if full else dict(H=32, De=1, eu=False, ctx=0)
    c = fz.make_case(rng, att=True, cu=True, rec=True, tanh=True, M=M, row=none, col=none, nm=True, em=None, weight_seed=33, **kw)
    got, ref = _check_case(c, "E=0")
    m = fz.hip_layer(c)
    _, abi = _abi_layer_step(m, c, [u.to(DEV) for u in c["ups"]] + [None] * (3 - len(c["ups"])), null_edges=True)
    scale = fz.grad_scale(c, ref)
    for name, g in (("layer", got), ("C ABI", abi)):
        for k, v in g.items():
            if k.split(".")[0] in ("mes_mlp", "edge_mlp", "coord_mlp", "att_mlp"):
                assert float(v.abs().max()) == 0.0, f"{name} d[{k}]"
            if k.startswith("node_mlp"):
                assert float(v.abs().max()) > 0.0, f"{name} d[{k}]"
            _close(v, ref[k], f"E=0 {name} d[{k}]", scale)
        assert torch.equal(g["x"].cpu(), c["ups"][1] * c["nm"]), name
        assert g["edge_attr"].shape == (0, c["De"])
