"""Refine model on the GPU: the new kernels (size-restricted softmax head, embedding gather, squared-distance edge attribute) against
torch, Node2Vec.forward / check_node / check_tree against the fixtures recorded from the reference, every parameter's gradient
against torch.autograd through tests/refine_oracle.py, determinism, the training module and the kernels a training step launches."""
import copy

import numpy as np
import pytest
import torch

from tests import refine_oracle as ro

pytestmark = [pytest.mark.gpu]

DEV = "cuda:0"
TRAIN = ["r1_refine_train_h64", "r2_refine_train_h256"]
CHECK = ["r3_refine_check_h64_k1", "r4_refine_check_h64_k3"]


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _close(got, ref, what, scale, tol=1e-4):
    """rel-L2 bar with the absolute floor of tests/test_gpu_stage2_training.py:_close."""
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    err = np.linalg.norm(got - ref)
    bound = tol * np.linalg.norm(ref) + 1e-7 * scale * np.sqrt(ref.size)
    assert err <= bound, f"{what}: |diff| {err:.3e} > {bound:.3e} (|ref| {np.linalg.norm(ref):.3e})"


def _model(fx):
    from hierdiff_amd.refine import Node2Vec
    size_dict, _ = ro.load_size_dict()
    H = int(fx["hidden"])
    m = Node2Vec(size_dict, 780, 8, H, 2)
    sd = {k: torch.from_numpy(v.copy()) for k, v in _weights(fx).items()}
    m.load_state_dict(sd)
    return m.to(DEV)


def _weights(fx):
    from hierdiff_amd.refine import synthetic_refine_state_dict
    return synthetic_refine_state_dict(780, 8, int(fx["hidden"]), 2, int(fx["weight_seed"]))


# ----------------------------------------------------------------------------- kernels
def _xent_case(sets, B_per_set=2, ncols=1000, seed=0, ties=False):
    from hierdiff_amd.refine import CandTable
    rng = np.random.Generator(np.random.PCG64(seed))
    logits = rng.standard_normal((B_per_set * len(sets), ncols)).astype(np.float32)
    if ties:
        logits = np.round(logits * 2) / 2                         # many exactly equal values
    set_idx = np.repeat(np.arange(len(sets)), B_per_set).astype(np.int32)
    target = np.asarray([sets[s][int(rng.integers(0, len(sets[s])))] for s in set_idx], np.int32)
    table = CandTable(sets, ncols, DEV)
    return logits, set_idx, target, table


def _sets(seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [list(rng.permutation(1000)[:n]) for n in (224, 1, 300, 7)]


def test_cand_xent_forward_against_torch():
    from hierdiff_amd.refine import cand_xent_forward
    sets = _sets()
    k = 5
    logits, set_idx, target, table = _xent_case(sets)
    B = logits.shape[0]
    lg = torch.from_numpy(logits).to(DEV)
    logp = torch.empty(B, device=DEV)
    hit = torch.empty(B, device=DEV, dtype=torch.int32)
    topk = torch.empty((B, k), device=DEV, dtype=torch.int32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    cand_xent_forward(lg, table, torch.from_numpy(set_idx).to(DEV), torch.from_numpy(target).to(DEV), k, logp, hit, topk, err)
    assert int(err.cpu()) == 0
    logp, hit, topk = logp.cpu().numpy(), hit.cpu().numpy(), topk.cpu().numpy()
    for b in range(B):
        c = sets[set_idx[b]]
        row = torch.from_numpy(logits[b, c])
        ref = torch.log_softmax(row, dim=0)[c.index(target[b])]
        assert abs(float(logp[b]) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), b
        assert hit[b] == int(int(torch.argmax(row)) == c.index(target[b]))
        kk = min(k, len(c))
        want = [c[int(j)] for j in torch.topk(row, kk)[1]]
        assert list(topk[b, :kk]) == want, b
        assert (topk[b, kk:] == -1).all()


def test_cand_xent_ties_follow_the_lower_position():
    from hierdiff_amd.refine import CandTable, cand_xent_forward
    sets = [[9, 4, 7, 2, 5], list(range(300))]
    logits = np.zeros((2, 400), np.float32)
    logits[0, [9, 4, 7, 2, 5]] = [1.0, 3.0, 3.0, 1.0, 3.0]
    logits[1, :300] = np.repeat(np.arange(100), 3)[::-1] * 0.25          # triples of equal values
    table = CandTable(sets, 400, DEV)
    k = 6
    logp = torch.empty(2, device=DEV)
    hit = torch.empty(2, device=DEV, dtype=torch.int32)
    topk = torch.empty((2, k), device=DEV, dtype=torch.int32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    cand_xent_forward(torch.from_numpy(logits).to(DEV), table, torch.tensor([0, 1], dtype=torch.int32, device=DEV),
                      torch.tensor([7, 1], dtype=torch.int32, device=DEV), k, logp, hit, topk, err)
    topk, hit = topk.cpu().numpy(), hit.cpu().numpy()
    assert list(topk[0]) == [4, 7, 5, 9, 2, -1]                 # value descending, equal values by position in the set
    assert list(topk[1]) == [0, 1, 2, 3, 4, 5]
    assert hit[0] == 0 and hit[1] == 0                          # argmax = the first of the tied maxima (torch.argmax's rule)
    assert int(torch.argmax(torch.from_numpy(logits[0, sets[0]]))) == 1


@pytest.mark.autograd
def test_cand_xent_gradient_against_autograd():
    from hierdiff_amd.refine import CandXent
    sets = _sets(2)
    logits, set_idx, target, table = _xent_case(sets, seed=3)
    w = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).standard_normal(logits.shape[0]).astype(np.float32))
    lg = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    logp, flags = CandXent.apply(lg, table, torch.from_numpy(set_idx).to(DEV), torch.from_numpy(target).to(DEV))
    (logp * w.to(DEV)).sum().backward()
    ref_lg = torch.from_numpy(logits).double().requires_grad_(True)
    tot = 0
    for b in range(logits.shape[0]):
        c = sets[set_idx[b]]
        tot = tot + w[b].double() * torch.log_softmax(ref_lg[b, c], dim=0)[c.index(target[b])]
    tot.backward()
    assert int(flags[-1]) == 0
    np.testing.assert_allclose(lg.grad.cpu().numpy(), ref_lg.grad.numpy(), rtol=0, atol=2e-6)
    off = np.ones(logits.shape, bool)
    for b in range(logits.shape[0]):
        off[b, sets[set_idx[b]]] = False
    assert (lg.grad.cpu().numpy()[off] == 0).all()


def test_cand_xent_reports_a_target_outside_its_set():
    from hierdiff_amd.refine import CandTable, cand_xent_forward
    table = CandTable([[1, 2, 3]], 8, DEV)
    logp = torch.empty(1, device=DEV)
    hit = torch.empty(1, device=DEV, dtype=torch.int32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    cand_xent_forward(torch.zeros((1, 8), device=DEV), table, torch.zeros(1, dtype=torch.int32, device=DEV),
                      torch.tensor([5], dtype=torch.int32, device=DEV), 0, logp, hit, None, err)
    assert int(err.cpu()) == 1


@pytest.mark.autograd
def test_embed_kernels_against_torch_and_deterministic():
    from hierdiff_amd.refine import _InputStage
    rng = np.random.Generator(np.random.PCG64(5))
    M, H, F = 300, 64, 8
    v = torch.from_numpy(rng.integers(0, 20, M)).to(DEV)              # few ids: many rows per id
    s = torch.from_numpy(rng.integers(0, 26, M)).to(DEV)
    f = torch.from_numpy(rng.standard_normal((M, F)).astype(np.float32)).to(DEV)
    prm = [torch.from_numpy(rng.standard_normal(shp).astype(np.float32)).to(DEV).requires_grad_(True)
           for shp in ((781, H), (26, H), (H, F), (H,), (H, H), (H,))]
    up = torch.from_numpy(rng.standard_normal((M, 3 * H)).astype(np.float32)).to(DEV)

    def run():
        for p in prm:
            p.grad = None
        comb, bad = _InputStage.apply(v, s, f, *prm)
        (comb * up).sum().backward()
        return comb.detach(), int(bad.cpu()), [p.grad.clone() for p in prm]
    comb, bad, g1 = run()
    _, _, g2 = run()
    assert bad == 0
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    cp = [p.detach().cpu().double().requires_grad_(True) for p in prm]
    ref = torch.cat([cp[0][v.cpu()], torch.nn.functional.linear(torch.nn.functional.silu(
        torch.nn.functional.linear(f.cpu().double(), cp[2], cp[3])), cp[4], cp[5]), cp[1][s.cpu()]], dim=1)
    (ref * up.cpu().double()).sum().backward()
    assert _rel(comb.cpu(), ref.detach()) < 1e-6
    for i, (a, b) in enumerate(zip(g1, cp)):
        assert _rel(a.cpu(), b.grad) < 1e-5, i


def test_embed_kernel_flags_an_out_of_range_id():
    from hierdiff_amd.refine import _input_forward
    H = 32
    v = torch.tensor([0, 781], device=DEV)
    s = torch.tensor([0, 1], device=DEV)
    z = lambda *shp: torch.zeros(shp, device=DEV)
    comb, bad, _, _ = _input_forward(v, s, z(2, 8), z(781, H), z(26, H), z(H, 8), z(H), z(H, H), z(H))
    assert int(bad.cpu()) == 1 and float(comb[1, :H].abs().sum()) == 0.0


@pytest.mark.autograd
def test_sqdist_kernels_against_torch_and_deterministic():
    from hierdiff_amd.refine import _SqDist
    from hierdiff_amd.stage2 import E_GCL
    rng = np.random.Generator(np.random.PCG64(6))
    M, E = 40, 90
    row = torch.from_numpy(rng.integers(0, M, E).astype(np.int32))
    col = torch.from_numpy(rng.integers(0, M, E).astype(np.int32))
    layer = E_GCL(32, 32, 32, edges_in_d=1, attention=True, tanh=True, coords_range=30, edge_update=False).to(DEV)
    g = layer._graph(row, col, M)
    x0 = rng.standard_normal((M, 3)).astype(np.float32)
    up = torch.from_numpy(rng.standard_normal((E, 1)).astype(np.float32))
    grads = []
    for _ in range(2):
        x = torch.from_numpy(x0).to(DEV).requires_grad_(True)
        ea = _SqDist.apply(g, x)
        (ea * up.to(DEV)).sum().backward()
        grads.append(x.grad.clone())
    xr = torch.from_numpy(x0).double().requires_grad_(True)
    ref = ((xr[row.long()] - xr[col.long()]) ** 2).sum(1, keepdim=True)
    (ref * up.double()).sum().backward()
    assert _rel(ea.detach().cpu(), ref.detach()) < 1e-6
    assert _rel(grads[0].cpu(), xr.grad) < 1e-5
    assert torch.equal(grads[0], grads[1])


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", TRAIN)
def test_forward_matches_the_reference_fixtures(name):
    fx = ro.load(name)
    m = _model(fx)
    out = m(ro.train_batch(fx))
    assert _rel(float(out["loss"]), float(fx["loss"])) <= 1e-4
    assert float(out["accuracy"]) == pytest.approx(float(fx["accuracy"]))


@pytest.mark.autograd
@pytest.mark.parametrize("name", TRAIN)
def test_parameter_gradients_match_autograd_through_the_oracle(name):
    fx = ro.load(name)
    size_dict, _ = ro.load_size_dict()
    sd = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in _weights(fx).items()}
    ref = ro.forward(sd, size_dict, 2, ro.train_batch(fx))
    ref["loss"].backward()
    m = _model(fx).train()
    out = m(ro.train_batch(fx))
    assert out["loss"].requires_grad
    assert _rel(float(out["loss"]), float(ref["loss"])) <= 1e-4
    out["loss"].backward()
    scale = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    for k, p in m.named_parameters():
        r = sd[k].grad
        if r is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        _close(p.grad, r, f"{name} d[{k}]", scale)


@pytest.mark.autograd
def test_gradients_are_bit_identical_across_steps():
    fx = ro.load("r1_refine_train_h64")
    m = _model(fx).train()
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m(ro.train_batch(fx))["loss"].backward()
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])


def _check_node(name):
    fx = ro.load(name)
    _, mol_sizes = ro.load_size_dict()
    nodes = ro.tree_nodes(fx)
    m = _model(fx)
    res = m.check_node(ro.StubVocab(mol_sizes), nodes, fx["edges"], list(range(len(nodes))), [nd.wid for nd in nodes], DEV,
                       int(fx["check_num"]))
    return fx, res


@pytest.mark.parametrize("name", CHECK)
def test_check_node_matches_the_reference_fixtures(name):
    fx, res = _check_node(name)
    logp = np.asarray([float(r[0]) for r in res])
    assert _rel(logp, fx["logp"]) <= 1e-4
    for i, r in enumerate(res):
        k = int(fx["ks"][i])
        if k == 1:
            assert isinstance(r[1], tuple)
            opts = [r[1]]
        else:
            assert isinstance(r[1], list)
            opts = r[1]
        assert [int(w) for _, w in opts] == list(fx["ids"][i, :k]), i
        assert [int(bool(f)) for f, _ in opts] == list(fx["flags"][i, :k]), i


def test_check_tree_matches_the_reference_fixture():
    from hierdiff_amd.refine import set_chem_hooks
    fx = ro.load("r5_refine_tree_h64")
    _, mol_sizes = ro.load_size_dict()
    n = len(fx["wid"])
    nodes = ro.tree_nodes(fx) + [ro.BlurNode()]
    adj = np.zeros((n + 1, n + 1), np.int64)
    adj[:n, :n] = fx["adj"]
    for i in range(n):
        nodes[i].neighbors = [nodes[j] for j in range(n) if adj[i, j]]
    tree = ro.BeamTree(ro.Tree(nodes, adj.tolist()))
    prev = set_chem_hooks(mol_from_smiles=ro.stub_mol_from_smiles, can_assemble=ro.stub_can_assemble)
    try:
        out, psum, edited = _model(fx).check_tree(tree, ro.StubVocab(mol_sizes), DEV)
    finally:
        set_chem_hooks(**prev)
    assert edited is True and int(fx["flag"]) == 1
    after = [nd.wid for nd in out.tree.nodes[:n]]
    changed = [i for i in range(n) if after[i] != int(fx["wid"][i])]
    assert changed == [int(fx["edited"])] and after[changed[0]] == int(fx["new_wid"])
    assert out.tree.nodes[changed[0]].mol == ro.stub_mol_from_smiles(f"S{int(fx['new_wid'])}")
    assert abs(psum - float(fx["pertube_p_sum"])) <= 1e-4 * max(1.0, abs(float(fx["pertube_p_sum"])))


@pytest.mark.autograd
def test_refine_module_trains():
    from hierdiff_amd.refine_train import CLIP_VAL, Refine
    from hierdiff_amd.trainer import ddp_step
    fx = ro.load("r1_refine_train_h64")
    size_dict, _ = ro.load_size_dict()
    torch.manual_seed(0)
    mod = Refine({"model": dict(size_dict=size_dict, vocab_size=780, feature_size=8, hidden_size=64, n_layers=2)}).to(DEV)
    [opt], _ = mod.configure_optimizers()
    losses = []
    for _ in range(5):
        r = ddp_step(mod, ro.train_batch(fx), opt, clip_val=CLIP_VAL, overlap=False)
        losses.append(float(r["loss"]))
        assert np.isfinite(float(r["grad_norm"]))
    assert losses[-1] < losses[0], losses


@pytest.mark.autograd
def test_training_step_launches_the_new_kernels_and_no_blas_library_kernel():
    from torch.profiler import ProfilerActivity, profile
    fx = ro.load("r1_refine_train_h64")
    m = _model(fx).train()
    m(ro.train_batch(fx))["loss"].backward()                     # warm-up: graphs, weight images
    m.zero_grad(set_to_none=True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        m(ro.train_batch(fx))["loss"].backward()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    blas = [n for n in names if n.startswith("Cijk_") or "rocblas" in n.lower() or "hipblas" in n.lower()]
    assert not blas, blas
    for k in ("k_cand_xent", "k_cand_xent_bwd", "k_refine_embed", "k_refine_embed_bwd", "k_sqdist", "k_sqdist_bwd", "k_tgemm"):
        assert any(k in n for n in names), k


# ----------------------------------------------------------------------------- the refine kernels at their edges
def _sqdist_both(row, col, M, seed):
    """(ea, dx) of hd_sqdist_forward / _backward on a graph and of float64 torch, for a random upstream gradient."""
    from hierdiff_amd.refine import _SqDist
    from hierdiff_amd.stage2 import E_GCL
    rng = np.random.Generator(np.random.PCG64(seed))
    E = int(row.numel())
    layer = E_GCL(32, 32, 32, edges_in_d=1, attention=True, tanh=True, coords_range=30, edge_update=False).to(DEV)
    g = layer._graph(row.to(torch.int32), col.to(torch.int32), M)
    x0 = rng.standard_normal((M, 3)).astype(np.float32)
    up = torch.from_numpy(rng.standard_normal((E, 1)).astype(np.float32))
    x = torch.from_numpy(x0).to(DEV).requires_grad_(True)
    ea = _SqDist.apply(g, x)
    (ea * up.to(DEV)).sum().backward()
    xr = torch.from_numpy(x0).double().requires_grad_(True)
    ref = ((xr[row.long()] - xr[col.long()]) ** 2).sum(1, keepdim=True)
    (ref * up.double()).sum().backward()
    return ea.detach().cpu(), x.grad.cpu(), ref.detach(), xr.grad


@pytest.mark.autograd
@pytest.mark.parametrize("M,E", [(300, 3001), (257, 700), (1000, 517)])
def test_sqdist_on_a_ragged_graph(M, E):
    """Isolated, send-only and receive-only nodes (empty CSR lists), a hub on 40 % of the edges, self and repeated edges; M not a
    multiple of the kernel's 256 nodes per workgroup."""
    from tests.fuzz_egcl_grads import ragged_graph
    rng = np.random.Generator(np.random.PCG64([9, M, E]))
    row, col = ragged_graph(rng, M, E, self_edges=True)
    row[:7], col[:7] = row[7:14], col[7:14]                                  # repeated edges for certain ...
    col[14:20] = row[14:20]                                                  # ... and self edges
    deg = torch.bincount(torch.cat([row, col]), minlength=M)
    assert int((deg == 0).sum()) > 0 and int(deg.max()) > E // 3
    ea, dx, ref, dref = _sqdist_both(row, col, M, 10)
    assert _rel(ea, ref) < 1e-6
    assert _rel(dx, dref) < 1e-5
    assert bool((dx[deg == 0] == 0).all()), "an isolated node has no gradient"


@pytest.mark.autograd
def test_sqdist_on_a_graph_without_edges():
    none = torch.zeros(0, dtype=torch.long)
    ea, dx, ref, dref = _sqdist_both(none, none, 5, 11)
    assert ea.shape == (0, 1) and bool((dx == 0).all()) and bool((dref == 0).all())


def _embed_bwd(v, s, dout, ldo, H, nv, ns, off_v, off_s):
    from hierdiff_amd import _lib
    M = int(v.numel())
    dEv, dEs = torch.full((nv, H), float("nan"), device=DEV), torch.full((ns, H), float("nan"), device=DEV)
    p = lambda t: None if t.numel() == 0 else t.data_ptr()
    _lib.check(_lib.load().hd_refine_embed_backward(0, p(v), p(s), M, H, nv, ns, p(dout), ldo, off_v, off_s, dEv.data_ptr(),
                                                    dEs.data_ptr(), torch.cuda.current_stream().cuda_stream), "hd_refine_embed_backward")
    torch.cuda.synchronize()
    return dEv.cpu(), dEs.cpu()


@pytest.mark.parametrize("M", [0, 1, 255, 257, 700])
@pytest.mark.parametrize("H", [32, 256])
def test_embed_backward_at_its_edges(M, H):
    """hd_refine_embed_backward through the C ABI: ids that never occur give exactly zero rows, one id carries every row (the size
    table), M = 0 and M = 1, and `ldo` wider than the three column blocks with the two blocks anywhere in the row."""
    rng = np.random.Generator(np.random.PCG64([12, M, H]))
    nv, ns = 41, 7
    ldo, off_v, off_s = 3 * H + 9, 5, 2 * H + 9
    v = torch.from_numpy(rng.integers(0, 20, M) * 2)                     # only even ids below 40 occur
    s = torch.full((M,), 3, dtype=torch.long)                            # one id carries every row
    dout = torch.from_numpy(rng.standard_normal((M, ldo)).astype(np.float32))
    dEv, dEs = _embed_bwd(v.to(DEV), s.to(DEV), dout.to(DEV), ldo, H, nv, ns, off_v, off_s)
    rv = torch.zeros(nv, H, dtype=torch.float64).index_add_(0, v, dout[:, off_v:off_v + H].double())
    rs = torch.zeros(ns, H, dtype=torch.float64).index_add_(0, s, dout[:, off_s:off_s + H].double())
    assert bool(torch.isfinite(dEv).all()) and bool(torch.isfinite(dEs).all())
    assert _rel(dEv, rv) < 1e-5 and _rel(dEs, rs) < 1e-5
    unused = torch.ones(nv, dtype=torch.bool)
    unused[v] = False
    assert int(unused.sum()) >= 21 and bool((dEv[unused] == 0).all())
    assert bool((dEs[torch.arange(ns) != 3] == 0).all())
    if M <= 1:
        assert torch.equal(dEs[3], dout[:, off_s:off_s + H].sum(0))


def test_embed_forward_with_a_wide_row_and_no_rows():
    from hierdiff_amd import _lib
    lib = _lib.load()
    H, nv, ns, ldo, off_v, off_s = 32, 11, 5, 3 * 32 + 6, 3, 70
    rng = np.random.Generator(np.random.PCG64(13))
    Ev = torch.from_numpy(rng.standard_normal((nv, H)).astype(np.float32)).to(DEV)
    Es = torch.from_numpy(rng.standard_normal((ns, H)).astype(np.float32)).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hd_refine_embed_forward(0, None, None, 0, H, nv, ns, Ev.data_ptr(), Es.data_ptr(), None, ldo, off_v, off_s,
                                           bad.data_ptr(), s), "hd_refine_embed_forward")
    v = torch.tensor([10, 0, 3], device=DEV)
    z = torch.tensor([4, 4, 0], device=DEV)
    out = torch.full((3, ldo), -7.0, device=DEV)
    _lib.check(lib.hd_refine_embed_forward(0, v.data_ptr(), z.data_ptr(), 3, H, nv, ns, Ev.data_ptr(), Es.data_ptr(), out.data_ptr(), ldo,
                                           off_v, off_s, bad.data_ptr(), s), "hd_refine_embed_forward")
    assert int(bad.cpu()) == 0
    assert torch.equal(out[:, off_v:off_v + H], Ev[v]) and torch.equal(out[:, off_s:off_s + H], Es[z])
    keep = torch.ones(ldo, dtype=torch.bool)
    keep[off_v:off_v + H] = False
    keep[off_s:off_s + H] = False
    assert bool((out[:, keep.to(DEV)] == -7.0).all())
