"""GPU tier of scoring (DiffusionQM9.nll_full / score, hd_set_nll_terms / hd_nll_terms / hd_nll_finish): parity of the score and of every
term's error with the restatement `nll_full_ref` (tests/test_nll_full_cpu.py, built from the oracle's pieces and pinned there to the
reference's estimator) - injected normals and the library's generator -, the bridge to today's one-timestep `nll`, the bit identities
(graph replay, cached graph, split term ranges, batch shards, reruns), the `score` round trip and the headline shape at T = 1000.
Bars: the project's own for the same quantities against the same oracle (tests/test_gpu_training.py:116,161)."""
import ctypes as C

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, scoring
from hierdiff_amd.weights import synthetic_state_dict
from oracle import egnn_oracle as orc
from tests.test_gpu_parity import PRECISIONS
from tests.test_nll_full_cpu import nll_full_ref, scoring_noises

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 2022
NLL_BAR = dict(rtol=1e-4, atol=1e-3)
ERR_BAR = dict(rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def dev(t):
    return None if t is None else t.to(DEV)


def make_model(H, L, T, C_=0, precision="fp32", elem=False, norm=None, seed=31, gain=1.0):
    """(model on the GPU, oracle state dict, oracle cfg, keywords of the oracle's nll_forward)."""
    from hierdiff_amd import DiffusionQM9, default_config
    nf = 4 if elem else 9
    sd_np = synthetic_state_dict(nf, C_, H, L, 2, True, seed, gain)
    cfg = default_config(hidden_nf=H, n_layers=L, context_node_nf=C_, timesteps=T)
    okw = {}
    if elem:
        cfg["node_coarse_type"] = "elem"
        okw["node_coarse_type"] = "elem"
    if norm is not None:
        cfg.norm_values, cfg.norm_biases = list(norm[0]), list(norm[1])
        okw.update(norm_values=norm[0], norm_biases=norm[1])
    model = DiffusionQM9(cfg)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd_np.items()})
    model.dynamics.precision = precision
    model.seed = SEED
    model = model.to(DEV).eval()
    ocfg = orc.DynCfg(in_node_nf=nf, context_node_nf=C_, hidden_nf=H, n_layers=L)
    return model, orc.as_torch_sd(sd_np), ocfg, okw


def data(n_list, F, C_=0, seed=3, scale=(1.0, 1.0)):
    xh, nm, em = orc.random_inputs(n_list, F, seed=seed)
    x, h = (xh[:, :, :3] * scale[0]).contiguous(), (xh[:, :, 3:] * scale[1]).contiguous()
    B, N = x.shape[:2]
    ctx = (torch.zeros(B, N, C_) + torch.linspace(0.5, 2.0, B).view(B, 1, 1)) if C_ else None
    return x, h, nm, em, ctx


def injected(t_count, B, N, F, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(torch.from_numpy(rng.standard_normal((B, N, 3)).astype(np.float32)),
             torch.from_numpy(rng.standard_normal((B, N, F)).astype(np.float32))) for _ in range(t_count + 1)]


def gamma_grid(model):
    return model._schedule()["gamma"].clone()


def check(got_nll, got_e, ref_nll, ref_e, what):
    g, r = got_nll.cpu().double().numpy(), ref_nll.double().numpy()
    ge, re_ = got_e.cpu().double().numpy(), ref_e.double().numpy()
    print(f"{what}: nll worst |diff| {np.abs(g - r).max():.3e} (rel {np.abs((g - r) / r).max():.2e}, values {r.min():.1f} .. {r.max():.1f}); "
          f"e_t worst |diff| {np.abs(ge - re_).max():.3e} (rel {np.abs((ge - re_) / re_).max():.2e}, values {re_.min():.1f} .. {re_.max():.1f})")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(ge))
    np.testing.assert_allclose(g, r, **NLL_BAR)
    np.testing.assert_allclose(ge, re_, **ERR_BAR)


CONFIGS = {
    "h32_T20": dict(H=32, L=2, T=20, C_=0, n_list=[8, 5, 3, 7]),
    "h32_T20_ctx": dict(H=32, L=2, T=20, C_=1, n_list=[8, 5, 3, 7]),
    "h256_l6_T50_mixed": dict(H=256, L=6, T=50, C_=0, n_list=[12, 1, 7, 2, 9, 4], gain=0.02),
    "h32_elem_norm": dict(H=32, L=2, T=20, C_=0, n_list=[8, 5, 3, 7], elem=True, norm=([2.0, 4.0, 2.0], [None, 0.5, 0.25])),
}


def _case(name, precision):
    c = dict(CONFIGS[name])
    n_list = c.pop("n_list")
    model, sd, ocfg, okw = make_model(precision=precision, **c)
    F = model.in_node_nf
    x, h, nm, em, ctx = data(n_list, F, c.get("C_", 0), scale=(3.0, 2.0) if c.get("norm") else (1.0, 1.0))
    return model, sd, ocfg, okw, x, h, nm, em, ctx


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_parity_with_injected_normals(name, precision):
    model, sd, ocfg, okw, x, h, nm, em, ctx = _case(name, precision)
    T, (B, N), F = model.T, x.shape[:2], model.in_node_nf
    for kw in (dict(), dict(terms=min(T, 5))):
        t_list = scoring.resolve_terms(T, **kw)
        raws = injected(len(t_list), B, N, F)
        nll, (t_idx, e) = model.nll_full(dev(x), dev(h), dev(nm), dev(em), dev(ctx), raw_noises=raws, return_terms=True, **kw)
        assert t_idx.tolist() == t_list and tuple(e.shape) == (len(t_list), B)
        ref, ref_e = nll_full_ref(sd, ocfg, T, x, h, nm, em, ctx, gamma_grid(model), t_list, raws, **okw)
        check(nll, e, ref, ref_e, f"{name} [{precision}] K={len(t_list)}")
        assert bool((e > 0).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_parity_with_the_generator(lib, precision):
    model, sd, ocfg, okw, x, h, nm, em, ctx = _case("h32_T20", precision)
    T, (B, N) = model.T, x.shape[:2]
    base = 5
    for kw in (dict(), dict(timesteps=[3, 20, 11])):
        t_list = scoring.resolve_terms(T, **kw)
        nll, (_, e) = model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, sample_id_base=base, return_terms=True, **kw)
        raws = scoring_noises(lib, SEED, base, t_list, B, N, 8)
        ref, ref_e = nll_full_ref(sd, ocfg, T, x, h, nm, em, None, gamma_grid(model), t_list, raws)
        check(nll, e, ref, ref_e, f"generator [{precision}] K={len(t_list)}")
    other = model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, sample_id_base=base, seed=SEED + 1)
    assert not torch.equal(other, model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, sample_id_base=base))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bridge_to_the_one_timestep_estimator(precision):
    """nll_full(timesteps=[t]) is eval-mode `nll` at that t on the eager path with the same normals."""
    model, sd, ocfg, okw, x, h, nm, em, ctx = _case("h32_T20", precision)
    T, (B, N) = model.T, x.shape[:2]
    gg = gamma_grid(model)
    for t in (1, T // 2, T):
        raws = injected(1, B, N, 8, seed=20 + t)
        got = model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, timesteps=[t], raw_noises=raws)
        eps, eps0 = (orc.combined_noise(r[0], r[1], nm.float()) for r in raws)
        col = lambda v: torch.full((B, 1), float(v))
        gam = {"gamma_s": col(gg[t - 1]), "gamma_t": col(gg[t]), "gamma_0": col(gg[0]), "gamma_T": col(gg[T])}
        assert not model.training
        eager = model.nll(dev(x), dev(h), dev(nm), dev(em), None, t_int=col(t), eps=eps, eps0=eps0, gammas=gam)
        g, r = got.cpu().double().numpy(), eager.cpu().double().numpy()
        print(f"bridge t={t} [{precision}]: worst |diff| {np.abs(g - r).max():.3e} on values {r.min():.1f} .. {r.max():.1f}")
        np.testing.assert_allclose(g, r, **NLL_BAR)
        model.train()                                  # independent of self.training
        assert torch.equal(model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, timesteps=[t], raw_noises=raws), got)
        model.eval()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bit_identities(lib, precision):
    model, sd, ocfg, okw, x, h, nm, em, ctx = _case("h32_T20_ctx", precision)
    T, (B, N) = model.T, x.shape[:2]
    args = (dev(x), dev(h), dev(nm), dev(em), dev(ctx))
    a, (_, ea) = model.nll_full(*args, return_terms=True)
    b, (_, eb) = model.nll_full(*args, return_terms=True, use_graph=False)
    assert torch.equal(a, b) and torch.equal(ea, eb), "graph replay vs plain launches"
    topo = model.dynamics.topology(dev(nm), dev(em), B, N).ptr
    builds = lib.hd_nll_graph_builds(topo)
    assert builds >= 1
    c, (_, ec) = model.nll_full(*args, return_terms=True)
    assert lib.hd_nll_graph_builds(topo) == builds, "a second call replays the cached graph"
    assert torch.equal(a, c) and torch.equal(ea, ec), "two runs"
    plain = model.nll_full(*args)                      # without the e_t table: another captured kernel argument, same bits
    assert torch.equal(plain, a)
    # the term range in one call vs two, with and without the graph
    for ug in (True, False):
        for cut in (1, 7, T - 1):
            st = model._nll_setup(*args, None, None, None, 0, None, True, ug)
            model._nll_terms(st, 0, cut)
            model._nll_terms(st, cut, st.K)
            assert torch.equal(model._nll_finish(st), a) and torch.equal(st.err, ea), (ug, cut)
    # a shard of the batch under its global ids vs its rows of the whole batch
    whole = model.nll_full(*args, sample_id_base=40)
    for lo, hi in ((0, 1), (1, 3), (2, 4)):
        part = model.nll_full(*(v[lo:hi].contiguous() for v in args), sample_id_base=40 + lo)
        assert torch.equal(part, whole[lo:hi]), (lo, hi)
    # the subset estimators take their terms from the same streams: e_t of a term does not depend on the list it is in
    _, (ti, e5) = model.nll_full(*args, terms=5, return_terms=True)
    assert torch.equal(e5, ea[[T - t for t in ti.tolist()]])


def test_documented_argument_errors(lib):
    """Every documented argument error of the new entry points returns its code and leaves the process and the handle usable."""
    model, sd, ocfg, okw, x, h, nm, em, ctx = _case("h32_T20", "fp32")
    B, N = x.shape[:2]
    topo = model.dynamics.topology(dev(nm), dev(em), B, N).ptr
    hnd = model._lib_handle()
    xh = torch.zeros(B, N, 11, device=DEV)
    acc = torch.zeros(B, dtype=torch.float64, device=DEV)
    nll = torch.zeros(B, device=DEV)
    consts = (C.c_float * 7)(1, 0.01, -9, 9, 1, 0, 0)
    terms = lambda **k: lib.hd_nll_terms(hnd, topo, k.get("xh", xh.data_ptr()), None, k.get("mol", -1), k.get("lo", 0), k.get("hi", 1),
                                         k.get("rx"), None, k.get("rows", B), 0, 0, 0, acc.data_ptr(), None, None)
    finish = lambda **k: lib.hd_nll_finish(hnd, topo, xh.data_ptr(), None, k.get("mol", -1), None, None, k.get("rows", B), 0, 0,
                                           k.get("K", 1), consts, 5, 3, acc.data_ptr(), nll.data_ptr(), None)
    ti, coef = (C.c_int * 2)(20, 10), (C.c_float * 8)()
    # before a schedule
    assert lib.hd_set_nll_terms(hnd, 2, ti, coef) == -4 and b"schedule not set" in lib.hd_last_error()
    assert terms() == -4 and b"schedule not set" in lib.hd_last_error()
    assert finish() == -4 and b"schedule not set" in lib.hd_last_error()
    model._schedule(rows=B)
    assert terms() == -4 and b"terms not set" in lib.hd_last_error()
    assert lib.hd_set_nll_terms(hnd, 2, (C.c_int * 2)(21, 10), coef) == -1 and b"t_idx" in lib.hd_last_error()
    assert lib.hd_set_nll_terms(hnd, 2, (C.c_int * 2)(20, 0), coef) == -1
    assert lib.hd_set_nll_terms(hnd, 21, ti, coef) == -1 and b"more terms" in lib.hd_last_error()
    assert lib.hd_set_nll_terms(hnd, 2, ti, coef) == 0
    # ranges, pocket rows, shared noise rows, half a noise pair, null tensors
    assert terms(lo=0, hi=3) == -1 and b"k_lo <= k_hi <= K" in lib.hd_last_error()
    assert terms(lo=2, hi=1) == -1 and terms(lo=-1, hi=1) == -1
    assert terms(mol=N - 1) == -1 and b"mol_shape" in lib.hd_last_error()
    assert finish(mol=N - 1) == -1 and b"mol_shape" in lib.hd_last_error()
    assert terms(rows=1) == -1 and b"noise_rows must be B" in lib.hd_last_error()
    assert finish(rows=1) == -1 and b"noise_rows must be B" in lib.hd_last_error()
    assert terms(rx=xh.data_ptr()) == -1 and b"go together" in lib.hd_last_error()
    assert terms(xh=None) == -1 and b"null xh" in lib.hd_last_error()
    assert finish(K=0) == -1 and finish(K=21) == -1
    assert lib.hd_nll_terms(hnd, None, xh.data_ptr(), None, -1, 0, 1, None, None, B, 0, 0, 0, acc.data_ptr(), None, None) == -1
    assert terms(mol=N) == 0 and terms(lo=1, hi=1) == 0           # mol_shape = N is no pocket; an empty range is valid
    # a stale schedule: a new upload of the plain schedule invalidates the terms
    model._sched_key = None
    model._schedule(rows=B)
    assert terms() == -4 and b"current schedule" in lib.hd_last_error()
    assert finish() == -4
    torch.cuda.synchronize()
    # the handle is as usable as before
    got = model.nll_full(dev(x), dev(h), dev(nm), dev(em), None, terms=4)
    assert bool(torch.isfinite(got).all())
    # Python: a context model without a context
    mc = make_model(32, 2, 20, C_=1)[0]
    with pytest.raises(ValueError, match="context required"):
        mc.nll_full(dev(x), dev(h), dev(nm), dev(em), None)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_score_round_trip(precision):
    model = make_model(32, 2, 20, precision=precision, gain=0.02)[0]
    torch.manual_seed(0)
    samples = model.sample(6, DEV)
    s = model.score(samples, DEV, batch_size=4, terms=5, sample_id_base=7)
    assert tuple(s.shape) == (6,) and s.device.type == "cpu" and bool(torch.isfinite(s).all())
    for lo in (0, 4):
        x, h, nm, _ = scoring.pad_samples(samples[lo:lo + 4], 3, 8, False)
        direct = model.nll_full(dev(x), dev(h), dev(nm), terms=5, sample_id_base=7 + lo).cpu()
        assert torch.equal(direct, s[lo:lo + 4])
    assert torch.equal(model.score(samples, DEV, batch_size=4, terms=5, sample_id_base=7), s)
    print(f"score [{precision}]: {s.tolist()}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_headline_shape_full_bound(precision):
    """B = 256, N = 30, H = 256, L = 6, all T = 1000 terms: finite, and a 32-molecule shard equals its rows bit for bit."""
    model = make_model(256, 6, 1000, precision=precision, gain=0.02)[0]
    rng = np.random.Generator(np.random.PCG64(1))
    n_list = [int(v) for v in rng.integers(18, 31, size=256)]
    n_list[0] = 30
    x, h, nm, em, _ = data(n_list, 8, seed=9)
    args = (dev(x), dev(h), dev(nm), dev(em))
    whole = model.nll_full(*args)
    assert tuple(whole.shape) == (256,) and bool(torch.isfinite(whole).all())
    part = model.nll_full(*(v[96:128].contiguous() for v in args), sample_id_base=96)
    assert torch.equal(part, whole[96:128])
    print(f"headline [{precision}]: nll {float(whole.min()):.1f} .. {float(whole.max()):.1f}")
