"""CPU tier of scoring (hierdiff_amd/scoring.py, DiffusionQM9.nll_full / score, hd_set_nll_terms / hd_nll_terms / hd_nll_finish): the
new C-ABI symbols and the argument checks that need no device, the term tables against an independent fp64 evaluation, the
restatement `nll_full_ref` of the bound from the oracle's pieces - pinned here, before a GPU sees it, to the reference's own estimator
term by term - and the Python / CLI argument errors.  All without a GPU."""
import ctypes as C
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib, paths, scoring
from hierdiff_amd.noise_model import PredefinedNoiseSchedule, schedule_tables
from oracle import egnn_oracle as orc
from tests.test_inpaint_cpu import cpu_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


def schedules(T):
    """(name, gamma module) of the learned and the two predefined schedules."""
    m, _ = cpu_model(T=T, L=1)
    return [("learned", m.gamma), ("cosine", PredefinedNoiseSchedule("cosine", T, 1e-4)),
            ("polynomial_2", PredefinedNoiseSchedule("polynomial_2", T, 1e-5))]


# ----------------------------------------------------------------------------- the restatement (shared with tests/test_gpu_nll_full.py)

def philox_raw(lib, seed, base, draw, B, N, F):
    """(randn_x [B,N,3], randn_h [B,N,F]) of the library's generator in the scoring layout: normal(seed, base + b, draw, n D + c)."""
    D = 3 + F
    out = np.empty((B, N, D), dtype=np.float32)
    for b in range(B):
        for n in range(N):
            for c in range(D):
                out[b, n, c] = lib.hd_philox_normal_host(int(seed), int(base) + b, int(draw), n * D + c)
    t = torch.from_numpy(out)
    return t[:, :, :3].contiguous(), t[:, :, 3:].contiguous()


def scoring_noises(lib, seed, base, t_list, B, N, F):
    """The K + 1 pairs `nll_full(raw_noises=...)` takes, from the host twin of the generator: term t at draw t, then eps_0 at draw 0."""
    return [philox_raw(lib, seed, base, t, B, N, F) for t in t_list] + [philox_raw(lib, seed, base, 0, B, N, F)]


def nll_full_ref(sd, cfg, T, x, h, node_mask, edge_mask, context, gg, t_list, raw_noises, node_coarse_type="prop",
                 norm_values=None, norm_biases=None, return_parts=False):
    """NLL(S) = rest + (T / K) sum_{t in S} w_t e_t from the oracle's pieces only.  e_t is the `error` of orc.nll_forward at
    t_int = t with eps_t and the grid's gammas; `rest` = kl_prior + neg_log_constants + L_0 (- delta_log_px) is the loss of one call
    with gamma_s = gamma_t, whose SNR weight exp(0) - 1 is exactly 0; w_t = 0.5 expm1(gg[t] - gg[t-1]) in float64.  Returns
    (nll [B] float64, e [K,B] float32) (+ rest, w with return_parts)."""
    gg = torch.as_tensor(gg, dtype=torch.float32).reshape(-1)
    nm = node_mask.float()
    B, K = x.shape[0], len(t_list)
    eps0 = orc.combined_noise(raw_noises[K][0], raw_noises[K][1], nm)
    kw = dict(node_coarse_type=node_coarse_type, norm_values=norm_values, norm_biases=norm_biases)
    col = lambda v: torch.full((B, 1), float(v))
    e_rows, w = [], []
    for k, t in enumerate(t_list):
        eps_t = orc.combined_noise(raw_noises[k][0], raw_noises[k][1], nm)
        gam = {"gamma_s": col(gg[t - 1]), "gamma_t": col(gg[t]), "gamma_0": col(gg[0]), "gamma_T": col(gg[T])}
        _, err = orc.nll_forward(sd, cfg, T, x, h, node_mask, edge_mask, context, col(t), eps_t, eps0, gammas=gam, **kw)
        e_rows.append(err)
        w.append(0.5 * math.expm1(float(gg[t]) - float(gg[t - 1])))
    t1 = t_list[0]
    gam = {"gamma_s": col(gg[t1]), "gamma_t": col(gg[t1]), "gamma_0": col(gg[0]), "gamma_T": col(gg[T])}
    rest, _ = orc.nll_forward(sd, cfg, T, x, h, node_mask, edge_mask, context, col(t1),
                              orc.combined_noise(raw_noises[0][0], raw_noises[0][1], nm), eps0, gammas=gam, **kw)
    e = torch.stack(e_rows)
    wt = torch.tensor(w, dtype=torch.float64)
    nll = rest.double() + (T / K) * (wt.view(-1, 1) * e.double()).sum(0)
    return (nll, e, rest, wt) if return_parts else (nll, e)


# ----------------------------------------------------------------------------- 1. C ABI

NEW_SYMBOLS = ["hd_set_nll_terms", "hd_nll_terms", "hd_nll_finish", "hd_nll_graph_builds"]


def test_nll_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
        m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12          # additive: the ABI version stays
    assert "draw = t" in hdr and "eps_0 of the t = 0 likelihood is draw 0" in hdr       # the scoring draw layout, at hd_noise


def test_nll_entry_points_reject_bad_arguments_without_a_gpu(lib):
    """The checks that need no handle, with the process alive.  A handle needs a device: terms before a schedule, a stale schedule,
    k_hi > K, pocket rows and noise_rows != B are tests/test_gpu_nll_full.py::test_documented_argument_errors."""
    ti, coef = (C.c_int * 2)(4, 2), (C.c_float * 8)()
    assert lib.hd_set_nll_terms(None, 2, ti, coef) == -1 and b"hd_set_nll_terms" in lib.hd_last_error()
    assert lib.hd_nll_terms(None, None, None, None, -1, 0, 1, None, None, 1, 0, 0, 0, None, None, None) == -1
    assert b"hd_nll_terms: null handle/topology" in lib.hd_last_error()
    assert lib.hd_nll_terms(None, None, None, None, -1, 2, 1, None, None, 1, 0, 0, 0, None, None, None) == -1
    assert b"k_lo <= k_hi" in lib.hd_last_error()
    assert lib.hd_nll_terms(None, None, None, None, -1, -1, 1, None, None, 1, 0, 0, 0, None, None, None) == -1
    assert b"k_lo <= k_hi" in lib.hd_last_error()
    assert lib.hd_nll_finish(None, None, None, None, -1, None, None, 1, 0, 0, 1, None, 5, 3, None, None, None) == -1
    assert b"hd_nll_finish: null handle/topology" in lib.hd_last_error()
    assert lib.hd_nll_graph_builds(None) == -1


# ----------------------------------------------------------------------------- 2. term tables

@pytest.mark.parametrize("T", [7, 1000])
def test_term_tables_match_an_independent_fp64_evaluation(T):
    assert scoring.resolve_terms(T) == scoring.resolve_terms(T, terms=T) == list(range(T, 0, -1))
    for K in sorted({1, 2, 3, min(T, 50), T}):
        assert scoring.resolve_terms(T, terms=K) == paths.uniform_path(T, K)[:-1]
        assert scoring.resolve_terms(T, terms=K)[0] == T
    assert scoring.resolve_terms(T, timesteps=[1, T, 3]) == [T, 3, 1]
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    for name, gamma in schedules(T):
        g = schedule_tables(gamma, T)["gamma"]
        for t_list in (scoring.resolve_terms(T), scoring.resolve_terms(T, terms=min(T, 5)), [T, 1]):
            tt = scoring.term_tables(g, t_list)
            assert tt["K"] == len(t_list) and tt["t_idx"].tolist() == list(t_list) and tuple(tt["coef"].shape) == (len(t_list), 4)
            for k, t in enumerate(t_list):
                gs, gt = float(g[t - 1]), float(g[t])
                w = 0.5 * math.expm1(gt - gs)
                assert w >= 0.0, (name, t, w)
                assert float(tt["coef"][k, 2]) >= 0.0
                assert abs(float(tt["coef"][k, 2]) - w) <= 1e-6 * abs(w), (name, t)
                assert abs(float(tt["coef"][k, 0]) - math.sqrt(sig(-gt))) <= 1e-6 * math.sqrt(sig(-gt)), (name, t)
                assert abs(float(tt["coef"][k, 1]) - math.sqrt(sig(gt))) <= 1e-6 * math.sqrt(sig(gt)), (name, t)
                assert float(tt["coef"][k, 3]) == 0.0


def test_bad_terms_and_timesteps_raise():
    T = 10
    for bad in (0, -1, 11, 2.0, True, "3"):
        with pytest.raises(ValueError, match="terms"):
            scoring.resolve_terms(T, terms=bad)
    for bad in ([0], [11], [3, 3], [], [2.5], [True], 5):
        with pytest.raises(ValueError, match="timesteps"):
            scoring.resolve_terms(T, timesteps=bad)
    with pytest.raises(ValueError, match="not both"):
        scoring.resolve_terms(T, terms=3, timesteps=[3])


# ----------------------------------------------------------------------------- 3. the restatement is the reference's estimator, term by term

def test_restatement_is_the_one_timestep_estimator_summed_over_t(lib):
    """For every t: loss(t) of the oracle's eval-mode nll_forward (the reference's estimator at that t) = rest + T w_t e_t, to fp32
    rounding of values of order 1e3 - which makes `nll_full_ref` that estimator summed over t, with nothing of its own.

    The bar is 5 ulp of loss(t) (6e-7 relative), from the number format: loss(t) is fp32 throughout - three additions of terms of its
    own size (0.5 ulp each), the product chain T (0.5 snr error) (three roundings on a term that is nearly the whole loss) and the
    weight exp(g_t - g_s) - 1, whose subtraction keeps the rounding of exp(.) ~ 2.1 as ~1 ulp of a weight ~ 1.1 - against w_t e_t
    evaluated in float64.  Measured: worst 2.7e-7 relative, 5.1e-4 absolute at loss(t) = 2129 (e_t between 20 and 240, loss(t)
    between 270 and 2580).  An absolute 1e-4 cannot hold here: one ulp of a loss above 2048 is 2.4e-4, so the final rounding of the
    reference's own sum already moves it by up to 1.2e-4."""
    H, L, T, n_list = 32, 2, 20, [8, 5, 3, 7]
    m, sd_np = cpu_model(H=H, L=L, T=T)
    sd = orc.as_torch_sd(sd_np)
    cfg = orc.DynCfg(in_node_nf=9, context_node_nf=0, hidden_nf=H, n_layers=L)
    xh, nm, em = orc.random_inputs(n_list, 8, seed=3)
    x, h = xh[:, :, :3].contiguous(), xh[:, :, 3:].contiguous()
    B, N = x.shape[:2]
    gg = schedule_tables(m.gamma, T)["gamma"]
    t_list = scoring.resolve_terms(T)
    raws = scoring_noises(lib, 2022, 0, t_list, B, N, 8)
    nll, e, rest, w = nll_full_ref(sd, cfg, T, x, h, nm, em, None, gg, t_list, raws, return_parts=True)
    eps0 = orc.combined_noise(raws[T][0], raws[T][1], nm.float())
    col = lambda v: torch.full((B, 1), float(v))
    worst = worst_rel = 0.0
    for k, t in enumerate(t_list):
        gam = {"gamma_s": col(gg[t - 1]), "gamma_t": col(gg[t]), "gamma_0": col(gg[0]), "gamma_T": col(gg[T])}
        loss_t, err = orc.nll_forward(sd, cfg, T, x, h, nm, em, None, col(t), orc.combined_noise(raws[k][0], raws[k][1], nm.float()),
                                      eps0, gammas=gam)
        assert torch.equal(err, e[k])
        diff = (loss_t.double() - rest.double() - T * w[k] * e[k].double()).abs()
        worst, worst_rel = max(worst, float(diff.max())), max(worst_rel, float((diff / loss_t.double().abs()).max()))
        assert bool((diff <= 5 * 2.0 ** -23 * loss_t.double().abs()).all()), (t, diff.tolist(), loss_t.tolist())
    print(f"worst |loss(t) - rest - T w_t e_t| = {worst:.3e} ({worst_rel:.2e} of loss(t)); rest {rest.tolist()}; "
          f"e_t in [{float(e.min()):.1f}, {float(e.max()):.1f}]")
    assert bool((e > 0).all()) and bool((w > 0).all())                 # every term is positive
    assert bool(torch.isfinite(nll).all())
    # K = 1 is the estimator itself
    one, _ = nll_full_ref(sd, cfg, T, x, h, nm, em, None, gg, [7], [raws[t_list.index(7)], raws[T]])
    assert float((one - (rest.double() + T * w[t_list.index(7)] * e[t_list.index(7)].double())).abs().max()) == 0.0


# ----------------------------------------------------------------------------- 4. Python and CLI

def test_nll_full_and_score_raise_on_bad_arguments_before_touching_the_gpu(monkeypatch):
    m, _ = cpu_model(T=6, L=1)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    B, N = 2, 4
    nm = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool).view(B, N, 1)
    x, h = torch.zeros(B, N, 3), torch.zeros(B, N, 8)
    mols = [{"x": torch.zeros(3, 3), "h": torch.zeros(3, 8)}, {"x": torch.zeros(2, 3), "h": torch.zeros(2, 8)}]
    for call in (lambda **kw: m.nll_full(x, h, nm, **kw), lambda **kw: m.score(mols, "cpu", **kw)):
        for bad in (0, 7, -3, 2.5, True):
            with pytest.raises(ValueError, match="terms"):
                call(terms=bad)
        for bad in ([0], [7], [2, 2], []):
            with pytest.raises(ValueError, match="timesteps"):
                call(timesteps=bad)
        with pytest.raises(ValueError, match="not both"):
            call(terms=3, timesteps=[3])
    with pytest.raises(ValueError, match="x must be"):
        m.nll_full(torch.zeros(B, N, 2), h, nm)
    with pytest.raises(ValueError, match="h must be"):
        m.nll_full(x, torch.zeros(B, N, 3), nm)
    with pytest.raises(ValueError, match="node_mask"):
        m.nll_full(x, h, nm.view(B, N))
    with pytest.raises(ValueError, match="raw_noises"):
        m.nll_full(x, h, nm, terms=2, raw_noises=[(torch.zeros(B, N, 3), torch.zeros(B, N, 8))] * 2)
    with pytest.raises(ValueError, match="sample_id_base"):
        m.nll_full(x, h, nm, sample_id_base=-1)
    # CPU tensors: the error of the other device-loop entry points
    with pytest.raises(_lib.HierDiffHipError, match="no CPU fallback"):
        m.nll_full(x, h, nm)
    m.pocket = True
    with pytest.raises(ValueError, match="pocket"):
        m.nll_full(x, h, nm)
    m.pocket = False
    m.dynamics.mode = "gnn_dynamics"
    with pytest.raises(NotImplementedError, match="gnn_dynamics"):
        m.nll_full(x, h, nm)
    m.dynamics.mode = "egnn_dynamics"
    # score's own arguments
    with pytest.raises(ValueError, match="no samples"):
        m.score([], "cpu")
    with pytest.raises(ValueError, match="batch_size"):
        m.score(mols, "cpu", batch_size=0)
    with pytest.raises(ValueError, match="unsupported keyword"):
        m.score(mols, "cpu", raw_noises=[])
    for bad in ([{"x": torch.zeros(3, 3)}], [{"x": torch.zeros(3, 2), "h": torch.zeros(3, 8)}], [{"x": torch.zeros(3, 3), "h": torch.zeros(2, 8)}],
                [{"x": torch.zeros(0, 3), "h": torch.zeros(0, 8)}], ["x"]):
        with pytest.raises(ValueError, match=r"samples\[0\]"):
            m.score(bad, "cpu")


def test_score_pads_recentres_and_assigns_global_ids(monkeypatch):
    """`score` on a hand-made list with a stub in place of the device call: batches of `batch_size`, node masks and padding, x
    re-centred per molecule, molecule i under sample id sample_id_base + i, keywords passed through, results in list order."""
    m, _ = cpu_model(T=6, L=1)
    gen = torch.Generator().manual_seed(1)
    sizes = [3, 1, 4, 2, 4]
    mols = [{"x": torch.randn(n, 3, generator=gen) + 5.0, "h": torch.randn(n, 8, generator=gen)} for n in sizes]
    calls = []

    def stub(x, h, node_mask, edge_mask=None, context=None, **kw):
        calls.append(dict(x=x.clone(), h=h.clone(), nm=node_mask.clone(), ctx=context, kw=dict(kw)))
        return kw["sample_id_base"] + torch.arange(x.shape[0], dtype=torch.float32)

    monkeypatch.setattr(m, "nll_full", stub)
    out = m.score(mols, "cpu", batch_size=2, sample_id_base=100, terms=3, seed=7)
    assert out.tolist() == [100.0, 101.0, 102.0, 103.0, 104.0] and out.device.type == "cpu"
    assert [c["kw"]["sample_id_base"] for c in calls] == [100, 102, 104]
    assert all(c["kw"]["terms"] == 3 and c["kw"]["seed"] == 7 and c["ctx"] is None for c in calls)
    assert [tuple(c["x"].shape) for c in calls] == [(2, 3, 3), (2, 4, 3), (1, 4, 3)]
    i = 0
    for c in calls:
        for b in range(c["x"].shape[0]):
            n = sizes[i]
            assert c["nm"][b, :, 0].tolist() == [True] * n + [False] * (c["x"].shape[1] - n)
            want = mols[i]["x"] - mols[i]["x"].mean(0, keepdim=True)
            assert torch.equal(c["x"][b, :n], want) and float(c["x"][b, :n].sum(0).abs().max()) < 1e-5
            assert torch.equal(c["h"][b, :n], mols[i]["h"])
            assert float(c["x"][b, n:].abs().sum()) == 0.0 and float(c["h"][b, n:].abs().sum()) == 0.0
            i += 1
    assert i == len(mols)
    # a context model takes the samples' own context
    mc, _ = cpu_model(T=6, L=1, C_=1)
    monkeypatch.setattr(mc, "nll_full", stub)
    del calls[:]
    with pytest.raises(ValueError, match="context"):
        mc.score(mols, "cpu")
    withc = [dict(mol, context=torch.full((mol["x"].shape[0], 1), 0.5 + k)) for k, mol in enumerate(mols)]
    mc.score(withc, "cpu", batch_size=8)
    assert tuple(calls[0]["ctx"].shape) == (5, 4, 1) and calls[0]["ctx"][2, :, 0].tolist() == [2.5] * 4
    assert calls[0]["ctx"][1, :, 0].tolist() == [1.5, 0.0, 0.0, 0.0]


def test_cli_score_flags(tmp_path, monkeypatch):
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--score", "s.pkl"])
    assert (a.score, a.terms, a.out) == ("s.pkl", None, "scores.pkl")
    a = sampler.parse_args(["--score", "s.pkl", "--terms", "50", "--out", "o.pkl"])
    assert (a.terms, a.out) == (50, "o.pkl")
    a = sampler.parse_args([])
    assert (a.score, a.terms, a.out) == (None, None, "sample_results.pkl")
    for bad in (["--score", "s.pkl", "--known", "k.pkl", "--grow", "2"], ["--score", "s.pkl", "--steps", "5"],
                ["--score", "s.pkl", "--grow", "2"], ["--terms", "5"], ["--score", "s.pkl", "--terms", "0"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
    # both input forms reach `score` as the bare list
    mols = [{"x": torch.zeros(2, 3), "h": torch.zeros(2, 8)}]
    for name, obj in (("tuple.pkl", (mols, [])), ("list.pkl", mols)):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(obj, f)
        got = sampler.read_known(str(tmp_path / name))
        assert isinstance(got, list) and len(got) == 1 and torch.equal(got[0]["x"], mols[0]["x"])
