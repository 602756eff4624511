"""CPU tier: the C-ABI library builds/loads and exports every symbol include/hierdiff_hip.h declares;
host-side logic (weight layout, module key layout, schedule tables, node distribution)."""
import os
import re

import numpy as np
import pytest
import torch

from hierdiff_amd import _lib
from hierdiff_amd.weights import (dynamics_param_count, dynamics_param_shapes, flatten_dynamics,
                                  synthetic_state_dict)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hierdiff_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_header_symbols_all_exported(lib):
    hdr = open(os.path.join(REPO, "include", "hierdiff_hip.h")).read()
    declared = set(re.findall(r"\b(hd_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.hd_version() == _lib.ABI_VERSION == 12


def test_live_allocations_zero_in_a_fresh_process(lib):
    """A process that loaded the library and never touched a GPU holds nothing (the counters work without one)."""
    import subprocess
    import sys
    from hierdiff_amd import build
    code = ("import ctypes as C, sys; lib = C.CDLL(sys.argv[1]); lib.hd_live_allocations.restype = C.c_longlong; "
            "b = C.c_longlong(-1); n = lib.hd_live_allocations(C.byref(b)); print(n, b.value, lib.hd_live_allocations(None))")
    out = subprocess.run([sys.executable, "-c", code, build.LIB], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["0", "0", "0"], out


def _csrc_files():
    d = os.path.join(REPO, "hierdiff_amd", "csrc")
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith((".hip", ".hpp", ".h"))}


def test_only_mem_hpp_allocates_and_frees():
    """csrc/mem.hpp owns every allocate / free / create / destroy call; outside it only the two raw functions of hierdiff_hip.hip
    (hd_raw_alloc / hd_raw_free) name hipMalloc / hipFree.  No object is memset."""
    banned = ["hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreate", "hipEventDestroy(", "hipStreamCreate",
              "hipStreamDestroy(", "hipGraphExecDestroy("]
    files = _csrc_files()
    assert "mem.hpp" in files and "hierdiff_hip.hip" in files
    main = files["hierdiff_hip.hip"]
    raw = re.findall(r"^(?:int|void) hd_raw_(?:alloc|free)\(.*?^}\n", main, flags=re.S | re.M)
    assert len(raw) == 2, "the two raw functions were not found"
    assert "hipMalloc(" in raw[0] and "hipFree(" in raw[1]
    for body in raw:
        main = main.replace(body, "")
    files["hierdiff_hip.hip"] = main
    for name, text in files.items():
        if name == "mem.hpp":
            continue
        for word in banned:
            assert word not in text, f"{name} contains {word}"
    for word in ("memset(t,", "memset(g,", "memset(h,"):
        assert word not in main, word


def test_no_gpu_fails_loudly(lib):
    if lib.hd_device_count() > 0:
        pytest.skip("a GPU is visible")
    import ctypes as C
    cfg = _lib.HdConfig(9, 0, 3, 32, 1, 2, 1, 1, 1, 0.0, 10.0, 30.0)
    h = C.c_void_p()
    rc = lib.hd_create(C.byref(cfg), 0, C.byref(h))
    assert rc != 0 and b"HIP device" in lib.hd_last_error()
    with pytest.raises(_lib.HierDiffHipError):
        _lib.require_gpu()
    from hierdiff_amd import EGNN_dynamics_QM9
    m = EGNN_dynamics_QM9(9, 0, 3, hidden_nf=32, n_layers=1, attention=True, tanh=True, normalization_factor=10)
    xh = torch.zeros(1, 2, 11)
    with pytest.raises(_lib.HierDiffHipError):
        m._forward(torch.zeros(1, 1), xh, torch.ones(1, 2, 1).bool(), torch.ones(1, 2, 2).bool(), None)


def test_philox_host_twin_statistics(lib):
    v = np.array([lib.hd_philox_normal_host(2022, 7, 3, i) for i in range(20000)], dtype=np.float64)
    assert abs(v.mean()) < 0.03 and abs(v.std() - 1.0) < 0.03
    # distinct (sample, draw) streams are uncorrelated, identical arguments reproduce
    w = np.array([lib.hd_philox_normal_host(2022, 8, 3, i) for i in range(20000)], dtype=np.float64)
    assert abs(np.corrcoef(v, w)[0, 1]) < 0.03
    assert lib.hd_philox_normal_host(1, 2, 3, 4) == lib.hd_philox_normal_host(1, 2, 3, 4)


@pytest.mark.parametrize("H,L,C_", [(256, 3, 0), (256, 6, 0), (256, 9, 0), (32, 2, 1)])
def test_param_layout_matches_reference_counts(H, L, C_):
    from hierdiff_amd import EGNN_dynamics_QM9
    m = EGNN_dynamics_QM9(9, C_, 3, hidden_nf=H, n_layers=L, attention=True, tanh=True, normalization_factor=10)
    shapes = dynamics_param_shapes(9, C_, H, L, 2, True)
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == shapes[k] for k in shapes)
    n = dynamics_param_count(9, C_, H, L, 2, True)
    if C_ == 0 and H == 256:
        assert n == {3: 2968591, 6: 5932309, 9: 8896027}[L]
    syn = synthetic_state_dict(9, C_, H, L)
    m.load_numpy_state_dict(syn, prefix="dynamics.")
    blob = m.canonical_blob().numpy()
    ref = flatten_dynamics(syn, 9, C_, H, L, 2, True, prefix="dynamics.")
    assert blob.shape == ref.shape == (n,) and np.array_equal(blob, ref)


def test_diffusion_state_dict_keys_and_schedule():
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.noise_model import schedule_tables
    from tests.helpers import load
    model = DiffusionQM9(default_config(hidden_nf=32, n_layers=1))
    syn = synthetic_state_dict(9, 0, 32, 1)
    assert sorted(model.state_dict().keys()) == sorted(syn.keys())
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.items()})
    fx = load("f4_schedule")
    # 1) the network evaluated in fp64 agrees with the reference's fp32 run within fp32's own noise
    tabs = schedule_tables(model.gamma, 1000)
    assert np.abs(tabs["gamma"].numpy() - fx["gamma"]).max() < 1e-3
    assert np.all(np.diff(tabs["gamma"].numpy()) > 0), "fp64-evaluated schedule must be monotone"
    # 2) given the reference's gamma grid, the derived per-step coefficients are the reference's
    tabs = schedule_tables(model.gamma, 1000, gammas=fx["gamma"])
    np.testing.assert_allclose(tabs["coef"][:, 0].numpy(), fx["alpha_t_given_s"], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(tabs["coef"][:, 1].numpy(), fx["sigma2_t_given_s"], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(tabs["coef"][:, 2].numpy(), fx["sigma_t"], rtol=2e-6, atol=1e-7)
    sig = fx["sigma_t_given_s"] * fx["sigma_s"] / fx["sigma_t"]
    np.testing.assert_allclose(tabs["coef"][:, 3].numpy(), sig, rtol=2e-4, atol=1e-7)
    assert abs(float(tabs["tau"][999]) - 0.99900001287) < 1e-9


def test_nodes_distribution_follows_histogram():
    from hierdiff_amd import DistributionNodes
    from hierdiff_amd.geom_stats import GEOM_FRAGMENT_HISTOGRAM as H
    d = DistributionNodes(H)
    torch.manual_seed(0)
    s = d.sample(20000)
    assert min(s) >= 1 and max(s) <= 83
    tot = sum(H.values())
    mean = sum(k * v for k, v in H.items()) / tot
    assert abs(np.mean(s) - mean) < 0.15
    assert len(H) == 67 and list(H)[:3] == [26, 14, 17]


def test_unsupported_modes_raise():
    from hierdiff_amd import EGNN_dynamics_QM9
    for kw in (dict(sin_embedding=True), dict(act_fn="relu"), dict(hidden_nf=48), dict(mode="gnn_dynamics", context_node_nf=1)):
        with pytest.raises(NotImplementedError):
            EGNN_dynamics_QM9(**{**dict(in_node_nf=9, context_node_nf=0, n_dims=3), **kw})
    with pytest.raises(Exception, match="Wrong mode"):
        EGNN_dynamics_QM9(9, 0, 3, mode="something")
    g = EGNN_dynamics_QM9(9, 0, 3, hidden_nf=32, n_layers=2, mode="gnn_dynamics")            # round 3: supported (fixture F21)
    assert list(g.state_dict().keys())[:4] == ["gnn.embedding.weight", "gnn.embedding.bias", "gnn.embedding_out.weight",
                                                "gnn.embedding_out.bias"]
    assert g.state_dict()["gnn.embedding.weight"].shape == (32, 12) and g.state_dict()["gnn.gcl_1.edge_mlp.0.weight"].shape == (32, 64)
    with pytest.raises(ValueError):
        EGNN_dynamics_QM9(9, 0, 3, aggregation_method="max")
    m = EGNN_dynamics_QM9(9, 0, 3, aggregation_method="mean")            # round 3: supported (fixture F19)
    assert m._cfg.aggregation_mean == 1 and EGNN_dynamics_QM9(9, 0, 3)._cfg.aggregation_mean == 0


def test_sample_results_wire_format(tmp_path):
    """`sample_results.pkl` = pickle((results, test_names)); the stage-2 consumer does pickle.load(f)[0] and reads
    'x' [n,3] / 'h' [n,8] float tensors per molecule (generation/ar_sampling_nosize.py:328-329,387-388)."""
    import pickle
    from hierdiff_amd.sampler import load_reference_state_dict, read_results, write_results
    res = [{"x": torch.randn(5, 3), "h": torch.randn(5, 8)}, {"x": torch.randn(2, 3), "h": torch.randn(2, 8)}]
    path = tmp_path / "sample_results.pkl"
    write_results(str(path), res)
    with open(path, "rb") as f:
        blob = pickle.load(f)
    assert isinstance(blob, tuple) and len(blob) == 2 and blob[1] == []
    got = blob[0]
    assert len(got) == 2 and torch.equal(got[0]["x"], res[0]["x"]) and got[1]["h"].shape == (2, 8)
    assert torch.round(got[0]["h"][:, :5]).shape == (5, 5)          # what the consumer does with it
    r2, names = read_results(str(path))
    assert names == [] and torch.equal(r2[1]["h"], res[1]["h"])
    # a Lightning-style checkpoint with the reference's optional 'model.' prefix loads key-for-key
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.weights import synthetic_state_dict
    syn = synthetic_state_dict(9, 0, 32, 1)
    ck = tmp_path / "diffusion.ckpt"
    torch.save({"state_dict": {("model." + k if i % 2 else k): torch.from_numpy(v.copy()) for i, (k, v) in enumerate(syn.items())},
                "epoch": 3}, ck)
    sd = load_reference_state_dict(str(ck))
    assert sorted(sd) == sorted(syn)
    m = DiffusionQM9(default_config(hidden_nf=32, n_layers=1))
    m.load_state_dict(sd)
    assert np.array_equal(m.state_dict()["dynamics.egnn.embedding.weight"].numpy(), syn["dynamics.egnn.embedding.weight"])


MODEL_YAML = """\
_target_: train_module.diffusion_qm9.DiffusionQM9
cfg:
  pocket: False
  node_coarse_type: prop
  loss_type: 'vlb'
  hcontinous: true
  noise_schedule: 'learned'
  timesteps: {T}
  norm_values: [1., 1., 1.]
  norm_biases: [null,0.,0.]
  parametrization: 'eps'
  include_charges: True
  dataset: "qm9"
  conditioning: []
  data_augmentation: False
  pre_noise:
    noise_schedule: 'learned'
    timesteps: {T}
    precision: 1e-4
  dynamics:
    in_node_nf: 0
    context_node_nf: 0
    n_dims: 3
    hidden_nf: {H}
    act_fn: "silu"
    n_layers: {L}
    attention: true
    condition_time: true
    tanh: true
    mode: "egnn_dynamics"
    norm_constant: 0
    inv_sublayers: 2
    sin_embedding: False
    normalization_factor: 10
    aggregation_method: "sum"
  analyze: conf/analyze/GEOM.yaml
"""


def write_reference_style_conf(root, H=32, L=1, T=4, batch_size=3, num_batches=2, with_analyze=True):
    """A config tree with the layout and keys of the reference's `endiffusion/conf` (model/ddpmgblur.yaml, sample/default.yaml,
    analyze/GEOM.yaml), written by the test: values are this test's, the schema is what Hydra hands to DiffusionQM9."""
    conf = root / "conf"
    (conf / "model").mkdir(parents=True)
    (conf / "sample").mkdir()
    (conf / "model" / "ddpmgblur.yaml").write_text(MODEL_YAML.format(H=H, L=L, T=T))
    (conf / "sample" / "default.yaml").write_text(f"batch_size: {batch_size}\nnum_batches: {num_batches}\n")
    if with_analyze:
        (conf / "analyze").mkdir()
        (conf / "analyze" / "GEOM.yaml").write_text("5: 10\n3: 30\n8: 60\n")
    return conf


def test_cli_reads_reference_yaml_configs(tmp_path):
    """`--model-config` / `--sample-config`: the reference's own YAML files (conf/model/ddpmgblur.yaml, conf/sample/default.yaml)
    build the same model as the keyword route; `analyze` resolves like a Hydra run and falls back to the built-in histogram."""
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.sampler import load_model_config, load_sample_config
    conf = write_reference_style_conf(tmp_path, H=32, L=1, T=7)
    cfg = load_model_config(str(conf / "model" / "ddpmgblur.yaml"))
    assert cfg.timesteps == 7 and cfg.dynamics.hidden_nf == 32 and cfg.dynamics.aggregation_method == "sum"
    assert cfg.norm_biases == [None, 0.0, 0.0] and cfg.pre_noise.precision == 1e-4          # OmegaConf's reading of `1e-4`
    assert cfg.analyze == str(conf / "analyze" / "GEOM.yaml")
    assert load_sample_config(str(conf / "sample" / "default.yaml")) == (3, 2)
    m = DiffusionQM9(cfg)
    ref = DiffusionQM9(default_config(hidden_nf=32, n_layers=1, timesteps=7))
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys()) and m.T == 7
    assert m.nodes_dist.n_nodes == [5, 3, 8]                               # YAML key order, like the reference's dict
    torch.manual_seed(0)
    assert set(m.nodes_dist.sample(200)) <= {3, 5, 8}
    # without the analyze file: the built-in GEOM histogram
    conf2 = write_reference_style_conf(tmp_path / "b", with_analyze=False)
    cfg2 = load_model_config(str(conf2 / "model" / "ddpmgblur.yaml"))
    assert cfg2.analyze is None and max(DiffusionQM9(cfg2).nodes_dist.sample(500)) > 8
    # the reference's own files, stored verbatim as fixtures (tests/golden/reference_conf/conf: model, sample, analyze)
    ref_conf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_conf", "conf")
    c = load_model_config(os.path.join(ref_conf, "model", "ddpmgblur.yaml"))
    assert c.dynamics.hidden_nf == 256 and c.dynamics.n_layers == 6 and c.timesteps == 1000
    assert c.analyze == os.path.join(ref_conf, "analyze", "GEOM.yaml") and os.path.isfile(c.analyze)
    assert load_sample_config(os.path.join(ref_conf, "sample", "default.yaml")) == (2, 16)
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.yaml"
        bad.write_text("_target_: something.Else\ncfg: {}\n")
        load_model_config(str(bad))


def test_no_register_spills_in_production_kernels():
    """The edge kernels hide loads from hipcc (inline-asm loads released by hand-counted waits); a VGPR spill next to
    one would save a destination before its data has landed.  The build records hipcc's resource remarks and refuses
    to produce a library whose production kernels spill; this re-checks the recorded figures."""
    import json
    from hierdiff_amd import build
    build.build(verbose=False)
    with open(build.RESOURCES) as fh:
        res = json.load(fh)
    assert build.audit(res) == []
    prod = {k: v for k, v in res.items() if build._production(k)}
    edge = [v for k, v in prod.items() if k.startswith("_Z6k_edgeILi256")]
    assert len(edge) == 4 and all(v["Occupancy"] >= 2 and v["ScratchSize"] == 0 for v in edge)
    node = [v for k, v in prod.items() if k.startswith("_Z6k_nodeILi256")]
    assert len(node) == 3 and all(v["ScratchSize"] == 0 for v in node)          # {no update, one AB image, two AB images} x fp16 two-piece


def test_nodes_distribution_draws_equal_reference():
    """F10: same key order, probabilities and - under the same torch seed - the same draws as the reference's
    DistributionNodes on conf/analyze/GEOM.yaml (models/distributions.py:62-101, diffusion_qm9.py:114-115,349)."""
    from hierdiff_amd import DistributionNodes
    from hierdiff_amd.geom_stats import GEOM_FRAGMENT_HISTOGRAM as H
    from tests.helpers import load
    fx = load("f10_nodes_dist")
    assert list(H.keys()) == [int(k) for k in fx["keys"]] and list(H.values()) == [int(v) for v in fx["counts"]]
    d = DistributionNodes(H)
    assert np.array_equal(d.prob.numpy(), fx["prob"])
    for seed in (2022, 7, 0):
        want = fx[f"draws_seed{seed}"]
        torch.manual_seed(seed)
        assert d.sample(len(want)) == [int(v) for v in want], seed
    np.testing.assert_array_equal(d.log_prob(torch.from_numpy(fx["log_prob_idx"])).numpy(), fx["log_prob"])


def test_predefined_noise_schedules_equal_reference():
    """F11: PredefinedNoiseSchedule 'polynomial_k' / 'cosine' tables and lookups (models/noise_model.py:125-160), and
    a DiffusionQM9 built with such a schedule (state_dict key `gamma.gamma`, check_issues_norm_values)."""
    from hierdiff_amd import DiffusionQM9, PredefinedNoiseSchedule, default_config
    from hierdiff_amd.noise_model import evaluate_gamma, schedule_tables
    from tests.helpers import load
    fx = load("f11_predefined_schedules")
    t = torch.from_numpy(fx["lookup_t"])
    for sched, T, prec in (("polynomial_2", 1000, 1e-4), ("cosine", 1000, 1e-4), ("polynomial_3", 500, 1e-5),
                           ("polynomial_2", 6, 1e-4)):
        m = PredefinedNoiseSchedule(sched, T, prec)
        assert np.array_equal(m.gamma.detach().numpy(), fx[f"{sched}_T{T}"]), sched
        assert np.array_equal(m(t).detach().numpy(), fx[f"{sched}_T{T}_lookup"]), sched
        assert np.array_equal(evaluate_gamma(m, t).numpy(), fx[f"{sched}_T{T}_lookup"]), sched
    with pytest.raises(ValueError):
        PredefinedNoiseSchedule("linear", 10, 1e-4)
    cfg = default_config(hidden_nf=32, n_layers=1, timesteps=6)
    cfg["noise_schedule"] = "polynomial_2"
    cfg["loss_type"] = "l2"
    cfg["pre_noise"] = dict(noise_schedule="polynomial_2", timesteps=6, precision=1e-4)
    model = DiffusionQM9(cfg)
    assert "gamma.gamma" in model.state_dict() and not any(k.startswith("gamma.l1") for k in model.state_dict())
    tabs = schedule_tables(model.gamma, 6)
    assert np.array_equal(tabs["gamma"].numpy(), fx["polynomial_2_T6"])
    cfg2 = default_config(hidden_nf=32, n_layers=1)
    cfg2["noise_schedule"] = "learned"
    cfg2["loss_type"] = "l2"
    with pytest.raises(AssertionError):          # 'A noise schedule can only be learned with a vlb objective.'
        DiffusionQM9(cfg2)
    cfg3 = dict(cfg)
    cfg3["node_coarse_type"] = "atoms"
    with pytest.raises(NotImplementedError):
        DiffusionQM9(cfg3)
    elem = default_config(hidden_nf=32, n_layers=1)
    elem["node_coarse_type"] = "elem"
    m = DiffusionQM9(elem)
    assert m.in_node_nf == 3 and m.state_dict()["dynamics.egnn.embedding.weight"].shape == (32, 4)


def test_loss_gamma_grid_equals_rowwise_evaluation():
    """The loss value (no autograd) reads gamma at s = (t_int - 1) / T, t = t_int / T, 0 and 1 (diffusion_qm9.py:541-552)
    from a tabulated grid k / T, k = -1 .. T: same bits as evaluating the fp64 schedule row by row, for the learned network
    and for a predefined table (whose lookup at -1/T wraps to the last entry, like the reference's negative index); the
    table follows in-place updates of the schedule parameters."""
    from hierdiff_amd import DiffusionQM9, default_config
    from hierdiff_amd.noise_model import evaluate_gamma
    g = torch.Generator().manual_seed(3)
    cfgs = [default_config(hidden_nf=32, n_layers=1, timesteps=1000)]
    c2 = default_config(hidden_nf=32, n_layers=1, timesteps=50)
    c2["noise_schedule"] = "cosine"
    c2["loss_type"] = "l2"
    c2["pre_noise"] = dict(noise_schedule="cosine", timesteps=50, precision=1e-4)
    cfgs.append(c2)
    for cfg in cfgs:
        model = DiffusionQM9(cfg)
        T = model.T
        t_int = torch.cat([torch.tensor([0., 1., float(T)]), torch.randint(0, T + 1, (61,), generator=g).float()]).view(-1, 1)
        with torch.no_grad():
            for t in ((t_int - 1) / T, t_int / T, torch.zeros_like(t_int), torch.ones_like(t_int)):
                assert torch.equal(model._gamma_rows(t, "gamma_t", None), evaluate_gamma(model.gamma, t).view(-1, 1))
            assert torch.equal(model._gamma_rows(t_int / T, "gamma_t", {"gamma_t": np.full(64, 0.25, np.float32)}),
                               torch.full((64, 1), 0.25))
            if hasattr(model.gamma, "l2"):                      # learned schedule: an optimiser step must invalidate the table
                before = model._gamma_rows(t_int / T, "gamma_t", None).clone()
                model.gamma.l2.weight.add_(0.05)
                after = model._gamma_rows(t_int / T, "gamma_t", None)
                assert torch.equal(after, evaluate_gamma(model.gamma, t_int / T).view(-1, 1)) and not torch.equal(after, before)
        if hasattr(model.gamma, "l2"):                          # with autograd the network itself is in the graph
            with torch.enable_grad():
                assert model._gamma_rows(t_int / T, "gamma_t", None).requires_grad


def test_sample_batches_merges_consecutive_batches_host_side():
    """Host logic of `DiffusionQM9.sample_batches` (diffusion_qm9.py:397-436): the molecule sizes are drawn batch by batch
    exactly as the reference's loop draws them, consecutive batches form device batches of at most `merge_batches`
    molecules (whole batches only), global sample ids and the per-batch context value follow the loop's order.  The
    device half is tests/test_gpu_configs.py::test_merged_sample_batches_equal_the_loop."""
    import torch
    from hierdiff_amd import DiffusionQM9, default_config
    m = DiffusionQM9(default_config(hidden_nf=32, n_layers=1, timesteps=4))
    torch.manual_seed(7)
    loop_sizes = [n for _ in range(5) for n in m.nodes_dist.sample(3)]
    calls = []
    m._sample_sizes = lambda sizes, dev, ctx, base, pocket=None, context_full=None: (
        calls.append((list(sizes), ctx, base, context_full)) or [{"x": None}] * len(sizes))
    torch.manual_seed(7)
    res, names = m.sample_batches(3, 5, "cpu", context_range=[0.5, 1.5], sample_id_base=100)
    assert names == [] and len(res) == 15 and len(calls) == 1
    assert calls[0][0] == loop_sizes and calls[0][2] == 100
    assert calls[0][1] == [0.5] * 3 + [1.5] * 3 + [0.5] * 3 + [1.5] * 3 + [0.5] * 3
    calls.clear()
    m.merge_batches = 7                                   # two whole batches of 3 per device batch
    torch.manual_seed(7)
    m.sample_batches(3, 5, "cpu", sample_id_base=100)
    assert [c[0] for c in calls] == [loop_sizes[0:6], loop_sizes[6:12], loop_sizes[12:15]]
    assert [c[2] for c in calls] == [100, 106, 112] and all(c[1] is None for c in calls)
    calls.clear()
    m.merge_batches = 2048                                # the edge limit cuts instead: whole batches, greedily
    per_batch = [sum(n * (n - 1) for n in loop_sizes[3 * i:3 * i + 3]) for i in range(5)]
    m.merge_edges = per_batch[0] + per_batch[1] + 1
    torch.manual_seed(7)
    m.sample_batches(3, 5, "cpu", sample_id_base=0)
    got = [len(c[0]) // 3 for c in calls]
    assert sum(got) == 5 and got[0] >= 2
    lo = 0
    for nb in got:                                        # every device batch is within the limit unless it is a single batch
        e = sum(per_batch[lo:lo + nb])
        assert nb == 1 or e <= m.merge_edges
        lo += nb


def test_sample_batches_does_not_merge_width_dependent_configurations():
    """`aggregation_method='mean'` divides by the padded N of the call and `mode='gnn_dynamics'` sends messages
    over padded nodes and draws with torch.randn - a molecule's result depends on the padded width of its batch, so these run the
    reference's loop, batch by batch (no merge); so does a context_range whose entries are not one scalar per batch."""
    import torch
    from hierdiff_amd import DiffusionQM9, default_config
    for kw in (dict(aggregation_method="mean"), dict(mode="gnn_dynamics")):
        cfg = default_config(hidden_nf=32, n_layers=1, timesteps=4)
        cfg.dynamics.update(kw)
        m = DiffusionQM9(cfg)
        assert m.merge_batches and m.noise_mode == "philox"
        calls = []
        m.sample = lambda n, dev, context=None, pocket_cond=None, sample_id_base=0: (calls.append((n, sample_id_base)) or [{"x": None}] * n)
        m._sample_sizes = lambda *a, **k: (_ for _ in ()).throw(AssertionError("merged"))
        res, _ = m.sample_batches(3, 4, "cpu", sample_id_base=10)
        assert calls == [(3, 10), (3, 13), (3, 16), (3, 19)] and len(res) == 12
    m = DiffusionQM9(default_config(hidden_nf=32, n_layers=1, timesteps=4, context_node_nf=1))
    calls = []
    m.sample = lambda n, dev, context=None, pocket_cond=None, sample_id_base=0: (calls.append(context) or [{"x": None}] * n)
    per_sample = torch.arange(3.0).reshape(3, 1, 1)
    m.sample_batches(3, 2, "cpu", context_range=[per_sample])
    assert len(calls) == 2 and all(c is per_sample for c in calls)


def test_sample_broadcasts_context_like_the_reference():
    """`sample(num_samples, device, context)`: `zeros([num_samples, n_max, 1]) + context` (diffusion_qm9.py:352) - a scalar or
    any tensor broadcastable against that shape, e.g. one value per sample; ADVICE round 3: the per-sample form must not be
    reduced to its first element."""
    import pytest
    import torch
    from hierdiff_amd import DiffusionQM9, default_config
    m = DiffusionQM9(default_config(hidden_nf=32, n_layers=1, timesteps=4, context_node_nf=1))
    seen = {}

    def fake(node_mask, edge_mask, context, sample_id_base=0, pocket=None):
        seen["ctx"] = context
        B, N = node_mask.shape[:2]
        return torch.zeros(B, N, 3), torch.zeros(B, N, 8)
    m.sample_from_masks = fake
    torch.manual_seed(3)
    sizes = m.nodes_dist.sample(4)
    per_sample = torch.tensor([0.5, 1.5, 2.5, 3.5]).reshape(4, 1, 1)
    torch.manual_seed(3)
    out = m.sample(4, "cpu", context=per_sample)
    assert seen["ctx"].shape == (4, max(sizes), 1)
    assert torch.equal(seen["ctx"], per_sample.expand(4, max(sizes), 1))
    assert [float(o["context"][0, 0]) for o in out] == [0.5, 1.5, 2.5, 3.5] and out[1]["context"].shape == (sizes[1], 1)
    torch.manual_seed(3)
    m.sample(4, "cpu", context=2.0)
    assert torch.equal(seen["ctx"], torch.full((4, max(sizes), 1), 2.0))
    with pytest.raises((ValueError, RuntimeError)):
        m.sample(4, "cpu", context=torch.zeros(3, 1, 1))


def test_optimizer_generation_counts_steps_of_any_optimizer():
    """Round 5: torch's fused optimizers change parameters without bumping their `_version`, which the packed-weight / schedule caches
    of the package were keyed by; the keys now also carry `_lib.optimizer_generation()`, a process-wide count of optimizer steps from
    a global post-step hook.  The count must move with every step of every optimizer (an over-approximation costs a re-pack, a
    missed step would leave an evaluation on stale weights)."""
    import torch
    from hierdiff_amd import _lib
    g0 = _lib.optimizer_generation()
    p, q = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    o1, o2 = torch.optim.SGD([p], lr=0.1), torch.optim.AdamW([q], lr=0.1)
    p.grad, q.grad = torch.ones(3), torch.ones(2)
    o1.step()
    assert _lib.optimizer_generation() == g0 + 1
    o2.step(); o1.step()
    assert _lib.optimizer_generation() == g0 + 3
    # and the schedule twin of the noise model is rebuilt on it even when no version moved
    from hierdiff_amd.noise_model import GammaNetwork, _fp64_twin
    net = GammaNetwork()
    t1 = _fp64_twin(net)
    assert _fp64_twin(net) is t1
    v0 = net.gamma_0._version
    net.gamma_0.data.add_(1.0)          # an in-place write that bumps no version counter of the parameter (what a fused optimizer does)
    assert net.gamma_0._version == v0
    # round 6: such a write is seen too (the key hit is confirmed by a content digest, _lib.ImageGuard) - rounds 2-5 documented
    # this case as a limit of the cache
    t2 = _fp64_twin(net)
    assert t2 is not t1 and float(t2.gamma_0) == float(net.gamma_0)
    assert _fp64_twin(net) is t2
    o1.step()
    assert _fp64_twin(net) is not t2          # the optimizer-step count is part of the key, whichever optimizer stepped


def test_configure_optimizers_picks_the_fused_form_only_on_the_gpu():
    """trainer.configure_optimizers: the reference's AdamW / StepLR values (conf/optim/adamw.yaml, conf/scheduler/step.yaml); torch's fused
    multi-tensor update only when every parameter lives on the GPU (a CPU model gets the default form), and on request."""
    import torch
    from hierdiff_amd.trainer import configure_optimizers
    m = torch.nn.Linear(4, 3)
    opt, sched = configure_optimizers(m)
    assert isinstance(opt, torch.optim.AdamW) and not opt.defaults.get("fused")
    assert opt.defaults["lr"] == 4.0e-4 and opt.defaults["weight_decay"] == 4.0e-8
    assert isinstance(sched, torch.optim.lr_scheduler.StepLR) and sched.step_size == 15 and sched.gamma == 0.1
    opt2, _ = configure_optimizers(m, fused=False)
    assert not opt2.defaults.get("fused")
    with torch.enable_grad():
        m(torch.ones(2, 4)).sum().backward()
    opt.step()          # the CPU form runs


def test_image_guard_confirms_key_hits_by_content():
    """_lib.ImageGuard (round 6): a cached image is valid only if the cheap key AND the content digest of the tensors it was made
    from are unchanged; on the CPU the digest is a host hash (cuda tensors: csrc/k_digest.hpp, tests/test_gpu_training.py)."""
    import torch
    a = [torch.arange(12, dtype=torch.float32).view(3, 4), torch.zeros(0), torch.ones(5, dtype=torch.float64)]
    g = _lib.ImageGuard()
    assert not g.valid(("k",), a)
    g.store(("k",), a)
    assert g.valid(("k",), a) and not g.valid(("other",), a)
    ver = a[0]._version
    a[0].data[2, 3] += 1.0                                   # `.data`: the tensor's own version counter does not move
    assert a[0]._version == ver and not g.valid(("k",), a)
    a[0].data[2, 3] -= 1.0
    assert g.valid(("k",), a)
    assert _lib.params_digest([torch.zeros(2, 3)]) != _lib.params_digest([torch.zeros(3, 2)])      # shape is part of the host hash
    g.clear()
    assert not g.valid(("k",), a)
