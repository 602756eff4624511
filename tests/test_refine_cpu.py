"""Refine model (hierdiff_amd.refine.Node2Vec, hierdiff_amd.refine_train.Refine), CPU tier: the oracle against the fixtures recorded
from the reference, parameter names / shapes, the host helpers, the C-ABI symbols, the missing CPU fallback, the optimiser
configuration and the reference's error quirks (raised on the host, before anything reaches a device)."""
import copy

import numpy as np
import pytest
import torch

from tests import refine_oracle as ro

TRAIN = ["r1_refine_train_h64", "r2_refine_train_h256"]
CHECK = ["r3_refine_check_h64_k1", "r4_refine_check_h64_k3"]


def _weights(fx):
    from hierdiff_amd.refine import synthetic_refine_state_dict
    sd = synthetic_refine_state_dict(780, 8, int(fx["hidden"]), 2, int(fx["weight_seed"]))
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


def _model(H=64):
    from hierdiff_amd.refine import Node2Vec
    size_dict, _ = ro.load_size_dict()
    return Node2Vec(size_dict, 780, 8, H, 2)


@pytest.mark.parametrize("name", TRAIN)
def test_oracle_reproduces_training_fixtures(name):
    fx = ro.load(name)
    size_dict, _ = ro.load_size_dict()
    out = ro.forward(_weights(fx), size_dict, 2, ro.train_batch(fx))
    np.testing.assert_allclose(out["logits"].numpy(), fx["logits"], rtol=0, atol=1e-5)
    assert abs(float(out["loss"]) - float(fx["loss"])) <= 1e-5 * max(1.0, abs(float(fx["loss"])))
    assert float(out["accuracy"]) == float(fx["accuracy"])


@pytest.mark.parametrize("name", CHECK)
def test_oracle_reproduces_check_node_fixtures(name):
    fx = ro.load(name)
    _, mol_sizes = ro.load_size_dict()
    nodes = ro.tree_nodes(fx)
    logp, ks, ids, flags = ro.check_node(_weights(fx), 2, ro.StubVocab(mol_sizes), nodes, fx["edges"], list(range(len(nodes))),
                                         [nd.wid for nd in nodes], int(fx["check_num"]))
    np.testing.assert_allclose(logp, fx["logp"], rtol=0, atol=1e-5)
    assert (ks == fx["ks"]).all() and (ids == fx["ids"]).all() and (flags == fx["flags"]).all()


def test_check_num_shrink_fixture_covers_the_quirk():
    fx = ro.load("r4_refine_check_h64_k3")
    ks = list(fx["ks"])
    first = next(i for i, k in enumerate(ks) if k < 3)
    assert all(k == ks[first] for k in ks[first:]) and ks[first] < 3


def test_state_dict_matches_the_reference_layout():
    from hierdiff_amd.refine import Node2Vec, refine_param_shapes
    z = ro.load("r0_refine_size_dict")
    names, shapes = [str(n) for n in z["names"]], z["shapes"]
    size_dict, _ = ro.load_size_dict()
    m = Node2Vec(size_dict, 780, 8, 256, 2)
    sd = m.state_dict()
    assert len(sd) == 94
    assert list(sd) == names
    assert [list(t.shape) for t in sd.values()] == shapes
    assert [list(s) for s in refine_param_shapes(780, 8, 256, 2).values()] == shapes
    ckpt = {"model." + k: v for k, v in sd.items()}                 # ar_sampling.py:340-341 strips the Lightning prefix
    m.load_state_dict({k.replace("model.", ""): v for k, v in ckpt.items()})


def test_size_dict_from_a_pickle_path(tmp_path):
    import pickle
    from hierdiff_amd.refine import Node2Vec
    size_dict, _ = ro.load_size_dict()
    p = tmp_path / "size_dict.pkl"
    p.write_bytes(pickle.dumps(size_dict))
    assert Node2Vec(str(p), 780, 8, 64, 2).size_dict == size_dict


def test_host_helpers_equal_the_reference():
    from hierdiff_amd.refine import flat_add_and_concat, get_bfs_depth_edges
    for case in ro.load("r0_refine_size_dict")["helpers"]:
        per = [get_bfs_depth_edges(case["edges"], c, case["n"]) for c in case["centers"]]
        assert per == case["bfs"]
        arg = copy.deepcopy(per) if per else [[], []]
        assert flat_add_and_concat(arg, case["n"]) == case["flat"]
    with pytest.raises(IndexError):                                # a lone node: the reference's own failure
        get_bfs_depth_edges([[], []], 0, 1)


def test_new_symbols_load_and_null_arguments_return_an_error_code():
    from hierdiff_amd import _lib
    lib = _lib.load()
    for name in ("hd_refine_embed_forward", "hd_refine_embed_backward", "hd_sqdist_forward", "hd_sqdist_backward",
                 "hd_cand_xent_forward", "hd_cand_xent_backward"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.hd_sqdist_forward(None, None, None, None) != 0
    assert b"null" in lib.hd_last_error()
    assert lib.hd_sqdist_backward(None, None, None, None, None) != 0
    assert lib.hd_refine_embed_forward(0, None, None, 4, 8, 2, 2, None, None, None, 24, 0, 16, None, None) != 0
    assert lib.hd_refine_embed_backward(0, None, None, 4, 8, 2, 2, None, 24, 0, 16, None, None, None) != 0
    assert lib.hd_cand_xent_forward(0, 2, None, 8, 8, None, None, 1, None, None, 1, None, None, None, None, None) != 0
    assert lib.hd_cand_xent_backward(0, 2, None, 8, 8, None, None, 1, None, None, None, None, None) != 0
    assert b"null" in lib.hd_last_error()


@pytest.mark.autograd
def test_cpu_tensors_raise_hierdiff_hip_error():
    from hierdiff_amd import _lib
    fx = ro.load("r1_refine_train_h64")
    m = _model()
    with pytest.raises(_lib.HierDiffHipError):
        m(ro.train_batch(fx))
    _, mol_sizes = ro.load_size_dict()
    nodes = ro.tree_nodes(ro.load("r3_refine_check_h64_k1"))
    with pytest.raises(_lib.HierDiffHipError):
        m.check_node(ro.StubVocab(mol_sizes), nodes, ro.load("r3_refine_check_h64_k1")["edges"], [0], [nodes[0].wid], "cpu")


def _check_args():
    fx = ro.load("r3_refine_check_h64_k1")
    _, mol_sizes = ro.load_size_dict()
    return ro.StubVocab(mol_sizes), ro.tree_nodes(fx), fx["edges"]


def test_pad_wid_outside_its_candidate_set_raises_value_error():
    vocab, nodes, edges = _check_args()
    wrong = next(i for i in range(780) if i not in vocab.get_size(nodes[0].size))
    with pytest.raises(ValueError):
        _model().check_node(vocab, nodes, edges, [0], [wrong], "cpu")


def test_label_outside_its_candidate_set_raises_value_error():
    fx = ro.load("r1_refine_train_h64")
    batch = ro.train_batch(fx)
    size_dict, _ = ro.load_size_dict()
    s = int(batch["size"][0, batch["predict_idx"][0]])
    batch["label"][0] = next(i for i in range(780) if i not in size_dict[s])
    with pytest.raises(ValueError):
        _model()(batch)


def test_size_out_of_range_raises_before_any_launch():
    vocab, nodes, edges = _check_args()
    nodes[2].size = 26
    with pytest.raises(IndexError):
        _model().check_node(vocab, nodes, edges, [0], [nodes[0].wid], "cpu")


def test_size_without_candidates_raises_type_error():
    vocab, nodes, edges = _check_args()
    nodes[1].size = 25                                            # no fragment of 25 heavy atoms in the shipped size_dict
    assert vocab.get_size(25) == []
    with pytest.raises(TypeError):
        _model().check_node(vocab, nodes, edges, [1], [nodes[1].wid], "cpu")


def test_configure_optimizers_carries_the_reference_values():
    from hierdiff_amd.refine_train import CLIP_VAL, Refine
    size_dict, _ = ro.load_size_dict()
    mod = Refine({"model": dict(size_dict=size_dict, vocab_size=780, feature_size=8, hidden_size=64, n_layers=2)})
    [opt], [sched] = mod.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW)
    g = opt.param_groups[0]
    assert g["lr"] == pytest.approx(4e-4) and g["weight_decay"] == pytest.approx(1e-8) and g["amsgrad"] is True
    assert sum(p.numel() for p in g["params"]) == sum(p.numel() for p in mod.model.parameters())
    s = sched["scheduler"]
    assert isinstance(s, torch.optim.lr_scheduler.StepLR) and s.step_size == 3 and s.gamma == pytest.approx(0.1)
    assert sched["interval"] == "epoch" and CLIP_VAL == 1.0
    for _ in range(3):
        mod.training_epoch_end([])
    assert opt.param_groups[0]["lr"] == pytest.approx(4e-5)


def test_epoch_end_metrics_gather_the_steps():
    from hierdiff_amd.refine_train import Refine
    size_dict, _ = ro.load_size_dict()
    mod = Refine({"model": dict(size_dict=size_dict, vocab_size=780, feature_size=8, hidden_size=64, n_layers=2)})
    steps = [{"loss": torch.tensor(2.0), "accuracy": torch.tensor(0.5)}, {"loss": torch.tensor(4.0), "accuracy": torch.tensor(0.0)}]
    m = mod.validation_epoch_end(steps)
    assert float(m["loss"]) == 3.0 and float(m["accuracy"]) == 0.25
