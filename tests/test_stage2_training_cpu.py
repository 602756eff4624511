"""Stage-2 training, CPU tier: the training module's optimiser configuration, the C-ABI symbols of the E_GCL backward and the
absence of a CPU fallback in the differentiable paths."""
import pytest
import torch

from oracle.edge_denoise_batches import train_batch


def _module_cfg(H=32):
    return {"model": dict(vocab_size=50, in_node_nf=8, hidden_nf=H, out_node_nf=49, array_dict=None, full_softmax=True,
                          focal_loss=5, edge_loss=1, node_loss=2)}


def test_configure_optimizers_carries_the_reference_values():
    from hierdiff_amd.edge_denoise_train import CLIP_VAL, EdgeDenoise
    mod = EdgeDenoise(_module_cfg())
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


def test_new_symbols_load():
    from hierdiff_amd import _lib
    lib = _lib.load()
    for name in ("hd_egcl_saved_floats", "hd_egcl_forward_train", "hd_egcl_backward"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.hd_egcl_saved_floats(None, 4, 4) == 0
    assert lib.hd_egcl_backward(*([None] * 16)) != 0          # null handle: an error code, no crash
    assert b"null" in lib.hd_last_error()


def test_training_forward_without_gpu_raises():
    from hierdiff_amd import _lib
    from hierdiff_amd.edge_denoise import Edge_denoise
    from hierdiff_amd.stage2 import E_GCL
    m = Edge_denoise(**_module_cfg()["model"])
    with pytest.raises(_lib.HierDiffHipError):
        m.training_forward(train_batch(2, [4, 5], [2, 3], vocab_size=50))
    layer = E_GCL(32, 32, 32, edges_in_d=32)
    with torch.enable_grad(), pytest.raises(_lib.HierDiffHipError):
        layer(torch.zeros(3, 32), [torch.tensor([0, 1]), torch.tensor([1, 2])], torch.zeros(3, 3), edge_attr=torch.zeros(2, 32))
