"""Refine training module `Refine` - drop-in for trainmodule/Refine.py of the reference (what train_refine_pl.py trains): the
`Node2Vec` refine model on MI355X, differentiable when autograd is recording (`refine.Node2Vec.forward`).

Like `EdgeDenoise` the class derives from LightningModule when pytorch_lightning is installed and from nn.Module otherwise;
without Lightning, `hierdiff_amd.trainer.ddp_step(module, batch, opt, clip_val=1.0, overlap=False)` is the optimisation step
(conf/trainer/default.yaml: gradient_clip_val 1) and `training_epoch_end` steps the scheduler.
"""
from __future__ import annotations

from typing import Any, Dict

import torch
import torch.nn as nn

from .diffusion import DiffusionQM9, _Base, _get
from .refine import Node2Vec

# conf/optim/adamw.yaml, conf/scheduler/step.yaml (stepped once per epoch), conf/trainer/default.yaml
OPTIM = {"lr": 4.0e-4, "weight_decay": 1.0e-8, "amsgrad": True}
SCHEDULER = {"step_size": 3, "gamma": 0.1}
CLIP_VAL = 1.0


class Refine(_Base):
    """trainmodule/Refine.py:Refine.  `cfg.model` holds Node2Vec's constructor arguments (conf/model/refine.yaml)."""

    def __init__(self, cfg: Dict[str, Any]) -> None:
        super().__init__()
        self.cfg = cfg
        model_cfg = _get(cfg, "model", None)
        self.model = Node2Vec(**dict(model_cfg if model_cfg is not None else {}))
        self._sched = None

    def forward(self, batch):
        return self.model(batch)

    # the reference's epoch-end plumbing: rank, all_gather over the base class or torch.distributed, logging without Lightning
    _rank = DiffusionQM9._rank
    _gather_ranks = DiffusionQM9._gather_ranks
    _log = DiffusionQM9._log

    def training_step(self, batch, batch_idx=0):
        result = self.forward(batch)
        self._log("training_loss", result["loss"], on_step=True, prog_bar=True, sync_dist=True)
        self._log("training_accuracy", result["accuracy"], on_step=True, prog_bar=True, sync_dist=True)
        return result["loss"]

    def training_epoch_end(self, result=None):
        sch = self.lr_schedulers() if _Base is not nn.Module else self._sched
        if isinstance(sch, (list, tuple)):
            sch = sch[0]
        if sch is not None:
            sch.step()

    def configure_optimizers(self):
        """AdamW(lr 4e-4, weight_decay 1e-8, amsgrad) and StepLR(3, 0.1) per epoch, the reference's shipped configuration."""
        optimizer = torch.optim.AdamW(self.model.parameters(), **OPTIM)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, **SCHEDULER)
        self._sched = scheduler
        return [optimizer], [{"scheduler": scheduler, "interval": "epoch", "frequency": 1}]

    def _compute_metrics(self, result):
        return {"loss": result["loss"].mean(), "accuracy": result["accuracy"].mean()}

    def _gather_result(self, result):
        """List of per-step dicts -> one dict of tensors: steps joined (tensors concatenated, scalars stacked), then ranks."""
        keys = list(result[0].keys())
        steps = {}
        for key in keys:
            first = result[0][key]
            if first.dim() > 0:
                steps[key] = torch.cat([r[key] for r in result])
            else:
                steps[key] = torch.stack([r[key].detach() for r in result]).to(first)
        return {key: torch.cat(list(self._gather_ranks(steps[key]))) for key in keys}

    def validation_step(self, batch, batch_idx=0):
        return self.forward(batch)

    def validation_epoch_end(self, result):
        metrics = self._compute_metrics(self._gather_result(result))
        self._log("val_loss", metrics["loss"], on_epoch=True, prog_bar=True, sync_dist=True)
        self._log("val_accuracy", metrics["accuracy"], on_epoch=True, prog_bar=True, sync_dist=True)
        return metrics

    def test_step(self, batch, batch_idx=0):
        return self.forward(batch)

    def test_epoch_end(self, result):
        result = self._gather_result(result)
        if self._rank() == 0:
            self._log("test_loss", result["loss"], on_epoch=True, sync_dist=True)
