"""Stage-2 training module `EdgeDenoise` - drop-in for /root/reference/trainmodule/Edge_denoise.py (what train_edge_denoise_pl.py
trains): the `Edge_denoise` decoder on MI355X with a differentiable objective (`Edge_denoise.training_forward`).

Like `DiffusionQM9` the class derives from LightningModule when pytorch_lightning is installed and from nn.Module otherwise;
without Lightning, `hierdiff_amd.trainer.ddp_step(module, batch, opt, clip_val=1.0, overlap=False)` is the optimisation step
(conf/trainer/default.yaml: gradient_clip_val 1, gradient_clip_algorithm norm) and `training_epoch_end` steps the scheduler.
"""
from __future__ import annotations

from typing import Any, Dict

import torch
import torch.nn as nn

from .diffusion import _Base, _get
from .edge_denoise import Edge_denoise

# conf/optim/adamw.yaml, conf/scheduler/step_denoise.yaml (stepped once per epoch), conf/trainer/default.yaml
OPTIM = {"lr": 4.0e-4, "weight_decay": 1.0e-8, "amsgrad": True}
SCHEDULER = {"step_size": 3, "gamma": 0.1}
CLIP_VAL = 1.0

_KEYS = ("focal_loss", "focal_accuracy", "edge_loss", "edge_accuracy", "node_loss", "node_accuracy")


class EdgeDenoise(_Base):
    """trainmodule/Edge_denoise.py:EdgeDenoise.  `cfg.model` holds Edge_denoise's constructor arguments."""

    def __init__(self, cfg: Dict[str, Any]) -> None:
        super().__init__()
        self.cfg = cfg
        model_cfg = _get(cfg, "model", None)
        self.model = Edge_denoise(**dict(model_cfg if model_cfg is not None else {}))
        self._sched = None

    def forward(self, batch):
        return self.model.training_forward(batch)

    def _log(self, prefix: str, result) -> None:
        if _Base is nn.Module or not hasattr(self, "log"):
            return
        self.log(f"{prefix}_loss", result["total_loss"], on_step=True, prog_bar=True, sync_dist=True)
        for k in _KEYS:
            self.log(f"{prefix}_{k}", result[k], on_step=True, prog_bar=True, sync_dist=True)

    def training_step(self, batch, batch_idx=0):
        result = self.forward(batch)
        self._log("training", result)
        return result["total_loss"]

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        was = self.model.training
        self.model.eval()
        try:
            result = self.model(batch)
        finally:
            self.model.train(was)
        self._log("validation", result)
        return result

    def configure_optimizers(self):
        """AdamW(lr 4e-4, weight_decay 1e-8, amsgrad) and StepLR(3, 0.1) per epoch, the reference's shipped configuration."""
        optimizer = torch.optim.AdamW(self.model.parameters(), **OPTIM)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, **SCHEDULER)
        self._sched = scheduler
        return [optimizer], [{"scheduler": scheduler, "interval": "epoch", "frequency": 1}]

    def training_epoch_end(self, result=None):
        sch = self.lr_schedulers() if _Base is not nn.Module else self._sched
        if isinstance(sch, (list, tuple)):
            sch = sch[0]
        if sch is not None:
            sch.step()
