"""Classifier-free guidance: host side (argument resolution, the null context, context dropout for training).

A guided transition evaluates the network under the context and under a null context and feeds
    eps^ = eps_u + w (eps_c - eps_u)
into the unchanged update (hd_sample_path_guided / hd_guide_combine, include/hierdiff_hip.h).  Everything here is host arithmetic:
`resolve` turns the `guidance_scale` / `guidance_context` / `guidance_rescale` keywords of the sampling entry points into None (the
unguided code path, untouched) or a `Guidance`, raising every argument error before a device is looked at.

Guidance needs a model that has seen the null context: `drop_context` is the training-side switch (`DiffusionQM9.context_drop_prob`).
Mechanism only - which scale helps on a trained checkpoint is for the user to validate."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch


class Guidance:
    """A resolved request: `w` float32 [1] (shared) or [B] (per molecule) on the CPU, `context` [B,N,C] or None (= the model's null
    context), `rescale` phi in [0, 1]."""

    def __init__(self, w: torch.Tensor, context: Optional[torch.Tensor], rescale: float):
        self.w, self.context, self.rescale = w, context, float(rescale)

    @property
    def rows(self) -> int:
        return int(self.w.numel())


def check_rescale(phi) -> float:
    if isinstance(phi, bool) or not isinstance(phi, (int, float, np.integer, np.floating)) or not (0.0 <= float(phi) <= 1.0):
        raise ValueError(f"guidance_rescale must be a number in [0, 1], got {phi!r}")
    return float(phi)


def check_null_context(null_context, C: int) -> torch.Tensor:
    """The model's `null_context` (a float or a [C] vector) as a float32 [C] tensor."""
    v = torch.as_tensor(null_context, dtype=torch.float32).detach().cpu()
    if v.dim() == 0:
        v = v.expand(C).clone()
    if tuple(v.shape) != (C,) or not bool(torch.isfinite(v).all()):
        raise ValueError(f"null_context must be a finite float or a [{C}] vector, got {null_context!r}")
    return v


def masked_null_context(null_context, node_mask: torch.Tensor, C: int) -> torch.Tensor:
    """[B,N,C]: the null context broadcast over the nodes, rows of masked nodes 0."""
    v = check_null_context(null_context, C).to(node_mask.device)
    B, N = int(node_mask.shape[0]), int(node_mask.shape[1])
    return (v.view(1, 1, C) * node_mask.reshape(B, N, 1).to(torch.float32)).contiguous()


def is_sequence_scale(scale) -> bool:
    """`sample_batches` also takes a list / tuple of scales, one per batch (cycled like context_range)."""
    return isinstance(scale, (list, tuple))


def check_model(model, what: str = "guidance", pocket=None, needs_noise: bool = True) -> None:
    """Configuration errors of a guided call (no device needed)."""
    C = int(getattr(model.dynamics, "context_node_nf", 0) or 0)
    if C < 1:
        raise ValueError(f"{what}: guidance needs a context-conditioned model (context_node_nf > 0)")
    from .plan import unsupported
    unsupported(model, f"{what}: guidance", pocket, needs_noise)


def resolve(model, scale, context, rescale, B: Optional[int] = None, N: Optional[int] = None, what: str = "guidance",
            pocket=None, needs_noise: bool = True) -> Optional[Guidance]:
    """Keywords (None: the model's `guidance_scale` / `guidance_context` / `guidance_rescale`) -> None for today's unguided path, or a
    `Guidance`.  `scale` None, or a scalar 1.0 without a `guidance_context`, is the unguided path.  B / N given: shapes are checked."""
    scale = model.guidance_scale if scale is None else scale
    context = model.guidance_context if context is None else context
    rescale = model.guidance_rescale if rescale is None else rescale
    phi = check_rescale(rescale)
    if scale is None:
        if context is not None:
            raise ValueError("guidance_context given without a guidance_scale")
        return None
    if isinstance(scale, bool):
        raise ValueError(f"guidance_scale must be a number or a [B] tensor, got {scale!r}")
    if isinstance(scale, (int, float, np.integer, np.floating)):
        w = torch.tensor([float(scale)], dtype=torch.float32)
        scalar = True
    else:
        try:
            w = torch.as_tensor(scale, dtype=torch.float32).detach().cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"guidance_scale must be a number or a [B] tensor, got {scale!r}") from None
        scalar = w.dim() == 0
        w = w.reshape(1) if scalar else w
        if w.dim() != 1 or w.numel() < 1:
            raise ValueError(f"guidance_scale must be a number or a [B] tensor, got shape {tuple(w.shape)}")
        if not scalar and B is not None and w.numel() != B:
            raise ValueError(f"guidance_scale must hold one scale per molecule ([{B}]), got {w.numel()}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("guidance_scale must be finite")
    if scalar and float(w[0]) == 1.0 and context is None:
        return None
    check_model(model, what, pocket, needs_noise)
    C = int(model.dynamics.context_node_nf)
    check_null_context(model.null_context, C)
    if context is not None:
        if not isinstance(context, torch.Tensor):
            raise ValueError("guidance_context must be a [B, N, C] tensor")
        if (context.dim() != 3 or context.shape[2] != C or (B is not None and int(context.shape[0]) != B)
                or (N is not None and int(context.shape[1]) != N)):
            raise ValueError(f"guidance_context must be [{B if B is not None else 'B'}, {N if N is not None else 'N'}, {C}], "
                             f"got {tuple(context.shape)}")
    return Guidance(w.contiguous(), context, phi)


def batch_scales(scale, num_batches: int, batch_size: int):
    """`sample_batches`: a sequence of scales cycled per batch -> one scale per molecule of the merged run (a [num_batches *
    batch_size] tensor), and the per-batch list for the unmerged loop."""
    per_batch = []
    for i in range(num_batches):
        v = scale[i % len(scale)]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"guidance_scale sequence entries must be finite numbers, got {v!r}")
        per_batch.append(float(v))
    if not per_batch:
        raise ValueError("guidance_scale sequence is empty")
    return per_batch


def drop_context(context: torch.Tensor, p: float, null_context, node_mask: torch.Tensor,
                 generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Context dropout for training: with probability p the WHOLE context of a molecule (all its nodes; one Bernoulli draw per
    molecule) is replaced by the masked null context.  p == 0 returns `context` itself.  The draws come from `generator` (a CPU
    generator, or None = torch's default CPU generator), so a seeded generator reproduces the result on any device."""
    if isinstance(p, bool) or not (0.0 <= float(p) <= 1.0):
        raise ValueError(f"context_drop_prob must lie in [0, 1], got {p!r}")
    if float(p) == 0.0:
        return context
    B, N = int(context.shape[0]), int(context.shape[1])
    C = int(context.shape[-1])
    nm = node_mask.reshape(B, N, 1).to(context.device)
    null = masked_null_context(null_context, nm, C).to(context.dtype)
    drop = (torch.rand(B, generator=generator) < float(p)).to(context.device)
    return torch.where(drop.view(B, 1, 1), null, context.reshape(B, N, C))
