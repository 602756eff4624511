"""Scoring given molecules: the term lists of the every-timestep variational bound and their rows (host arithmetic only).

`DiffusionQM9.nll_full` evaluates  NLL(S) = kl_prior + (T / K) sum_{t in S} L_t + neg_log_constants + L_0 - delta_log_px  with
L_t = w_t e_t, e_t = sum (eps_t - eps^_t)^2 and w_t = 0.5 expm1(gamma_t - gamma_{t-1}) inside the library's loop (hd_nll_terms,
include/hierdiff_hip.h).  Here: which t belong to S, and the rows {alpha_t, sigma_t, w_t, 0} from the SAME gamma grid the samplers
use (`noise_model.schedule_tables`).  Scores of untrained weights mean nothing chemically; this is the mechanism.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import paths


def resolve_terms(T: int, terms: Optional[int] = None, timesteps: Optional[Sequence[int]] = None) -> List[int]:
    """The term list in the order the library adds it (descending t): all of T .. 1 (default, the full bound), the visited t of a
    K-step uniform path `paths.uniform_path(T, K)[:-1]` (`terms=K`; T is always among them), or an explicit subset of 1 .. T
    (`timesteps`, any order, no repeats - sorted here, so that a score does not depend on how the caller wrote the list)."""
    T = int(T)
    if terms is not None and timesteps is not None:
        raise ValueError("give either terms or timesteps, not both")
    if timesteps is not None:
        try:
            vals = list(timesteps)
        except TypeError:
            raise ValueError(f"timesteps must be a sequence of integers, got {timesteps!r}") from None
        out = []
        for v in vals:
            if isinstance(v, torch.Tensor) and v.numel() == 1 and not v.is_floating_point():
                v = int(v)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"timesteps must hold integers, got {v!r}")
            if not (1 <= int(v) <= T):
                raise ValueError(f"timesteps must lie in 1 .. {T}, got {int(v)}")
            out.append(int(v))
        if not out:
            raise ValueError("timesteps must name at least one term")
        if len(set(out)) != len(out):
            raise ValueError("timesteps must not repeat a term")
        return sorted(out, reverse=True)
    if terms is None:
        return list(range(T, 0, -1))
    if isinstance(terms, bool) or not isinstance(terms, (int, np.integer)) or not (1 <= int(terms) <= T):
        raise ValueError(f"terms must be an integer in 1 .. {T} (the trained grid), got {terms!r}")
    return paths.uniform_path(T, int(terms))[:-1]


@torch.no_grad()
def term_tables(gamma: torch.Tensor, t_list: Sequence[int]) -> Dict[str, object]:
    """Rows of the terms from the gamma grid [T+1] (fp32): t_idx int32 [K], coef fp32 [K,4] = {alpha_t, sigma_t, w_t, 0}.  alpha / sigma
    as the loss computes them (fp32 sqrt(sigmoid(-+gamma_t))); w_t = 0.5 expm1(gamma_t - gamma_{t-1}) in float64 from the fp32 table,
    rounded once."""
    g = torch.as_tensor(gamma, dtype=torch.float32).reshape(-1)
    idx = torch.as_tensor(list(t_list), dtype=torch.int64)
    gt, gs = g[idx], g[idx - 1]
    w = 0.5 * torch.expm1(gt.to(torch.float64) - gs.to(torch.float64))
    coef = torch.stack([torch.sqrt(torch.sigmoid(-gt)), torch.sqrt(torch.sigmoid(gt)), w.to(torch.float32), torch.zeros_like(gt)], dim=1)
    return {"t_idx": idx.to(torch.int32).contiguous(), "coef": coef.to(torch.float32).contiguous(), "K": int(idx.numel())}


def pad_samples(samples: Sequence[dict], n_dims: int, n_feat: int, with_context: bool):
    """A list of {'x': [n,3], 'h': [n,F] (, 'context': [n,1])} (what `sample` returns and stage 2 consumes) -> padded CPU tensors
    x [B,n_max,3] (re-centred per molecule, as `forward` does for a data batch), h [B,n_max,F], node_mask [B,n_max,1] and the context
    [B,n_max,1] or None."""
    xs, hs, cs = [], [], []
    for i, mol in enumerate(samples):
        if not isinstance(mol, dict) or "x" not in mol or "h" not in mol:
            raise ValueError(f"samples[{i}]: expected a dict with 'x' and 'h' (the sampler's output format)")
        x, h = torch.as_tensor(mol["x"], dtype=torch.float32), torch.as_tensor(mol["h"], dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != n_dims or tuple(h.shape) != (x.shape[0], n_feat):
            raise ValueError(f"samples[{i}]: need 'x' [n, {n_dims}] and 'h' [n, {n_feat}] with n >= 1")
        xs.append(x - x.mean(0, keepdim=True))
        hs.append(h)
        if with_context:
            if "context" not in mol:
                raise ValueError(f"samples[{i}]: the model takes a context, the sample carries none")
            c = torch.as_tensor(mol["context"], dtype=torch.float32).reshape(-1, 1)
            if c.shape[0] not in (1, x.shape[0]):
                raise ValueError(f"samples[{i}]: 'context' must hold one value, or one per node")
            cs.append(c.expand(x.shape[0], 1))
    B, n_max = len(xs), max(x.shape[0] for x in xs)
    X, Hh = torch.zeros(B, n_max, n_dims), torch.zeros(B, n_max, n_feat)
    nm = torch.zeros(B, n_max, 1, dtype=torch.bool)
    ctx = torch.zeros(B, n_max, 1) if with_context else None
    for i, (x, h) in enumerate(zip(xs, hs)):
        n = x.shape[0]
        X[i, :n], Hh[i, :n], nm[i, :n] = x, h, True
        if with_context:
            ctx[i, :n] = cs[i]
    return X, Hh, nm, ctx
