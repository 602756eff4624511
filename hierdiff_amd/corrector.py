"""Predictor-corrector sampling: Langevin correctors inside the path loop - host side (the `Corrector` keyword, its checks, the
per-transition rows).

Every loop term changes eps^ and hands it to an unchanged predictor step, which makes one move per noise level and never
equilibrates.  A corrector (Song et al. 2021, predictor-corrector samplers; Du et al. 2023, MCMC for composed and guided diffusion)
runs C unadjusted Langevin steps at the DEPARTURE level t_k of transition k, on the score the network and the call's terms define,
with fresh noise each step; then the predictor steps down.  Per molecule b (hd_set_corrector / hd_corrector_attach / k_langevin.hpp,
include/hierdiff_hip.h):

    z' = (z - (g_b sigma_t) eps~) + (sigma_t sqrt(2 g_b)) xi~            = z + delta score + sqrt(2 delta) xi,  delta = g_b sigma_t^2

with the gain g_b = q_k in mode "fixed" (`gain`), and in mode "snr" g_b = min(max_gain, q_k |xi~|^2 / |eps~|^2), q_k = 2 r_k^2
alpha^2_{t_k|s_k}: Song's signal-to-noise ratio r (`snr`) and the per-step alpha of the path.  Level 0 never gets a corrector (the
decode follows it); level T (or t_start) does.  Each corrector step costs one network call (two in a guided call) and one launch.

Mechanism only: r = 0.16 is Song et al.'s image value; which C and r help is for a trained checkpoint to show."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

MAX_STEPS = 8                   # HD_MAX_CORRECTORS
MODES = ("snr", "fixed")
WHERE = "sample / sample_from_masks / path_steps / sample_from_latent / latent_steps / vary / sample_chain"


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _per_step(v, name: str):
    """A finite number >= 0, or a sequence of them (one per transition; its length is checked against K by `resolve`)."""
    if isinstance(v, bool):
        raise ValueError(f"Corrector: {name} must be a number >= 0 or a length-K sequence, got {v!r}")
    if isinstance(v, (int, float, np.integer, np.floating)):
        out = float(v)
        if not (math.isfinite(out) and out >= 0.0):
            raise ValueError(f"Corrector: {name} must be finite and >= 0, got {v!r}")
        return out
    try:
        seq = tuple(float(x) for x in torch.as_tensor(v, dtype=torch.float64).reshape(-1).tolist())
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"Corrector: {name} must be a number >= 0 or a length-K sequence, got {v!r}") from None
    if not seq or not all(math.isfinite(x) and x >= 0.0 for x in seq):
        raise ValueError(f"Corrector: a {name} sequence holds one finite value >= 0 per transition")
    return seq


class Corrector:
    """The `corrector=` keyword of the sampling entry points.

    steps      C in 0 .. 8 Langevin steps per transition (0: the call without correctors)
    snr        mode "snr": Song's r, a number or one per transition (default 0.16)
    mode       "snr" (the gain follows the norms of noise and score per molecule) or "fixed" (the gain is `gain`)
    gain       mode "fixed": g_k, a number or one per transition
    max_gain   mode "snr": the cap of the gain (default inf: none)"""

    def __init__(self, steps: int = 1, snr=0.16, mode: str = "snr", gain=None, max_gain: float = math.inf):
        if not _is_int(steps) or not 0 <= int(steps) <= MAX_STEPS:
            raise ValueError(f"Corrector: steps must be an integer in 0 .. {MAX_STEPS}, got {steps!r}")
        if mode not in MODES:
            raise ValueError(f"Corrector: mode must be one of {MODES}, got {mode!r}")
        self.steps, self.mode = int(steps), mode
        self.snr = _per_step(snr, "snr")
        if mode == "fixed":
            if gain is None:
                raise ValueError("Corrector: mode 'fixed' needs gain (a number >= 0 or a length-K sequence)")
            self.gain = _per_step(gain, "gain")
        else:
            if gain is not None:
                raise ValueError("Corrector: gain goes with mode 'fixed' (mode 'snr' derives the gain from snr)")
            self.gain = None
        try:
            self.max_gain = float(max_gain)
        except (TypeError, ValueError):
            raise ValueError(f"Corrector: max_gain must be a number > 0 (inf: no cap), got {max_gain!r}") from None
        if not self.max_gain > 0.0:
            raise ValueError(f"Corrector: max_gain must be a number > 0 (inf: no cap), got {max_gain!r}")

    @property
    def strength(self):
        """What scales the step: `gain` in mode "fixed", `snr` in mode "snr"."""
        return self.gain if self.mode == "fixed" else self.snr

    @property
    def active(self) -> bool:
        s = self.strength
        return self.steps > 0 and (any(x != 0.0 for x in s) if isinstance(s, tuple) else s != 0.0)

    @property
    def adaptive(self) -> int:
        return 1 if self.mode == "snr" else 0

    def key(self):
        """What the uploaded rows depend on, besides the path tables."""
        return (self.mode, self.strength, self.max_gain)

    def __repr__(self):
        return f"Corrector(steps={self.steps}, snr={self.snr}, mode={self.mode!r}, gain={self.gain}, max_gain={self.max_gain})"


def wanted(model, corrector=None) -> bool:
    """Whether the keyword (None: the model's `corrector`) asks for corrector steps at all.  None, steps = 0, or a strength of 0
    everywhere is the code path without them; anything else - a value that is no `Corrector` included, which `resolve` then refuses -
    asks for them."""
    cr = getattr(model, "corrector", None) if corrector is None else corrector
    if cr is None:
        return False
    return cr.active if isinstance(cr, Corrector) else True


def rows(gamma, path: Sequence[int], cr: Corrector) -> np.ndarray:
    """[K, 3] float32 rows {sigma_t, q_k, g_max_k} of the transitions of `path` (grid indices, path[k] -> path[k + 1]; the departure
    level t = path[k] counts) from the gamma grid, in float64 and rounded once.  Mode "snr": q_k = 2 r_k^2 alpha^2_{t|s} with
    alpha^2_{t|s} = sigmoid(-gamma_t) / sigmoid(-gamma_s); mode "fixed": q_k = gain_k."""
    g = torch.as_tensor(gamma).detach().to(torch.float64).reshape(-1)
    K = len(path) - 1
    if K < 1:
        raise ValueError("corrector rows: the path has no transition")
    t = torch.as_tensor(list(path[:-1]), dtype=torch.int64)
    s = torch.as_tensor(list(path[1:]), dtype=torch.int64)
    sp = torch.nn.functional.softplus
    sigma_t = torch.sqrt(torch.sigmoid(g[t]))
    st = cr.strength
    v = torch.tensor(list(st) if isinstance(st, tuple) else [st] * K, dtype=torch.float64)
    if v.numel() != K:
        raise ValueError(f"the corrector's {'gain' if cr.mode == 'fixed' else 'snr'} holds one value per transition ({K}), got {v.numel()}")
    q = v if cr.mode == "fixed" else 2.0 * v * v * torch.exp(sp(g[s]) - sp(g[t]))
    out = np.empty((K, 3), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2] = sigma_t.numpy(), q.numpy(), np.float32(cr.max_gain)
    if not np.isfinite(out[:, :2]).all():
        raise ValueError("the corrector's rows are not finite in float32 (snr / gain too large)")
    return out


def resolve(model, corrector, K: int, what: str = "corrector", steered: bool = False) -> Optional[Corrector]:
    """Keyword (None: the model's `corrector`) -> None for the code path without it, or the `Corrector`.  `K`: the plan's transitions;
    `steered`: the plan steers.  Pure host checks."""
    if not wanted(model, corrector):
        return None
    cr = getattr(model, "corrector", None) if corrector is None else corrector
    if not isinstance(cr, Corrector):
        raise ValueError(f"{what}: corrector must be a hierdiff_amd.corrector.Corrector, got {type(cr).__name__}")
    if steered:
        raise NotImplementedError(f"{what}: corrector= and steering (particles=) in one call are not supported: the particles' weights "
                                  "follow the predictor's moves alone")
    st = cr.strength
    if isinstance(st, tuple) and len(st) != int(K):
        raise ValueError(f"{what}: the corrector's {'gain' if cr.mode == 'fixed' else 'snr'} holds one value per transition ({K}), "
                         f"got {len(st)}")
    return cr


def refuse(model, what: str, corrector=None, why: str = "") -> None:
    """Entry points that take no corrector: an error when the keyword or the model's attribute asks for one, instead of ignoring it."""
    if wanted(model, corrector):
        raise NotImplementedError(f"{what}: predictor-corrector sampling is not supported here{why} (the `corrector` keyword, or "
                                  f"model.corrector); it acts in {WHERE}")


def attach(topo, cr: Corrector, stream) -> None:
    """Attach the corrector to `topo` (hd_corrector_attach): C steps per transition in its mode."""
    from . import _lib
    _lib.check(_lib.load().hd_corrector_attach(topo.ptr, int(cr.steps), int(cr.adaptive), stream), "hd_corrector_attach")


def read_gains(topo, cr: Corrector, B: int, dev, stream) -> torch.Tensor:
    """[C, B] float64 (CPU): the gains g_b of the last transition that ran (hd_corrector_read); 0 where a molecule kept its bits."""
    from . import _lib
    out = torch.zeros((int(cr.steps), int(B)), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().hd_corrector_read(topo.ptr, out.data_ptr(), stream), "hd_corrector_read")
    return out.cpu()
