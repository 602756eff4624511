"""Steered sampling: particle resampling on the restraint energy inside the path loop - host side (argument resolution, the group
checks, the per-transition rows, the result entries).

A steered call runs P particles per requested molecule: the batch is B = G * P rows, group g owns rows g P .. g P + P - 1.  At every
transition, behind the network call, guidance and the restraint update of eps^, the rows of a group are weighted by how the restraint
energy U of their data prediction changed, logw += -beta_k (U_k - U_prev), and when the effective sample size (sum w)^2 / sum w^2 falls
below rho P the group is resampled systematically with one counter-based uniform: low-energy particles are duplicated, high-energy ones
dropped, and the stochastic update that follows lets the duplicates diverge (hd_set_steer / hd_steer_attach / k_steer.hpp,
include/hierdiff_hip.h).  No gradient, no second network call; it composes with `restraint_scale`, which may now be None or 0.

THE CONTRACT.  A group's result depends on the seed, the ids of its rows, P, its masks, context and tables, the weights, the schedule
and the path only - not on the other groups of the batch, on where the batch was cut (at group boundaries), on graph replay versus
plain launches, or on how `path_steps` cuts the chain.  Rows of a group interact; groups do not.

Everything in this module is host arithmetic.  Mechanism only: which beta, rho and P help is for a trained checkpoint to show."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

MAX_PARTICLES = 256
WHERE = "sample / sample_from_masks / path_steps / sample_from_latent / latent_steps / vary"


class Steer(NamedTuple):
    P: int                                        # particles per group
    beta: float                                   # steer_scale
    ess: float                                    # rho: resample when ESS < rho P
    schedule: Optional[Tuple[float, ...]]         # K multipliers of beta, or None

    def key(self):
        return (self.beta, self.schedule)


def _attrs(model, particles, steer_scale):
    particles = getattr(model, "particles", None) if particles is None else particles
    steer_scale = getattr(model, "steer_scale", None) if steer_scale is None else steer_scale
    return particles, steer_scale


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_num(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def wanted(model, particles=None, steer_scale=None) -> bool:
    """Whether the keywords (None: the model's attributes) ask for steering at all.  particles of None or 1, or a steer_scale of None
    or 0, is the unsteered code path; anything else - malformed values included, which `resolve` then refuses - asks for it."""
    particles, steer_scale = _attrs(model, particles, steer_scale)
    if particles is None or steer_scale is None:
        return False
    if _is_int(particles) and int(particles) == 1:
        return False
    if _is_num(steer_scale) and float(steer_scale) == 0.0:
        return False
    return True


def resolve(model, particles, steer_scale, steer_ess, steer_schedule, eta, K: int, restrained: bool, B: Optional[int] = None,
            what: str = "steering", injected: bool = False) -> Optional[Steer]:
    """Keywords (None: the model's `particles` / `steer_scale` / `steer_ess`) -> None for the unsteered code path, untouched, or a
    `Steer`.  `eta`: the plan's update (a float, or the `paths.Multistep` of solver "dpm2m" - refused - or "sde2m"); `K`: its transitions; `restrained`:
    the plan holds restraints.  Pure host checks."""
    if not wanted(model, particles, steer_scale):
        return None
    particles, steer_scale = _attrs(model, particles, steer_scale)
    steer_ess = getattr(model, "steer_ess", None) if steer_ess is None else steer_ess
    steer_ess = 0.5 if steer_ess is None else steer_ess
    if not _is_int(particles) or int(particles) < 1:
        raise ValueError(f"{what}: particles must be an integer >= 1, got {particles!r}")
    P = int(particles)
    if P > MAX_PARTICLES:
        raise ValueError(f"{what}: particles must be <= {MAX_PARTICLES} (one workgroup resamples a group), got {P}")
    if not _is_num(steer_scale) or not math.isfinite(float(steer_scale)) or float(steer_scale) < 0.0:
        raise ValueError(f"{what}: steer_scale must be a finite number >= 0, got {steer_scale!r}")
    if not _is_num(steer_ess) or not (0.0 < float(steer_ess) <= 1.0):
        raise ValueError(f"{what}: steer_ess must lie in (0, 1], got {steer_ess!r}")
    sched = None
    if steer_schedule is not None:
        try:
            sched = tuple(float(v) for v in torch.as_tensor(steer_schedule, dtype=torch.float64).reshape(-1).tolist())
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{what}: steer_schedule must be a sequence of K numbers, got {steer_schedule!r}") from None
        if len(sched) != int(K) or not all(math.isfinite(v) and v >= 0.0 for v in sched):
            raise ValueError(f"{what}: steer_schedule holds one finite multiplier >= 0 per transition ({K})")
    if not restrained:
        raise ValueError(f"{what}: steering weighs the particles by their restraint energy: restraints= is required")
    if getattr(eta, "stochastic", False):
        eta = 1.0                                 # solver "sde2m": second order, and the ancestral noise on the path
    if not isinstance(eta, (int, float)) or isinstance(eta, bool):
        raise ValueError(f"{what}: steering needs a stochastic update, and solver 'dpm2m' draws nothing on the path (duplicated "
                         "particles would never diverge)")
    if float(eta) == 0.0:
        raise ValueError(f"{what}: steering needs a stochastic update (eta > 0): with eta = 0 duplicated particles never diverge")
    if injected:
        raise NotImplementedError(f"{what}: steering draws its resampling uniforms from the counter-based generator: injected "
                                  "noise (raw_noises) is not supported")
    if B is not None and int(B) % P != 0:
        raise ValueError(f"{what}: the batch ({B}) must be a multiple of particles ({P}): group g owns rows g P .. g P + P - 1")
    return Steer(P, float(steer_scale), float(steer_ess), sched)


def refuse(model, what: str, why: str = "") -> None:
    """Entry points that do not steer: an error when the model's attributes ask for it, instead of ignoring them."""
    if wanted(model):
        raise NotImplementedError(f"{what}: steered sampling is not supported here{why} (model.particles with a non-zero "
                                  f"model.steer_scale); it acts in {WHERE}")


def _rows_equal(t: torch.Tensor, P: int) -> bool:
    g = t.reshape(t.shape[0] // P, P, -1)
    return bool((g == g[:, :1]).all())


def check_groups(st: Steer, node_mask, context=None, rs=None, scale=None, what: str = "steering") -> None:
    """All rows of a group must have equal node masks, context rows and per-molecule restraint rows (shared tables are trivially
    equal; so are field values, only their weights can differ) and restraint scales.  Compared on the host."""
    P = st.P
    nm = torch.as_tensor(node_mask).detach().cpu()
    B = int(nm.shape[0])
    if B % P != 0:
        raise ValueError(f"{what}: the batch ({B}) must be a multiple of particles ({P}): group g owns rows g P .. g P + P - 1")
    bad = None
    if not _rows_equal(nm.reshape(B, -1), P):
        bad = "node masks"
    elif context is not None and not _rows_equal(torch.as_tensor(context).detach().cpu().reshape(B, -1), P):
        bad = "context rows"
    elif rs is not None:
        for name in ("obs", "pair_idx", "pair_f", "anc_idx", "anc_f"):
            t = getattr(rs, name)
            if t.shape[0] == B and B > 1 and t.numel() and not _rows_equal(t.reshape(B, -1), P):
                bad = f"restraint rows ({name})"
                break
        if bad is None:
            for f in getattr(rs, "fields", ()):
                w = f.weights
                if w is not None and w.shape[0] == B and B > 1 and not _rows_equal(w.reshape(B, -1), P):
                    bad = "restraint rows (field weights)"
                    break
        if bad is None:
            for t in getattr(rs, "templates", ()):
                if t.rows == B and B > 1 and not all(_rows_equal(v.reshape(B, -1), P) for v in (t.index, t.positions, t.weights)):
                    bad = "restraint rows (templates)"
                    break
        ft = getattr(rs, "features", None)
        if bad is None and ft is not None and B > 1:
            per = [t for t in (ft.lo, ft.hi, ft.k) if t is not None and t.shape[0] == B] + \
                  [t for r in ft.sums for t in (r.lo, r.hi) if t.shape[0] == B]
            if not all(_rows_equal(t.reshape(B, -1), P) for t in per):
                bad = "restraint rows (features)"
    if bad is None and scale is not None and torch.as_tensor(scale).numel() == B and not _rows_equal(torch.as_tensor(scale).cpu().reshape(B, 1), P):
        bad = "restraint scales"
    if bad is not None:
        raise ValueError(f"{what}: the {bad} differ inside a group of {P} particles (rows g P .. g P + P - 1 must be equal)")


def beta_rows(gamma, path, st: Steer) -> np.ndarray:
    """[K, 3] float32 rows {alpha_t, sigma_t, beta_k} of the transitions of `path`: alpha / sigma are the fp32 values of
    `restraints.lambda_rows` (those a record="x0" frame uses); beta_k = steer_scale (times the schedule's k-th value), evaluated in
    float64 and rounded once."""
    g32 = torch.as_tensor(gamma).detach().to(torch.float32).reshape(-1)
    K = len(path) - 1
    t = torch.as_tensor(list(path[:-1]), dtype=torch.int64)
    rows = np.empty((K, 3), dtype=np.float32)
    rows[:, 0] = torch.sqrt(torch.sigmoid(-g32[t])).numpy()
    rows[:, 1] = torch.sqrt(torch.sigmoid(g32[t])).numpy()
    mult = np.ones(K) if st.schedule is None else np.asarray(st.schedule, dtype=np.float64)
    rows[:, 2] = (st.beta * mult).astype(np.float32)
    return rows


class Result(NamedTuple):
    """The steering state behind a call (CPU tensors): per row the normalised log-weight within its group, the index within the group
    of the initial particle it descends from and its group number; per group the resampling events, the smallest ESS and the
    transitions in which every weight was 0, since the chain started."""
    logw: torch.Tensor          # [B] float64
    root: torch.Tensor          # [B] int64
    group: torch.Tensor         # [B] int64
    events: torch.Tensor        # [G] int64
    min_ess: torch.Tensor       # [G] float64
    dead: torch.Tensor          # [G] int64


def normalise(logw: torch.Tensor, P: int) -> torch.Tensor:
    """logw - logsumexp over the group; a group whose weights are all 0 keeps -inf."""
    g = logw.reshape(-1, P)
    lse = torch.logsumexp(g, dim=1, keepdim=True)
    out = torch.where(torch.isfinite(lse), g - lse, g)
    return out.reshape(-1)


def attach(topo, st: Steer, reset: bool, stream) -> None:
    """Attach the steering `st` to `topo` (hd_steer_attach).  `reset`: start a chain; else continue on the state the topology holds."""
    from . import _lib
    _lib.check(_lib.load().hd_steer_attach(topo.ptr, st.P, st.ess, int(bool(reset)), stream), "hd_steer_attach")


def close(model, topo, st: Steer, B: int, dev, stream, ran: bool) -> None:
    """Detach (hd_steer_detach) and, behind a call that `ran`, keep the state it left as `model.steer_last` (hd_steer_read)."""
    from . import _lib
    lib = _lib.load()
    _lib.check(lib.hd_steer_detach(topo.ptr), "hd_steer_detach")
    if not ran:
        return
    logw = torch.empty(B, device=dev, dtype=torch.float64)
    root = torch.empty(B, device=dev, dtype=torch.int32)
    stats = torch.empty((B // st.P, 3), device=dev, dtype=torch.float64)
    _lib.check(lib.hd_steer_read(topo.ptr, logw.data_ptr(), None, root.data_ptr(), None, stats.data_ptr(), stream), "hd_steer_read")
    stats = stats.cpu()
    model.steer_last = Result(normalise(logw.cpu(), st.P), root.cpu().long(), torch.arange(B) // st.P, stats[:, 0].long(),
                              stats[:, 1].clone(), stats[:, 2].long())


def into(results, res: Result, lo: int = 0, group0: int = 0) -> None:
    """'steer_logw', 'steer_root', 'steer_group' into the dicts of rows lo .. lo + len(results) - 1 of `res`."""
    for i, r in enumerate(results):
        r['steer_logw'] = res.logw[lo + i].clone()
        r['steer_root'] = res.root[lo + i].clone()
        r['steer_group'] = res.group[lo + i] + group0
